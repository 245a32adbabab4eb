// The division-step inversion (go-curdleproofs_amd/csrc/invert_ds.h) as a stand-alone host program, TEST INFRASTRUCTURE
// ONLY: built with -fsanitize=address,undefined by tests/test_invert_ds_host.py, which writes the cases of
// tests/fp_divsteps_model.py to a file and compares what this program prints with the model bit for bit.  The header's
// own code runs here -- the body, the repackings, the masked canonical step and both entry forms; the one thing restated
// is fp28.h's Montgomery product (device-only there), as a word-serial reduction on the same 14 limbs of 28 bits.
//
//   invert_ds_flow <cases>      a line per case: "G <hex>" a gnark element (the integer of its 12 words), "R <hex>" a raw
//                               element (the integer of its 14 limbs, below 2p), "X <hex>" a gnark word pattern at or
//                               above p: run, nothing compared (the sanitizers are the check)
//   prints                      "G <violation> <12 words>", "R <violation> <14 limbs>", "X <violation>", hex, a line each
#include <stdio.h>
#include <string.h>

#include "../../go-curdleproofs_amd/csrc/invert_ds.h"

using namespace curdle;

namespace {
constexpr u32 kN0 = 0x0ffcfffdu;  // -p^-1 mod 2^28 (fp28.h's N0)

// r = a b / 2^392 mod p on 14 limbs of 28 bits: below 2p, limbs 0..12 below 2^28, for normalised a, b below 2p
void mul28(u32* r, const u32* a, const u32* b) {
  u64 t[29] = {};
  for (int i = 0; i < 14; i++)
    for (int j = 0; j < 14; j++) t[i + j] += (u64)a[i] * b[j];
  for (int k = 0; k < 14; k++) {
    const u32 m = ((u32)t[k] * kN0) & ds::M28;
    for (int j = 0; j < 14; j++) t[k + j] += (u64)m * ds::kP28(j);
    t[k + 1] += t[k] >> 28;
  }
  for (int i = 0; i < 13; i++) {
    r[i] = (u32)t[14 + i] & ds::M28;
    t[15 + i] += t[14 + i] >> 28;
  }
  r[13] = (u32)t[27];
}

// a hex integer of at most 416 bits into 13 words of 32
bool parse(const char* s, u32 w[13]) {
  memset(w, 0, 13 * sizeof(u32));
  const size_t n = strlen(s);
  if (n == 0 || n > 104) return false;
  for (size_t i = 0; i < n; i++) {
    const char c = s[n - 1 - i];
    u32 v;
    if (c >= '0' && c <= '9') v = c - '0';
    else if (c >= 'a' && c <= 'f') v = c - 'a' + 10;
    else return false;
    w[i / 8] |= v << (4 * (i % 8));
  }
  return true;
}

void print_words(const char* tag, u32 viol, const u32* w, int n) {
  printf("%s %x", tag, viol);
  for (int i = 0; i < n; i++) printf(" %x", w[i]);
  printf("\n");
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* fp = fopen(argv[1], "r");
  if (!fp) return 2;
  char form, hex[128];
  int cases = 0;
  while (fscanf(fp, " %c %127s", &form, hex) == 2) {
    u32 w[13];
    if (!parse(hex, w)) return 3;
    if (form == 'G' || form == 'X') {
      u32 y[12];
      const u32 viol = ds::invert_gnark_words(y, w, mul28);
      if (form == 'G')
        print_words("G", viol, y, 12);
      else
        printf("X %x\n", viol);
    } else if (form == 'R') {
      u32 a[14], y[14];
      ds::repack<32, 13, 28, 14>(a, w);
      const u32 viol = ds::invert_limbs28(y, a, mul28);
      print_words("R", viol, y, 14);
    } else {
      return 3;
    }
    cases++;
  }
  fclose(fp);
  printf("invert_ds_flow OK %d\n", cases);
  return 0;
}
