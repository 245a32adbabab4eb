// Host-only probe of the library's MSM plan (tests/test_plan.py): calls make_plan over a grid of calls and prints, per
// call, the inputs and the plan fields the plan invariants are about.  No device is touched.
//   plan_probe n glv pipelined chunked c: the plan of ONE single-MSM call instead (tests/test_msm_large_gpu.py), with
//   the window widths and the bucket counts per window.
//   plan_probe members n_tot k: the plan of the device accumulator's member form (curdle_dacc_run_members) instead: ONE
//   call of k MSMs of n_tot pairs each over shared bases (tests/test_dacc_members_model.py, tests/test_dacc_members_mid_gpu.py).
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "msm_internal.h"

static void probe(const char* shape, const std::vector<uint32_t>& off, MsmCall call) {
  call.off = off.data();
  call.k = off.size() - 1;
  MsmPlan p;
  const int rc = make_plan(p, call);
  printf("%s n=%u k=%zu sets=%zu c=%d wb=%d we=%d pipelined=%d joined=%d chunked=%d many=%d light=%d glv=%d seg=%u rc=%d", shape,
         off.back(), call.k, call.sets, call.c, call.win_begin, call.win_end, call.pipelined, call.joined, call.chunked, call.many,
         call.light_host, call.glv, call.seg, rc);
  if (rc == CURDLE_OK)
    printf(" terms=%u nw=%d pk=%u psets=%u NB=%u L=%u max_small=%u max_large=%u fuse_scan=%u two_level=%u c=%d", p.n,
           p.win_end - p.win_begin, p.k, p.sets, p.NB, p.L, p.max_small, p.max_large, p.fuse_scan, p.two_level, p.c);
  printf("\n");
}

static int one(char** argv) {
  const uint32_t n = (uint32_t)strtoul(argv[1], nullptr, 0);
  const std::vector<uint32_t> off = {0, n};
  MsmCall call;
  call.off = off.data();
  call.glv = atoi(argv[2]) != 0;
  call.pipelined = atoi(argv[3]) != 0;
  call.joined = call.chunked = atoi(argv[4]) != 0;
  call.c = atoi(argv[5]);
  probe("one", off, call);
  MsmPlan p;
  if (make_plan(p, call) != CURDLE_OK) return 1;
  printf("windows");
  for (int w = 0; w < p.W; w++) printf(" %u:%u", p.bits[w], p.nbkt[w]);
  printf("\n");
  return 0;
}

// k equal offsets, shared_bases: what curdle_dacc_run_members hands make_plan.  `slots` is k * NB, what the scans walk and what
// the form's limit (kMaxSlotsPerPass) is about; `sort_blocks` is ceil(2 n_tot / chunk), the k_hist / k_scatter blocks per member.
static int members(char** argv) {
  const uint32_t n_tot = (uint32_t)strtoul(argv[2], nullptr, 0);
  const size_t k = (size_t)strtoul(argv[3], nullptr, 0);
  std::vector<uint32_t> off(k + 1);
  for (size_t j = 0; j <= k; j++) off[j] = (uint32_t)(j * n_tot);
  MsmCall call;
  call.off = off.data();
  call.k = k;
  call.shared_bases = true;
  MsmPlan p;
  const int rc = make_plan(p, call);
  printf("members n_tot=%u k=%zu rc=%d", n_tot, k, rc);
  if (rc == CURDLE_OK) {
    const uint64_t slots = (uint64_t)k * p.NB;
    printf(" c=%d NB=%u L=%u chunk=%u max_small=%u max_large=%u fuse_scan=%u gpu_combine=%u slots=%llu sort_blocks=%u fits=%d\nwindows",
           p.c, p.NB, p.L, p.chunk, p.max_small, p.max_large, p.fuse_scan, p.gpu_combine, (unsigned long long)slots,
           p.chunk ? (2 * n_tot + p.chunk - 1) / p.chunk : 0, slots <= kMaxSlotsPerPass ? 1 : 0);
    for (int w = 0; w < p.W; w++) printf(" %u:%u", p.bits[w], p.nbkt[w]);
  }
  printf("\n");
  return rc == CURDLE_OK ? 0 : 1;
}

int main(int argc, char** argv) {
  if (argc == 6) return one(argv);
  if (argc == 4 && !strcmp(argv[1], "members")) return members(argv);
  // single MSMs and batches, every mode flag, several window ranges and widths
  const uint32_t sizes[] = {1, 300, 1268, 8192, 16384, 65536, 131072, 1u << 18, 1u << 20, 1u << 22, 1u << 24, 22369622,
                            1u << 25, 1u << 26, 1u << 27};
  const int ranges[][2] = {{0, -1}, {0, 1}, {1, 3}};
  for (uint32_t n : sizes)
    for (size_t k : {1, 3, 16})
      for (size_t sets : {1, 3}) {
        if ((k > 1 || sets > 1) && (uint64_t)n * k * sets > (1u << 27)) continue;
        std::vector<uint32_t> off(k + 1);
        for (size_t j = 0; j <= k; j++) off[j] = (uint32_t)(j * n);
        for (int c : {0, 16})
          for (auto& r : ranges)
            for (int flags = 0; flags < 64; flags++) {
              MsmCall call;
              call.sets = sets;
              call.c = c;
              call.win_begin = r[0];
              call.win_end = r[1];
              call.pipelined = flags & 1;
              call.many = flags & 2;
              call.light_host = flags & 4;
              call.glv = !(flags & 8);
              call.joined = flags & 16;
              call.chunked = (flags & 48) == 48;
              call.seg = call.chunked ? 8 : 0;
              probe("grid", off, call);
            }
      }
  // the chunks of host-buffer calls as run_host_chunked cuts them: 2..8 graded chunks over one plan of the whole call's width
  const uint32_t whole[] = {1u << 19, 1u << 20, 1u << 22, 1u << 24, 48u << 20, 1u << 26, 80u << 20, 1u << 27};
  for (uint32_t n : whole)
    for (uint32_t nchunks = 2; nchunks <= 8; nchunks++) {
      std::vector<uint32_t> sizes_of;
      if (nchunks >= 3) {
        const uint64_t unit = (n + 2 * (nchunks - 1) - 1) / (2 * (nchunks - 1));
        uint64_t at = 0;
        for (uint32_t i = 0; i < nchunks; i++) {
          const uint64_t next = at + (i < 2 ? unit : 2 * unit) < n ? at + (i < 2 ? unit : 2 * unit) : n;
          sizes_of.push_back((uint32_t)(next - at));
          at = next;
        }
      } else {
        sizes_of = {n / 2, n - n / 2};
      }
      for (uint32_t m : sizes_of) {
        if (!m) continue;
        MsmCall call;
        call.c = curdle_msm_window_bits(n);
        call.joined = call.chunked = true;
        call.seg = nchunks >= 3 ? 8 : 0;
        for (bool glv : {true, false}) {
          call.glv = glv;
          probe("chunk", {0, m}, call);
        }
      }
    }
  // beyond the supported size: refused
  probe("over", {0, (1u << 27) + 1}, MsmCall());
  return 0;
}
