// curdle_crs_from_points / _from_bytes / _export_points / _to_bytes on the host backend (stub_backend.cpp).  A stand-alone
// program for the sanitizer build of tests/test_crs_import_host.py (address + undefined, leaks counted); it ends with
// "crs_import_flow OK" or a non-zero exit.  The stub backend decodes compressed points on the host; the two membership
// checks it does not have are defined here over the host's decoder.  The import's staging, its verdict over the status
// bytes, what every way out frees and the handle it makes are under test, not the point checks.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../go-curdleproofs_amd/host/algebra.h"
#include "../../go-curdleproofs_amd/host/common_rand.h"
#include "../../include/curdle_msm.h"

using namespace curdle;
using alg::Point;
using alg::Scalar;

#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                       \
    }                                                                \
  } while (0)

static int g_affine_checks, g_jac_checks;
static size_t g_affine_points;

static uint8_t CheckAffine(const G1Affine& a) {
  if (g1_affine_is_inf(a)) return CURDLE_DECODE_INFINITY;
  uint8_t enc[48];
  alg::CompressAffine(a, enc);
  Point q;
  if (!Point::FromCompressed(enc, &q, false)) return CURDLE_DECODE_NOT_ON_CURVE;
  const G1Affine b = q.Affine();
  if (memcmp(&a, &b, sizeof(a))) return CURDLE_DECODE_NOT_ON_CURVE;
  return Point::FromCompressed(enc, &q, true) ? CURDLE_DECODE_OK : CURDLE_DECODE_NOT_IN_SUBGROUP;
}
extern "C" int curdle_g1_check_batch(const uint64_t* points, size_t n, int subgroup_check, uint8_t* status) {
  CHECK(subgroup_check == 1);
  g_affine_checks++;
  g_affine_points += n;
  for (size_t i = 0; i < n; i++) {
    G1Affine a;
    memcpy(&a, points + 12 * i, sizeof(a));
    status[i] = CheckAffine(a);
  }
  return CURDLE_OK;
}
extern "C" int curdle_g1_check_jac_batch(const uint64_t* jac_points, size_t n, int subgroup_check, uint8_t* status) {
  CHECK(subgroup_check == 1);
  g_jac_checks++;
  for (size_t i = 0; i < n; i++) {
    const Point p = Point::FromJac(jac_points + 18 * i);
    status[i] = p.IsInfinity() ? CURDLE_DECODE_INFINITY : CheckAffine(p.Affine());
  }
  return CURDLE_OK;
}

struct curdle_rand {  // same layout as in misc_api.hip / proto_api.cpp
  common::Rand r;
  explicit curdle_rand(uint64_t seed) : r(seed) {}
};

struct Exported {
  size_t ell;
  std::vector<uint64_t> Gs, Hs, H, Gt, Gu, Gsum, Hsum;
  explicit Exported(size_t n) : ell(n), Gs(12 * n), Hs(48), H(18), Gt(18), Gu(18), Gsum(12), Hsum(12) {}
  curdle_crs_points View() const { return curdle_crs_points{Gs.data(), ell, Hs.data(), H.data(), Gt.data(), Gu.data(), Gsum.data(), Hsum.data()}; }
  bool operator==(const Exported& o) const {
    return Gs == o.Gs && Hs == o.Hs && H == o.H && Gt == o.Gt && Gu == o.Gu && Gsum == o.Gsum && Hsum == o.Hsum;
  }
};
static Exported Export(const curdle_crs* crs) {
  Exported e(curdle_crs_size(crs));
  CHECK(curdle_crs_export_points(crs, e.Gs.data(), e.Hs.data(), e.H.data(), e.Gt.data(), e.Gu.data(), e.Gsum.data(), e.Hsum.data()) == CURDLE_OK);
  return e;
}
static std::vector<uint8_t> Bytes(const curdle_crs* crs) {
  size_t need = 0;
  CHECK(curdle_crs_to_bytes(crs, nullptr, 0, &need) == CURDLE_EINVAL && need == 48 * (curdle_crs_size(crs) + 9));
  std::vector<uint8_t> b(need);
  size_t len = 0;
  CHECK(curdle_crs_to_bytes(crs, b.data(), b.size(), &len) == CURDLE_OK && len == need);
  return b;
}
static bool LastErrorHas(const char* text) {
  char buf[256];
  curdle_last_error(buf, sizeof(buf));
  return strstr(buf, text) != nullptr;
}

static const curdle_crs_fault kSentinel = {0x5a5a, 0x1234567, 0x7e7e};
static bool Untouched(const curdle_crs_fault& f) { return f.field == kSentinel.field && f.index == kSentinel.index && f.reason == kSentinel.reason; }

// A TRUSTED import of an exported CRS proves the generated handle's bytes from the same seeds, and either handle verifies.
static void TrustedEquivalence(size_t ell) {
  curdle_rand crs_rand(11 + ell);
  curdle_crs* gen = curdle_crs_generate(ell, &crs_rand);
  CHECK(gen);
  const Exported e = Export(gen);
  const curdle_crs_points view = e.View();
  const int affine0 = g_affine_checks, jac0 = g_jac_checks;
  curdle_crs* imp = nullptr;
  curdle_crs_fault fault = kSentinel;
  CHECK(curdle_crs_from_points(&view, CURDLE_CRS_TRUSTED, &imp, &fault) == CURDLE_OK && imp);
  CHECK(fault.field == -1 && fault.index == 0 && fault.reason == 0);
  CHECK(g_affine_checks == affine0 && g_jac_checks == jac0);  // nothing was checked
  CHECK(curdle_crs_size(imp) == ell && Export(imp) == e && Bytes(imp) == Bytes(gen));

  std::vector<G1Affine> Rs, Ss, Ts(ell), Us(ell);
  std::vector<uint32_t> perm;
  uint64_t M[18], k[4], rs_m[16];
  {
    common::Rand r(100 + ell);
    r.GetG1Affines(ell, Rs);
    r.GetG1Affines(ell, Ss);
    r.GeneratePermutation(ell, perm);
    Fr kk;
    r.GetFr(kk);
    memcpy(k, &kk, 32);
    curdle_rand cr(200);
    CHECK(curdle_shuffle_permute_commit(imp, (const uint64_t*)Rs.data(), (const uint64_t*)Ss.data(), ell, perm.data(), k, &cr,
                                        (uint64_t*)Ts.data(), (uint64_t*)Us.data(), M, rs_m) == CURDLE_OK);
  }
  const uint64_t *R = (const uint64_t*)Rs.data(), *S = (const uint64_t*)Ss.data(), *T = (const uint64_t*)Ts.data(),
                 *U = (const uint64_t*)Us.data();
  const size_t cap = 1 << 14;
  std::vector<uint8_t> a(cap), b(cap);
  size_t a_len = 0, b_len = 0;
  Fr next_a, next_b;
  {
    curdle_rand cr(300);
    CHECK(curdle_prove(gen, R, S, T, U, ell, M, perm.data(), k, rs_m, &cr, a.data(), cap, &a_len) == CURDLE_OK);
    cr.r.GetFr(next_a);
  }
  {
    curdle_rand cr(300);
    CHECK(curdle_prove(imp, R, S, T, U, ell, M, perm.data(), k, rs_m, &cr, b.data(), cap, &b_len) == CURDLE_OK);
    cr.r.GetFr(next_b);
  }
  CHECK(a_len == b_len && a_len > 0 && !memcmp(a.data(), b.data(), a_len) && !memcmp(&next_a, &next_b, 32));
  for (const curdle_crs* crs : {(const curdle_crs*)gen, (const curdle_crs*)imp}) {
    curdle_rand vr(400);
    int ok = 0;
    CHECK(curdle_verify(crs, a.data(), a_len, R, S, T, U, ell, M, &vr, &ok) == CURDLE_OK && ok == 1);
  }
  a[a_len / 2] ^= 1;  // ... and both refuse the same damaged proof the same way
  int rc[2], oks[2];
  const curdle_crs* both[2] = {gen, imp};
  for (int i = 0; i < 2; i++) {
    curdle_rand vr(400);
    oks[i] = 7;
    rc[i] = curdle_verify(both[i], a.data(), a_len, R, S, T, U, ell, M, &vr, &oks[i]);
  }
  CHECK(rc[0] == rc[1] && oks[0] == oks[1] && oks[0] == 0);
  curdle_crs_free(imp);
  curdle_crs_free(gen);
}

// Every refusal and every fault leaves *out NULL and frees what the call allocated (the leak check is the witness).
static void RefusalsAndFaults() {
  const size_t ell = 12;
  curdle_rand crs_rand(5);
  curdle_crs* gen = curdle_crs_generate(ell, &crs_rand);
  CHECK(gen);
  const Exported e = Export(gen);
  const std::vector<uint8_t> wire = Bytes(gen);
  curdle_crs* out = reinterpret_cast<curdle_crs*>(0x10);
  curdle_crs_fault fault = kSentinel;
  auto refused = [&](int rc, const char* text) {
    CHECK(rc == CURDLE_EINVAL && out == nullptr && Untouched(fault) && LastErrorHas(text));
    out = reinterpret_cast<curdle_crs*>(0x10);
  };
  // step 1, in its order: null, flags, ell
  curdle_crs_points view = e.View();
  refused(curdle_crs_from_points(nullptr, 2, &out, &fault), "null argument");
  view.Gu = nullptr;
  view.ell = 0;
  refused(curdle_crs_from_points(&view, 2, &out, &fault), "null argument");
  view = e.View();
  CHECK(curdle_crs_from_points(&view, 0, nullptr, &fault) == CURDLE_EINVAL && Untouched(fault));
  view.ell = 0;
  refused(curdle_crs_from_points(&view, 2, &out, &fault), "unknown flag bits");
  refused(curdle_crs_from_points(&view, 0, &out, &fault), "ell must be");
  refused(curdle_crs_from_points(&view, CURDLE_CRS_TRUSTED, &out, &fault), "ell must be");
  view.ell = CURDLE_CRS_MAX_ELL + 1;
  refused(curdle_crs_from_points(&view, CURDLE_CRS_TRUSTED, &out, &fault), "ell must be");
  refused(curdle_crs_from_bytes(nullptr, wire.size(), &out, &fault), "null argument");
  for (size_t len : {(size_t)0, (size_t)48 * 9, wire.size() - 1, wire.size() + 1, (size_t)48 * (((size_t)1 << 20) + 10)})
    refused(curdle_crs_from_bytes(wire.data(), len, &out, &fault), "is not 48 (ell + 9)");
  CHECK(g_affine_checks == 0 && g_jac_checks == 0);

  // the validated forms accept what was generated: one affine check of ell + 6 records, one Jacobian check
  view = e.View();
  CHECK(curdle_crs_from_points(&view, 0, &out, &fault) == CURDLE_OK && out && out != reinterpret_cast<curdle_crs*>(0x10));
  CHECK(fault.field == -1 && g_affine_checks == 1 && g_jac_checks == 1 && g_affine_points == ell + 6);
  CHECK(Export(out) == e && Bytes(out) == wire);
  curdle_crs_free(out);
  fault = kSentinel;
  CHECK(curdle_crs_from_bytes(wire.data(), wire.size(), &out, &fault) == CURDLE_OK && out && fault.field == -1);
  CHECK(Export(out) == e && Bytes(out) == wire);
  curdle_crs_free(out);

  auto faulted = [&](int rc, int field, size_t index, int reason, const char* text) {
    CHECK(rc == CURDLE_EINVAL && out == nullptr && LastErrorHas(text));
    CHECK(fault.field == field && fault.index == index && fault.reason == reason);
    out = reinterpret_cast<curdle_crs*>(0x10);
    fault = kSentinel;
  };
  out = reinterpret_cast<curdle_crs*>(0x10);
  fault = kSentinel;
  {  // a point fault, a duplicate and a sum in one CRS: reported in that order as each is repaired
    Exported bad = e;
    memcpy(&bad.Hs[12 * 3], &bad.Gs[12 * 1], 96);         // Hs[3] = Gs[1]: a duplicate, and Hsum no longer the sum
    bad.Gs[12 * 7] ^= 1;                                  // Gs[7] off the curve
    view = bad.View();
    faulted(curdle_crs_from_points(&view, 0, &out, &fault), CURDLE_CRS_GS, 7, CURDLE_DECODE_NOT_ON_CURVE, "Gs[7]: not on the curve");
    bad.Gs[12 * 7] ^= 1;
    faulted(curdle_crs_from_points(&view, 0, &out, &fault), CURDLE_CRS_HS, 3, CURDLE_CRS_DUPLICATE, "Hs[3]: equal to Gs[1]");
    memcpy(&bad.Hs[12 * 3], &e.Gsum[0], 96);              // distinct from every generator, still not what Hsum sums
    faulted(curdle_crs_from_points(&view, 0, &out, &fault), CURDLE_CRS_HSUM, 0, CURDLE_CRS_SUM_MISMATCH, "Hsum: not the sum of Hs");
  }
  {  // the Jacobian fields: infinity is no generator; Gu equal to H under another Z is a duplicate of H
    Exported bad = e;
    memset(&bad.Gt[12], 0, 48);
    view = bad.View();
    faulted(curdle_crs_from_points(&view, 0, &out, &fault), CURDLE_CRS_GT, 0, CURDLE_DECODE_INFINITY, "Gt: the point at infinity");
    bad = e;
    Fp z, z2, z3, x, y;
    memcpy(&x, &e.H[0], 48);
    memcpy(&y, &e.H[6], 48);
    memcpy(&z, &e.Gs[0], 48);  // any field element that is not zero
    fp_sqr(z2, z);
    fp_mul(z3, z2, z);
    fp_mul(x, x, z2);
    fp_mul(y, y, z3);
    memcpy(&bad.Gu[0], &x, 48);
    memcpy(&bad.Gu[6], &y, 48);
    memcpy(&bad.Gu[12], &z, 48);
    view = bad.View();
    faulted(curdle_crs_from_points(&view, 0, &out, &fault), CURDLE_CRS_GU, 0, CURDLE_CRS_DUPLICATE, "Gu: equal to H");
    // TRUSTED takes the same fields and stores Gu with Z = 1
    CHECK(curdle_crs_from_points(&view, CURDLE_CRS_TRUSTED, &out, nullptr) == CURDLE_OK && out);
    CHECK(Export(out).Gu == e.H);
    curdle_crs_free(out);
    out = reinterpret_cast<curdle_crs*>(0x10);
  }
  {  // bytes: a record that is no compressed encoding, Gsum and Hsum swapped, an infinity among the blinders
    std::vector<uint8_t> bad = wire;
    bad[48 * (ell + 1)] &= 0x7f;
    faulted(curdle_crs_from_bytes(bad.data(), bad.size(), &out, &fault), CURDLE_CRS_HS, 1, CURDLE_DECODE_BAD_ENCODING, "Hs[1]: not a valid compressed encoding");
    bad = wire;
    std::swap_ranges(bad.begin() + 48 * (ell + 7), bad.begin() + 48 * (ell + 8), bad.begin() + 48 * (ell + 8));
    faulted(curdle_crs_from_bytes(bad.data(), bad.size(), &out, &fault), CURDLE_CRS_GSUM, 0, CURDLE_CRS_SUM_MISMATCH, "Gsum: not the sum of Gs");
    bad = wire;
    memset(&bad[48 * (ell + 2)], 0, 48);
    bad[48 * (ell + 2)] = 0xc0;
    faulted(curdle_crs_from_bytes(bad.data(), bad.size(), &out, &fault), CURDLE_CRS_HS, 2, CURDLE_DECODE_INFINITY, "Hs[2]: the point at infinity");
    bad = wire;
    memcpy(&bad[48 * (ell - 1)], &bad[0], 48);
    CHECK(curdle_crs_from_bytes(bad.data(), bad.size(), &out, nullptr) == CURDLE_EINVAL && out == nullptr);  // no fault record asked for
    CHECK(LastErrorHas("Gs[11]: equal to Gs[0]"));
  }
  curdle_crs_free(gen);
}

// Import, free, import again; a sum at infinity makes a handle too (its fixed-base table is built from (0, 0)).
static void ImportFreeImport() {
  curdle_rand crs_rand(9);
  curdle_crs* gen = curdle_crs_generate(4, &crs_rand);
  CHECK(gen);
  Exported e = Export(gen);
  const std::vector<uint8_t> wire = Bytes(gen);
  curdle_crs_free(gen);
  for (int rep = 0; rep < 3; rep++) {
    const curdle_crs_points view = e.View();
    curdle_crs *a = nullptr, *b = nullptr;
    CHECK(curdle_crs_from_points(&view, rep ? CURDLE_CRS_TRUSTED : 0, &a, nullptr) == CURDLE_OK && a);
    CHECK(curdle_crs_from_bytes(wire.data(), wire.size(), &b, nullptr) == CURDLE_OK && b && a != b);
    CHECK(Bytes(a) == wire && Bytes(b) == wire);
    curdle_crs_free(a);
    curdle_crs_free(b);
  }
  std::fill(e.Gsum.begin(), e.Gsum.end(), 0);
  const curdle_crs_points view = e.View();
  curdle_crs* c = nullptr;
  CHECK(curdle_crs_from_points(&view, CURDLE_CRS_TRUSTED, &c, nullptr) == CURDLE_OK && c);
  const std::vector<uint8_t> b = Bytes(c);
  CHECK(b[48 * 11] == 0xc0 && Export(c) == e);
  curdle_crs_free(c);
  curdle_crs_free(nullptr);
}

int main() {
  RefusalsAndFaults();
  TrustedEquivalence(4);
  TrustedEquivalence(12);
  ImportFreeImport();
  printf("crs_import_flow OK\n");
  return 0;
}
