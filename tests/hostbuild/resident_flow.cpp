// alg::ResidentBases and the route under an alg::ResidentBasesScope, and curdle_prover_ct over them, on the host
// backend (stub_backend.cpp).  A stand-alone program for the sanitizer build of tests/test_resident_flow_host.py
// (address + undefined); it ends with "resident_flow OK" or a non-zero exit.  The device's entry points the routes need
// and the stub backend does not have are defined here over the stub's plain ones: curdle_ct_bases_create / _free and
// curdle_msm_g1_ct_bases_sets_batch gather the points by row into curdle_msm_g1_ct_batch.  The routing, the registry and
// the prover's use of them are under test, not the primitives.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <stdexcept>
#include <thread>
#include <vector>

#include "../../go-curdleproofs_amd/host/algebra.h"
#include "../../go-curdleproofs_amd/host/curdleproofs.h"
#include "../../go-curdleproofs_amd/host/knobs.h"
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

static int g_ct_single, g_ct_batch, g_ct_multi, g_sets_calls, g_tables_made, g_tables_freed;
static size_t g_sets_pairs, g_last_n_sets;

extern "C" int curdle_device_available(void) { return 1; }
extern "C" int curdle_msm_g1_ct(const uint64_t* points, const uint64_t* scalars, size_t n, unsigned scalar_bits, uint64_t out_jac[18]) {
  g_ct_single++;
  return scalar_bits == 255 ? curdle_msm_g1(points, scalars, n, out_jac) : CURDLE_EINVAL;
}
extern "C" int curdle_msm_g1_ct_batch(const uint64_t* points, const uint64_t* scalars, const size_t* offsets, size_t k,
                                      unsigned scalar_bits, uint64_t* out_jac) {
  g_ct_batch++;
  return scalar_bits == 255 ? curdle_msm_g1_batch(points, scalars, offsets, k, out_jac) : CURDLE_EINVAL;
}
extern "C" int curdle_msm_g1_ct_multi(const uint64_t* const* points_sets, size_t k, const uint64_t* scalars, size_t n,
                                      unsigned scalar_bits, uint64_t* out_jac) {
  g_ct_multi++;
  return scalar_bits == 255 ? curdle_msm_g1_multi(points_sets, k, scalars, n, out_jac) : CURDLE_EINVAL;
}
extern "C" int curdle_fr_permute_ct(const uint64_t* in, const uint32_t* perm, size_t n, uint64_t* out) {
  for (size_t i = 0; i < n; i++) {
    if (perm[i] < n)
      memcpy(out + 4 * i, in + 4 * perm[i], 32);
    else
      memset(out + 4 * i, 0, 32);
  }
  return CURDLE_OK;
}
extern "C" int curdle_g1_scalar_mul_batch_ex(const uint64_t* points, const uint64_t* scalars, size_t n_scalars,
                                             const uint64_t* addends, size_t n, unsigned flags, uint64_t* out_affine) {
  if (flags != CURDLE_G1_MUL_CONSTANT_TIME || addends) return CURDLE_EINVAL;
  return curdle_g1_scalar_mul_batch(points, scalars, n_scalars, nullptr, n, out_affine);
}

// ---- the stand-ins for the tables and the call over several of them ----
struct curdle_ct_bases {
  std::vector<G1Affine> pts;
  unsigned c;
};
extern "C" int curdle_ct_bases_create(const uint64_t* points, size_t n, unsigned chunk_bits, curdle_ct_bases** out) {
  if (chunk_bits != 8 && chunk_bits != 16 && chunk_bits != 32 && chunk_bits != 64) return CURDLE_EINVAL;  // 0 never arrives
  curdle_ct_bases* b = new curdle_ct_bases();
  b->pts.resize(n);
  if (n) memcpy(b->pts.data(), points, n * 96);
  b->c = chunk_bits;
  g_tables_made++;
  *out = b;
  return CURDLE_OK;
}
extern "C" void curdle_ct_bases_free(curdle_ct_bases* b) {
  if (b) g_tables_freed++;
  delete b;
}
extern "C" int curdle_msm_g1_ct_bases_sets_batch(const curdle_ct_bases* const* sets, size_t n_sets, const uint32_t* rows,
                                                 const uint64_t* scalars, const size_t* offsets, size_t k, unsigned scalar_bits,
                                                 uint64_t* out_jac) {
  if (!sets || n_sets < 1 || n_sets > CURDLE_CT_BASES_MAX_SETS) return CURDLE_EINVAL;
  std::vector<G1Affine> all;
  for (size_t s = 0; s < n_sets; s++) {
    if (!sets[s] || sets[s]->c != sets[0]->c) return CURDLE_EINVAL;
    all.insert(all.end(), sets[s]->pts.begin(), sets[s]->pts.end());
  }
  const size_t n = offsets[k];
  if ((size_t)((255 + sets[0]->c - 1) / sets[0]->c) * n > 65536) return CURDLE_EINVAL;
  std::vector<G1Affine> P(n);
  for (size_t p = offsets[0]; p < n; p++) {
    if (rows[p] >= all.size()) return CURDLE_EINVAL;
    P[p] = all[rows[p]];
  }
  g_sets_calls++;
  g_sets_pairs += n - offsets[0];
  g_last_n_sets = n_sets;
  const int before = g_ct_batch;
  const int rc = curdle_msm_g1_ct_batch(reinterpret_cast<const uint64_t*>(P.data()), scalars, offsets, k, scalar_bits, out_jac);
  g_ct_batch = before;  // the stand-in's own use of it is not the funnel's
  return rc;
}

struct curdle_rand {  // same layout as in misc_api.hip / proto_api.cpp
  common::Rand r;
  explicit curdle_rand(uint64_t seed) : r(seed) {}
};

static std::vector<G1Affine> Pts(size_t n, uint64_t seed) {
  std::vector<G1Affine> v(n);
  Point p = Point::Generator().Mul(Scalar::FromU64(seed + 3));
  for (size_t i = 0; i < n; i++) {
    v[i] = p.Affine();
    p = p + Point::Generator();
  }
  return v;
}
static std::vector<Scalar> Scs(size_t n, uint64_t seed) {
  std::vector<Scalar> v(n);
  Scalar s = Scalar::FromU64(0x9e3779b97f4a7c15ull ^ seed);
  for (size_t i = 0; i < n; i++) {
    s = s * s + Scalar::FromU64(seed + i);
    v[i] = s;
  }
  return v;
}
static G1Affine Zero() {
  G1Affine z;
  memset(&z, 0, sizeof(z));
  return z;
}

struct Counters {
  unsigned long long alg[4], res[4];
  int single, batch, multi, sets;
  size_t sets_pairs;
};
static Counters Now() {
  Counters c;
  alg::ReadMsmCounters(c.alg);
  alg::ReadResidentCounters(c.res);
  c.single = g_ct_single;
  c.batch = g_ct_batch;
  c.multi = g_ct_multi;
  c.sets = g_sets_calls;
  c.sets_pairs = g_sets_pairs;
  return c;
}

// The registry: duplicates keep their first row, the zero record is a record like any other, a fifth Add is refused.
static void Registry() {
  const std::vector<G1Affine> a = Pts(3, 1), b = Pts(2, 50);
  const int made0 = g_tables_made, freed0 = g_tables_freed;
  {
    alg::ResidentBases reg(0);
    CHECK(reg.ChunkBits() == 16 && reg.Chunks() == 16 && reg.Sets() == 0 && reg.Rows() == 0);
    uint32_t row = 99;
    CHECK(!reg.Find(a[0], &row) && row == 99);
    reg.Add({a[0], a[1], a[0], Zero(), a[2]});  // rows 0 ... 4; a[0] again at 2
    reg.Add({});                                // an empty set covers nothing
    reg.Add({b[0], a[1], Zero(), b[1]});        // rows 5 ... 8; a[1] and the zero record are resident already
    CHECK(reg.Sets() == 3 && reg.Rows() == 9);
    CHECK(reg.Find(a[0], &row) && row == 0);
    CHECK(reg.Find(a[1], &row) && row == 1);
    CHECK(reg.Find(Zero(), &row) && row == 3);
    CHECK(reg.Find(a[2], &row) && row == 4);
    CHECK(reg.Find(b[0], &row) && row == 5);
    CHECK(reg.Find(b[1], &row) && row == 8);
    CHECK(!reg.Find(Pts(1, 777)[0], &row));
    reg.Add({b[1]});
    CHECK(reg.Sets() == 4);
    bool refused = false;
    try {
      reg.Add({b[0]});
    } catch (const alg::MsmError& e) {
      refused = e.rc == CURDLE_EINVAL;
    }
    CHECK(refused && reg.Sets() == 4 && reg.Rows() == 10);
    CHECK(g_tables_made - made0 == 4);
  }
  CHECK(g_tables_freed - freed0 == 4);  // the registry frees what it made
  for (unsigned c : {8u, 32u, 64u}) {
    alg::ResidentBases reg(c);
    CHECK(reg.ChunkBits() == c && reg.Chunks() == (255 + c - 1) / c);
  }
  bool refused = false;
  try {
    alg::ResidentBases reg(12);
  } catch (const alg::MsmError& e) {
    refused = e.rc == CURDLE_EINVAL;
  }
  CHECK(refused);
  CHECK(alg::ResidentBasesScope::Available());
}

// The three funnels on both routes, a call with an unregistered base, the term cap under the knob, a lockstep member.
static void Funnels() {
  const std::vector<G1Affine> p5 = Pts(5, 100), p3 = Pts(3, 200), p5b = Pts(5, 300), other = Pts(5, 900);
  const std::vector<Scalar> s5 = Scs(5, 1), s3 = Scs(3, 2);
  // what every route must give: the bucket MSM's results, outside any scope
  const Point want_a = alg::MultiExp(p5, s5);
  const std::vector<Point> want_b = alg::MultiExpBatch({&p5, &p3}, {&s5, &s3});
  const std::vector<Point> want_c = alg::MultiExpShared({&p5, &p5b}, s5);
  auto same = [&](const Point& a, const std::vector<Point>& b, const std::vector<Point>& c) {
    CHECK(a == want_a && b.size() == 2 && c.size() == 2);
    CHECK(b[0] == want_b[0] && b[1] == want_b[1] && c[0] == want_c[0] && c[1] == want_c[1]);
  };
  alg::ResidentBases reg(16);
  reg.Add(p5);
  std::vector<G1Affine> second = p3;
  second.insert(second.end(), p5b.begin(), p5b.end());
  reg.Add(second);
  auto three = [&] { same(alg::MultiExp(p5, s5), alg::MultiExpBatch({&p5, &p3}, {&s5, &s3}), alg::MultiExpShared({&p5, &p5b}, s5)); };

  // a ResidentBasesScope alone changes nothing: the bucket MSM, and nothing counted
  {
    alg::ResidentBasesScope scope(reg);
    const Counters c0 = Now();
    three();
    const Counters c1 = Now();
    CHECK(c1.alg[0] - c0.alg[0] == 3 && c1.alg[2] == c0.alg[2] && c1.sets == c0.sets);
    for (int i = 0; i < 4; i++) CHECK(c1.res[i] == c0.res[i]);
  }
  // the constant-time switch alone: the unchunked calls, nothing counted as resident or fallback
  {
    alg::ConstantTimeMsmScope ct;
    const Counters c0 = Now();
    three();
    const Counters c1 = Now();
    CHECK(c1.single - c0.single == 1 && c1.batch - c0.batch == 1 && c1.multi - c0.multi == 1 && c1.sets == c0.sets);
    CHECK(c1.alg[2] - c0.alg[2] == 3 && c1.alg[3] - c0.alg[3] == 5 + 8 + 10);
    for (int i = 0; i < 4; i++) CHECK(c1.res[i] == c0.res[i]);
  }
  // both: three resident calls of 5, 5 + 3 and 2 x 5 pairs over the registry's two sets
  {
    alg::ConstantTimeMsmScope ct;
    alg::ResidentBasesScope scope(reg);
    CHECK(alg::ResidentBasesScope::Active() == &reg);
    const Counters c0 = Now();
    three();
    const Counters c1 = Now();
    CHECK(c1.sets - c0.sets == 3 && c1.sets_pairs - c0.sets_pairs == 23 && g_last_n_sets == 2);
    CHECK(c1.single == c0.single && c1.batch == c0.batch && c1.multi == c0.multi);
    CHECK(c1.alg[2] - c0.alg[2] == 3 && c1.alg[3] - c0.alg[3] == 23 && c1.alg[0] == c0.alg[0]);  // the constant-time half counts both routes
    CHECK(c1.res[0] - c0.res[0] == 3 && c1.res[1] - c0.res[1] == 23 && c1.res[2] == c0.res[2] && c1.res[3] == c0.res[3]);
    // one unregistered base among registered ones: the old path, counted as such, the same result
    std::vector<G1Affine> mixed = p5;
    mixed[3] = other[0];
    const Point old_path = alg::MultiExp(mixed, s5);
    const Counters c2 = Now();
    CHECK(c2.sets == c1.sets && c2.single - c1.single == 1);
    CHECK(c2.res[0] == c1.res[0] && c2.res[2] - c1.res[2] == 1 && c2.res[3] - c1.res[3] == 5);
    std::vector<Point> batch_old = alg::MultiExpBatch({&p5, &other}, {&s5, &s5});
    std::vector<Point> shared_old = alg::MultiExpShared({&other, &p5b}, s5);
    const Counters c3 = Now();
    CHECK(c3.sets == c2.sets && c3.batch - c2.batch == 1 && c3.multi - c2.multi == 1);
    CHECK(c3.res[2] - c2.res[2] == 2 && c3.res[3] - c2.res[3] == 20);
    CHECK(batch_old[0] == want_a && shared_old[1] == want_c[1]);
    {
      alg::ConstantTimeMsmScope inner;  // (nesting keeps the switch on)
      CHECK(old_path == alg::MultiExp(mixed, s5));
    }
  }
  // the term cap under the knob: 16 chunks a pair, so 100 terms hold 6 pairs -- the call of 5 pairs is resident, those
  // of 8 and 10 are not; 0 and a value above 65,536 mean "not set"
  {
    alg::ConstantTimeMsmScope ct;
    alg::ResidentBasesScope scope(reg);
    CHECK(knobs::set("PROVE_RESIDENT_TERMS", 100) == 0);
    Counters c0 = Now();
    three();
    Counters c1 = Now();
    CHECK(c1.res[0] - c0.res[0] == 1 && c1.res[1] - c0.res[1] == 5 && c1.res[2] - c0.res[2] == 2 && c1.res[3] - c0.res[3] == 18);
    CHECK(c1.sets - c0.sets == 1 && c1.batch - c0.batch == 1 && c1.multi - c0.multi == 1);
    for (long long v : {0ll, 65537ll, 1ll << 40, -1ll}) {
      CHECK(knobs::set("CURDLE_PROVE_RESIDENT_TERMS", v) == 0);
      c0 = Now();
      three();
      c1 = Now();
      CHECK(c1.res[0] - c0.res[0] == 3 && c1.res[2] == c0.res[2]);
    }
    CHECK(knobs::set("PROVE_RESIDENT_TERMS", 79) == 0);  // 4 pairs: nothing fits
    c0 = Now();
    three();
    c1 = Now();
    CHECK(c1.res[0] == c0.res[0] && c1.res[2] - c0.res[2] == 3);
    CHECK(knobs::set("PROVE_RESIDENT_TERMS", -1) == 0);
  }
  // a registry that declines: not Active(), every call on the old path and counted as such
  {
    alg::ResidentBases declining(16);
    declining.Decline();
    alg::ConstantTimeMsmScope ct;
    alg::ResidentBasesScope scope(declining);
    CHECK(alg::ResidentBasesScope::Active() == nullptr);
    const Counters c0 = Now();
    three();
    const Counters c1 = Now();
    CHECK(c1.sets == c0.sets && c1.res[0] == c0.res[0] && c1.res[2] - c0.res[2] == 3 && c1.res[3] - c0.res[3] == 23);
  }
  // under a LockstepScope nothing is consulted: the member's requests go to the group's coalesced constant-time batch
  {
    const Counters c0 = Now();
    alg::Lockstep group(1);
    std::thread t([&] {
      alg::LockstepScope member(group, 0);
      alg::ConstantTimeMsmScope ct;
      alg::ResidentBasesScope scope(reg);
      three();
    });
    t.join();
    const Counters c1 = Now();
    CHECK(c1.sets == c0.sets && c1.batch - c0.batch == 3 && group.DeviceCalls() == 3);
    for (int i = 0; i < 4; i++) CHECK(c1.res[i] == c0.res[i]);
    CHECK(c1.alg[2] - c0.alg[2] == 3);
  }
  CHECK(alg::ResidentBasesScope::Active() == nullptr);
}

// curdle_prover_ct_prove against curdle_prove_ct and curdle_prove: bytes, length, rand's next draw; the counters by hand.
static void Prover(size_t ell, unsigned chunk_bits) {
  curdle_rand crs_rand(7 + ell);
  curdle_crs* crs = curdle_crs_generate(ell, &crs_rand);
  CHECK(crs);
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
    CHECK(curdle_shuffle_permute_commit(crs, (const uint64_t*)Rs.data(), (const uint64_t*)Ss.data(), ell, perm.data(), k, &cr,
                                        (uint64_t*)Ts.data(), (uint64_t*)Us.data(), M, rs_m) == CURDLE_OK);
  }
  const uint64_t *R = (const uint64_t*)Rs.data(), *S = (const uint64_t*)Ss.data(), *T = (const uint64_t*)Ts.data(),
                 *U = (const uint64_t*)Us.data();
  const size_t cap = 1 << 14;
  std::vector<uint8_t> plain(cap), ct(cap), res(cap, 0x5a);
  size_t plain_len = 0, ct_len = 0, res_len = 77;
  Fr next_plain, next_ct, next_res;
  {
    curdle_rand cr(300);
    CHECK(curdle_prove(crs, R, S, T, U, ell, M, perm.data(), k, rs_m, &cr, plain.data(), cap, &plain_len) == CURDLE_OK);
    cr.r.GetFr(next_plain);
  }
  const Counters c0 = Now();
  {
    curdle_rand cr(300);
    CHECK(curdle_prove_ct(crs, R, S, T, U, ell, M, perm.data(), k, rs_m, &cr, ct.data(), cap, &ct_len) == CURDLE_OK);
    cr.r.GetFr(next_ct);
  }
  const Counters c1 = Now();
  // the funnel calls of one constant-time Prove, by hand: A, B's betas, C, D, the self-check, B_c | B_d, R | S, the two
  // commitment pairs and B_a | B_t | B_u are ten; each of the two recursions adds one per round
  size_t rounds = 0;
  while (((size_t)1 << rounds) < ell + 4) rounds++;
  const unsigned long long calls = 10 + 2 * rounds;
  CHECK(c1.alg[2] - c0.alg[2] == calls && c1.sets == c0.sets);
  for (int i = 0; i < 4; i++) CHECK(c1.res[i] == c0.res[i]);

  curdle_prover_ct* prover = nullptr;
  const int made0 = g_tables_made;
  CHECK(curdle_prover_ct_create(crs, chunk_bits, &prover) == CURDLE_OK && prover);
  CHECK(g_tables_made - made0 == 1);  // the CRS table, once
  // refusals, curdle_prove_ct's, in its order; outputs untouched, rand not advanced
  {
    curdle_rand cr(300), untouched(300);
    char buf[256];
    auto text = [&](const char* t) {
      curdle_last_error(buf, sizeof(buf));
      return strstr(buf, t) != nullptr;
    };
    CHECK(curdle_prover_ct_prove(nullptr, R, S, T, U, ell + 1, M, perm.data(), k, rs_m, &cr, res.data(), cap, &res_len) == CURDLE_EINVAL && text("null argument"));
    CHECK(curdle_prover_ct_prove(prover, R, nullptr, T, U, ell + 1, M, perm.data(), k, rs_m, &cr, res.data(), cap, &res_len) == CURDLE_EINVAL && text("null argument"));
    CHECK(curdle_prover_ct_prove(prover, R, S, T, U, ell + 1, M, perm.data(), k, rs_m, &cr, res.data(), cap, &res_len) == CURDLE_EINVAL && text("does not match the CRS"));
    CHECK(knobs::set("PROVER_FOLD_BASES", 1) == 0);
    CHECK(curdle_prover_ct_prove(prover, R, S, T, U, ell, M, perm.data(), k, rs_m, &cr, res.data(), cap, &res_len) == CURDLE_EINVAL && text("PROVER_FOLD_BASES"));
    CHECK(knobs::set("PROVER_FOLD_BASES", -1) == 0);
    CHECK(res_len == 77);
    for (uint8_t b : res) CHECK(b == 0x5a);
    Fr a, b;
    cr.r.GetFr(a);
    untouched.r.GetFr(b);
    CHECK(!memcmp(&a, &b, 32));
    CHECK(g_tables_made - made0 == 1);
  }
  for (int rep = 0; rep < 2; rep++) {
    const int made1 = g_tables_made, freed1 = g_tables_freed;
    const Counters c2 = Now();
    curdle_rand cr(300);
    CHECK(curdle_prover_ct_prove(prover, R, S, T, U, ell, M, perm.data(), k, rs_m, &cr, res.data(), cap, &res_len) == CURDLE_OK);
    cr.r.GetFr(next_res);
    const Counters c3 = Now();
    CHECK(res_len == ct_len && ct_len == plain_len && plain_len > 0);
    CHECK(!memcmp(res.data(), ct.data(), ct_len) && !memcmp(res.data(), plain.data(), plain_len));
    CHECK(!memcmp(&next_res, &next_ct, 32) && !memcmp(&next_res, &next_plain, 32));
    // every funnel call resident, none on the old path; the instance set and the late set made and freed by the call
    CHECK(c3.alg[2] - c2.alg[2] == calls && c3.alg[3] - c2.alg[3] == c1.alg[3] - c0.alg[3]);
    CHECK(c3.res[0] - c2.res[0] == calls && c3.res[1] - c2.res[1] == c1.alg[3] - c0.alg[3]);
    CHECK(c3.res[2] == c2.res[2] && c3.res[3] == c2.res[3]);
    CHECK(c3.sets - c2.sets == (int)calls && c3.single == c2.single && c3.batch == c2.batch && c3.multi == c2.multi);
    CHECK(g_tables_made - made1 == 2 && g_tables_freed - freed1 == 2);
  }
  // under the knob some calls fall back and the bytes stay
  {
    CHECK(knobs::set("PROVE_RESIDENT_TERMS", (long long)((255 + (chunk_bits ? chunk_bits : 16) - 1) / (chunk_bits ? chunk_bits : 16)) * 6) == 0);
    const Counters c2 = Now();
    curdle_rand cr(300);
    std::fill(res.begin(), res.end(), 0);
    CHECK(curdle_prover_ct_prove(prover, R, S, T, U, ell, M, perm.data(), k, rs_m, &cr, res.data(), cap, &res_len) == CURDLE_OK);
    const Counters c3 = Now();
    CHECK(res_len == ct_len && !memcmp(res.data(), ct.data(), ct_len));
    CHECK(c3.res[0] - c2.res[0] > 0 && c3.res[2] - c2.res[2] > 0 && (c3.res[0] - c2.res[0]) + (c3.res[2] - c2.res[2]) == calls);
    CHECK(knobs::set("PROVE_RESIDENT_TERMS", -1) == 0);
  }
  const int freed2 = g_tables_freed;
  curdle_prover_ct_free(prover);
  curdle_prover_ct_free(nullptr);
  CHECK(g_tables_freed - freed2 == 1);
  curdle_crs_free(crs);
}

static void ProverCreateRefusals() {
  curdle_rand crs_rand(5);
  curdle_crs* crs = curdle_crs_generate(4, &crs_rand);
  CHECK(crs);
  curdle_prover_ct* p = reinterpret_cast<curdle_prover_ct*>(0x10);
  char buf[256];
  CHECK(curdle_prover_ct_create(nullptr, 7, &p) == CURDLE_EINVAL && p == nullptr);
  CHECK(curdle_prover_ct_create(crs, 7, nullptr) == CURDLE_EINVAL);
  for (unsigned c : {1u, 7u, 12u, 65u}) {
    p = reinterpret_cast<curdle_prover_ct*>(0x10);
    CHECK(curdle_prover_ct_create(crs, c, &p) == CURDLE_EINVAL && p == nullptr);
    curdle_last_error(buf, sizeof(buf));
    CHECK(strstr(buf, "chunk_bits"));
  }
  curdle_crs_free(crs);
}

int main() {
  Registry();
  Funnels();
  ProverCreateRefusals();
  Prover(4, 0);
  Prover(12, 0);
  Prover(4, 64);
  CHECK(g_tables_made == g_tables_freed);
  printf("resident_flow OK\n");
  return 0;
}
