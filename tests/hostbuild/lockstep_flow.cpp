// alg::Lockstep over the host backend (stub_backend.cpp): members in lockstep through all five funnels, members that
// throw, members whose shapes disagree, two groups at once.  A stand-alone program for the sanitizer builds of
// tests/test_lockstep_host.py (thread; address + undefined); it ends with "lockstep_flow OK" or a non-zero exit, and a
// hang is what it guards against.  The constant-time routes' coalesced entry points, which the stub backend does not
// have, are defined here over the stub's plain ones: the scope's routing is under test, not the primitives.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
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

static std::atomic<int> g_ct_msm_calls{0}, g_ct_mul_calls{0}, g_gather_calls{0};

extern "C" int curdle_msm_g1_ct_batch(const uint64_t* points, const uint64_t* scalars, const size_t* offsets, size_t k,
                                      unsigned scalar_bits, uint64_t* out_jac) {
  g_ct_msm_calls++;
  return scalar_bits == 255 ? curdle_msm_g1_batch(points, scalars, offsets, k, out_jac) : CURDLE_EINVAL;
}
extern "C" int curdle_g1_scalar_mul_batch_ex(const uint64_t* points, const uint64_t* scalars, size_t n_scalars,
                                             const uint64_t* addends, size_t n, unsigned flags, uint64_t* out_affine) {
  g_ct_mul_calls++;
  if (flags != CURDLE_G1_MUL_CONSTANT_TIME || addends) return CURDLE_EINVAL;
  return curdle_g1_scalar_mul_batch(points, scalars, n_scalars, nullptr, n, out_affine);
}
extern "C" int curdle_fr_permute_ct_batch(const uint64_t* in, const uint32_t* perm, size_t n, size_t k, uint64_t* out) {
  g_gather_calls++;
  for (size_t j = 0; j < k; j++)
    for (size_t i = 0; i < n; i++) {
      const uint32_t p = perm[j * n + i];
      if (p < n)
        memcpy(out + 4 * (j * n + i), in + 4 * (j * n + p), 32);
      else
        memset(out + 4 * (j * n + i), 0, 32);
    }
  return CURDLE_OK;
}

struct curdle_rand {  // same layout as in misc_api.hip / proto_api.cpp
  common::Rand r;
  explicit curdle_rand(uint64_t seed) : r(seed) {}
};

#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                     \
    }                                                              \
  } while (0)

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

struct Outcome {
  Point a;
  std::vector<Point> b, c;
  std::vector<G1Affine> d, f;
  std::vector<Scalar> e;
  int msm_error_at = -1;  // the step whose call threw MsmError
  bool threw = false;     // left by its own exception
  int steps_done = 0;
};

static constexpr int kSteps = 6;
static constexpr size_t kPairsPerMember = 5 + (5 + 3) + (5 + 5);

// The sequence every member runs: one call of each funnel (ScalarMulBatch twice: a shared scalar, per-point scalars).
// throw_at: the member throws before that step; odd_at: it hands in another shape at that step.
static Outcome Sequence(size_t member, bool secret, int throw_at, int odd_at) {
  Outcome o;
  const uint64_t m = 100 * (member + 1);
  const std::vector<G1Affine> p5 = Pts(5, m), p3 = Pts(3, m + 1), p5b = Pts(5, m + 2), p6 = Pts(6, m + 3), p4 = Pts(4, m + 4),
                              adds = Pts(6, m + 5);
  const std::vector<Scalar> s5 = Scs(5, m), s3 = Scs(3, m + 1), s1 = Scs(1, m + 2), s6 = Scs(6, m + 3), s4 = Scs(4, m + 4);
  // under the constant-time switches an entry out of range: the oblivious gather's zero record (the plain gather indexes)
  const std::vector<uint32_t> perm = {5, 3, (uint32_t)(member % 6), 0, 1, alg::SecretOpsScope::Active() ? 77u : 2u};
  int step = 0;
  try {
    for (; step < kSteps; step++) {
      if (step == throw_at) throw std::runtime_error("a member's own failure");
      const bool odd = step == odd_at;
      switch (step) {
        case 0:
          o.a = odd ? alg::MultiExp(p3, s3) : alg::MultiExp(p5, s5);
          break;
        case 1:
          o.b = odd ? alg::MultiExpBatch({&p5}, {&s5}) : alg::MultiExpBatch({&p5, &p3}, {&s5, &s3});
          break;
        case 2:
          o.c = odd ? alg::MultiExpShared({&p5}, s5) : alg::MultiExpShared({&p5, &p5b}, s5);
          break;
        case 3:
          o.d = odd ? alg::ScalarMulBatch(p4, s1) : alg::ScalarMulBatch(p6, s1, secret ? nullptr : &adds);
          break;
        case 4:
          o.e = alg::PermuteSecret(s6, perm);
          break;
        case 5:
          o.f = odd ? alg::ScalarMulBatch(p3, s3) : alg::ScalarMulBatch(p4, s4);
          break;
      }
      o.steps_done++;
    }
  } catch (const alg::MsmError&) {
    o.msm_error_at = step;
  } catch (const std::runtime_error&) {
    o.threw = true;
  }
  return o;
}

static void ExpectSame(const Outcome& got, const Outcome& want) {
  CHECK(got.steps_done == kSteps && got.msm_error_at < 0 && !got.threw);
  CHECK(got.a == want.a);
  CHECK(got.b.size() == want.b.size() && got.c.size() == want.c.size());
  for (size_t i = 0; i < got.b.size(); i++) CHECK(got.b[i] == want.b[i]);
  for (size_t i = 0; i < got.c.size(); i++) CHECK(got.c[i] == want.c[i]);
  CHECK(got.d.size() == want.d.size() && !memcmp(got.d.data(), want.d.data(), got.d.size() * sizeof(G1Affine)));
  CHECK(got.f.size() == want.f.size() && !memcmp(got.f.data(), want.f.data(), got.f.size() * sizeof(G1Affine)));
  CHECK(got.e.size() == want.e.size());
  for (size_t i = 0; i < got.e.size(); i++) CHECK(got.e[i] == want.e[i]);
}

// The members' own calls, outside any scope: what each must get back (with the zero record where the members under the
// constant-time switches have their out-of-range entry).
static Outcome ComputeReference(size_t member, bool secret) {
  Outcome o = Sequence(member, secret, -1, -1);
  CHECK(o.steps_done == kSteps);
  if (secret) {
    const std::vector<Scalar> s6 = Scs(6, 100 * (member + 1) + 3);
    o.e = {s6[5], s6[3], s6[member % 6], s6[0], s6[1], Scalar::Zero()};
  }
  return o;
}

static const Outcome& Reference(size_t member, bool secret) {  // computed once: main is the only caller
  static std::vector<Outcome> cache[2];
  std::vector<Outcome>& c = cache[secret];
  while (c.size() <= member) c.push_back(ComputeReference(c.size(), secret));
  return c[member];
}

static std::vector<Outcome> RunGroup(size_t k, size_t group, bool secret, size_t bad, int throw_at, int odd_at) {
  std::vector<Outcome> out(k);
  alg::RunInLockstep(
      k, group, secret,
      [&](size_t i) { out[i] = Sequence(i, secret, i == bad ? throw_at : -1, i == bad ? odd_at : -1); },
      [&](size_t) { CHECK(!"a member thread could not be started"); });
  return out;
}

// curdle_prove_batch through the C ABI over the stub: three members at ell = 4 against three single calls with the same
// seeds -- bytes, lengths and the rands' next draw -- with ONE bucket-MSM call per step for the three.
static void ProveBatchOverTheStub() {
  const size_t ell = 4, k = 3;
  curdle_rand crs_rand(7);
  curdle_crs* crs = curdle_crs_generate(ell, &crs_rand);
  CHECK(crs);
  std::vector<std::vector<G1Affine>> Rs(k), Ss(k), Ts(k, std::vector<G1Affine>(ell)), Us(k, std::vector<G1Affine>(ell));
  std::vector<std::vector<uint32_t>> perms(k);
  std::vector<uint64_t> Ms(18 * k), ks(4 * k), rs_ms(16 * k);
  for (size_t i = 0; i < k; i++) {
    common::Rand r(100 + i);
    r.GetG1Affines(ell, Rs[i]);
    r.GetG1Affines(ell, Ss[i]);
    r.GeneratePermutation(ell, perms[i]);
    Fr kk;
    r.GetFr(kk);
    memcpy(&ks[4 * i], &kk, 32);
    curdle_rand cr(200 + i);
    CHECK(curdle_shuffle_permute_commit(crs, (const uint64_t*)Rs[i].data(), (const uint64_t*)Ss[i].data(), ell, perms[i].data(),
                                        &ks[4 * i], &cr, (uint64_t*)Ts[i].data(), (uint64_t*)Us[i].data(), &Ms[18 * i],
                                        &rs_ms[16 * i]) == CURDLE_OK);
  }
  const size_t stride = 1 << 14;
  std::vector<std::vector<uint8_t>> single(k, std::vector<uint8_t>(stride));
  std::vector<size_t> single_len(k);
  std::vector<Fr> single_next(k);
  unsigned long long c0[4], c1[4], c2[4];
  alg::ReadMsmCounters(c0);
  for (size_t i = 0; i < k; i++) {
    curdle_rand cr(300 + i);
    CHECK(curdle_prove(crs, (const uint64_t*)Rs[i].data(), (const uint64_t*)Ss[i].data(), (const uint64_t*)Ts[i].data(),
                       (const uint64_t*)Us[i].data(), ell, &Ms[18 * i], perms[i].data(), &ks[4 * i], &rs_ms[16 * i], &cr,
                       single[i].data(), stride, &single_len[i]) == CURDLE_OK);
    cr.r.GetFr(single_next[i]);
  }
  alg::ReadMsmCounters(c1);
  std::vector<const uint64_t*> pR(k), pS(k), pT(k), pU(k);
  std::vector<const uint32_t*> pP(k);
  std::vector<curdle_rand*> rands(k);
  for (size_t i = 0; i < k; i++) {
    pR[i] = (const uint64_t*)Rs[i].data();
    pS[i] = (const uint64_t*)Ss[i].data();
    pT[i] = (const uint64_t*)Ts[i].data();
    pU[i] = (const uint64_t*)Us[i].data();
    pP[i] = perms[i].data();
    rands[i] = new curdle_rand(300 + i);
  }
  std::vector<uint8_t> out(stride * k);
  std::vector<size_t> lens(k);
  std::vector<int> status(k, -1);
  CHECK(curdle_prove_batch(crs, k, ell, pR.data(), pS.data(), pT.data(), pU.data(), Ms.data(), pP.data(), ks.data(), rs_ms.data(),
                           rands.data(), 0, out.data(), stride, lens.data(), status.data()) == CURDLE_OK);
  alg::ReadMsmCounters(c2);
  for (size_t i = 0; i < k; i++) {
    CHECK(status[i] == CURDLE_OK && lens[i] == single_len[i] && lens[i] > 0);
    CHECK(!memcmp(out.data() + stride * i, single[i].data(), lens[i]));
    Fr next;
    rands[i]->r.GetFr(next);
    CHECK(!memcmp(&next, &single_next[i], 32));
    delete rands[i];
  }
  CHECK((c2[0] - c1[0]) * k == c1[0] - c0[0]);  // the calls of ONE single Prove ...
  CHECK(c2[1] - c1[1] == c1[1] - c0[1]);        // ... with the pairs of all three
  // refusals before any thread starts: an undefined flag bit (with a null argument), then a null argument (with a wrong
  // ell; two members sharing a rand counts as one), then ell.  No rand is read and no status is written.
  auto refused = [&](const curdle_crs* c, size_t e, const uint64_t* const* rs, unsigned flags, const char* text) {
    std::fill(status.begin(), status.end(), -1);
    CHECK(curdle_prove_batch(c, k, e, rs, pS.data(), pT.data(), pU.data(), Ms.data(), pP.data(), ks.data(), rs_ms.data(),
                             rands.data(), flags, out.data(), stride, lens.data(), status.data()) == CURDLE_EINVAL);
    char buf[256];
    curdle_last_error(buf, sizeof(buf));
    CHECK(strstr(buf, text));
    for (int s : status) CHECK(s == -1);
  };
  refused(nullptr, ell, pR.data(), 2, "unknown flag bits");
  refused(crs, ell + 1, nullptr, 0, "null argument");
  for (size_t i = 0; i < k; i++) rands[i] = &crs_rand;  // non-null and shared: refused as an argument, still before ell
  refused(crs, ell + 1, pR.data(), 0, "share one rand");
  curdle_rand fresh[3] = {curdle_rand(1), curdle_rand(2), curdle_rand(3)};
  for (size_t i = 0; i < k; i++) rands[i] = &fresh[i];
  refused(crs, ell + 1, pR.data(), 0, "does not match the CRS");
  curdle_crs_free(crs);
}

int main() {
  const size_t none = (size_t)-1;
  ProveBatchOverTheStub();
  // 1, 2 and 7 members through all five funnels, on the default route and under the constant-time switches
  for (int secret = 0; secret < 2; secret++)
    for (size_t k : {(size_t)1, (size_t)2, (size_t)7}) {
      unsigned long long c0[4], c1[4];
      alg::ReadMsmCounters(c0);
      const int ct_msm0 = g_ct_msm_calls, ct_mul0 = g_ct_mul_calls, gather0 = g_gather_calls;
      const std::vector<Outcome> got = RunGroup(k, 64, secret, none, -1, -1);
      alg::ReadMsmCounters(c1);
      // a coalesced call counts once, with all its pairs
      CHECK(c1[secret ? 2 : 0] - c0[secret ? 2 : 0] == 3);
      CHECK(c1[secret ? 3 : 1] - c0[secret ? 3 : 1] == k * kPairsPerMember);
      CHECK(c1[secret ? 0 : 2] == c0[secret ? 0 : 2]);
      CHECK(g_ct_msm_calls - ct_msm0 == (secret ? 3 : 0));
      CHECK(g_ct_mul_calls - ct_mul0 == (secret ? 2 : 0));
      CHECK(g_gather_calls - gather0 == (secret ? 1 : 0));
      for (size_t i = 0; i < k; i++) {
        ExpectSame(got[i], Reference(i, secret));
      }
    }
  // a split by whole members changes nothing: 7 members, at most 2 x 23 pairs a call
  {
    CHECK(knobs::set("PROVE_BATCH_PAIRS", 50) == 0);
    unsigned long long c0[4], c1[4];
    alg::ReadMsmCounters(c0);
    const std::vector<Outcome> got = RunGroup(7, 64, false, none, -1, -1);
    alg::ReadMsmCounters(c1);
    CHECK(c1[0] - c0[0] > 3 && c1[1] - c0[1] == 7 * kPairsPerMember);
    for (size_t i = 0; i < 7; i++) ExpectSame(got[i], Reference(i, false));
    CHECK(knobs::set("PROVE_BATCH_PAIRS", -1) == 0);
  }
  // groups of 3: 7 members are three groups
  {
    const std::vector<Outcome> got = RunGroup(7, 3, false, none, -1, -1);
    for (size_t i = 0; i < 7; i++) ExpectSame(got[i], Reference(i, false));
  }
  // a member that throws at step 0, at a middle step and at the last step: the others finish with their own results
  for (int secret = 0; secret < 2; secret++)
    for (int at : {0, 3, kSteps - 1}) {
      const size_t bad = at == 3 ? 0 : 2;
      {
        const std::vector<Outcome> got = RunGroup(3, 64, secret, bad, at, -1);
        for (size_t i = 0; i < 3; i++) {
          if (i == bad) {
            CHECK(got[i].threw && got[i].steps_done == at);
            continue;
          }
          ExpectSame(got[i], Reference(i, secret));
        }
      }
    }
  // a member whose shapes disagree: everyone at that step gets the error, and the program ends
  for (int at : {0, 2, 3, 5})
    for (size_t k : {(size_t)2, (size_t)4}) {
      const std::vector<Outcome> got = RunGroup(k, 64, false, k - 1, -1, at);
      for (size_t i = 0; i < k; i++) CHECK(got[i].msm_error_at == at && got[i].steps_done == at && !got[i].threw);
    }
  // two groups at once, each from a thread of its own
  {
    std::vector<Outcome> g1, g2;
    std::thread t1([&] { g1 = RunGroup(4, 64, false, none, -1, -1); });
    std::thread t2([&] { g2 = RunGroup(3, 64, true, none, -1, -1); });
    t1.join();
    t2.join();
    for (size_t i = 0; i < 4; i++) ExpectSame(g1[i], Reference(i, false));
    for (size_t i = 0; i < 3; i++) ExpectSame(g2[i], Reference(i, true));
  }
  // a member that never starts leaves its group by Leave(); the others go on
  {
    alg::Lockstep group(3);
    std::vector<Outcome> out(3);
    group.Leave(1);
    std::vector<std::thread> ts;
    for (size_t i : {(size_t)0, (size_t)2})
      ts.emplace_back([&, i] {
        alg::LockstepScope scope(group, i);
        out[i] = Sequence(i, false, -1, -1);
      });
    for (std::thread& t : ts) t.join();
    ExpectSame(out[0], Reference(0, false));
    ExpectSame(out[2], Reference(2, false));
    CHECK(group.DeviceCalls() == 5);
  }
  printf("lockstep_flow OK\n");
  return 0;
}
