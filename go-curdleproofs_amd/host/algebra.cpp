// Fr / G1 value types, wire encodings and the MSM funnel -- see algebra.h.
#include "algebra.h"

#include <stdlib.h>

#include "host_ops.h"
#include "knobs.h"

#include <string.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <stdexcept>
#include <system_error>
#include <thread>
#include <unordered_map>

#include "../../include/curdle_msm.h"

// The constant-time MSM lives in the GPU backend (csrc/msm_ct_api.hip).  Weak here: a backend without it -- the host
// layer linked over a plain CPU backend, as the sanitizer builds are -- still links, and an MSM under a
// ConstantTimeMsmScope fails with CURDLE_ENODEV instead of running anywhere else.
extern "C" int curdle_msm_g1_ct(const uint64_t* points, const uint64_t* scalars, size_t n, unsigned scalar_bits,
                                uint64_t out_jac[18]) __attribute__((weak));
extern "C" int curdle_msm_g1_ct_batch(const uint64_t* points, const uint64_t* scalars, const size_t* offsets, size_t k,
                                      unsigned scalar_bits, uint64_t* out_jac) __attribute__((weak));
extern "C" int curdle_msm_g1_ct_multi(const uint64_t* const* points_sets, size_t k, const uint64_t* scalars, size_t n,
                                      unsigned scalar_bits, uint64_t* out_jac) __attribute__((weak));
// ... and so does the oblivious gather over scalars, which PermuteSecret uses under a SecretOpsScope.
extern "C" int curdle_fr_permute_ct(const uint64_t* in, const uint32_t* perm, size_t n, uint64_t* out) __attribute__((weak));

// What a lockstep group's coalesced requests go to besides the calls above (alg::Lockstep): the batched gather, and the
// constant-time multiplication for a scalar multiplication batch whose scalars are secrets.
extern "C" int curdle_fr_permute_ct_batch(const uint64_t* in, const uint32_t* perm, size_t n, size_t k, uint64_t* out)
    __attribute__((weak));
extern "C" int curdle_g1_scalar_mul_batch_ex(const uint64_t* points, const uint64_t* scalars, size_t n_scalars,
                                             const uint64_t* addends, size_t n, unsigned flags, uint64_t* out_affine)
    __attribute__((weak));

// The constant-time base tables and the MSM over several of them (csrc/msm_ct_bases_api.hip), weak like the names above:
// alg::ResidentBases and the route under an alg::ResidentBasesScope need them, and ResidentBasesScope::Available() says
// whether they are linked.
extern "C" int curdle_ct_bases_create(const uint64_t* points, size_t n, unsigned chunk_bits, curdle_ct_bases** out)
    __attribute__((weak));
extern "C" void curdle_ct_bases_free(curdle_ct_bases* b) __attribute__((weak));
extern "C" int curdle_msm_g1_ct_bases_sets_batch(const curdle_ct_bases* const* sets, size_t n_sets, const uint32_t* rows,
                                                 const uint64_t* scalars, const size_t* offsets, size_t k,
                                                 unsigned scalar_bits, uint64_t* out_jac) __attribute__((weak));

namespace curdle {
namespace alg {

// single-point group operations go through the ISA-dispatched builds (host_ops.cpp)
static void ScalarMulImpl(G1XYZZ& r, const G1XYZZ& p, const u32* k) { curdle_host_scalar_mul(&r, &p, k); }
static void AddImpl(G1XYZZ& acc, const G1XYZZ& b) { curdle_host_add(&acc, &b); }
static bool ToAffineImpl(G1Affine& out, const G1XYZZ& p) { return curdle_host_to_affine(&out, &p) != 0; }
static void FpPowImpl(Fp& r, const Fp& a, const u32* e) { curdle_host_fp_pow(&r, &a, e); }
static void FpFromMontImpl(Fp& r, const Fp& a) { curdle_host_fp_from_mont(&r, &a); }

// ------------------------------------------------------------------ Scalar ---
Scalar Scalar::FromU64(uint64_t x) {
  Fr c;
  f_zero(c);
  c.l[0] = (u32)x;
  c.l[1] = (u32)(x >> 32);
  Scalar s;
  fr_to_mont(s.v, c);
  return s;
}

void Scalar::Canonical(u32 out[8]) const {
  Fr c;
  f_from_mont<FrParams>(c, v);
  memcpy(out, c.l, 32);
}

void Scalar::Bytes(uint8_t out[32]) const {
  u32 c[8];
  Canonical(c);
  for (int i = 0; i < 8; i++) {
    u32 w = c[7 - i];
    out[4 * i] = (uint8_t)(w >> 24);
    out[4 * i + 1] = (uint8_t)(w >> 16);
    out[4 * i + 2] = (uint8_t)(w >> 8);
    out[4 * i + 3] = (uint8_t)w;
  }
}

bool Scalar::SetBytesCanonical(const uint8_t in[32], Scalar* out) {
  Fr c;
  for (int i = 0; i < 8; i++) {
    const uint8_t* q = in + 28 - 4 * i;
    c.l[i] = ((u32)q[0] << 24) | ((u32)q[1] << 16) | ((u32)q[2] << 8) | (u32)q[3];
  }
  for (int i = 7; i >= 0; i--) {
    u32 m = FrParams::mod(i);
    if (c.l[i] < m) break;
    if (c.l[i] > m || i == 0) return false;  // >= r
  }
  fr_to_mont(out->v, c);
  return true;
}

Scalar Scalar::Inverse() const {
  if (IsZero()) return Zero();
  static const u32 e[8] = {0xffffffffu, 0xfffffffeu, 0xfffe5bfeu, 0x53bda402u,
                           0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u};  // r - 2
  Scalar acc = One();
  for (int i = 255; i >= 0; i--) {
    acc = acc * acc;
    if ((e[i / 32] >> (i % 32)) & 1) acc = acc * *this;
  }
  return acc;
}

Scalar Scalar::Pow(uint64_t e) const {
  Scalar acc = One(), base = *this;
  while (e) {
    if (e & 1) acc = acc * base;
    base = base * base;
    e >>= 1;
  }
  return acc;
}

std::vector<Scalar> BatchInvert(const std::vector<Scalar>& xs) {
  // Montgomery's trick; zero entries are skipped and stay zero (fr.BatchInvert).
  std::vector<Scalar> out(xs.size());
  std::vector<Scalar> pref(xs.size());
  Scalar acc = Scalar::One();
  for (size_t i = 0; i < xs.size(); i++) {
    pref[i] = acc;
    if (!xs[i].IsZero()) acc = acc * xs[i];
  }
  Scalar inv = acc.Inverse();
  for (size_t i = xs.size(); i-- > 0;) {
    if (xs[i].IsZero()) {
      out[i] = Scalar::Zero();
      continue;
    }
    out[i] = inv * pref[i];
    inv = inv * xs[i];
  }
  return out;
}

Scalar InnerProduct(const std::vector<Scalar>& a, const std::vector<Scalar>& b) {
  if (a.size() != b.size()) throw std::runtime_error("IPA: len(a) != len(b)");  // util.go:27-29
  Scalar acc = Scalar::Zero();
  for (size_t i = 0; i < a.size(); i++) acc = acc + a[i] * b[i];
  return acc;
}

// ------------------------------------------------------------------- Point ---
static void fp_from_be48(Fp& canonical, const uint8_t in[48], uint8_t top_mask) {
  for (int i = 0; i < 12; i++) {
    const uint8_t* q = in + 44 - 4 * i;
    u32 b0 = q[0];
    if (i == 11) b0 &= top_mask;
    canonical.l[i] = (b0 << 24) | ((u32)q[1] << 16) | ((u32)q[2] << 8) | (u32)q[3];
  }
}
static bool fp_lt(const Fp& a, const u32* m) {
  for (int i = 11; i >= 0; i--) {
    if (a.l[i] != m[i]) return a.l[i] < m[i];
  }
  return false;
}
static const u32 kFpR2[12] = {0x1c341746u, 0xf4df1f34u, 0x09d104f1u, 0x0a76e6a6u, 0x4c95b6d5u, 0x8de5476cu,
                              0x939d83c0u, 0x67eb88a9u, 0xb519952du, 0x9a793e85u, 0x92cae3aau, 0x11988fe5u};
static const u32 kFpHalf[12] = {0xffffd555u, 0xdcff7fffu, 0x58a9ffffu, 0x0f55ffffu, 0x7b587b12u, 0xb3986950u,
                                0x79c2895fu, 0xb23ba5c2u, 0x21a5d66bu, 0x258dd3dbu, 0x1cbff34du, 0x0d0088f5u};  // (p-1)/2
static const u32 kFpSqrtExp[12] = {0xffffeaabu, 0xee7fbfffu, 0xac54ffffu, 0x07aaffffu, 0x3dac3d89u, 0xd9cc34a8u,
                                   0x3ce144afu, 0xd91dd2e1u, 0x90d2eb35u, 0x92c6e9edu, 0x8e5ff9a6u, 0x0680447au};  // (p+1)/4

static bool y_is_larger(const Fp& y_mont) {
  Fp c;
  FpFromMontImpl(c, y_mont);
  return !fp_lt(c, kFpHalf) && !f_eq(c, *reinterpret_cast<const Fp*>(kFpHalf));  // y > (p-1)/2
}

Point Point::operator+(const Point& o) const {
  NeedValue();
  o.NeedValue();
  Point r;
  r.p = p;
  AddImpl(r.p, o.p);
  return r;
}

G1Affine Point::Affine() const {
  NeedValue();
  G1Affine a;
  ToAffineImpl(a, p);
  return a;
}

bool Point::operator==(const Point& o) const {
  NeedValue();
  o.NeedValue();
  return curdle_host_equal(&p, &o.p) != 0;
}

Point Point::FromJac(const uint64_t jac[18]) {
  G1Jac j;
  memcpy(&j, jac, sizeof(j));
  Point r;
  g1_from_jac(r.p, j);
  return r;
}

Point Point::Generator() {
  G1Affine g;
  g1_generator(g);
  return FromAffine(g);
}

static thread_local unsigned long long t_point_mul_calls = 0;
unsigned long long PointMulCalls() { return t_point_mul_calls; }

Point Point::Mul(const Scalar& k) const {
  NeedValue();
  t_point_mul_calls++;
  u32 c[8];
  k.Canonical(c);
  Point r;
  ScalarMulImpl(r.p, p, c);
  return r;
}

void Point::Compressed(uint8_t out[48]) const {
  if (wire) {
    memcpy(out, wire, 48);
    return;
  }
  G1Affine a;
  if (!ToAffineImpl(a, p)) {
    memset(out, 0, 48);
    out[0] = 0xc0;
    return;
  }
  Fp xc;
  FpFromMontImpl(xc, a.x);
  for (int i = 0; i < 12; i++) {
    u32 w = xc.l[11 - i];
    out[4 * i] = (uint8_t)(w >> 24);
    out[4 * i + 1] = (uint8_t)(w >> 16);
    out[4 * i + 2] = (uint8_t)(w >> 8);
    out[4 * i + 3] = (uint8_t)w;
  }
  out[0] |= 0x80;
  if (y_is_larger(a.y)) out[0] |= 0x20;
}

void CompressAffine(const G1Affine& a, uint8_t out[48]) {
  if (g1_affine_is_inf(a)) {
    memset(out, 0, 48);
    out[0] = 0xc0;
    return;
  }
  Fp xc;
  FpFromMontImpl(xc, a.x);
  for (int i = 0; i < 12; i++) {
    u32 w = xc.l[11 - i];
    out[4 * i] = (uint8_t)(w >> 24);
    out[4 * i + 1] = (uint8_t)(w >> 16);
    out[4 * i + 2] = (uint8_t)(w >> 8);
    out[4 * i + 3] = (uint8_t)w;
  }
  out[0] |= 0x80;
  if (y_is_larger(a.y)) out[0] |= 0x20;
}

void CompressAffineAvx512(const G1Affine* pts, size_t n, uint8_t* out);  // compress_avx512.cpp

void CompressAffineBatch(const G1Affine* pts, size_t n, uint8_t* out) {
  static const bool ifma = [] {
    __builtin_cpu_init();
    return __builtin_cpu_supports("avx512f") && __builtin_cpu_supports("avx512ifma") && __builtin_cpu_supports("avx512vl") &&
           __builtin_cpu_supports("avx512bw") && __builtin_cpu_supports("avx512dq");
  }();
  if (!ifma || n < 8) {
    for (size_t i = 0; i < n; i++) CompressAffine(pts[i], out + 48 * i);
    return;
  }
  CompressAffineAvx512(pts, n, out);
  for (size_t i = 0; i < n; i++)  // the vector routine knows no point at infinity
    if (g1_affine_is_inf(pts[i])) CompressAffine(pts[i], out + 48 * i);
}

FixedBase::FixedBase(const G1Affine& p) : table_(32 * 255) { curdle_host_fixed_base_table(table_.data(), &p); }
Point FixedBase::Mul(const Scalar& k) const {
  u32 kc[8];
  k.Canonical(kc);
  Point r;
  curdle_host_fixed_base_mul(&r.p, table_.data(), kc);
  return r;
}

bool Point::FromCompressed(const uint8_t in[48], Point* out, bool subgroup_check) {
  const uint8_t flags = in[0] & 0xe0;
  if (!(flags & 0x80)) return false;  // only the compressed form is used on this wire
  if (flags & 0x40) {
    if (flags & 0x20) return false;
    if (in[0] & 0x1f) return false;
    for (int i = 1; i < 48; i++)
      if (in[i]) return false;
    *out = Infinity();
    return true;
  }
  Fp xc;
  fp_from_be48(xc, in, 0x1f);
  u32 pm[12];
  for (int i = 0; i < 12; i++) pm[i] = FpParams::mod(i);
  if (!fp_lt(xc, pm)) return false;
  Fp x, r2, x3, rhs, four, y, y2;
  memcpy(&r2, kFpR2, 48);
  fp_mul(x, xc, r2);  // to Montgomery
  fp_sqr(x3, x);
  fp_mul(x3, x3, x);
  f_one(four);
  fp_dbl(four, four);
  fp_dbl(four, four);
  fp_add(rhs, x3, four);  // x^3 + 4
  FpPowImpl(y, rhs, kFpSqrtExp);
  fp_sqr(y2, y);
  if (!f_eq(y2, rhs)) return false;  // not on the curve
  if (y_is_larger(y) != ((flags & 0x20) != 0)) fp_neg(y, y);
  G1Affine a;
  a.x = x;
  a.y = y;
  *out = FromAffine(a);
  if (subgroup_check) {
    if (!curdle_host_in_subgroup(&out->p)) return false;  // endomorphism test, host_math.h
  }
  return true;
}

std::vector<G1Affine> BatchToAffine(const std::vector<Point>& pts) {
  std::vector<G1Affine> out(pts.size());
  for (size_t i = 0; i < pts.size(); i++) ToAffineImpl(out[i], pts[i].p);
  return out;
}

// --------------------------------------------------------------------- MSM ---
static MsmError msm_error(int rc) {
  char buf[256];
  curdle_last_error(buf, sizeof(buf));
  return MsmError(std::string("computing msm: ") + buf + " (rc " + std::to_string(rc) + ")", rc);
}

static thread_local bool t_msm_ct = false;
static std::atomic<unsigned long long> g_msm_counters[4];
static constexpr unsigned kCtScalarBits = 255;  // every canonical scalar: r < 2^255

ConstantTimeMsmScope::ConstantTimeMsmScope() : prev_(t_msm_ct) { t_msm_ct = true; }
ConstantTimeMsmScope::~ConstantTimeMsmScope() { t_msm_ct = prev_; }
bool ConstantTimeMsmScope::Available() { return curdle_msm_g1_ct && curdle_msm_g1_ct_batch && curdle_msm_g1_ct_multi; }

void ReadMsmCounters(unsigned long long out[4]) {
  for (int i = 0; i < 4; i++) out[i] = g_msm_counters[i].load(std::memory_order_relaxed);
}

static void count_msm(bool ct, size_t pairs) {
  g_msm_counters[ct ? 2 : 0].fetch_add(1, std::memory_order_relaxed);
  g_msm_counters[ct ? 3 : 1].fetch_add(pairs, std::memory_order_relaxed);
}

// ------------------------------------------------------------ the third switch ---
static thread_local Lockstep* t_lockstep = nullptr;
static thread_local size_t t_lockstep_member = 0;
static bool secret_ops_on();

struct Lockstep::Request {
  enum Funnel { kMultiExp, kMultiExpBatch, kMultiExpShared, kScalarMul, kPermute } funnel;
  bool ct = false, secret = false;  // the member thread's two switches
  struct Msm {
    const G1Affine* P;
    const Scalar* S;
    size_t n;
  };
  std::vector<Msm> msms;  // the MSM funnels: member-major, in the call's order
  std::vector<Point> msm_out;
  const G1Affine* points = nullptr;  // ScalarMulBatch
  const Scalar* scalars = nullptr;
  const G1Affine* addends = nullptr;
  size_t n_scalars = 0, n = 0;  // n: also PermuteSecret's
  G1Affine* mul_out = nullptr;
  const Scalar* vs = nullptr;  // PermuteSecret
  const uint32_t* perm = nullptr;
  Scalar* perm_out = nullptr;
  bool failed = false;  // the step's verdict, the same for every member of it
  int rc = 0;
  std::string what;
};

struct LockstepAccess {
  static void Go(Lockstep::Request* r) {
    r->ct = t_msm_ct;
    r->secret = secret_ops_on();
    t_lockstep->Rendezvous(t_lockstep_member, r);
  }
};

static std::vector<Point> LockstepMsms(Lockstep::Request::Funnel funnel, std::vector<Lockstep::Request::Msm> msms) {
  Lockstep::Request r;
  r.funnel = funnel;
  r.msms = std::move(msms);
  LockstepAccess::Go(&r);
  return std::move(r.msm_out);
}

static int no_ct_backend() {
  return curdle_set_last_error(CURDLE_ENODEV, "the constant-time MSM is not part of this backend: no device code to run it on");
}

// ------------------------------------------------------------ the fourth switch ---
static_assert(sizeof(G1Affine) == 96, "a base record is a gnark G1Affine");
struct ResidentBases::Impl {
  using Key = std::array<uint64_t, 12>;
  struct Hash {
    size_t operator()(const Key& k) const {
      uint64_t h = 0x9e3779b97f4a7c15ull;
      for (uint64_t w : k) h = (h ^ w) * 0xff51afd7ed558ccdull + (h >> 29);
      return (size_t)h;
    }
  };
  std::unordered_map<Key, uint32_t, Hash> rows;
  static Key KeyOf(const G1Affine& p) {
    Key k;
    memcpy(k.data(), &p, 96);
    return k;
  }
};

static thread_local ResidentBases* t_resident = nullptr;
static std::atomic<unsigned long long> g_resident_counters[4];

ResidentBases::ResidentBases(unsigned chunk_bits) : chunk_bits_(ChunkBitsOf(chunk_bits)), map_(new Impl()) {
  if (chunk_bits_ != 8 && chunk_bits_ != 16 && chunk_bits_ != 32 && chunk_bits_ != 64) {
    delete map_;
    throw MsmError("resident bases: chunk_bits is not 8, 16, 32, 64 or 0", CURDLE_EINVAL);
  }
}

ResidentBases::~ResidentBases() {
  for (size_t s = 0; s < handles_.size(); s++)
    if (owned_[s] && curdle_ct_bases_free) curdle_ct_bases_free(static_cast<curdle_ct_bases*>(const_cast<void*>(handles_[s])));
  delete map_;
}

void ResidentBases::Index(const std::vector<G1Affine>& points) {
  for (size_t i = 0; i < points.size(); i++) map_->rows.emplace(Impl::KeyOf(points[i]), (uint32_t)(rows_ + i));  // the first occurrence wins
  rows_ += points.size();
}

void ResidentBases::Add(const std::vector<G1Affine>& points) {
  if (handles_.size() >= kMaxSets) throw MsmError("resident bases: a registry holds at most four sets", CURDLE_EINVAL);
  if (!ResidentBasesScope::Available()) {
    const int rc = curdle_set_last_error(CURDLE_ENODEV, "the constant-time base tables are not part of this backend: no device code to run them on");
    throw msm_error(rc);
  }
  curdle_ct_bases* h = nullptr;
  const int rc = curdle_ct_bases_create(reinterpret_cast<const uint64_t*>(points.data()), points.size(), chunk_bits_, &h);
  if (rc != CURDLE_OK) throw msm_error(rc);
  handles_.push_back(h);
  owned_.push_back(1);
  Index(points);
}

void ResidentBases::AddShared(const void* handle, const std::vector<G1Affine>& points) {
  if (handles_.size() >= kMaxSets) throw MsmError("resident bases: a registry holds at most four sets", CURDLE_EINVAL);
  handles_.push_back(handle);
  owned_.push_back(0);
  Index(points);
}

bool ResidentBases::Find(const G1Affine& p, uint32_t* row) const {
  const auto it = map_->rows.find(Impl::KeyOf(p));
  if (it == map_->rows.end()) return false;
  *row = it->second;
  return true;
}

ResidentBasesScope::ResidentBasesScope(ResidentBases& bases) : prev_(t_resident) { t_resident = &bases; }
ResidentBasesScope::~ResidentBasesScope() { t_resident = prev_; }
ResidentBases* ResidentBasesScope::Active() { return t_resident && !t_resident->Declined() ? t_resident : nullptr; }
bool ResidentBasesScope::Available() { return curdle_ct_bases_create && curdle_ct_bases_free && curdle_msm_g1_ct_bases_sets_batch; }

void ReadResidentCounters(unsigned long long out[4]) {
  for (int i = 0; i < 4; i++) out[i] = g_resident_counters[i].load(std::memory_order_relaxed);
}

namespace {
template <class T>
struct WipeOnExit {  // a concatenated copy of secrets does not outlive the call that made it
  std::vector<T>& v;
  bool on;
  ~WipeOnExit() {
    if (on && !v.empty()) explicit_bzero(v.data(), v.size() * sizeof(T));
  }
};

struct BaseRun {
  const G1Affine* p;
  size_t n;
};
constexpr size_t kResidentMaxTerms = 65536, kResidentMaxMsms = 4096;  // curdle_msm_g1_ct_bases_sets_batch's limits

// The registry this call consults: the thread's, under a ConstantTimeMsmScope and outside a lockstep group.
ResidentBases* resident_registry(bool ct) { return ct && !t_lockstep ? t_resident : nullptr; }

// Whether a call of `msms` MSMs over the base runs goes to the resident tables, and then its row list: the shape fits
// one pass and every base is a resident record.  Public shapes and public points only.
bool resident_rows(const ResidentBases* rb, const std::vector<BaseRun>& runs, size_t msms, std::vector<uint32_t>* rows) {
  if (!rb || !rb->Sets() || !ResidentBasesScope::Available() || msms > kResidentMaxMsms) return false;
  size_t pairs = 0, cap = kResidentMaxTerms;
  for (const BaseRun& r : runs) pairs += r.n;
  const long long knob = knobs::get(knobs::PROVE_RESIDENT_TERMS);
  if (knob > 0 && (size_t)knob < cap) cap = (size_t)knob;
  if (pairs > cap / rb->Chunks()) return false;
  rows->resize(pairs);
  size_t q = 0;
  for (const BaseRun& r : runs)
    for (size_t i = 0; i < r.n; i++)
      if (!rb->Find(r.p[i], &(*rows)[q++])) return false;
  return true;
}

int resident_call(const ResidentBases* rb, const std::vector<uint32_t>& rows, const uint64_t* scalars, const size_t* offsets,
                  size_t k, uint64_t* out) {
  return curdle_msm_g1_ct_bases_sets_batch(reinterpret_cast<const curdle_ct_bases* const*>(rb->Handles()), rb->Sets(), rows.data(),
                                           scalars, offsets, k, kCtScalarBits, out);
}

// A successful constant-time call under an active registry: which of the two routes it took.
void count_resident(const ResidentBases* rb, bool resident, size_t pairs) {
  if (!rb) return;
  g_resident_counters[resident ? 0 : 2].fetch_add(1, std::memory_order_relaxed);
  g_resident_counters[resident ? 1 : 3].fetch_add(pairs, std::memory_order_relaxed);
}
}  // namespace

Point MultiExp(const std::vector<G1Affine>& points, const std::vector<Scalar>& scalars) {
  if (points.size() != scalars.size()) throw std::runtime_error("computing msm: len(points) != len(scalars)");
  if (t_lockstep) return LockstepMsms(Lockstep::Request::kMultiExp, {{points.data(), scalars.data(), points.size()}})[0];
  const bool ct = t_msm_ct;
  const ResidentBases* rb = resident_registry(ct);
  std::vector<uint32_t> rows;
  const bool resident = resident_rows(rb, {{points.data(), points.size()}}, 1, &rows);
  const uint64_t* P = reinterpret_cast<const uint64_t*>(points.data());
  const uint64_t* S = reinterpret_cast<const uint64_t*>(scalars.data());
  uint64_t out[18];
  int rc;
  if (!ct) {
    rc = curdle_msm_g1(P, S, points.size(), out);
  } else if (resident) {
    const size_t off[2] = {0, points.size()};
    rc = resident_call(rb, rows, S, off, 1, out);
  } else {
    rc = curdle_msm_g1_ct ? curdle_msm_g1_ct(P, S, points.size(), kCtScalarBits, out) : no_ct_backend();
  }
  if (rc != CURDLE_OK) throw msm_error(rc);
  count_msm(ct, points.size());
  count_resident(rb, resident, points.size());
  return Point::FromJac(out);
}

std::vector<Point> MultiExpBatch(const std::vector<const std::vector<G1Affine>*>& points,
                                 const std::vector<const std::vector<Scalar>*>& scalars) {
  if (points.size() != scalars.size()) throw std::runtime_error("computing msm: batch shape");
  const bool ct = t_msm_ct;
  const size_t k = points.size();
  std::vector<size_t> off(k + 1, 0);
  for (size_t j = 0; j < k; j++) {
    if (points[j]->size() != scalars[j]->size()) throw std::runtime_error("computing msm: len(points) != len(scalars)");
    off[j + 1] = off[j] + points[j]->size();
  }
  if (t_lockstep) {
    std::vector<Lockstep::Request::Msm> msms(k);
    for (size_t j = 0; j < k; j++) msms[j] = {points[j]->data(), scalars[j]->data(), points[j]->size()};
    return LockstepMsms(Lockstep::Request::kMultiExpBatch, std::move(msms));
  }
  const ResidentBases* rb = resident_registry(ct);
  std::vector<uint32_t> rows;
  std::vector<BaseRun> runs(k);
  for (size_t j = 0; j < k; j++) runs[j] = {points[j]->data(), points[j]->size()};
  const bool resident = resident_rows(rb, runs, k, &rows);
  std::vector<G1Affine> P(resident ? 0 : off[k]);  // the resident call names its bases by row
  std::vector<Scalar> S(off[k]);
  struct Clear {  // the concatenated copy of the scalars does not outlive a constant-time call
    std::vector<Scalar>& v;
    bool on;
    ~Clear() {
      if (on && !v.empty()) explicit_bzero(v.data(), v.size() * sizeof(Scalar));
    }
  } clear{S, ct};
  for (size_t j = 0; j < k; j++) {
    if (!resident) std::copy(points[j]->begin(), points[j]->end(), P.begin() + off[j]);
    std::copy(scalars[j]->begin(), scalars[j]->end(), S.begin() + off[j]);
  }
  std::vector<uint64_t> out(18 * k);
  const uint64_t* Pw = reinterpret_cast<const uint64_t*>(P.data());
  const uint64_t* Sw = reinterpret_cast<const uint64_t*>(S.data());
  int rc;
  if (!ct)
    rc = curdle_msm_g1_batch(Pw, Sw, off.data(), k, out.data());
  else if (resident)
    rc = resident_call(rb, rows, Sw, off.data(), k, out.data());
  else
    rc = curdle_msm_g1_ct_batch ? curdle_msm_g1_ct_batch(Pw, Sw, off.data(), k, kCtScalarBits, out.data()) : no_ct_backend();
  if (rc != CURDLE_OK) throw msm_error(rc);
  count_msm(ct, off[k]);
  count_resident(rb, resident, off[k]);
  std::vector<Point> res(k);
  for (size_t j = 0; j < k; j++) res[j] = Point::FromJac(out.data() + 18 * j);
  return res;
}

std::vector<Point> MultiExpShared(const std::vector<const std::vector<G1Affine>*>& sets,
                                  const std::vector<Scalar>& scalars) {
  const bool ct = t_msm_ct;
  const size_t k = sets.size();
  std::vector<const uint64_t*> ptrs(k);
  for (size_t j = 0; j < k; j++) {
    if (sets[j]->size() != scalars.size()) throw std::runtime_error("computing msm: len(points) != len(scalars)");
    ptrs[j] = reinterpret_cast<const uint64_t*>(sets[j]->data());
  }
  std::vector<uint64_t> out(18 * k);
  if (scalars.empty()) {
    std::vector<Point> res(k, Point::Infinity());
    return res;
  }
  if (t_lockstep) {
    std::vector<Lockstep::Request::Msm> msms(k);
    for (size_t j = 0; j < k; j++) msms[j] = {sets[j]->data(), scalars.data(), scalars.size()};
    return LockstepMsms(Lockstep::Request::kMultiExpShared, std::move(msms));
  }
  const uint64_t* Sw = reinterpret_cast<const uint64_t*>(scalars.data());
  const ResidentBases* rb = resident_registry(ct);
  std::vector<uint32_t> rows;
  std::vector<BaseRun> runs(k);
  for (size_t j = 0; j < k; j++) runs[j] = {sets[j]->data(), sets[j]->size()};
  const bool resident = resident_rows(rb, runs, k, &rows);
  int rc;
  if (!ct) {
    rc = curdle_msm_g1_multi(ptrs.data(), k, Sw, scalars.size(), out.data());
  } else if (resident) {
    // one batch of k MSMs: the scalar vector once per set, in a copy that does not outlive the call
    const size_t n = scalars.size();
    std::vector<Scalar> S(k * n);
    WipeOnExit<Scalar> wipe{S, true};
    std::vector<size_t> off(k + 1, 0);
    for (size_t j = 0; j < k; j++) {
      std::copy(scalars.begin(), scalars.end(), S.begin() + j * n);
      off[j + 1] = off[j] + n;
    }
    rc = resident_call(rb, rows, reinterpret_cast<const uint64_t*>(S.data()), off.data(), k, out.data());
  } else {
    rc = curdle_msm_g1_ct_multi ? curdle_msm_g1_ct_multi(ptrs.data(), k, Sw, scalars.size(), kCtScalarBits, out.data())
                                : no_ct_backend();
  }
  if (rc != CURDLE_OK) throw msm_error(rc);
  count_msm(ct, k * scalars.size());
  count_resident(rb, resident, k * scalars.size());
  std::vector<Point> res(k);
  for (size_t j = 0; j < k; j++) res[j] = Point::FromJac(out.data() + 18 * j);
  return res;
}

// ------------------------------------------------------- the second switch ---
static thread_local bool t_secret_ops = false;

SecretOpsScope::SecretOpsScope() : prev_(t_secret_ops) { t_secret_ops = true; }
SecretOpsScope::~SecretOpsScope() { t_secret_ops = prev_; }
bool SecretOpsScope::Active() { return t_secret_ops; }
static bool secret_ops_on() { return t_secret_ops; }
bool SecretOpsScope::Available() { return curdle_fr_permute_ct && ConstantTimeMsmScope::Available(); }

std::vector<Scalar> PermuteSecret(const std::vector<Scalar>& vs, const std::vector<uint32_t>& perm) {
  std::vector<Scalar> out(vs.size());
  if (!t_secret_ops) {
    for (size_t i = 0; i < perm.size(); i++) out[i] = vs[perm[i]];
    return out;
  }
  if (perm.size() != vs.size()) throw std::runtime_error("permuting: len(perm) != len(values)");
  static_assert(sizeof(Scalar) == 32, "the gather's record is an fr.Element");
  if (t_lockstep) {
    Lockstep::Request r;
    r.funnel = Lockstep::Request::kPermute;
    r.vs = vs.data();
    r.perm = perm.data();
    r.n = vs.size();
    r.perm_out = out.data();
    LockstepAccess::Go(&r);
    return out;
  }
  // perm goes to the device from where it lies and the records arrive in `out`, the prover's own vector: nothing is
  // created here that would have to be wiped (the call wipes its staging).
  const int rc = curdle_fr_permute_ct
                     ? curdle_fr_permute_ct(reinterpret_cast<const uint64_t*>(vs.data()), perm.data(), vs.size(),
                                            reinterpret_cast<uint64_t*>(out.data()))
                     : curdle_set_last_error(CURDLE_ENODEV, "the oblivious gather is not part of this backend: no device code to run it on");
  if (rc != CURDLE_OK) {
    char buf[256];
    curdle_last_error(buf, sizeof(buf));
    throw MsmError(std::string("permuting: ") + buf + " (rc " + std::to_string(rc) + ")", rc);
  }
  return out;
}

std::vector<G1Affine> ScalarMulBatch(const std::vector<G1Affine>& points, const std::vector<Scalar>& scalars,
                                     const std::vector<G1Affine>* addends) {
  const size_t n = points.size();
  if (scalars.size() != n && scalars.size() != 1) throw std::runtime_error("scalar mul batch: len(scalars) must be n or 1");
  if (addends && addends->size() != n) throw std::runtime_error("scalar mul batch: len(addends) != len(points)");
  std::vector<G1Affine> out(n);
  if (n == 0) return out;
  if (t_lockstep) {
    Lockstep::Request r;
    r.funnel = Lockstep::Request::kScalarMul;
    r.points = points.data();
    r.scalars = scalars.data();
    r.n_scalars = scalars.size();
    r.addends = addends ? addends->data() : nullptr;
    r.n = n;
    r.mul_out = out.data();
    LockstepAccess::Go(&r);
    return out;
  }
  if (t_secret_ops) {  // the scalars are secrets: the constant-time multiplication at every size, never the host loop
    if (addends) throw std::runtime_error("scalar mul batch: the constant-time multiplication takes no addends");
    const int rc = curdle_g1_scalar_mul_batch_ex
                       ? curdle_g1_scalar_mul_batch_ex(reinterpret_cast<const uint64_t*>(points.data()),
                                                       reinterpret_cast<const uint64_t*>(scalars.data()), scalars.size(), nullptr, n,
                                                       CURDLE_G1_MUL_CONSTANT_TIME, reinterpret_cast<uint64_t*>(out.data()))
                       : curdle_set_last_error(CURDLE_ENODEV, "the constant-time multiplication is not part of this backend: no device code to run it on");
    if (rc != CURDLE_OK) throw msm_error(rc);
    return out;
  }
  if (n >= kScalarMulBatchMin) {
    int rc = curdle_g1_scalar_mul_batch(reinterpret_cast<const uint64_t*>(points.data()),
                                        reinterpret_cast<const uint64_t*>(scalars.data()), scalars.size(),
                                        addends ? reinterpret_cast<const uint64_t*>(addends->data()) : nullptr, n,
                                        reinterpret_cast<uint64_t*>(out.data()));
    if (rc != CURDLE_OK) throw msm_error(rc);
    return out;
  }
  for (size_t i = 0; i < n; i++) {  // a handful of points: a kernel launch would cost more than it saves
    Point r = Point::FromAffine(points[i]).Mul(scalars.size() == 1 ? scalars[0] : scalars[i]);
    if (addends) r = r + Point::FromAffine((*addends)[i]);
    out[i] = r.Affine();
  }
  return out;
}

// ------------------------------------------------------------ the lockstep group ---
Lockstep::Lockstep(size_t members) : reqs_(members, nullptr), live_flag_(members, 1), live_(members) {}
Lockstep::~Lockstep() {}

unsigned long long Lockstep::DeviceCalls() const {
  std::lock_guard<std::mutex> lk(mu_);
  return device_calls_;
}

unsigned long long Lockstep::Disagreements() const {
  std::lock_guard<std::mutex> lk(mu_);
  return disagreements_;
}

void Lockstep::Leave(size_t member) {
  std::lock_guard<std::mutex> lk(mu_);
  if (member >= live_flag_.size() || !live_flag_[member]) return;
  live_flag_[member] = 0;
  live_--;
  if (arrived_ && arrived_ == live_) cv_.notify_all();  // the step was waiting for this member alone: a waiter runs it
}

LockstepScope::LockstepScope(Lockstep& group, size_t member) : prev_group_(t_lockstep), prev_member_(t_lockstep_member) {
  t_lockstep = &group;
  t_lockstep_member = member;
}
LockstepScope::~LockstepScope() {
  t_lockstep->Leave(t_lockstep_member);
  t_lockstep = prev_group_;
  t_lockstep_member = prev_member_;
}

void Lockstep::Rendezvous(size_t member, Request* r) {
  {
    std::unique_lock<std::mutex> lk(mu_);
    reqs_[member] = r;
    arrived_++;
    const unsigned long long step = step_;
    while (step_ == step) {
      if (arrived_ == live_) {
        // Every live member is in this loop, so nobody else wants the lock while the step runs under it.
        RunStep();
        std::fill(reqs_.begin(), reqs_.end(), nullptr);
        arrived_ = 0;
        step_++;
        cv_.notify_all();
        break;
      }
      cv_.wait(lk);
    }
  }
  if (r->failed) throw MsmError(r->what, r->rc);
}

namespace {
// Members per coalesced call: as many whole members as fit `cap` units (and `cap_members`), at least one -- a member
// that alone is too large for the primitive gets the primitive's own refusal, as its single call would.
size_t members_per_call(size_t unit, size_t cap, size_t cap_members) {
  const long long knob = knobs::get(knobs::PROVE_BATCH_PAIRS);
  if (knob > 0 && (size_t)knob < cap) cap = (size_t)knob;
  size_t m = unit ? cap / unit : cap_members;
  if (m > cap_members) m = cap_members;
  return m ? m : 1;
}

std::string last_error_text(const char* what, int rc) {
  char buf[256];
  curdle_last_error(buf, sizeof(buf));
  return std::string(what) + buf + " (rc " + std::to_string(rc) + ")";
}
}  // namespace

void Lockstep::RunStep() {
  using R = Request;
  std::vector<R*> rs;
  for (R* r : reqs_)
    if (r) rs.push_back(r);
  if (rs.empty()) return;
  auto fail_all = [&](int rc, const std::string& what) {
    for (R* r : rs) {
      r->failed = true;
      r->rc = rc;
      r->what = what;
    }
  };
  const R& a = *rs[0];
  for (const R* r : rs) {  // funnel, switches and shapes: public, and the same for every member of a sound group
    bool same = r->funnel == a.funnel && r->ct == a.ct && r->secret == a.secret && r->msms.size() == a.msms.size() &&
                r->n == a.n && r->n_scalars == a.n_scalars && !r->addends == !a.addends;
    for (size_t j = 0; same && j < a.msms.size(); j++) same = r->msms[j].n == a.msms[j].n;
    if (!same) {
      disagreements_++;
      return fail_all(CURDLE_EINVAL, "lockstep: the members' requests disagree at step " + std::to_string(step_) +
                                         " (funnel, shapes or constant-time switches)");
    }
  }
  try {
    const size_t k = rs.size();
    if (a.funnel == R::kMultiExp || a.funnel == R::kMultiExpBatch || a.funnel == R::kMultiExpShared) {
      const size_t per = a.msms.size();
      size_t unit = 0;
      for (const R::Msm& m : a.msms) unit += m.n;
      if (a.funnel == R::kMultiExpShared && unit == 0) {  // as MultiExpShared: no call for an empty scalar vector
        for (R* r : rs) r->msm_out.assign(per, Point::Infinity());
        return;
      }
      // curdle_msm_g1_ct_batch: 65,536 pairs and 4,096 MSMs a call; the bucket MSM splits a batch into passes itself
      const size_t step_members = a.ct ? members_per_call(unit, 65536, std::max<size_t>(1, 4096 / std::max<size_t>(1, per)))
                                       : members_per_call(unit, (size_t)1 << 24, k);
      for (size_t lo = 0; lo < k; lo += step_members) {
        const size_t hi = std::min(k, lo + step_members), nm = (hi - lo) * per;
        std::vector<size_t> off(nm + 1, 0);
        std::vector<G1Affine> P((hi - lo) * unit);
        std::vector<Scalar> S((hi - lo) * unit);
        WipeOnExit<Scalar> wipe{S, a.ct};
        size_t q = 0;
        for (size_t i = lo; i < hi; i++)
          for (const R::Msm& m : rs[i]->msms) {
            std::copy(m.P, m.P + m.n, P.begin() + off[q]);
            std::copy(m.S, m.S + m.n, S.begin() + off[q]);
            off[q + 1] = off[q] + m.n;
            q++;
          }
        std::vector<uint64_t> out(18 * nm);
        const uint64_t* Pw = reinterpret_cast<const uint64_t*>(P.data());
        const uint64_t* Sw = reinterpret_cast<const uint64_t*>(S.data());
        int rc;
        if (!a.ct)
          rc = curdle_msm_g1_batch(Pw, Sw, off.data(), nm, out.data());
        else
          rc = curdle_msm_g1_ct_batch ? curdle_msm_g1_ct_batch(Pw, Sw, off.data(), nm, kCtScalarBits, out.data()) : no_ct_backend();
        if (rc != CURDLE_OK) return fail_all(rc, last_error_text("computing msm: ", rc));
        count_msm(a.ct, off[nm]);
        device_calls_++;
        for (size_t i = lo; i < hi; i++) {
          rs[i]->msm_out.resize(per);
          for (size_t j = 0; j < per; j++) rs[i]->msm_out[j] = Point::FromJac(out.data() + 18 * ((i - lo) * per + j));
        }
      }
      return;
    }
    if (a.funnel == R::kScalarMul) {
      const size_t n = a.n;
      if (a.secret && a.addends)
        return fail_all(CURDLE_EINVAL, "scalar mul batch: the constant-time multiplication takes no addends");
      const size_t step_members = members_per_call(n, (size_t)1 << 24, k);
      for (size_t lo = 0; lo < k; lo += step_members) {
        const size_t hi = std::min(k, lo + step_members), m = (hi - lo) * n;
        std::vector<G1Affine> P(m), A(a.addends ? m : 0), out(m);
        std::vector<Scalar> S(m);
        WipeOnExit<Scalar> wipe{S, a.secret || a.ct};
        WipeOnExit<G1Affine> wipe_out{out, a.secret};  // multiples by a secret: the members keep (and wipe) their own
        for (size_t i = lo; i < hi; i++) {
          const R& r = *rs[i];
          std::copy(r.points, r.points + n, P.begin() + (i - lo) * n);
          if (r.addends) std::copy(r.addends, r.addends + n, A.begin() + (i - lo) * n);
          for (size_t t = 0; t < n; t++) S[(i - lo) * n + t] = r.scalars[r.n_scalars == 1 ? 0 : t];
        }
        const uint64_t* Pw = reinterpret_cast<const uint64_t*>(P.data());
        const uint64_t* Sw = reinterpret_cast<const uint64_t*>(S.data());
        uint64_t* Ow = reinterpret_cast<uint64_t*>(out.data());
        int rc;
        if (!a.secret)
          rc = curdle_g1_scalar_mul_batch(Pw, Sw, m, a.addends ? reinterpret_cast<const uint64_t*>(A.data()) : nullptr, m, Ow);
        else
          rc = curdle_g1_scalar_mul_batch_ex
                   ? curdle_g1_scalar_mul_batch_ex(Pw, Sw, m, nullptr, m, CURDLE_G1_MUL_CONSTANT_TIME, Ow)
                   : curdle_set_last_error(CURDLE_ENODEV, "the constant-time multiplication is not part of this backend: no device code to run it on");
        if (rc != CURDLE_OK) return fail_all(rc, last_error_text("computing msm: ", rc));
        device_calls_++;
        for (size_t i = lo; i < hi; i++) std::copy(out.begin() + (i - lo) * n, out.begin() + (i - lo + 1) * n, rs[i]->mul_out);
      }
      return;
    }
    // PermuteSecret under a SecretOpsScope (without one the members never come here)
    const size_t n = a.n;
    if (n == 0) return;
    const size_t step_members = members_per_call(n, (size_t)1 << 20, 4096);  // curdle_fr_permute_ct_batch's limits
    for (size_t lo = 0; lo < k; lo += step_members) {
      const size_t hi = std::min(k, lo + step_members), m = (hi - lo) * n;
      std::vector<Scalar> in(m), out(m);
      std::vector<uint32_t> perm(m);
      WipeOnExit<Scalar> wipe_in{in, true}, wipe_out{out, true};
      WipeOnExit<uint32_t> wipe_perm{perm, true};
      for (size_t i = lo; i < hi; i++) {
        std::copy(rs[i]->vs, rs[i]->vs + n, in.begin() + (i - lo) * n);
        std::copy(rs[i]->perm, rs[i]->perm + n, perm.begin() + (i - lo) * n);
      }
      const int rc = curdle_fr_permute_ct_batch
                         ? curdle_fr_permute_ct_batch(reinterpret_cast<const uint64_t*>(in.data()), perm.data(), n, hi - lo,
                                                      reinterpret_cast<uint64_t*>(out.data()))
                         : curdle_set_last_error(CURDLE_ENODEV, "the batched oblivious gather is not part of this backend: no device code to run it on");
      if (rc != CURDLE_OK) return fail_all(rc, last_error_text("permuting: ", rc));
      device_calls_++;
      for (size_t i = lo; i < hi; i++) std::copy(out.begin() + (i - lo) * n, out.begin() + (i - lo + 1) * n, rs[i]->perm_out);
    }
  } catch (const std::bad_alloc&) {
    fail_all(CURDLE_ENOMEM, "lockstep: out of memory in a coalesced call");
  } catch (const std::exception& e) {
    fail_all(CURDLE_EHIP, std::string("lockstep: ") + e.what());
  }
}

LockstepRun RunInLockstep(size_t members, size_t group_size, bool constant_time, const std::function<void(size_t)>& job,
                          const std::function<void(size_t)>& could_not_start) {
  LockstepRun run;
  if (group_size == 0) group_size = 1;
  const int device = curdle_get_device();  // the batch runs where its caller is
  for (size_t lo = 0; lo < members; lo += group_size) {
    const size_t m = std::min(group_size, members - lo);
    Lockstep group(m);
    std::vector<std::thread> threads;
    threads.reserve(m);
    for (size_t j = 0; j < m; j++) {
      try {
        threads.emplace_back([&group, &job, lo, j, constant_time, device]() {
          LockstepScope in_group(group, j);
          (void)curdle_set_device(device);
          if (!constant_time) {
            job(lo + j);
            return;
          }
          ConstantTimeMsmScope msms;
          SecretOpsScope secret_ops;
          job(lo + j);
        });
      } catch (const std::system_error&) {
        group.Leave(j);
        run.not_started++;
        could_not_start(lo + j);
      }
    }
    for (std::thread& t : threads) t.join();
    run.groups++;
    run.device_calls += group.DeviceCalls();
    run.disagreements += group.Disagreements();
  }
  return run;
}

}  // namespace alg
}  // namespace curdle
