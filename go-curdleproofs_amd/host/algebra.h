// Small algebra layer for the host-side protocol code: Fr scalars and G1 points as
// value types with operators, the byte encodings gnark uses on the wire, and the one
// function every MSM of the protocol goes through (alg::MultiExp -> the GPU, via the
// C ABI).  Built on bls12_381.h / host_math.h.
//
// Replaces what the reference's protocol packages get from gnark-crypto
// (fr.Element, bls12381.G1Jac / G1Affine and their Bytes / SetBytes, go.mod:6).
#pragma once
#include <stdexcept>
#include <string>
#include <stdint.h>
#include <string.h>

#include <condition_variable>
#include <functional>
#include <mutex>
#include <string>
#include <vector>

#include "../csrc/host_math.h"

namespace curdle {
namespace alg {

// A failed call into the MSM entry points (no device, HIP error, ...): distinct from the
// protocol's structural errors so callers can tell "reject" from "could not compute".
struct MsmError : std::runtime_error {
  int rc;
  MsmError(const std::string& what, int code) : std::runtime_error(what), rc(code) {}
};

struct Scalar {
  Fr v;  // Montgomery form, as fr.Element

  static Scalar Zero() {
    Scalar s;
    f_zero(s.v);
    return s;
  }
  static Scalar One() {
    Scalar s;
    f_one(s.v);
    return s;
  }
  static Scalar FromU64(uint64_t x);  // fr.NewElement
  static Scalar FromMont(const uint64_t limbs[4]) {
    Scalar s;
    memcpy(&s.v, limbs, 32);
    return s;
  }
  Scalar operator+(const Scalar& o) const {
    Scalar r;
    fr_add(r.v, v, o.v);
    return r;
  }
  Scalar operator-(const Scalar& o) const {
    Scalar r;
    fr_sub(r.v, v, o.v);
    return r;
  }
  Scalar operator-() const {
    Scalar r;
    f_neg<FrParams>(r.v, v);
    return r;
  }
  Scalar operator*(const Scalar& o) const {
    Scalar r;
    fr_mul(r.v, v, o.v);
    return r;
  }
  Scalar Neg() const { return Zero() - *this; }
  Scalar Inverse() const;          // 0 -> 0, as fr.Element.Inverse
  Scalar Pow(uint64_t e) const;    // fr.Element.Exp with a small exponent
  bool IsZero() const { return f_is_zero(v); }
  bool operator==(const Scalar& o) const { return f_eq(v, o.v); }
  bool operator!=(const Scalar& o) const { return !f_eq(v, o.v); }
  void Canonical(u32 out[8]) const;             // the integer, little-endian limbs (fr.Element.BigInt)
  void Bytes(uint8_t out[32]) const;            // fr.Element.Bytes: big-endian canonical
  static bool SetBytesCanonical(const uint8_t in[32], Scalar* out);  // false if >= r
};

std::vector<Scalar> BatchInvert(const std::vector<Scalar>& xs);      // fr.BatchInvert (zeros stay zero)
Scalar InnerProduct(const std::vector<Scalar>& a, const std::vector<Scalar>& b);  // common.IPA, util.go:26

struct Point {
  G1XYZZ p;
  // Set only by the verifier's lazy proof reader (proto::Reader with `lazy`), for points whose
  // decoding is still running on the GPU: `wire` is the 48-byte record the point comes from --
  // what the transcript absorbs, so it needs no coordinates -- and `pending` >= 0 says the
  // coordinates are NOT known yet (the record's index in the proto::PointDecoder).  A pending
  // point can be hashed and listed as a base; arithmetic on it is a logic error.  Both die with
  // the verification call: results of operators never carry them.
  const uint8_t* wire = nullptr;
  int32_t pending = -1;
  void NeedValue() const {
    if (pending >= 0) throw std::logic_error("arithmetic on a point that is still being decoded");
  }

  static Point Infinity() {
    Point r;
    g1_set_inf(r.p);
    return r;
  }
  static Point FromAffine(const G1Affine& a) {
    Point r;
    g1_from_affine(r.p, a);
    return r;
  }
  static Point FromJac(const uint64_t jac[18]);
  static Point Generator();
  Point operator+(const Point& o) const;
  Point Neg() const {
    NeedValue();
    Point r;
    r.p = p;
    if (!g1_is_inf(r.p)) fp_neg(r.p.y, r.p.y);
    return r;
  }
  Point operator-(const Point& o) const { return *this + o.Neg(); }
  Point Mul(const Scalar& k) const;   // ScalarMultiplication with FrToBigInt(k)
  bool IsInfinity() const {
    NeedValue();
    return g1_is_inf(p);
  }
  bool operator==(const Point& o) const;   // G1Jac.Equal
  G1Affine Affine() const;
  void Jac(uint64_t out[18]) const {
    NeedValue();
    g1_to_canonical_jac(out, p);
  }
  // gnark G1Affine.Bytes(): 48 bytes, big-endian x, flags in the top three bits
  // (0x80 compressed, 0x40 infinity, 0x20 y is the lexicographically larger root).  A point
  // that carries its wire record hands that back (a valid record is its point's only encoding).
  void Compressed(uint8_t out[48]) const;
  // G1Affine.SetBytes: false on a malformed encoding or a point not on the curve;
  // the (slow, [r]P) subgroup check is optional.
  static bool FromCompressed(const uint8_t in[48], Point* out, bool subgroup_check);
};

std::vector<G1Affine> BatchToAffine(const std::vector<Point>& pts);   // BatchJacobianToAffineG1

// gnark G1Affine.Bytes() of an affine point without the round trip through Point: two
// Montgomery reductions (x to canonical bytes, y for the sign bit).
void CompressAffine(const G1Affine& a, uint8_t out[48]);
// n points -> 48 n bytes.  Eight at a time with AVX-512 IFMA where the CPU has it (the verifier
// hashes 4 ell instance points per verification), the scalar routine otherwise and for the tail
// of fewer than eight.
void CompressAffineBatch(const G1Affine* pts, size_t n, uint8_t* out);

// k * P for a base that never changes (CRS points): 8-bit windows precomputed once, then at
// most 32 mixed additions per multiplication instead of ~255 doublings + 64 additions.
class FixedBase {
 public:
  explicit FixedBase(const G1Affine& p);
  Point Mul(const Scalar& k) const;
 private:
  std::vector<G1Affine> table_;  // 32 x 255
};

// common.MultiExp: every MSM of the protocol code funnels through
// here and runs on the GPU (curdle_msm_g1).  Throws std::runtime_error on a length
// mismatch or a device error, with the Go error text.
Point MultiExp(const std::vector<G1Affine>& points, const std::vector<Scalar>& scalars);
// Several MSMs in one GPU pass (curdle_msm_g1_batch): results[i] = MultiExp(points[i], scalars[i]).
std::vector<Point> MultiExpBatch(const std::vector<const std::vector<G1Affine>*>& points,
                                 const std::vector<const std::vector<Scalar>*>& scalars);

// One scalar vector against several base sets (curdle_msm_g1_multi): results[i] = MultiExp(*sets[i],
// scalars), with the scalars uploaded, recoded and bucket-sorted once for all sets
// (samemultiscalarargument.go:64-70; curdleproof.go:110,:114).
std::vector<Point> MultiExpShared(const std::vector<const std::vector<G1Affine>*>& sets,
                                  const std::vector<Scalar>& scalars);

// While one of these lives on a thread, the three functions above send that thread's MSMs to the constant-time
// primitive (curdle_msm_g1_ct, _ct_batch, _ct_multi at scalar_bits = 255) instead of the bucket MSM: same results, bit
// for bit.  Thread-local and scoped: other threads, and this one afterwards, are as before.  A backend without the
// primitive makes the first such MSM throw MsmError(CURDLE_ENODEV); Available() says so beforehand.
class ConstantTimeMsmScope {
 public:
  ConstantTimeMsmScope();
  ~ConstantTimeMsmScope();
  ConstantTimeMsmScope(const ConstantTimeMsmScope&) = delete;
  ConstantTimeMsmScope& operator=(const ConstantTimeMsmScope&) = delete;
  static bool Available();

 private:
  bool prev_;
};
// bucket-MSM calls | their pairs | constant-time calls | their pairs, counted in the three functions above when the
// call they made succeeded; one scalar vector against k sets of n counts k n pairs.
void ReadMsmCounters(unsigned long long out[4]);

// The second switch of the constant-time prover (curdle_prove_ct), thread-local and scoped like the first: while one
// lives on a thread, the prover's operations on secrets that are NOT MSMs leave the host too -- its scalar
// multiplications by r_k, k, r_a, r_b, r_t, r_u become MSMs of one and two terms (curdleproofs.cpp), its gathers by the
// secret permutation go through PermuteSecret to the oblivious gather, and an MSM pair whose first half alone would be an
// unblinded commitment is ONE MSM.  Without it every site runs as it always did.  Meant to live inside a
// ConstantTimeMsmScope: alone it would send the new MSMs to the bucket MSM.
class SecretOpsScope {
 public:
  SecretOpsScope();
  ~SecretOpsScope();
  SecretOpsScope(const SecretOpsScope&) = delete;
  SecretOpsScope& operator=(const SecretOpsScope&) = delete;
  static bool Active();     // on this thread
  static bool Available();  // the backend has the gather and the constant-time MSMs

 private:
  bool prev_;
};
// common.Permute for a SECRET permutation: out[i] = vs[perm[i]].  Under a SecretOpsScope one curdle_fr_permute_ct (every
// output reads every record; no address is made of perm; a backend without it: MsmError(CURDLE_ENODEV)); otherwise the
// indexed gather the prover always ran.  perm.size() == vs.size(), entries below it (the caller's check).
std::vector<Scalar> PermuteSecret(const std::vector<Scalar>& vs, const std::vector<uint32_t>& perm);
// Calls of Point::Mul on the calling thread since it started (a thread-local counter, no atomic: the batch verifiers
// multiply on many threads): the diagnostic that shows which route a Prove took.
unsigned long long PointMulCalls();

// out[i] = addends[i] + scalars[i] * points[i]; scalars.size() is points.size(), or 1 for one
// scalar shared by all; addends may be null.  The independent scalar multiplications that
// dominate the prover: a batch of at least kScalarMulBatchMin goes to
// the GPU (curdle_g1_scalar_mul_batch), smaller ones run on the host one by one.
// Under a SecretOpsScope the scalars are secrets: every size goes to curdle_g1_scalar_mul_batch_ex under
// CURDLE_G1_MUL_CONSTANT_TIME (which takes no addends), the same records bit for bit.
static constexpr size_t kScalarMulBatchMin = 24;
std::vector<G1Affine> ScalarMulBatch(const std::vector<G1Affine>& points, const std::vector<Scalar>& scalars,
                                     const std::vector<G1Affine>* addends = nullptr);

// The third switch: k provers in lockstep.  A Lockstep is a group of `members` threads that all make the same sequence
// of funnel calls with the same shapes (k Proves over one CRS at one ell do); while a LockstepScope lives on a member's
// thread, a call of MultiExp, MultiExpBatch, MultiExpShared, ScalarMulBatch -- and PermuteSecret under a SecretOpsScope
// -- does not go to the device from that thread: it is handed to the group as a request (the funnel, the shapes, the
// pointers) and the thread waits.  When every LIVE member has handed in its next request, one of the waiting threads
// checks that funnels, shapes and the two constant-time switches agree (they are read on the member threads), issues
// ONE coalesced call, member-major -- or as few as fit the primitive's limits, split by whole members -- hands each
// member its results and wakes them:
//   the three MSM funnels   one curdle_msm_g1_batch over all members' MSMs (a shared-scalar request is its k MSMs with
//                           the scalar vector repeated); under a ConstantTimeMsmScope one curdle_msm_g1_ct_batch at 255 bits
//   ScalarMulBatch          one curdle_g1_scalar_mul_batch over the concatenation with per-point scalars (a member's
//                           shared scalar is replicated); under a SecretOpsScope, where the scalars are secrets, one
//                           curdle_g1_scalar_mul_batch_ex under CURDLE_G1_MUL_CONSTANT_TIME (no addends there)
//   PermuteSecret           one curdle_fr_permute_ct_batch (without a SecretOpsScope: the member's own indexed gather,
//                           no rendezvous)
// Results are, bit for bit, those of the member's own call.  A member is live from the group's construction until its
// LockstepScope dies (an exception leaves through the destructor) or Leave(member) says it will never start: the others
// then go on without it, and a step that was only waiting for it runs.  Funnels, shapes or switches that disagree, or a
// failed device call, fail the STEP: every member that handed in a request for it throws the same MsmError, and nobody
// is left waiting.  Under the constant-time switches every concatenated host copy of scalars, entries and gathered
// records is explicit_bzero-ed on every way out.  ReadMsmCounters counts a coalesced call once, with all its pairs.
class Lockstep {
 public:
  explicit Lockstep(size_t members);
  ~Lockstep();
  Lockstep(const Lockstep&) = delete;
  Lockstep& operator=(const Lockstep&) = delete;
  void Leave(size_t member);                  // a member that never gets a scope (its thread could not be started)
  unsigned long long DeviceCalls() const;     // coalesced calls issued so far
  unsigned long long Disagreements() const;   // steps failed because funnels, shapes or switches differed
  struct Request;                             // algebra.cpp

 private:
  friend class LockstepScope;
  friend struct LockstepAccess;
  void Rendezvous(size_t member, Request* r);  // throws MsmError when the step failed
  void RunStep();
  mutable std::mutex mu_;
  std::condition_variable cv_;
  std::vector<Request*> reqs_;   // per member: its request of the current step, or null
  std::vector<char> live_flag_;
  size_t live_, arrived_ = 0;
  unsigned long long step_ = 0, device_calls_ = 0, disagreements_ = 0;
};

class LockstepScope {
 public:
  LockstepScope(Lockstep& group, size_t member);
  ~LockstepScope();
  LockstepScope(const LockstepScope&) = delete;
  LockstepScope& operator=(const LockstepScope&) = delete;

 private:
  Lockstep* prev_group_;
  size_t prev_member_;
};

// The fourth switch: the constant-time MSMs over RESIDENT tables of PUBLIC bases.  Every base of the prover's MSMs is
// public and known before its scalars exist -- a CRS point, a record of the instance vectors, the point at infinity,
// the aggregates R and S -- so it can live in a curdle_ct_bases table (csrc/msm_ct_bases_api.hip), over which a lane walks
// chunk_bits steps instead of 255.
//
// ResidentBases is the registry of such tables for one Prove: an ordered list of at most kMaxSets sets at one
// chunk_bits, and an index of every 96-byte G1Affine record by value -- a hash map from the record to its global row
// (set s covers the rows [B_s, B_s + n_s)), the first occurrence wins, the all-zero record (infinity) included.  The
// points are public, so hashing them is fine; nothing about a scalar ever reaches the map.  Add creates a table and
// owns it; AddShared names a table someone else owns (the prover handle's CRS set) and only indexes it.  Not
// thread-safe: one registry per call.
class ResidentBases {
 public:
  static constexpr size_t kMaxSets = 4;  // CURDLE_CT_BASES_MAX_SETS
  // 0 is the library's choice, 16; the width in force is what every table is created with, so 0 never reaches a creator.
  static unsigned ChunkBitsOf(unsigned chunk_bits) { return chunk_bits ? chunk_bits : 16; }
  explicit ResidentBases(unsigned chunk_bits);
  ~ResidentBases();                             // frees the sets Add made
  ResidentBases(const ResidentBases&) = delete;
  ResidentBases& operator=(const ResidentBases&) = delete;
  // A new set over `points`.  Throws MsmError: a fifth set (CURDLE_EINVAL), a backend without the tables
  // (CURDLE_ENODEV), or curdle_ct_bases_create's own refusal.
  void Add(const std::vector<G1Affine>& points);
  // A set over `points` whose table `handle` (a curdle_ct_bases* over exactly these points at this registry's
  // chunk_bits) belongs to the caller and outlives the registry.
  void AddShared(const void* handle, const std::vector<G1Affine>& points);
  // A registry that declines: it stays empty, ResidentBasesScope::Active() does not name it (so the prover changes
  // nothing), and the funnel only counts the calls under its scope as having taken the old path.  What a prover handle
  // runs under when a Prove's instance vectors do not fit a table.
  void Decline() { declined_ = true; }
  bool Declined() const { return declined_; }
  size_t Sets() const { return handles_.size(); }
  size_t Rows() const { return rows_; }
  unsigned ChunkBits() const { return chunk_bits_; }                       // the width in force
  unsigned Chunks() const { return (255 + chunk_bits_ - 1) / chunk_bits_; }  // C = Cb at 255 bits
  bool Find(const G1Affine& p, uint32_t* row) const;            // the record's global row
  const void* const* Handles() const { return handles_.data(); }

 private:
  struct Impl;
  void Index(const std::vector<G1Affine>& points);
  unsigned chunk_bits_;
  bool declined_ = false;
  size_t rows_ = 0;
  std::vector<const void*> handles_;
  std::vector<char> owned_;
  Impl* map_;
};

// While one lives on a thread that is also under a ConstantTimeMsmScope and NOT in a LockstepScope, MultiExp,
// MultiExpBatch and MultiExpShared resolve every base of a call to a row of `bases`; if all resolve, the call's terms
// fit one pass (pairs x Cb <= 65,536, or the knob PROVE_RESIDENT_TERMS when a test lowered it) and it has at most 4,096
// MSMs, the call is ONE curdle_msm_g1_ct_bases_sets_batch at 255 bits (MultiExpShared repeats the scalar vector per set in
// a concatenated copy that is cleared on every way out).  Otherwise the call takes the path it takes without this
// scope, untouched.  The route depends on shapes and public points only.  Same results, bit for bit.
class ResidentBasesScope {
 public:
  explicit ResidentBasesScope(ResidentBases& bases);
  ~ResidentBasesScope();
  ResidentBasesScope(const ResidentBasesScope&) = delete;
  ResidentBasesScope& operator=(const ResidentBasesScope&) = delete;
  static ResidentBases* Active();  // the registry this thread's MSMs consult, or null (also for one that declines)
  static bool Available();         // the backend has the tables and the call over several of them

 private:
  ResidentBases* prev_;
};
// resident calls | their pairs | calls under an active scope (and a ConstantTimeMsmScope, outside a lockstep group) that
// took the old path | their pairs; counted when the call they made succeeded.
void ReadResidentCounters(unsigned long long out[4]);

// k jobs in lockstep: job(i) for i < members, in groups of at most group_size, ONE std::thread per member of a group (a
// member blocked at the rendezvous cannot be suspended, so no pool) and each under a LockstepScope of its group -- with
// constant_time also under a ConstantTimeMsmScope and a SecretOpsScope -- and on the device the calling thread has
// selected.  The calling thread only starts and joins.  A job must not throw.  A member whose thread cannot be started
// gets could_not_start(i) on the calling thread and leaves its group.  Returns the groups run, the coalesced device
// calls they made, and the two things that can go wrong without the device's doing: steps at which the members'
// requests disagreed, and members that could not be started.
struct LockstepRun {
  size_t groups = 0;
  unsigned long long device_calls = 0;
  unsigned long long disagreements = 0;
  size_t not_started = 0;
};
LockstepRun RunInLockstep(size_t members, size_t group_size, bool constant_time, const std::function<void(size_t)>& job,
                          const std::function<void(size_t)>& could_not_start);

}  // namespace alg
}  // namespace curdle
