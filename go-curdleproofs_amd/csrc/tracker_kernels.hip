// The check of IsValidWhiskTrackerProof (the reference's whisk/whisk.go:116-147) for a batch of
// tracker proofs: for member i with decoded records rG, krG, kG, A, B and scalars s, c (the
// proof's response and the transcript's challenge),
//
//     A' = s G  + c kG   == A      (whisk.go:136-139)
//     B' = s rG + c krG  == B      (:141-144)
//
// Each equation is one joint (Straus) double-scalar multiplication on one quad (quad28.h): s and
// c through the GLV split (glv_quad.h), ONE chain of 127 doublings over the four points
// {P, phi(P), Q, phi(Q)} with at most one addition from P's table and one from Q's per bit.  The
// two equations of a member run on the two quads of one eight-lane group, side by side, over the
// same scalars, so they take the same branches.  Equality is decided on the device, exactly:
// -A (or -B) is added at the end and the sum must be infinity -- quad28.h add() handles equal
// and opposite operands, and infinity on either side.  One byte per member leaves the device.
#include <hip/hip_runtime.h>

#include "../../include/curdle_msm.h"
#include "fp28.h"
#include "quad28.h"
#include "glv_quad.h"
#include "msm_kernels.h"

namespace curdle {

using d28::F28;

static constexpr int kBlock = 256;

namespace {
__device__ __forceinline__ void load_scalar(Fr& k, const uint4* __restrict__ src) {
  const uint4 lo = src[0], hi = src[1];
  k.l[0] = lo.x; k.l[1] = lo.y; k.l[2] = lo.z; k.l[3] = lo.w;
  k.l[4] = hi.x; k.l[5] = hi.y; k.l[6] = hi.z; k.l[7] = hi.w;
}

// The table of a GLV chain for a point that may be infinity (then every entry is infinity, and
// adding one leaves the sum as it is).
__device__ __forceinline__ void table_or_inf(F28& p1, F28& p2, F28& p3, bool finite, const F28& x, const F28& y,
                                             u32 neg_a, u32 neg_b) {
  if (finite) {
    glvq::table(p1, p2, p3, x, y, neg_a, neg_b);
  } else {
    q28::set_inf(p1);
    q28::set_inf(p2);
    q28::set_inf(p3);
  }
}
}  // namespace

// points: 5 n decoded records (gnark affine, (0, 0) = infinity), rG krG kG A B per member;
// status: their CURDLE_DECODE_* bytes; scalars: s then c per member, canonical, 8 little-endian
// words each; skip[i] != 0: member i is not to be checked (its S is not canonical).
__global__ void __launch_bounds__(kBlock, 2)
    k_tracker_check(const uint4* __restrict__ points, const uint8_t* __restrict__ status,
                    const uint4* __restrict__ scalars, const uint8_t* __restrict__ skip, G1Affine gen, u32 n,
                    uint8_t* __restrict__ out) {
  const u32 lane = blockIdx.x * kBlock + threadIdx.x;
  const u32 i = lane >> 3;
  if (i >= n) return;  // whole members leave together
  const u32 chain = (lane >> 2) & 1u;  // 0: A' = s G + c kG,  1: B' = s rG + c krG
  const size_t rec = 5 * (size_t)i;
  bool bad = skip[i] != 0;
#pragma unroll
  for (int j = 0; j < 5; j++) bad |= status[rec + j] > CURDLE_DECODE_INFINITY;
  if (bad) {  // uniform over the member: nothing of it is computed
    if ((lane & 7u) == 0) out[i] = kTrackerError;
    return;
  }
  Fr s, c;
  load_scalar(s, scalars + 4 * (size_t)i);
  load_scalar(c, scalars + 4 * (size_t)i + 2);
  u32 sa[4], sb[4], ca[4], cb[4], neg_sa, neg_sb, neg_ca, neg_cb;
  glv_split(s, sa, sb, neg_sa, neg_sb);
  glv_split(c, ca, cb, neg_ca, neg_cb);

  F28 x, y, p1, p2, p3, q1, q2, q3, p, acc;
  bool finite;
  if (chain) {
    finite = glvq::load_affine(x, y, points, rec + 0);  // rG
  } else {
    d28::from_gnark(x, gen.x.l);
    d28::from_gnark(y, gen.y.l);
    finite = true;
  }
  table_or_inf(p1, p2, p3, finite, x, y, neg_sa, neg_sb);
  finite = glvq::load_affine(x, y, points, rec + (chain ? 1 : 2));  // krG | kG
  table_or_inf(q1, q2, q3, finite, x, y, neg_ca, neg_cb);

  q28::set_inf(acc);
  glvq::shift(sa, sb);
  glvq::shift(ca, cb);
  for (int bit = 126; bit >= 0; bit--) {
    q28::dbl(acc);
    // one addition site for both tables keeps the loop body to one inlined addition and one doubling
#pragma unroll 1
    for (int t = 0; t < 2; t++) {
      const bool ba = glvq::top_bit(t ? ca : sa), bb = glvq::top_bit(t ? cb : sb);
      if (ba || bb) {
        q28::sel(p, ba && bb, t ? q3 : p3, ba ? (t ? q1 : p1) : (t ? q2 : p2));
        q28::add(acc, p);
      }
    }
    glvq::shift(sa, sb);
    glvq::shift(ca, cb);
  }
  // acc - T == infinity  <=>  acc == T, for T = A (chain 0) or B (chain 1), infinity included
  if (glvq::load_affine(x, y, points, rec + (chain ? 4 : 3))) {
    F28 yn, z;
    d28::set_zero(z);
    d28::sub<4>(yn, z, y);  // 4p - y
    q28::from_affine(p, x, yn);
    q28::add(acc, p);
  }
  const int equal = q28::is_inf(acc) ? 1 : 0;
  const int other = __shfl_down(equal, 4, 64);  // lane 8m reads the verdict of chain 1 (lane 8m + 4)
  if ((lane & 7u) == 0) out[i] = (equal && other) ? kTrackerAccept : kTrackerReject;
}

// --- the device-hashed form (curdle_whisk_is_valid_tracker_proof_batch_ex / _device): from the caller's three
// arrays to what the decoder, the transcript kernel and k_tracker_check read, with no host arithmetic ---------------

namespace {
constexpr u32 kGatherLanes = 72;  // per member: 30 record words, 38 row words, one lane for S, three idle
constexpr u32 kRecWords = 30;     // 5 records of 48 bytes
constexpr u32 kRowWords = 38;     // transcript::TapeRowWords(6 * 48)

// eight bytes from any address, as the little-endian word the transcript kernel and the decoder read; `aligned`
// (the same for the whole launch): the address is a multiple of 8 and one load does
__device__ __forceinline__ uint64_t load8(const uint8_t* __restrict__ p, bool aligned) {
  if (aligned) return *reinterpret_cast<const uint64_t*>(p);
  uint64_t v = 0;
#pragma unroll
  for (int b = 0; b < 8; b++) v |= (uint64_t)p[b] << (8 * b);
  return v;
}
}  // namespace

// Member i of the caller's arrays (trackers: rG | krG, 96 B; k_comms: kG, 48 B; proofs: A | B | S, 128 B) into
//   rec:  rG krG kG A B, the order launch_g1_decompress and launch_g1_subgroup_from_bytes read;
//   rows: 8 zero bytes | kG g1Gen krG rG A B | 8 zero bytes, the tape's row of whisk.go:131-134;
//   sc:   S as eight little-endian words at sc + 16 i (zero where S >= r), skip[i] = (S >= r).
// S is the proof's last 32 bytes as a big-endian integer; it is compared with r by the borrow of S - r over all
// eight words, whatever the bytes are (TrackerProof.FromBytes, types.go:105-117: equal to r is refused).
__global__ void __launch_bounds__(kBlock)
    k_tracker_gather(const uint8_t* __restrict__ trackers, const uint8_t* __restrict__ k_comms,
                     const uint8_t* __restrict__ proofs, const uint64_t* __restrict__ gen, u32 n,
                     uint64_t* __restrict__ rec, uint64_t* __restrict__ rows, u32* __restrict__ sc,
                     uint8_t* __restrict__ skip) {
  const u32 t = blockIdx.x * kBlock + threadIdx.x;
  const u32 i = t / kGatherLanes, j = t % kGatherLanes;
  if (i >= n) return;
  const uint8_t* tr = trackers + 96 * (size_t)i;
  const uint8_t* kc = k_comms + 48 * (size_t)i;
  const uint8_t* pf = proofs + 128 * (size_t)i;
  // every offset below is a multiple of 8: aligned arrays (the library's own upload always) take whole words
  const bool al = (((uintptr_t)trackers | (uintptr_t)k_comms | (uintptr_t)proofs) & 7u) == 0;
  if (j < kRecWords) {
    const uint8_t* src = j < 12 ? tr + 8 * j : j < 18 ? kc + 8 * (j - 12) : pf + 8 * (j - 18);
    rec[kRecWords * (size_t)i + j] = load8(src, al);
  } else if (j < kRecWords + kRowWords) {
    const u32 w = j - kRecWords;
    uint64_t v = 0;
    if (w >= 1 && w <= 36) {
      const u32 u = w - 1;  // six words each of kG, g1Gen, krG, rG, A | B
      if (u < 6) v = load8(kc + 8 * u, al);
      else if (u < 12) v = gen[u - 6];
      else if (u < 18) v = load8(tr + 48 + 8 * (u - 12), al);
      else if (u < 24) v = load8(tr + 8 * (u - 18), al);
      else v = load8(pf + 8 * (u - 24), al);
    }
    rows[kRowWords * (size_t)i + w] = v;
  } else if (j == kRecWords + kRowWords) {
    constexpr u32 kR[8] = {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u, 0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u};
    u32 l[8], borrow = 0;
#pragma unroll
    for (int w = 0; w < 8; w++) {
      const uint8_t* q = pf + 96 + 4 * (7 - w);
      l[w] = ((u32)q[0] << 24) | ((u32)q[1] << 16) | ((u32)q[2] << 8) | (u32)q[3];
      const uint64_t d = (uint64_t)l[w] - kR[w] - borrow;
      borrow = (u32)(d >> 63);
    }
    const u32 keep = 0u - borrow;  // all ones iff S < r
#pragma unroll
    for (int w = 0; w < 8; w++) sc[16 * (size_t)i + w] = l[w] & keep;
    skip[i] = (uint8_t)(1u - borrow);
  }
}

// The transcript kernel's challenge of member i (32 big-endian bytes, < r) as the eight little-endian words
// k_tracker_check reads at sc + 16 i + 8.  A member whose S was refused, or whose transcript came back with a
// non-zero status (the host settles that one), has zero scalars and is not checked.
__global__ void __launch_bounds__(kBlock)
    k_tracker_challenge(const u32* __restrict__ challenges, const uint8_t* __restrict__ tr_status, u32 n,
                        u32* __restrict__ sc, uint8_t* __restrict__ skip) {
  const u32 i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const bool failed = tr_status[i] != 0;
  const u32 keep = (skip[i] != 0 || failed) ? 0u : ~0u;
  const uint4 hi = *reinterpret_cast<const uint4*>(challenges + 8 * (size_t)i);      // bytes 0..15: the top words
  const uint4 lo = *reinterpret_cast<const uint4*>(challenges + 8 * (size_t)i + 4);  // bytes 16..31
  uint4* out = reinterpret_cast<uint4*>(sc + 16 * (size_t)i + 8);
  out[0] = make_uint4(__builtin_bswap32(lo.w) & keep, __builtin_bswap32(lo.z) & keep, __builtin_bswap32(lo.y) & keep,
                      __builtin_bswap32(lo.x) & keep);
  out[1] = make_uint4(__builtin_bswap32(hi.w) & keep, __builtin_bswap32(hi.z) & keep, __builtin_bswap32(hi.y) & keep,
                      __builtin_bswap32(hi.x) & keep);
  if (failed) {  // its S is dropped too: the member is settled on the host, nothing of it is computed here
    out[-2] = make_uint4(0, 0, 0, 0);
    out[-1] = make_uint4(0, 0, 0, 0);
    skip[i] = 1;
  }
}

hipError_t launch_tracker_gather(const uint8_t* trackers, const uint8_t* k_comms, const uint8_t* proofs, const void* gen,
                                 uint32_t n, void* rec, void* rows, void* scalars, uint8_t* skip, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_tracker_gather, dim3((unsigned)(((uint64_t)kGatherLanes * n + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                     stream, trackers, k_comms, proofs, (const uint64_t*)gen, (u32)n, (uint64_t*)rec, (uint64_t*)rows,
                     (u32*)scalars, skip);
  return hipGetLastError();
}

hipError_t launch_tracker_challenge(const void* challenges, const uint8_t* tr_status, uint32_t n, void* scalars,
                                    uint8_t* skip, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_tracker_challenge, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, (const u32*)challenges,
                     tr_status, (u32)n, (u32*)scalars, skip);
  return hipGetLastError();
}

hipError_t launch_tracker_check(const void* points, const uint8_t* status, const void* scalars, const uint8_t* skip,
                                const G1Affine& gen, uint32_t n, uint8_t* out, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_tracker_check, dim3((unsigned)(((uint64_t)8 * n + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream,
                     (const uint4*)points, status, (const uint4*)scalars, skip, gen, (u32)n, out);
  return hipGetLastError();
}

}  // namespace curdle
