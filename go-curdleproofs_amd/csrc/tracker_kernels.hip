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

hipError_t launch_tracker_check(const void* points, const uint8_t* status, const void* scalars, const uint8_t* skip,
                                const G1Affine& gen, uint32_t n, uint8_t* out, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_tracker_check, dim3((unsigned)(((uint64_t)8 * n + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream,
                     (const uint4*)points, status, (const uint4*)scalars, skip, gen, (u32)n, out);
  return hipGetLastError();
}

}  // namespace curdle
