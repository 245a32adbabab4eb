// Per-point setup of a GLV double-and-add on quads (quad28.h), shared by the batched scalar
// multiplications (group_kernels.hip k_scalar_mul_batch_quad) and the tracker-proof check
// (tracker_kernels.hip k_tracker_check).
//
// bls12_381.h glv_split writes a canonical scalar k as k P = +-k1 P +- k2 phi(P) with 127-bit
// halves k1, k2; phi(x, y) = (beta x, y).  A chain over such a split runs 127 doublings and, per
// bit, adds one entry of the point's table {+-P, +-phi(P), +-P +- phi(P)} picked by the two bits.
#pragma once
#include "bls12_381.h"
#include "fp28.h"
#include "quad28.h"

namespace curdle {
namespace glvq {

using d28::F28;

// gnark affine point -> internal affine; false for (0, 0) = infinity
__device__ __forceinline__ bool load_affine(F28& x, F28& y, const uint4* __restrict__ points, size_t i) {
  u32 w[24];
  d28::load_words<24>(w, points + i * 6);
  u32 any = 0;
#pragma unroll
  for (int j = 0; j < 24; j++) any |= w[j];
  if (!any) return false;
  d28::from_gnark(x, w);
  d28::from_gnark(y, w + 12);
  return true;
}

// The table of an affine point (x, y), not infinity, for the halves' signs neg_a / neg_b of
// glv_split: p1 = +-P, p2 = +-phi(P), p3 = p1 + p2.
__device__ __forceinline__ void table(F28& p1, F28& p2, F28& p3, const F28& x, const F28& y, u32 neg_a, u32 neg_b) {
  F28 yn, z, beta, bx;
  d28::set_zero(z);
  d28::sub<4>(yn, z, y);  // 4p - y
#pragma unroll
  for (int j = 0; j < d28::N; j++) beta.l[j] = d28::kBeta(j);
  d28::mul(bx, x, beta);
  q28::from_affine(p1, x, neg_a ? yn : y);
  q28::from_affine(p2, bx, neg_b ? yn : y);
  p3 = p1;
  q28::add(p3, p2);
}

// One step of a chain over the two 127-bit halves of a split: each half shifted left by one, so
// that its next bit (most significant first) is the top bit of word 3.  Called once before the
// first bit, which brings bit 126 up there.
__device__ __forceinline__ void shift(u32 a[4], u32 b[4]) {
#pragma unroll
  for (int j = 3; j > 0; j--) {
    a[j] = (a[j] << 1) | (a[j - 1] >> 31);
    b[j] = (b[j] << 1) | (b[j - 1] >> 31);
  }
  a[0] <<= 1;
  b[0] <<= 1;
}
__device__ __forceinline__ bool top_bit(const u32 h[4]) { return h[3] >> 31; }

}  // namespace glvq
}  // namespace curdle
