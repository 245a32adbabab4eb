// Membership checks for G1 points that arrive IN MEMORY, in gnark's affine layout: the instance
// vectors of curdleproof.Verify (curdleproof.go:199-207 takes []G1Affine from its
// caller and checks nothing) and any base array handed to the MSM.  Points that arrive as bytes are
// checked by the decoder (decode_kernels.hip); these were checked by nothing, and every fast path of
// the library splits scalars with an endomorphism that is multiplication by lambda on G1 only.
// Per point, in this order:
//   all 24 words zero            -> infinity (gnark's IsInfinity)
//   X or Y >= p as an integer    -> not a field element
//   y^2 != x^3 + 4               -> not on the curve.  The group law for a = 0 never uses b, so a point
//                                   of y^2 = x^3 + b' runs through every kernel without a trace: this
//                                   equation is the only thing that stops it
//   [z^2] phi(P) + P != inf      -> not in the prime-order subgroup (subgroup28.h, the decoder's test)
// Five field products for the first three steps, ~1,300 for the last.
#include <hip/hip_runtime.h>

#include "../../include/curdle_msm.h"
#include "fp28.h"
#include "quad28.h"
#include "subgroup28.h"
#include "msm_kernels.h"

namespace curdle {

// QUAD: four adjacent lanes per point.  They read the point and decide range and curve equation
// redundantly, so every verdict before the subgroup test is uniform over the quad and whole quads
// leave together: q28::dbl / q28::add exchange data across the quad and never run with part of one gone.
// SUB = false is the five products alone and carries none of the point arithmetic's registers (nor its LDS).
template <bool QUAD, bool SUB>
__global__ void __launch_bounds__(kBlock, QUAD ? 2 : CURDLE_LANE_WAVES)
    k_g1_check_affine(const u32* __restrict__ pts, u32 n, uint8_t* __restrict__ status) {
  // x and y wait in LDS (limb-major: conflict-free) while the subgroup test runs, as in k_g1_decompress
  __shared__ u32 sh_x[SUB ? d28::N : 1][kBlock];
  __shared__ u32 sh_y[SUB ? d28::N : 1][kBlock];
  const u32 tid = threadIdx.x;
  const u32 lane = blockIdx.x * kBlock + tid;
  const u32 i = QUAD ? lane >> 2 : lane;
  const bool writer = !QUAD || (tid & 3u) == 0;
  if (i >= n) return;  // whole quads leave together
  u32 w[24];
  const uint2* p2 = reinterpret_cast<const uint2*>(pts + (size_t)i * 24);  // gnark's words are uint64: 8-byte aligned
#pragma unroll
  for (int k = 0; k < 12; k++) {
    const uint2 v = p2[k];
    w[2 * k] = v.x;
    w[2 * k + 1] = v.y;
  }
  auto done = [&](uint8_t code) {
    if (writer) status[i] = code;
  };
  u32 any = 0;
#pragma unroll
  for (int k = 0; k < 24; k++) any |= w[k];
  if (!any) return done(CURDLE_DECODE_INFINITY);
  if (cmp12([&](int k) { return w[k]; }, [](int k) { return kP32(k); }) >= 0 ||
      cmp12([&](int k) { return w[12 + k]; }, [](int k) { return kP32(k); }) >= 0)
    return done(CURDLE_DECODE_BAD_ENCODING);

  F28 x, y, lhs, rhs, c;
  d28::from_gnark(x, w);
  d28::from_gnark(y, w + 12);
  d28::sqr(lhs, y);  // < 2p, normalised
  d28::sqr(rhs, x);
  d28::mul(rhs, rhs, x);
#pragma unroll
  for (int k = 0; k < d28::N; k++) c.l[k] = kFour(k);
  d28::add(rhs, rhs, c);  // x^3 + 4 < 3p
  // canonical forms (the lazily-reduced values are not unique): both sides are internal form already,
  // so conditional subtractions do it and no product is spent
  d28::cond_sub_pshl<1>(rhs);
  d28::canonical_lt2p(rhs);
  d28::canonical_lt2p(lhs);
  u32 diff = 0;
#pragma unroll
  for (int k = 0; k < d28::N; k++) diff |= lhs.l[k] ^ rhs.l[k];
  if (diff) return done(CURDLE_DECODE_NOT_ON_CURVE);

  if constexpr (SUB) {
#pragma unroll
    for (int k = 0; k < d28::N; k++) {
      sh_x[k][tid] = x.l[k];
      sh_y[k][tid] = y.l[k];
    }
    if (!in_subgroup<QUAD>(x, y, sh_x, sh_y, tid)) return done(CURDLE_DECODE_NOT_IN_SUBGROUP);
  }
  done(CURDLE_DECODE_OK);
}

hipError_t launch_g1_check_affine(const uint32_t* pts, uint32_t n, int subgroup_check, uint8_t* status, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  // four lanes per point while even that is at most one round of the chip, as launch_g1_decompress
  if (subgroup_check && (uint64_t)n * 4 <= quad_max_lanes())
    hipLaunchKernelGGL((k_g1_check_affine<true, true>), dim3((4 * n + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, pts, n,
                       status);
  else if (subgroup_check)
    hipLaunchKernelGGL((k_g1_check_affine<false, true>), dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, pts, n,
                       status);
  else
    hipLaunchKernelGGL((k_g1_check_affine<false, false>), dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, pts, n,
                       status);
  return hipGetLastError();
}

}  // namespace curdle
