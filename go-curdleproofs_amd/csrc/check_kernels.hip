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

// The same check for gnark G1Jac values (18 words: X, Y, Z in Montgomery form), the layout of the verifier's M, of
// crs.H / Gt / Gu and of every []G1Jac a Go caller holds.  Per point, in this order:
//   Z all zero words                -> infinity (gnark's rule for G1Jac: X and Y are not looked at)
//   X, Y or Z >= p as an integer    -> not a field element
//   Y^2 != X^3 + 4 Z^6              -> not on the curve (the affine equation, homogeneous in Z)
//   [z^2] phi(P) + P != inf         -> not in the prime-order subgroup
// The subgroup test runs FROM PROJECTIVE COORDINATES: (X, Y, Z) is the XYZZ point (X, Y, Z^2, Z^3), and Z^2, Z^3 are
// products the curve equation spends anyway (Z^6 = (Z^3)^2).  Nothing is inverted: an inversion is ~570 products beside
// the test's ~1,300, the projective form costs the one-lane build five full additions where the affine kernel has mixed
// ones (5 x 4 products) and both builds one full last addition, ~25 products; on quads an addition is four product
// steps whatever its operand.  Ten products (three conversions, seven for the equation) before the test, against the
// affine kernel's five.
// What waits for the last addition: on quads each lane parks its own coordinate of P in LDS (14 words a lane, half
// the affine kernel's); the one-lane build would need 56 words a lane (56 KB a block) and reads the point again
// instead -- five products in 1,300.
// Registers (VGPRs / scratch bytes a lane): quad 137 / 0, one lane 256 / 928, no subgroup test 102 / 0; the affine
// builds keep 150 / 0, 256 / 80, 74 / 0.  The one-lane build's scratch is the ADDEND, not the loop: phi(P), then
// [z] phi(P), is a whole XYZZ point (56 words, the affine kernel's addend is x and y) that must outlive the out-of-line
// products of 63 doublings, and the compiler keeps it in scratch -- stored once per multiplication, read back by the
// five additions of each.  ~620 scratch words moved per point beside ~1,300 products of ~400 instructions.
// Measured against curdle_g1_check_batch on as many points from host memory (profiles/r11_batch_checked.json):
// 1.02x at 1,024 points, 0.98x at 32,768 (both on quads), 1.09x at 32,769 and 1.16x at 2^20 (one lane; the points are
// 1.5x the bytes).
__device__ __forceinline__ void jac_words(u32* w, const u32* __restrict__ pts, u32 i) {
  const uint2* p2 = reinterpret_cast<const uint2*>(pts + (size_t)i * 36);  // gnark's words are uint64: 8-byte aligned
#pragma unroll
  for (int k = 0; k < 18; k++) {
    const uint2 v = p2[k];
    w[2 * k] = v.x;
    w[2 * k + 1] = v.y;
  }
}
// (X, Y, Z) in gnark's words -> the XYZZ point (X, Y, Z^2, Z^3) in internal form, every coordinate < 2p
__device__ __forceinline__ void jac_to_xyzz(F28& x, F28& y, F28& zz, F28& zzz, const u32* w) {
  F28 z;
  d28::from_gnark(x, w);
  d28::from_gnark(y, w + 12);
  d28::from_gnark(z, w + 24);
  d28::sqr(zz, z);
  d28::mul(zzz, zz, z);
}

template <bool QUAD, bool SUB>
__global__ void __launch_bounds__(kBlock, QUAD ? 2 : CURDLE_LANE_WAVES)
    k_g1_check_jac(const u32* __restrict__ pts, u32 n, uint8_t* __restrict__ status) {
  __shared__ u32 sh_p[SUB && QUAD ? d28::N : 1][kBlock];  // this lane's coordinate of P (limb-major: conflict-free)
  const u32 tid = threadIdx.x;
  const u32 lane = blockIdx.x * kBlock + tid;
  const u32 i = QUAD ? lane >> 2 : lane;
  const bool writer = !QUAD || (tid & 3u) == 0;
  if (i >= n) return;  // whole quads leave together
  auto done = [&](uint8_t code) {
    if (writer) status[i] = code;
  };
  // every lane of a quad reads the same words: the verdicts before the subgroup test are uniform over the quad
  u32 w[36];
  jac_words(w, pts, i);
  u32 any = 0;
#pragma unroll
  for (int k = 24; k < 36; k++) any |= w[k];
  if (!any) return done(CURDLE_DECODE_INFINITY);
  if (cmp12([&](int k) { return w[k]; }, [](int k) { return kP32(k); }) >= 0 ||
      cmp12([&](int k) { return w[12 + k]; }, [](int k) { return kP32(k); }) >= 0 ||
      cmp12([&](int k) { return w[24 + k]; }, [](int k) { return kP32(k); }) >= 0)
    return done(CURDLE_DECODE_BAD_ENCODING);
  F28 x, y, zz, zzz;
  jac_to_xyzz(x, y, zz, zzz, w);
  {
    F28 lhs, rhs, z6, c;
    d28::sqr(lhs, y);  // < 2p, normalised
    d28::sqr(rhs, x);
    d28::mul(rhs, rhs, x);
    d28::sqr(z6, zzz);
#pragma unroll
    for (int k = 0; k < d28::N; k++) c.l[k] = kFour(k);
    d28::mul(z6, z6, c);
    d28::add(rhs, rhs, z6);  // X^3 + 4 Z^6 < 4p
    // canonical forms, as in k_g1_check_affine: the lazily-reduced values are not unique
    d28::cond_sub_pshl<1>(rhs);
    d28::canonical_lt2p(rhs);
    d28::canonical_lt2p(lhs);
    u32 diff = 0;
#pragma unroll
    for (int k = 0; k < d28::N; k++) diff |= lhs.l[k] ^ rhs.l[k];
    if (diff) return done(CURDLE_DECODE_NOT_ON_CURVE);
  }
  if constexpr (SUB) {
    // [z^2] phi(P) + P == inf, phi(X, Y, ZZ, ZZZ) = (beta X, Y, ZZ, ZZZ); |z| as in subgroup28.h
    const unsigned long long zabs = 0xd201000000010000ull;
    F28 c, bx;
#pragma unroll
    for (int k = 0; k < d28::N; k++) c.l[k] = kBeta(k);
    d28::mul(bx, x, c);
    if constexpr (QUAD) {
      X28 p{x, y, zz, zzz};
      F28 q, acc;
      q28::from_x28(q, p);
#pragma unroll
      for (int k = 0; k < d28::N; k++) sh_p[k][tid] = q.l[k];
      q28::sel(q, q28::role() == 0, bx, q);
      acc = q;
      for (int pass = 0; pass < 2; pass++) {
        q = acc;
        for (int bit = 62; bit >= 0; bit--) {
          q28::dbl(acc);
          if ((zabs >> bit) & 1ull) q28::add(acc, q);
        }
      }
#pragma unroll
      for (int k = 0; k < d28::N; k++) q.l[k] = sh_p[k][tid];
      q28::add(acc, q);
      if (!q28::is_inf(acc)) return done(CURDLE_DECODE_NOT_IN_SUBGROUP);
    } else {
      X28 q{bx, y, zz, zzz};
      X28 acc = q;
      for (int pass = 0; pass < 2; pass++) {
        q = acc;
        for (int bit = 62; bit >= 0; bit--) {
          d28::dbl(acc);
          if ((zabs >> bit) & 1ull) d28::add(acc, q);
        }
      }
      jac_words(w, pts, i);
      jac_to_xyzz(q.x, q.y, q.zz, q.zzz, w);
      d28::add(acc, q);
      if (!d28::is_inf(acc)) return done(CURDLE_DECODE_NOT_IN_SUBGROUP);
    }
  }
  done(CURDLE_DECODE_OK);
}

// The builds and the rule that selects them are those of launch_g1_check_affine.
hipError_t launch_g1_check_jac(const uint32_t* pts, uint32_t n, int subgroup_check, uint8_t* status, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  if (subgroup_check && (uint64_t)n * 4 <= quad_max_lanes())
    hipLaunchKernelGGL((k_g1_check_jac<true, true>), dim3((4 * n + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, pts, n, status);
  else if (subgroup_check)
    hipLaunchKernelGGL((k_g1_check_jac<false, true>), dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, pts, n, status);
  else
    hipLaunchKernelGGL((k_g1_check_jac<false, false>), dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, pts, n, status);
  return hipGetLastError();
}

}  // namespace curdle
