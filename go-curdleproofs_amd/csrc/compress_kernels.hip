// Batched normalisation and compression of G1 points on the GPU: n points in memory -> n x 48 bytes of gnark's
// compressed encoding (G1Affine.Bytes; what curdle_g1_compress writes for one point on the host).  The way out of
// the device for a group element: until this kernel every result of a point kernel left as XYZZ and the host
// normalised it; the batched tracker-proof generator (tracker_api.hip) hashes and emits kG, A and B from here.
//
// Three input forms, the template parameter:
//   kCompressJac   gnark G1Jac, 18 Montgomery u64 limbs (X, Y, Z): x = X / Z^2, y = Y / Z^3; Z = 0 is infinity;
//   kCompressXyzz  G1XYZZ in gnark limbs, as k_scalar_mul_batch_quad writes it: x = X / ZZ, y = Y / ZZZ; ZZ = 0 is
//                  infinity;
//   kCompressAffine gnark G1Affine, 96 bytes, as k_g1_normalize writes it: both coordinates zero is infinity.  Internal
//                  (no CURDLE_G1_FORM_* value): the fixed-base calls (fbase_api.hip) normalise their XYZZ results with
//                  ONE shared inversion per wave and encode the records here, where NOTHING is inverted.
// Per point: infinity -> 0xC0 and 47 zero bytes, whatever X and Y hold.  Otherwise ONE inversion by Fermat
// (invert28.h): 381 squarings and 120 products, table included.
// Then x and y leave Montgomery form, x is written big-endian, and the flag is 0xA0 if y > (p-1)/2, else 0x80.
//
// ONE LANE per point, not a quad: the chain is a field exponentiation, which quad28.h cannot shorten (its four
// lanes share the four independent products of a GROUP-law step; an exponentiation has one product per step), so
// four lanes would run the same chain four times.  One lane gives the same latency at a quarter of the lanes, and
// the 196,608 points of a full generator pass fit three waves per SIMD instead of twelve.  No inversion is shared
// between points: nothing of one point can reach another.  No LDS, no scratch; plain vector loads and stores.
#include <hip/hip_runtime.h>

#include "../../include/curdle_msm.h"
#include "fp28.h"
#include "invert28.h"
#include "quad28.h"
#include "subgroup28.h"
#include "msm_kernels.h"

namespace curdle {

namespace {

__device__ __forceinline__ u32 kHalfPm1(int i) {  // (p - 1) / 2
  constexpr u32 t[12] = {0xffffd555u, 0xdcff7fffu, 0x58a9ffffu, 0x0f55ffffu, 0x7b587b12u, 0xb3986950u,
                         0x79c2895fu, 0xb23ba5c2u, 0x21a5d66bu, 0x258dd3dbu, 0x1cbff34du, 0x0d0088f5u};
  return t[i];
}
// One coordinate, 12 words at any address; `al` (the same for the whole launch): the address is a multiple of 16.
__device__ __forceinline__ void load12(u32 w[12], const uint8_t* __restrict__ p, bool al) {
  if (al) {
    d28::load_words<12>(w, p);
    return;
  }
#pragma unroll
  for (int k = 0; k < 12; k++)
    w[k] = (u32)p[4 * k] | ((u32)p[4 * k + 1] << 8) | ((u32)p[4 * k + 2] << 16) | ((u32)p[4 * k + 3] << 24);
}
// ... into internal form; returns whether any word is set
__device__ __forceinline__ bool load_coord(F28& r, const uint8_t* __restrict__ p, bool al) {
  u32 w[12], any = 0;
  load12(w, p, al);
#pragma unroll
  for (int k = 0; k < 12; k++) any |= w[k];
  d28::from_gnark(r, w);
  return any != 0;
}

}  // namespace

template <int FORM>
__global__ void __launch_bounds__(kBlock, 2)
    k_g1_compress(const uint8_t* __restrict__ in, u32 n, uint8_t* __restrict__ out) {
  constexpr size_t kStride = FORM == kCompressJac ? 144 : (FORM == kCompressXyzz ? 192 : 96);
  const u32 i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint8_t* src = in + kStride * (size_t)i;
  uint8_t* dst = out + 48 * (size_t)i;
  const bool al_in = ((uintptr_t)in & 15u) == 0, al_out = ((uintptr_t)out & 3u) == 0;
  // the 12 big-endian words of an encoding, most significant first in memory
  auto put = [&](const u32 w[12]) {
#pragma unroll
    for (int k = 0; k < 12; k++) {
      const u32 v = w[11 - k];
      if (al_out) {
        reinterpret_cast<u32*>(dst)[k] = __builtin_bswap32(v);
      } else {
        dst[4 * k] = (uint8_t)(v >> 24);
        dst[4 * k + 1] = (uint8_t)(v >> 16);
        dst[4 * k + 2] = (uint8_t)(v >> 8);
        dst[4 * k + 3] = (uint8_t)v;
      }
    }
  };
  u32 xw[12], yw[12];
  F28 d, inv, a, c;
  if constexpr (FORM == kCompressAffine) {
    const bool any_x = load_coord(a, src, al_in), any_y = load_coord(c, src + 48, al_in);
    if (!any_x && !any_y) {
#pragma unroll
      for (int k = 0; k < 11; k++) xw[k] = 0;
      xw[11] = 0xc0000000u;
      return put(xw);
    }
    to_canonical(xw, a);
    to_canonical(yw, c);
    const bool larger = cmp12([&](int k) { return yw[k]; }, [](int k) { return kHalfPm1(k); }) > 0;
    xw[11] |= larger ? 0xa0000000u : 0x80000000u;
    return put(xw);
  }
  // the denominator: Z, or ZZ ZZZ (then 1 / ZZ = ZZZ / d and 1 / ZZZ = ZZ / d)
  const bool finite = load_coord(d, src + 96, al_in);  // Z | ZZ
  if (!finite) {
#pragma unroll
    for (int k = 0; k < 11; k++) xw[k] = 0;
    xw[11] = 0xc0000000u;
    return put(xw);
  }
  if constexpr (FORM == kCompressXyzz) {
    load_coord(a, src + 144, al_in);
    d28::mul(d, d, a);
  }
  invert(inv, d);
  if constexpr (FORM == kCompressJac) {
    d28::sqr(a, inv);       // 1 / Z^2
    d28::mul(c, a, inv);    // 1 / Z^3
  } else {
    load_coord(d, src + 144, al_in);
    d28::mul(a, inv, d);    // 1 / ZZ
    load_coord(d, src + 96, al_in);
    d28::mul(c, inv, d);    // 1 / ZZZ
  }
  load_coord(d, src, al_in);
  d28::mul(a, a, d);        // x
  load_coord(d, src + 48, al_in);
  d28::mul(c, c, d);        // y
  to_canonical(xw, a);
  to_canonical(yw, c);
  const bool larger = cmp12([&](int k) { return yw[k]; }, [](int k) { return kHalfPm1(k); }) > 0;
  xw[11] |= larger ? 0xa0000000u : 0x80000000u;
  put(xw);
}

hipError_t launch_g1_compress(const void* in, int form, uint32_t n, uint8_t* out, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  if (form != kCompressJac && form != kCompressXyzz && form != kCompressAffine) return hipErrorInvalidValue;
  const dim3 grid((n + kBlock - 1) / kBlock), block(kBlock);
  if (form == kCompressJac)
    hipLaunchKernelGGL(k_g1_compress<kCompressJac>, grid, block, 0, stream, (const uint8_t*)in, n, out);
  else if (form == kCompressXyzz)
    hipLaunchKernelGGL(k_g1_compress<kCompressXyzz>, grid, block, 0, stream, (const uint8_t*)in, n, out);
  else
    hipLaunchKernelGGL(k_g1_compress<kCompressAffine>, grid, block, 0, stream, (const uint8_t*)in, n, out);
  return hipGetLastError();
}

}  // namespace curdle
