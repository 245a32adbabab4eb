// The field inversion of the point kernels that normalise: d^(p-2) by Fermat, on the fixed 3-bit windows of the
// decoder's square root.  The exponent is the same for every lane, so the digit is wave-uniform and picks one of
// seven call sites: 381 squarings and 120 products, table included.  Included by compress_kernels.hip (one
// inversion per point) and normalize_kernels.hip (one per group of points); the code is the compression kernel's,
// moved here unchanged.
#pragma once
#include <hip/hip_runtime.h>

#include "fp28.h"

namespace curdle {

namespace {

__device__ __forceinline__ u32 kInvExp(int i) {  // p - 2, 381 bits
  constexpr u32 t[12] = {0xffffaaa9u, 0xb9feffffu, 0xb153ffffu, 0x1eabfffeu, 0xf6b0f624u, 0x6730d2a0u,
                         0xf38512bfu, 0x64774b84u, 0x434bacd7u, 0x4b1ba7b6u, 0x397fe69au, 0x1a0111eau};
  return t[i];
}
// the top window of p - 2 (bits 380..378) is 6: the chain below starts from d^6
static_assert(((0x1a0111eau >> 26) & 7u) == 6u, "top window of p - 2");

// d^(p-2): left to right over 127 windows of 3 bits
__device__ __forceinline__ void invert(d28::F28& y, const d28::F28& d) {
  d28::F28 t2, t3, t4, t5, t6, t7;
  d28::sqr(t2, d);
  d28::mul(t3, t2, d);
  d28::sqr(t4, t2);
  d28::mul(t5, t4, d);
  d28::sqr(t6, t3);
  d28::mul(t7, t6, d);
  y = t6;  // window 126
  for (int w = 125; w >= 0; w--) {
    d28::sqr_inl(y, y);
    d28::sqr_inl(y, y);
    d28::sqr_inl(y, y);
    const int bit = 3 * w;
    u32 e = kInvExp(bit >> 5) >> (bit & 31);
    if ((bit & 31) > 29) e |= kInvExp((bit >> 5) + 1) << (32 - (bit & 31));
    switch (e & 7u) {
      case 1: d28::mul(y, y, d); break;
      case 2: d28::mul(y, y, t2); break;
      case 3: d28::mul(y, y, t3); break;
      case 4: d28::mul(y, y, t4); break;
      case 5: d28::mul(y, y, t5); break;
      case 6: d28::mul(y, y, t6); break;
      case 7: d28::mul(y, y, t7); break;
      default: break;
    }
  }
}

}  // namespace

}  // namespace curdle
