// The prime-order-subgroup test of the point kernels and what it shares with them: the block size, the rule for
// quads against single lanes, the constants in internal form and the comparison with p.  Included by
// decode_kernels.hip (points that arrive as bytes) and check_kernels.hip (points that arrive in memory); the code
// is the decoder's, moved here unchanged.
#pragma once
#include <hip/hip_runtime.h>

#include "fp28.h"
#include "quad28.h"
#include "../host/knobs.h"

namespace curdle {
// Up to this many lanes the latency-bound kernels of this file run on quads (four lanes per
// point, quad28.h); beyond it on one lane per point.  knob QUAD_MAX_LANES overrides (tuning; host/knobs.h).
static inline uint64_t quad_max_lanes() {
  return knobs::is_set(knobs::QUAD_MAX_LANES) ? (uint64_t)knobs::get(knobs::QUAD_MAX_LANES) : (uint64_t)131072;
}


using d28::F28;
using d28::X28;

static constexpr int kBlock = 256;


#ifndef CURDLE_LANE_WAVES
#define CURDLE_LANE_WAVES 2
#endif

namespace {

#define CURDLE_DEC_TABLE28(name, ...)                    \
  __device__ __forceinline__ u32 name(int i) {           \
    constexpr u32 t[d28::N] = {__VA_ARGS__};             \
    return t[i];                                         \
  }
// 2^784 mod p: a Montgomery product with it maps a canonical residue to internal form
CURDLE_DEC_TABLE28(kCanonToInt, 0x10370edu, 0x6d1c345u, 0xe243d62u, 0xec45c53u, 0x3b1d65au, 0x093317du, 0xb4f36a0u,
                   0x5d74088u, 0xc10ea72u, 0x865d118u, 0x7320a75u, 0xfd5cd50u, 0xcc8a759u, 0x000c8d4u)
// 4 in internal form (the curve constant b)
CURDLE_DEC_TABLE28(kFour, 0xd1ff2e0u, 0x6000000u, 0x00ac467u, 0x3379b48u, 0x1c84b80u, 0x0e88243u, 0x0dd9a7eu,
                   0x683dcf8u, 0x6c26d0bu, 0x4a5eec2u, 0x457663cu, 0x04b29f1u, 0x967f3e8u, 0x0015de9u)
// beta in internal form: the cube root of unity with phi(x, y) = (beta x, y) = [z^2 - 1](x, y) on G1
CURDLE_DEC_TABLE28(kBeta, 0x2421b59u, 0xbee4867u, 0x1d31002u, 0x4760184u, 0x4cc5086u, 0xc76dc00u, 0xaae891bu,
                   0xac70ad2u, 0xfe377c4u, 0xe4686b8u, 0x5ed1568u, 0x8f5a180u, 0x02b5c1fu, 0x000d1a4u)
#undef CURDLE_DEC_TABLE28

__device__ __forceinline__ u32 kP32(int i) {
  constexpr u32 t[12] = {0xffffaaabu, 0xb9feffffu, 0xb153ffffu, 0x1eabfffeu, 0xf6b0f624u, 0x6730d2a0u,
                         0xf38512bfu, 0x64774b84u, 0x434bacd7u, 0x4b1ba7b6u, 0x397fe69au, 0x1a0111eau};
  return t[i];
}

// a > b for 12-limb little-endian integers
template <class FA, class FB>
__device__ __forceinline__ int cmp12(FA a, FB b) {
  int r = 0;
#pragma unroll
  for (int i = 0; i < 12; i++) {
    const u32 x = a(i), y = b(i);
    r = x > y ? 1 : (x < y ? -1 : r);  // higher limbs decide last
  }
  return r;
}

// internal (< 32p) -> canonical residue as 12 saturated limbs
__device__ __forceinline__ void to_canonical(u32* w, const F28& a) {
  F28 one, t;
  d28::set_zero(one);
  one.l[0] = 1;
  d28::mul(t, a, one);
  d28::canonical_lt2p(t);
  d28::pack(w, t);
}

}  // namespace

// [z^2] phi(P) + P == inf for the point whose internal-form coordinates are parked in
// sh_x / sh_y [.][tid] (and passed in x, y); |z| = 0xd201000000010000, the sign cancels in
// z^2.  QUAD: the four lanes of a quad hold one coordinate each of every point (quad28.h).
template <bool QUAD>
__device__ __forceinline__ bool in_subgroup(F28& x, F28& y, u32 (*sh_x)[kBlock], u32 (*sh_y)[kBlock], u32 tid) {
  F28 c;
  F28 bx;
#pragma unroll
  for (int k = 0; k < d28::N; k++) c.l[k] = kBeta(k);
  d28::mul(bx, x, c);
  const unsigned long long zabs = 0xd201000000010000ull;
  if constexpr (QUAD) {
    // the point lives spread over the quad's four lanes (quad28.h)
    F28 q, acc;
    q28::from_affine(q, bx, y);
    acc = q;
    for (int bit = 62; bit >= 0; bit--) {
      q28::dbl(acc);
      if ((zabs >> bit) & 1ull) q28::add(acc, q);
    }
    q = acc;
    for (int bit = 62; bit >= 0; bit--) {
      q28::dbl(acc);
      if ((zabs >> bit) & 1ull) q28::add(acc, q);
    }
#pragma unroll
    for (int k = 0; k < d28::N; k++) {
      x.l[k] = sh_x[k][tid];
      y.l[k] = sh_y[k][tid];
    }
    q28::from_affine(q, x, y);
    q28::add(acc, q);
    return q28::is_inf(acc);
  } else {
    X28 q;
    q.x = bx;
    q.y = y;
    d28::set_one(q.zz);
    d28::set_one(q.zzz);
    X28 acc = q;
    // first multiplication: the addend is affine (mixed additions)
    for (int bit = 62; bit >= 0; bit--) {
      d28::dbl(acc);
      if ((zabs >> bit) & 1ull) d28::madd(acc, bx, y);
    }
    // second: the addend is the first result
    q = acc;
    for (int bit = 62; bit >= 0; bit--) {
      d28::dbl(acc);
      if ((zabs >> bit) & 1ull) d28::add(acc, q);
    }
#pragma unroll
    for (int k = 0; k < d28::N; k++) {
      x.l[k] = sh_x[k][tid];
      y.l[k] = sh_y[k][tid];
    }
    d28::madd(acc, x, y);
    return d28::is_inf(acc);
  }
}

}  // namespace curdle
