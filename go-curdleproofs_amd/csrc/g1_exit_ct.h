// How a constant-time G1 result leaves its kernel: the masked canonical step and the single-inversion affine exit, shared
// by k_g1_mul_ct (g1_mul_ct_kernels.hip), k_msm_ct_finish / _seg (msm_ct_kernels.hip) and k_fbase_mul_ct
// (fbase_ct_kernels.hip).  Device-only; every function is forced inline into its kernel.
//
// The masked canonical step.  d28::canonical_lt2p takes its subtraction under `if (!borrow)`, which the fixed-base build
// turned into an exec mask on whether the product's representative reached p: a property of the accumulator's projective
// coordinates, which are made of the secret's digits.  Here the choice between t and t - p is a select on the borrow.
//
// The affine exit.  ONE inversion of zz zzz -- by default the Fermat one on the fixed exponent chain of invert28.h (the
// exponent is p - 2 for every lane: its window switch is wave-uniform and public); under InvertDivsteps the division
// steps of invert_ds.h, which k_msm_ct_finish_ds / _seg_ds take --, x = X zzz / (zz zzz), y = Y zz / (zz zzz), and both
// coordinates through the masked canonical step.  A record that is not a point (nothing added yet, or infinity) inverts
// whatever it holds -- 0 gives 0 -- and the CALLER masks the words away.
#pragma once
#include <hip/hip_runtime.h>

#include "msm_kernels_common.h"
#include "invert28.h"
#include "invert_ds.h"

namespace curdle {

namespace {
// d28::to_gnark with a masked canonical step.  Const is the conversion constant, chosen at compile time: d28::kToExt, or
// d28::kToExtX16 / d28::kToExtY64 for the X and Y of a result on the curve of from_gnark_iso (d28::to_gnark_msm's roles).
template <u32 (*Const)(int)>
__device__ __forceinline__ void to_gnark_ct(u32* w, const F28& a) {
  using namespace d28;
  F28 t, c;
#pragma unroll
  for (int i = 0; i < N; i++) c.l[i] = Const(i);
  mul(t, a, c);
  u32 d[N], borrow = 0;
#pragma unroll
  for (int i = 0; i < N; i++) {
    const u32 s = t.l[i] - kP(i) - borrow;
    borrow = s >> 31;  // limbs are below 2^28 (the top one below 2^31): bit 31 of the difference is the borrow
    d[i] = i < N - 1 ? s & MASK : s;
  }
  const u32 lt = 0u - borrow;  // t < p: keep t
#pragma unroll
  for (int i = 0; i < N; i++) t.l[i] = (t.l[i] & lt) | (d[i] & ~lt);
  pack(w, t);
}

// The exit's inversion, a template parameter of affine_words_ct.  Both take a product (normalised, below 2p) and give
// the Montgomery form of its inverse under the same bounds, 0 for 0 and for p.
struct InvertFermat {  // the fixed exponent chain of invert28.h: what every kernel took before there was a choice
  static __device__ __forceinline__ void run(F28& y, const F28& d) { invert(y, d); }
};
struct InvertDivsteps {  // the division steps of invert_ds.h
  // The violation word is dropped: invert_ds takes the canonical representative first, and no value below p sets it.
  static __device__ __forceinline__ void run(F28& y, const F28& d) { (void)invert_ds(y, d); }
};

// w = the canonical gnark record (x | y) of acc: x = X / zz, y = Y / zzz with one inversion
template <class Inv = InvertFermat>
__device__ __forceinline__ void affine_words_ct(u32 w[24], const X28& acc) {
  F28 d, inv, ix, iy;
  d28::mul(d, acc.zz, acc.zzz);
  Inv::run(inv, d);
  d28::mul(ix, inv, acc.zzz);
  d28::mul(iy, inv, acc.zz);
  d28::mul(ix, acc.x, ix);
  d28::mul(iy, acc.y, iy);
  to_gnark_ct<d28::kToExt>(w, ix);
  to_gnark_ct<d28::kToExt>(w + 12, iy);
}
}  // namespace

}  // namespace curdle
