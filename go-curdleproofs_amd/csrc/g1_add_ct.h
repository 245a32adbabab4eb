// ONE complete XYZZ addition by selection: add_ct(acc, b) is d28::add (fp28.h) without a branch, for sums whose
// operands depend on secrets (k_g1_sum_ct of msm_ct_kernels.hip folds the terms k_i P_i of a constant-time MSM with
// it).  Device-only; every function is forced inline into its kernel.  The two mask helpers below it,
// finite_mask and equal_mod_p, are shared with k_tracker_own_ct (tracker_own_ct_kernels.hip); finite_mask with
// k_g1_mul_ct (g1_mul_ct_kernels.hip) too.
//
// What it computes, ALWAYS all of it:
//     the main path of add-2008-s on (acc, b)                      12 products, 2 squarings
//     d28::dbl of a copy of acc (which has no exceptional arm)      6 products, 3 squarings
//     four masks:  a_inf, b_inf   the OR of the operand's zz limbs is zero (infinity is ZZ = 0, all limbs zero)
//                  eq_x, eq_y     P = U2 - U1 == 0 and R = S2 - S1 == 0 mod p, decided by equal_mod_p
// and takes the result by mask arithmetic, in this priority:
//     1. b          if a_inf
//     2. acc        if b_inf
//     3. the double if eq_x & eq_y          (the same point)
//     4. infinity   if eq_x & ~eq_y         (a point and its negative): all four coordinates ZERO WORDS
//     5. the sum    otherwise
// The five masks are disjoint and cover everything, so the selection is one OR of five ANDs per limb.
//
// Bounds.  Inputs: x < 10p, y < 10p, zz, zzz < 2p, limbs normalised -- what add_ct, d28::dbl, madd_bit (g1_walk_ct.h)
// and an all-zero record leave.  Output: x < 10p (x3_fused), y < 6p (sub<4>; the double's too), zz, zzz < 2p, limbs
// normalised; or one of the inputs; or zeros.  So the output is a legal input of add_ct and of d28::dbl.  A finite
// result never has zz == 0 as an integer: zz is a product of nonzero residues, below 2p, and the only such integers
// that are 0 mod p are 0 and p, which a nonzero residue is not.  Infinity is always the integer 0: arm 4 writes zero
// words, d28::dbl and the products keep 0 at 0, and arms 1 and 2 copy.
//
// Discarded arms may be nonsense (the sum of P and P has P = R = 0 and gives zeros; the double of a record that is not
// a point is field arithmetic): they are integer arithmetic inside the limb bounds above and trap nothing.
//
// What may depend on a secret is the rule of g1_walk_ct.h: data operands of arithmetic and of mask selects only.
// Which arm an addition takes depends on the operands, so NOTHING here branches, and the caller's addresses and trip
// counts are made of public counts alone.  Every product goes through the out-of-line d28::mul / d28::sqr, which see
// no constant (the multiply-accumulate trap of DESIGN.md section 0, round 19).
#pragma once
#include <hip/hip_runtime.h>

#include "msm_kernels_common.h"

namespace curdle {

namespace {
// all ones iff the 24 words of a gnark affine record are not all zero ((0, 0) = infinity); public
__device__ __forceinline__ u32 finite_mask(const u32* w) {
  u32 any = 0;
#pragma unroll
  for (int j = 0; j < 24; j++) any |= w[j];
  return 0u - ((any | (0u - any)) >> 31);
}
// all ones iff a - b == 0 mod p; a < 2p, b < 10p, both normalised.  No comparison instruction: masks only.
// Inside these bounds the difference a - b + 16p is at least 6p, never the integer 0, so for congruent operands the product
// e below is always p and never 0: the `== 0` leg cannot be reached and is kept for operands outside the contract
// (tests/g1_ct_model.py asserts it on every call).
__device__ __forceinline__ u32 equal_mod_p(const F28& a, const F28& b) {
  using namespace d28;
  F28 d, e, c;
  sub_raw<16>(d, a, b);  // a - b + 16p < 18p
#pragma unroll
  for (int i = 0; i < N; i++) c.l[i] = kOne(i);
  mul(e, d, c);  // the same residue, below 2p and normalised: 0 or p iff a == b mod p
  u32 o0 = 0, op = 0;
#pragma unroll
  for (int i = 0; i < N; i++) {
    o0 |= e.l[i];
    op |= e.l[i] ^ kP(i);
  }
  const u32 neither = ((o0 | (0u - o0)) & (op | (0u - op))) >> 31;  // 1 iff e is neither 0 nor p
  return neither - 1u;
}
// all ones iff every limb of a is zero
__device__ __forceinline__ u32 zero_mask(const F28& a) {
  u32 any = 0;
#pragma unroll
  for (int i = 0; i < d28::N; i++) any |= a.l[i];
  return ((any | (0u - any)) >> 31) - 1u;
}
// r = (a & ma) | (b & mb) | (c & mc) | (d & md); the masks are disjoint, and where none is set r is zero
__device__ __forceinline__ void select4(F28& r, u32 ma, const F28& a, u32 mb, const F28& b, u32 mc, const F28& c, u32 md,
                                        const F28& d) {
#pragma unroll
  for (int i = 0; i < d28::N; i++) r.l[i] = (a.l[i] & ma) | (b.l[i] & mb) | (c.l[i] & mc) | (d.l[i] & md);
}

// acc += b, complete, branch-free.  Bounds at the top of the file.
__device__ __forceinline__ void add_ct(X28& acc, const X28& b) {
  using namespace d28;
  const u32 a_inf = zero_mask(acc.zz), b_inf = zero_mask(b.zz);
  X28 twice = acc;
  dbl(twice);
  // the main path of d28::add
  F28 u1, u2, s1, s2, p, r, pp, ppp, q, t;
  X28 sum;
  mul(u1, acc.x, b.zz);
  mul(u2, b.x, acc.zz);
  mul(s1, acc.y, b.zzz);
  mul(s2, b.y, acc.zzz);
  const u32 eq_x = equal_mod_p(u2, u1), eq_y = equal_mod_p(s2, s1);
  sub_raw<4>(p, u2, u1);  // < 6p
  sub_raw<4>(r, s2, s1);  // < 6p
  sqr(pp, p);
  mul(ppp, p, pp);
  mul(q, u1, pp);
  mul(t, acc.zz, b.zz);
  mul(sum.zz, t, pp);
  mul(t, acc.zzz, b.zzz);
  mul(sum.zzz, t, ppp);
  sqr(t, r);
  x3_fused(sum.x, t, ppp, q);  // X3 < 10p
  sub_raw<16>(q, q, sum.x);    // < 18p
  mul(q, r, q);
  mul(s1, s1, ppp);
  sub<4>(sum.y, q, s1);  // < 6p
  // the five arms; the fourth is zeros, which the OR below gives when no mask is set
  const u32 both = ~a_inf & ~b_inf;
  const u32 take_b = a_inf, take_a = ~a_inf & b_inf, take_dbl = both & eq_x & eq_y, take_sum = both & ~eq_x;
  select4(acc.x, take_b, b.x, take_a, acc.x, take_dbl, twice.x, take_sum, sum.x);  // a limb is read before it is written
  select4(acc.y, take_b, b.y, take_a, acc.y, take_dbl, twice.y, take_sum, sum.y);
  select4(acc.zz, take_b, b.zz, take_a, acc.zz, take_dbl, twice.zz, take_sum, sum.zz);
  select4(acc.zzz, take_b, b.zzz, take_a, acc.zzz, take_dbl, twice.zzz, take_sum, sum.zzz);
}
}  // namespace

}  // namespace curdle
