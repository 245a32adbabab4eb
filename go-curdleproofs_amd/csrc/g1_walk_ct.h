// The constant-time walk over a VARIABLE base, shared by k_g1_mul_ct (g1_mul_ct_kernels.hip), k_msm_ct_walk
// (msm_ct_kernels.hip) and k_tracker_own_ct (tracker_own_ct_kernels.hip): the scalar's load, its bits, the selections,
// the ONE constant-time mixed addition of the tree for a lane's own affine point, the walk itself (walk_ct) and the
// masked store behind it.  k_fbase_mul_ct (fbase_ct_kernels.hip) walks windows of a table on its own and takes
// load_fr_lane, select3 and store_words_masked from here.  Device-only; every function is forced inline into its kernel.
//
// The walk.  The 255 bits of k (r < 2^255) MSB first, a rolled loop.  Every step does ONE XYZZ doubling (d28::dbl,
// which has no exceptional arm) and ALWAYS one mixed addition of the lane's own affine point (the main path of
// d28::madd without its three exceptional arms); the new accumulator is taken by mask selection:
//     bit == 0                      keep the doubled accumulator            (the sum is discarded)
//     bit == 1, nothing added yet   the affine point, zz = zzz = one
//     otherwise                     the sum
// "Nothing added yet" is a mask word (started |= bit), never a test of zz: until the first set bit the accumulator is
// not a point at all (it starts as four ones and is doubled as field arithmetic), and k = 0 is `started == 0` at the
// end.  The next bit is bit 255 of the eight scalar words, which are shifted left every step: no register is indexed
// by the step.
//
// Exactness.  P has prime order r and 0 < k < r.  Before a step the accumulator is m P with m the prefix of k read so
// far (0 < m once started).  The doubling gives 2m P, never infinity for m != 0 because r is odd and 2m < 2r.  A KEPT
// sum is 2m P + P with the bit set: 2m >= 2 != 1, so the addend is not the accumulator, and 2m + 1 <= k < r, so it is
// not its negative.  A DISCARDED sum may be nonsense: it is integer arithmetic inside the limb bounds of fp28.h (x, y
// < 10p, zz, zzz < 2p, the affine operand below 2p) and traps nothing.  k = r - 1 is where that happens with real
// points: its last bit is 0, the prefix is (r - 1) / 2 and the last step discards exactly (r - 1) P + P = -P + P.
// tests/g1_mul_ct_model.py asserts the argument on every kept sum of every case the tests use and reports the
// exceptional discarded ones.  A point outside the prime-order subgroup gives an unspecified result and no fault.
//
// What may depend on a scalar: data operands of arithmetic and of selects written as mask arithmetic, m = 0 - (cond),
// (a & m) | (b & ~m).  What may not: a branch condition, an exec mask (beyond i >= n), a load, store or LDS address, a
// readfirstlane, a loop trip count.
//
// The scalar must be loaded at an address made of the LANE INDEX (load_fr_lane below on such a pointer): the load is
// then a per-lane vector load and the scalar lives in VGPRs.  A wave-uniform load would put it in SGPRs, where the
// compiler is free to turn a select into a scalar branch on the bit.
//
// The multiply-accumulate trap: no product may see a limb the compiler knows.  The
// initial accumulator is constants, so the bit loop of walk_ct stays rolled (#pragma unroll 1); the constant `one`
// reaches products only through a select under a lane mask.
#pragma once
#include <hip/hip_runtime.h>

#include "msm_kernels_common.h"

namespace curdle {

namespace {
__device__ __forceinline__ void load_fr_lane(Fr& f, const uint4* src) {
  const uint4 lo = src[0], hi = src[1];
  f.l[0] = lo.x; f.l[1] = lo.y; f.l[2] = lo.z; f.l[3] = lo.w;
  f.l[4] = hi.x; f.l[5] = hi.y; f.l[6] = hi.z; f.l[7] = hi.w;
}
// bit 255 of k, and k << 1: every bit is read from the top of word 7, so no register is indexed by the step
__device__ __forceinline__ u32 next_bit_msb(Fr& k) {
  const u32 b = k.l[7] >> 31;
#pragma unroll
  for (int j = 7; j > 0; j--) k.l[j] = (k.l[j] << 1) | (k.l[j - 1] >> 31);
  k.l[0] <<= 1;
  return b;
}
// r = sum ? a : (first ? b : c); sum, first and ~(sum | first) are disjoint masks
__device__ __forceinline__ void select3(F28& r, u32 sum, const F28& a, u32 first, const F28& b, const F28& c) {
  const u32 keep = ~(sum | first);
#pragma unroll
  for (int i = 0; i < d28::N; i++) r.l[i] = (a.l[i] & sum) | (b.l[i] & first) | (c.l[i] & keep);
}
// r = sum ? a : (first ? one : r)
__device__ __forceinline__ void select3_one(F28& r, u32 sum, const F28& a, u32 first) {
  const u32 keep = ~(sum | first);
#pragma unroll
  for (int i = 0; i < d28::N; i++) r.l[i] = (a.l[i] & sum) | (d28::kOne(i) & first) | (r.l[i] & keep);
}

// One step's addition.  acc: x < 10p, y < 6p, zz, zzz < 2p, limbs normalised (what d28::dbl leaves); (x2, y2) affine
// below 2p, normalised.  bit = 0 - (the scalar's bit), started = all ones once something was added.  d28::madd's main
// path (EFD madd-2008-s) with madd's bounds (X3 < 10p, Y3 < 2p, products < 2p), then the selection described at the top.
__device__ __forceinline__ void madd_bit(X28& acc, const F28& x2, const F28& y2, u32 bit, u32 started) {
  using namespace d28;
  const u32 sum = bit & started, first = bit & ~started;
  F28 pp, r, t, q, ppp, p;
  mul_inl(p, x2, acc.zz);
  sub_raw<16>(p, p, acc.x);  // P = U2 - X1 < 18p
  mul_inl(r, y2, acc.zzz);
  sub_raw<16>(r, r, acc.y);  // R = S2 - Y1 < 18p
  sqr_inl(pp, p);            // PP < 2p
  mul_inl(ppp, p, pp);       // PPP
  mul_inl(q, acc.x, pp);     // Q
  mul_inl(p, acc.zz, pp);
  select3_one(acc.zz, sum, p, first);
  mul_inl(p, acc.zzz, ppp);
  select3_one(acc.zzz, sum, p, first);
  sqr_inl(t, r);
  x3_fused(t, t, ppp, q);    // X3 = R^2 - PPP - 2Q < 10p
  sub_raw<16>(q, q, t);      // Q - X3 < 18p
  F28 ny, z;
  set_zero(z);
  sub_raw<16>(ny, z, acc.y); // 16p - Y1 (Y1 < 6p)
  mul2_inl(p, r, q, ny, ppp);  // Y3 = R (Q - X3) - Y1 PPP  (mod p), < 2p
  select3(acc.x, sum, t, first, x2, acc.x);
  select3(acc.y, sum, p, first, y2, acc.y);
}

// The walk: `steps` bits of k from bit 255 down (the caller dropped bit 255 or shifted k left by 256 - steps; steps is
// public), one d28::dbl and one madd_bit a step.  acc starts as four ones and is not a point until the returned
// `started` is all ones; started == 0 is k = 0.  The loop stays rolled: the multiply-accumulate trap at the top.
__device__ __forceinline__ u32 walk_ct(X28& acc, Fr& k, const F28& x2, const F28& y2, u32 steps) {
  d28::set_one(acc.x);
  d28::set_one(acc.y);
  d28::set_one(acc.zz);
  d28::set_one(acc.zzz);
  u32 started = 0;
#pragma unroll 1
  for (u32 step = 0; step < steps; step++) {
    const u32 bit = 0u - next_bit_msb(k);
    d28::dbl(acc);
    madd_bit(acc, x2, y2, bit, started);
    started |= bit;
  }
  return started;
}

// dst[0 .. N16) = the 4 N16 words of w under the lane mask m: what a lane with no result stores is zeros
template <int N16>
__device__ __forceinline__ void store_words_masked(uint4* dst, const u32* w, u32 m) {
#pragma unroll
  for (int j = 0; j < N16; j++) dst[j] = make_uint4(w[4 * j] & m, w[4 * j + 1] & m, w[4 * j + 2] & m, w[4 * j + 3] & m);
}
}  // namespace

}  // namespace curdle
