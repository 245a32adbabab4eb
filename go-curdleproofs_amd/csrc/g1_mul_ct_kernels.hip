// Constant-time VARIABLE-base G1 multiplication: out_i = k_i * P_i, one lane per (point, scalar) pair, with an
// instruction stream and an address stream that do not depend on the scalars.  The twin of k_scalar_mul_batch_quad
// (group_kernels.hip), whose GLV chain branches on scalar bits, in the manner of k_fbase_mul_ct (fbase_ct_kernels.hip).
// P_i: a gnark G1Affine record, canonical Montgomery limbs, (0, 0) = infinity; k_i: a Montgomery fr.Element below r.
//
// The walk.  The 255 bits of k (r < 2^255) MSB first, a rolled loop.  Every step does ONE XYZZ doubling (d28::dbl,
// which has no exceptional arm) and ALWAYS one mixed addition of the lane's own affine point (the main path of
// d28::madd without its three exceptional arms, as madd_select of fbase_ct_kernels.hip); the new accumulator is taken
// by mask selection:
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
// exceptional discarded ones.  A point outside the prime-order subgroup gives an unspecified record and no fault.
//
// The exit.  The lane normalises its own result: ONE Fermat inversion of zz zzz on the fixed exponent chain of
// invert28.h (the exponent is p - 2 for every lane: its window switch is wave-uniform and public), x = X zzz / (zz zzz),
// y = Y zz / (zz zzz), and the canonical gnark record leaves through a MASKED canonical step (to_gnark_ct below: a
// select, not d28::canonical_lt2p's `if (!borrow)`).  The twelve words of each coordinate are masked with
// started & point_is_finite, so k = 0 or P = infinity stores zeros.  Nothing unnormalised leaves the kernel: no kernel
// behind it sees a value that depends on the path the bits chose (projective coordinates do), which is what the
// in-lane inversion, about a tenth of the walk's products, pays for.  Whether P is infinity is public.
//
// What may depend on a scalar: data operands of arithmetic and of selects written as mask arithmetic, m = 0 - (cond),
// (a & m) | (b & ~m).  What may not: a branch condition, an exec mask (beyond i >= n), a load, store or LDS address, a
// readfirstlane, a loop trip count.
//
// One shared scalar.  The scalar of lane i is read at scalars + 32 i scalar_stride with scalar_stride a kernel
// ARGUMENT (1, or 0 for one scalar shared by the launch): the address is made of the lane index, so the load is a
// per-lane vector load in both cases and the scalar lives in VGPRs.  A wave-uniform load would put it in SGPRs, where
// the compiler is free to turn a select into a scalar branch on the bit; there is ONE instantiation of the kernel and
// DESIGN.md section 0 (round 24) reads its assembly.  point_stride (in records) lets a caller walk every second record.
//
// The multiply-accumulate trap: no product may see a limb the compiler knows.  The
// initial accumulator is constants, so the bit loop stays rolled (#pragma unroll 1); the constant `one` reaches
// products only through a select under a lane mask.
//
// Not built: a fixed-window form (15 projective multiples per lane are 3,360 bytes: workspace traffic or LDS for about
// 1.4x fewer operations), GLV (its chains take exceptional additions: tests/glv_chain_model.py) and a lane-quad form.
//
// Plain loads and stores, no LDS, no scratch, no inline assembly beyond the field layer's.
#include <hip/hip_runtime.h>

#include "msm_kernels_common.h"
#include "invert28.h"

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

// d28::to_gnark with a masked canonical step (to_gnark_msm_ct of fbase_ct_kernels.hip with the plain constant): the
// choice between t and t - p is a select on the borrow, never an exec mask.
__device__ __forceinline__ void to_gnark_ct(u32* w, const F28& a) {
  using namespace d28;
  F28 t, c;
#pragma unroll
  for (int i = 0; i < N; i++) c.l[i] = kToExt(i);
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
}  // namespace

__global__ void __launch_bounds__(kBlock, 2)
    k_g1_mul_ct(const uint4* points, u32 point_stride, const uint4* __restrict__ scalars, u32 scalar_stride, u32 n, uint4* out) {
  const u32 i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  // the lane's record is read whole before anything is written: out may be points
  u32 pw[24];
  d28::load_words<24>(pw, points + 6 * ((size_t)i * point_stride));
  u32 any = 0;
#pragma unroll
  for (int j = 0; j < 24; j++) any |= pw[j];
  const u32 finite = 0u - (u32)(any != 0u);  // public
  F28 x2, y2;
  d28::from_gnark(x2, pw);
  d28::from_gnark(y2, pw + 12);
  Fr k;
  {
    Fr s;
    load_fr_lane(s, scalars + 2 * ((size_t)i * scalar_stride));
    f_from_mont<FrParams>(k, s);
  }
  (void)next_bit_msb(k);  // k < r < 2^255: bit 255 is zero, bit 254 is next
  X28 acc;  // not a point until `started`
  d28::set_one(acc.x);
  d28::set_one(acc.y);
  d28::set_one(acc.zz);
  d28::set_one(acc.zzz);
  u32 started = 0;
#pragma unroll 1
  for (u32 step = 0; step < 255; step++) {
    const u32 bit = 0u - next_bit_msb(k);
    d28::dbl(acc);
    madd_bit(acc, x2, y2, bit, started);
    started |= bit;
  }
  // x = X / zz, y = Y / zzz with one inversion; a lane that stores zeros inverts whatever it holds (0 gives 0)
  F28 d, inv, ix, iy;
  d28::mul(d, acc.zz, acc.zzz);
  invert(inv, d);
  d28::mul(ix, inv, acc.zzz);
  d28::mul(iy, inv, acc.zz);
  d28::mul(ix, acc.x, ix);
  d28::mul(iy, acc.y, iy);
  const u32 m = started & finite;
  u32 w[24];
  to_gnark_ct(w, ix);
  to_gnark_ct(w + 12, iy);
  uint4* dst = out + 6 * (size_t)i;
#pragma unroll
  for (int j = 0; j < 6; j++) dst[j] = make_uint4(w[4 * j] & m, w[4 * j + 1] & m, w[4 * j + 2] & m, w[4 * j + 3] & m);
}

hipError_t launch_g1_mul_ct(const void* points, uint32_t point_stride, const void* scalars, int shared_scalar, uint32_t n,
                            void* out_affine, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_g1_mul_ct, dim3(cdiv(n, kBlock)), dim3(kBlock), 0, stream, (const uint4*)points, (u32)point_stride,
                     (const uint4*)scalars, shared_scalar ? 0u : 1u, (u32)n, (uint4*)out_affine);
  return hipGetLastError();
}

}  // namespace curdle
