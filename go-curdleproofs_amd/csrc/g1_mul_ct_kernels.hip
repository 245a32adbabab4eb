// Constant-time VARIABLE-base G1 multiplication: out_i = k_i * P_i, one lane per (point, scalar) pair, with an
// instruction stream and an address stream that do not depend on the scalars.  The twin of k_scalar_mul_batch_quad
// (group_kernels.hip), whose GLV chain branches on scalar bits, in the manner of k_fbase_mul_ct (fbase_ct_kernels.hip).
// P_i: a gnark G1Affine record, canonical Montgomery limbs, (0, 0) = infinity; k_i: a Montgomery fr.Element below r.
//
// The walk, its exactness argument (P of prime order r, 0 < k < r; k = r - 1 is where a DISCARDED sum is exceptional
// with real points) and the rule of what may depend on a scalar are at the top of g1_walk_ct.h, with the walk's
// helpers: k_tracker_own_ct (tracker_own_ct_kernels.hip) walks the same way.
//
// The exit.  The lane normalises its own result: ONE Fermat inversion of zz zzz on the fixed exponent chain of
// invert28.h (the exponent is p - 2 for every lane: its window switch is wave-uniform and public), x = X zzz / (zz zzz),
// y = Y zz / (zz zzz), and the canonical gnark record leaves through a MASKED canonical step (to_gnark_ct below: a
// select, not d28::canonical_lt2p's `if (!borrow)`).  The twelve words of each coordinate are masked with
// started & point_is_finite, so k = 0 or P = infinity stores zeros.  Nothing unnormalised leaves the kernel: no kernel
// behind it sees a value that depends on the path the bits chose (projective coordinates do), which is what the
// in-lane inversion, about a tenth of the walk's products, pays for.  Whether P is infinity is public.
//
// One shared scalar.  The scalar of lane i is read at scalars + 32 i scalar_stride with scalar_stride a kernel
// ARGUMENT (1, or 0 for one scalar shared by the launch): the address is made of the lane index, so the load is a
// per-lane vector load in both cases and the scalar lives in VGPRs.  A wave-uniform load would put it in SGPRs, where
// the compiler is free to turn a select into a scalar branch on the bit; there is ONE instantiation of the kernel and
// DESIGN.md section 0 (round 24) reads its assembly.  point_stride (in records) lets a caller walk every second record.
//
// Not built: a fixed-window form (15 projective multiples per lane are 3,360 bytes: workspace traffic or LDS for about
// 1.4x fewer operations), GLV (its chains take exceptional additions: tests/glv_chain_model.py) and a lane-quad form.
//
// Plain loads and stores, no LDS, no scratch, no inline assembly beyond the field layer's.
#include <hip/hip_runtime.h>

#include "msm_kernels_common.h"
#include "g1_walk_ct.h"
#include "invert28.h"

namespace curdle {

namespace {
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
