// Constant-time VARIABLE-base G1 multiplication: out_i = k_i * P_i, one lane per (point, scalar) pair, with an
// instruction stream and an address stream that do not depend on the scalars.  The twin of k_scalar_mul_batch_quad
// (group_kernels.hip), whose GLV chain branches on scalar bits, in the manner of k_fbase_mul_ct (fbase_ct_kernels.hip).
// P_i: a gnark G1Affine record, canonical Montgomery limbs, (0, 0) = infinity; k_i: a Montgomery fr.Element below r.
//
// The walk, its exactness argument (P of prime order r, 0 < k < r; k = r - 1 is where a DISCARDED sum is exceptional
// with real points) and the rule of what may depend on a scalar are at the top of g1_walk_ct.h, with the walk
// itself (walk_ct): k_msm_ct_walk (msm_ct_kernels.hip) and k_tracker_own_ct (tracker_own_ct_kernels.hip) call the same.
//
// The exit.  The lane normalises its own result through affine_words_ct (g1_exit_ct.h: one Fermat inversion of zz zzz,
// the masked canonical step).  The twelve words of each coordinate are masked with started & point_is_finite, so k = 0
// or P = infinity stores zeros.  Nothing unnormalised leaves the kernel: no kernel behind it sees a value that depends
// on the path the bits chose (projective coordinates do), which is what the in-lane inversion, about a tenth of the
// walk's products, pays for.  Whether P is infinity is public.
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
#include "g1_add_ct.h"  // finite_mask
#include "g1_exit_ct.h"

namespace curdle {

__global__ void __launch_bounds__(kBlock, 2)
    k_g1_mul_ct(const uint4* points, u32 point_stride, const uint4* __restrict__ scalars, u32 scalar_stride, u32 n, uint4* out) {
  const u32 i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  // the lane's record is read whole before anything is written: out may be points
  u32 pw[24];
  d28::load_words<24>(pw, points + 6 * ((size_t)i * point_stride));
  const u32 finite = finite_mask(pw);  // public
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
  X28 acc;
  const u32 started = walk_ct(acc, k, x2, y2, 255);
  // a lane that stores zeros normalises whatever it holds
  u32 w[24];
  affine_words_ct(w, acc);
  store_words_masked<6>(out + 6 * (size_t)i, w, started & finite);
}

hipError_t launch_g1_mul_ct(const void* points, uint32_t point_stride, const void* scalars, int shared_scalar, uint32_t n,
                            void* out_affine, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_g1_mul_ct, dim3(cdiv(n, kBlock)), dim3(kBlock), 0, stream, (const uint4*)points, (u32)point_stride,
                     (const uint4*)scalars, shared_scalar ? 0u : 1u, (u32)n, (uint4*)out_affine);
  return hipGetLastError();
}

}  // namespace curdle
