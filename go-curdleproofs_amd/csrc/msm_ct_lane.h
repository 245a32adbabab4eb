// One lane of the constant-time MSM's walk kernels, k_msm_ct_walk (msm_ct_kernels.hip) and k_msm_ct_walk_rows
// (msm_ct_bases_kernels.hip): everything behind the addresses.  The kernels differ in where a lane's point record, scalar
// and term live and in which bits of the scalar the lane walks; the rule of what may depend on a secret is the one of
// g1_walk_ct.h.  Device-only; forced inline into its kernel.
#pragma once
#include "g1_walk_ct.h"
#include "g1_add_ct.h"  // finite_mask

namespace curdle {

namespace {
// point: the lane's gnark G1Affine record (96 bytes; an address made of public values).  k: the lane's PLAIN scalar,
// loaded at an address made of the lane index and converted by the caller.  The lane walks bits
// [bits - skip - steps, bits - skip) of k; bits, skip and steps are public.  term: where the lane's X28 record goes
// (224 bytes, not normalised): all-zero words when nothing was added (the walked bits are 0) or the point is infinity,
// which is public.  status: the call's ONE status word, at an address made of the lane index.
__device__ __forceinline__ void msm_ct_lane(const uint4* point, Fr& k, u32 bits, u32 skip, u32 steps, uint4* term, u32* status) {
  u32 pw[24];
  d28::load_words<24>(pw, point);
  const u32 finite = finite_mask(pw);  // public
  F28 x2, y2;
  d28::from_gnark(x2, pw);
  d28::from_gnark(y2, pw + 12);
  // k << (256 - bits): the trip count is the argument alone; a set bit at or above `bits` is the violation.  Then the
  // bits between the walk's top and `bits` go, by the same rolled loop.
  u32 over = 0;
#pragma unroll 1
  for (u32 s = bits; s < 256; s++) over |= next_bit_msb(k);
#pragma unroll 1
  for (u32 s = 0; s < skip; s++) (void)next_bit_msb(k);
  X28 acc;
  const u32 started = walk_ct(acc, k, x2, y2, steps);
  // Unconditional, 0 or 1: no branch is taken on it.  The address is made of the lane index so that it is a per-lane
  // atomic: on a wave-uniform address the compiler first folds the wave's values through v_readlane into SGPRs.
  atomicOr(status, over);
  store_words_masked<14>(term, reinterpret_cast<const u32*>(&acc), started & finite);
}
}  // namespace

}  // namespace curdle
