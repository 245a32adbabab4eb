// Which trackers does a set of keys own, with an instruction stream and an address stream that do not depend on the
// keys: the twin of k_tracker_own (tracker_own_kernels.hip), whose GLV chain BRANCHES ON KEY BITS, in the manner of
// k_g1_mul_ct (g1_mul_ct_kernels.hip).  Key j owns tracker (rG, krG) iff k_j rG and krG are the same group element.
//
// The layout.  One LANE per (key, tracker) pair, flattened: lane g of a launch over trackers [t0, t0 + tc) of keys
// [key0, key0 + kc) takes key0 + g / tc and t0 + g % tc, g < tc kc, in a 1-D grid of blocks of 256.  Nothing is padded
// to waves or blocks: a wave may hold several keys, and nothing below needs a uniform key.  That is deliberate.  The
// key's address is made of the lane index, so its two 16-byte loads are per-lane VECTOR loads and the key lives in
// VGPRs (the reasoning of k_g1_mul_ct's scalar_stride); k_tracker_own's blockIdx.y key would land in SGPRs, where the
// compiler is free to turn a select into a scalar branch on a bit.  No readfirstlane, no readlane, no LDS.
//
// What is public and may branch: g >= tc kc leaves; a status byte beyond CURDLE_DECODE_INFINITY on either record stores
// CURDLE_TRACKER_BAD with no chain (the trackers are public); whether rG or krG is infinity is public too, and is
// nevertheless folded into masks.  Everything from the key's load to the store is straight-line code under one exec.
//
// The walk is k_g1_mul_ct's, from g1_walk_ct.h, on the lane's rG: f_from_mont on the key, bit 255 dropped, walk_ct over
// 255 steps.  The exactness argument of g1_walk_ct.h carries over word for
// word: the decoder's subgroup test (launch_g1_decompress) is what makes rG of prime order r.
//
// The end.  There is NO inversion.  The result (X, Y, ZZ, ZZZ) equals the affine krG = (x2, y2) iff x2 ZZ = X and
// y2 ZZZ = Y (mod p).  Each difference is formed with sub_raw, brought below 2p by ONE Montgomery product (by `one`,
// through the out-of-line product, which sees no constant), and "0 mod p" is decided on the reduced value, which is
// then 0 or p (normalize_kernels.hip decides d = 0 the same way): the OR of the limbs and the OR of the limbs' XOR
// with p, combined as MASKS.  With res_finite = started & rG_finite:
//     owned = res_finite ? (krG_finite & eq_x & eq_y) : ~krG_finite
// and one byte, CURDLE_TRACKER_OWNED or _NOT_OWNED chosen by mask arithmetic, goes to out[key * stride + t].  The
// verdict IS the result: the store's value may depend on the key, its address does not.  When the result is not finite
// the accumulator is not a point; the products above are then integer arithmetic inside the limb bounds and their
// verdicts are masked away.
//
// Plain loads and stores, no LDS, no scratch, no inline assembly beyond the field layer's.
#include <hip/hip_runtime.h>

#include "../../include/curdle_msm.h"
#include "msm_kernels_common.h"
#include "g1_walk_ct.h"
#include "g1_add_ct.h"  // finite_mask, equal_mod_p

namespace curdle {

// points: the decoded records of a pass (gnark affine, (0, 0) = infinity), rG_t at 2 t and krG_t at 2 t + 1; status:
// their CURDLE_DECODE_* bytes (subgroup test included); keys: Montgomery fr.Elements.  The launch covers trackers
// [t0, t0 + tc) of keys [key0, key0 + kc), pairs = tc kc; out[key * stride + t] gets the verdict.
__global__ void __launch_bounds__(kBlock, 2)
    k_tracker_own_ct(const uint4* __restrict__ points, const uint8_t* __restrict__ status, const uint4* __restrict__ keys,
                     u32 t0, u32 tc, u32 key0, u32 pairs, size_t stride, uint8_t* __restrict__ out) {
  const u32 g = blockIdx.x * kBlock + threadIdx.x;
  if (g >= pairs) return;
  const u32 kq = g / tc;
  const u32 t = t0 + (g - kq * tc);
  const u32 key = key0 + kq;
  uint8_t* dst = out + (size_t)key * stride + t;
  if (status[2 * (size_t)t] > CURDLE_DECODE_INFINITY || status[2 * (size_t)t + 1] > CURDLE_DECODE_INFINITY) {
    *dst = CURDLE_TRACKER_BAD;  // public: no chain
    return;
  }
  u32 pw[24];
  d28::load_words<24>(pw, points + 6 * (2 * (size_t)t));
  const u32 rg_finite = finite_mask(pw);
  F28 x2, y2;
  d28::from_gnark(x2, pw);
  d28::from_gnark(y2, pw + 12);
  Fr k;
  {
    Fr s;
    load_fr_lane(s, keys + 2 * (size_t)key);  // an address made of the lane index: a vector load, the key in VGPRs
    f_from_mont<FrParams>(k, s);
  }
  (void)next_bit_msb(k);  // k < r < 2^255: bit 255 is zero, bit 254 is next
  X28 acc;
  const u32 started = walk_ct(acc, k, x2, y2, 255);
  // acc == krG without an inversion: x2 ZZ == X and y2 ZZZ == Y
  d28::load_words<24>(pw, points + 6 * (2 * (size_t)t + 1));
  const u32 krg_finite = finite_mask(pw);
  d28::from_gnark(x2, pw);
  d28::from_gnark(y2, pw + 12);
  F28 u;
  d28::mul(u, x2, acc.zz);
  const u32 eq_x = equal_mod_p(u, acc.x);
  d28::mul(u, y2, acc.zzz);
  const u32 eq_y = equal_mod_p(u, acc.y);
  const u32 res_finite = started & rg_finite;
  const u32 owned = (res_finite & krg_finite & eq_x & eq_y) | (~res_finite & ~krg_finite);
  *dst = (uint8_t)(((u32)CURDLE_TRACKER_OWNED & owned) | ((u32)CURDLE_TRACKER_NOT_OWNED & ~owned));
}

hipError_t launch_tracker_own_ct(const void* points, const uint8_t* status, const void* keys, uint32_t t0, uint32_t tc,
                                 uint32_t key0, uint32_t kc, uint8_t* out, size_t stride, hipStream_t stream) {
  if (tc == 0 || kc == 0) return hipSuccess;
  const u64 pairs = (u64)tc * kc;
  if (pairs > ((u64)1 << 31)) return hipErrorInvalidValue;  // the lane index is 32 bits
  hipLaunchKernelGGL(k_tracker_own_ct, dim3(cdiv(pairs, kBlock)), dim3(kBlock), 0, stream, (const uint4*)points, status,
                     (const uint4*)keys, (u32)t0, (u32)tc, (u32)key0, (u32)pairs, stride, out);
  return hipGetLastError();
}

}  // namespace curdle
