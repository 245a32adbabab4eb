// Which trackers does a set of keys own?  A Whisk tracker is (rG, krG) with krG = k rG (the reference's
// whisk/whisk_test.go:98-104, computeTracker); key j owns tracker i iff k_j rG_i and krG_i are the same group element.
// That is m n independent 255-bit scalar multiplications with an equality test, and nothing is shared between keys.
//
// k_tracker_own takes one (key, tracker) pair per quad (quad28.h).  Its body is that of k_scalar_mul_batch_quad
// (group_kernels.hip): f_from_mont, glv_split, the table {+-P, +-phi(P), their sum}, 127 doublings with at most one
// addition each.  Its end is that of k_tracker_check (tracker_kernels.hip): -krG is added and the sum must be infinity
// -- quad28.h add() handles equal and opposite operands and infinity on either side, so the verdict is exact.  One
// byte per pair leaves the quad.
//
// What the shape adds: a block of 256 lanes is 64 trackers of ONE key, and the key is chosen by blockIdx.y.  So the
// key, its split and every tested bit are wave-uniform: the key comes in by scalar loads, the split's results and
// the two tested bits of every step are formed through readfirstlane, and the per-bit "add or skip" is a scalar
// branch (s_cmp + s_cbranch_scc1 in the gfx950 assembly, no exec mask; the choice of the table entry is a select under
// an SGPR mask).  With per-point scalars a wave runs an addition whenever ANY of its 16 quads needs one (DESIGN.md
// section 8.2); here all need it or none does.
#include <hip/hip_runtime.h>

#include "../../include/curdle_msm.h"
#include "fp28.h"
#include "quad28.h"
#include "glv_quad.h"
#include "msm_kernels.h"

namespace curdle {

using d28::F28;

static constexpr int kBlock = 256;
static constexpr u32 kBlockTrackers = kBlock / 4;

namespace {
__device__ __forceinline__ u32 uniform(u32 v) { return (u32)__builtin_amdgcn_readfirstlane((int)v); }
}  // namespace

// points: the decoded records of a pass (gnark affine, (0, 0) = infinity), rG_t at 2 t and krG_t at 2 t + 1; status:
// their CURDLE_DECODE_* bytes (subgroup test included); keys: Montgomery fr.Elements.  The launch covers trackers
// [t0, t0 + cnt) (blockIdx.x: 64 each) of keys [key0, key0 + gridDim.y); out[key * stride + t] gets the verdict.
__global__ void __launch_bounds__(kBlock, 2)
    k_tracker_own(const uint4* __restrict__ points, const uint8_t* __restrict__ status, const uint4* __restrict__ keys,
                  u32 t0, u32 cnt, u32 key0, size_t stride, uint8_t* __restrict__ out) {
  const u32 local = blockIdx.x * kBlockTrackers + (threadIdx.x >> 2);
  if (local >= cnt) return;  // whole quads leave together
  const u32 t = t0 + local;
  const u32 key = key0 + blockIdx.y;
  uint8_t* dst = out + (size_t)key * stride + t;
  if (status[2 * (size_t)t] > CURDLE_DECODE_INFINITY || status[2 * (size_t)t + 1] > CURDLE_DECODE_INFINITY) {
    if (q28::role() == 0) *dst = CURDLE_TRACKER_BAD;  // uniform over the quad: no chain
    return;
  }
  // the key and its split: the same for every lane of the block, kept in SGPRs
  u32 a[4], b[4], neg_a, neg_b;
  {
    const uint4 lo = keys[2 * (size_t)key], hi = keys[2 * (size_t)key + 1];
    Fr m, k;
    m.l[0] = uniform(lo.x); m.l[1] = uniform(lo.y); m.l[2] = uniform(lo.z); m.l[3] = uniform(lo.w);
    m.l[4] = uniform(hi.x); m.l[5] = uniform(hi.y); m.l[6] = uniform(hi.z); m.l[7] = uniform(hi.w);
    f_from_mont<FrParams>(k, m);
    glv_split(k, a, b, neg_a, neg_b);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      a[j] = uniform(a[j]);
      b[j] = uniform(b[j]);
    }
    neg_a = uniform(neg_a);
    neg_b = uniform(neg_b);
  }
  F28 x, y, p, acc;
  q28::set_inf(acc);
  if (glvq::load_affine(x, y, points, 2 * (size_t)t)) {  // k * inf = inf
    F28 p1, p2, p3;
    glvq::table(p1, p2, p3, x, y, neg_a, neg_b);
    glvq::shift(a, b);
    for (int bit = 126; bit >= 0; bit--) {
      q28::dbl(acc);
      // the two tested bits as SGPR values: the shifted halves themselves end up in VGPRs (the funnel shifts of
      // glvq::shift are selected as v_alignbit), so the bits are brought back; the branch below is then s_cbranch_scc
      const bool ba = uniform(a[3]) >> 31, bb = uniform(b[3]) >> 31;
      if (ba || bb) {
        q28::sel(p, ba, p1, p2);
        q28::sel(p, ba && bb, p3, p);
        q28::add(acc, p);
      }
      glvq::shift(a, b);
    }
  }
  // acc - krG == infinity  <=>  acc == krG, infinity included
  if (glvq::load_affine(x, y, points, 2 * (size_t)t + 1)) {
    F28 yn, z;
    d28::set_zero(z);
    d28::sub<4>(yn, z, y);  // 4p - y
    q28::from_affine(p, x, yn);
    q28::add(acc, p);
  }
  const bool owned = q28::is_inf(acc);
  if (q28::role() == 0) *dst = owned ? CURDLE_TRACKER_OWNED : CURDLE_TRACKER_NOT_OWNED;
}

hipError_t launch_tracker_own(const void* points, const uint8_t* status, const void* keys, uint32_t t0, uint32_t cnt,
                              uint32_t key0, uint32_t nkeys, uint8_t* out, size_t stride, hipStream_t stream) {
  if (cnt == 0 || nkeys == 0) return hipSuccess;
  if (nkeys > 65535u) return hipErrorInvalidValue;  // a grid dimension
  const u32 bx = (cnt + kBlockTrackers - 1) / kBlockTrackers;
  if (bx > 65535u) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_tracker_own, dim3(bx, nkeys), dim3(kBlock), 0, stream, (const uint4*)points, status,
                     (const uint4*)keys, (u32)t0, (u32)cnt, (u32)key0, stride, out);
  return hipGetLastError();
}

}  // namespace curdle
