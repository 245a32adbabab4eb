// Batched normalisation of G1 points on the GPU with a SHARED inversion: n points in memory -> n gnark G1Affine
// records (96 bytes: x then y, canonical Montgomery limbs; infinity is 96 zero bytes), the layout of every base array
// of this library -- what gnark's BatchJacobianToAffineG1 does on the host, and what curdle_host_batch_to_affine did
// for every result of a point kernel until now.  k_g1_compress (compress_kernels.hip) normalises too, but pays one
// Fermat inversion per point; here one inversion serves a whole group by Montgomery's trick.
//
// Two input forms, the template parameter (the two k_g1_compress reads):
//   kNormalizeJac   gnark G1Jac, 144 bytes (X, Y, Z): x = X / Z^2, y = Y / Z^3; the denominator d is Z;
//   kNormalizeXyzz  G1XYZZ in gnark limbs, 192 bytes (X, Y, ZZ, ZZZ), as k_scalar_mul_batch_quad writes it:
//                   x = X / ZZ, y = Y / ZZZ for ANY non-zero ZZ, ZZZ (they need not be z^2, z^3); d = ZZ ZZZ.
// A point whose d is 0 mod p is infinity, whatever X and Y hold: decided on the REDUCED value (a Montgomery product,
// below 2p, is 0 or p), so limbs that spell p, or ZZ != 0 with ZZZ = 0, are infinity as well.  Such a point, and
// every lane position beyond n, enters the shared product as 1: it can never reach a neighbour's result.
//
// THE GROUP IS ONE WAVE: 64 lanes with K points each (K = 1 or 8, the second template parameter; point k of a lane
// is base + 64 k + lane, so a wave's loads and stores of one k are neighbours).  Per lane a running product over its
// K denominators; across the wave an inclusive prefix and an inclusive suffix scan of the 64 lane products,
// Hillis-Steele, six steps of one product each, the operands moved with __shfl_up / __shfl_down (cross-lane moves).
// With K = 8 the lane's seven prefixes wait in LDS while the inversion runs (98 words a lane, word-interleaved over
// the lanes so that a wave's access is one bank row; beside the inversion's table they would not fit 256 registers),
// each read back by the lane that wrote it: there is no barrier in either build, and waves never meet -- a block is
// four waves for K = 1 and one wave for K = 8, so that six blocks' 24.5 KB of LDS fit a CU.
// Lane 63's prefix is the group's product T; every lane runs the ONE inversion of T (invert28.h: the digits are
// wave-uniform, so 64 lanes cost what one would), and 1 / (its own product) = T^-1 x (prefix of the lanes below) x
// (suffix of the lanes above).  The lane then walks its K points backwards -- at most 8 steps, the only loop over
// points -- peeling one denominator per step.  The dependent chain of a launch is one inversion, the 12 scan
// products and 3 + 9 K - 4 products (K = 1: 8).  No scratch, no global temporaries.
//
// The coordinates never enter or leave the internal form by a product of their own: a gnark limb vector read as it
// stands is the integer X 2^384, and its Montgomery product (radix 2^392) with the internal form a 2^392 of the
// inverted denominator power is X a 2^384 -- the gnark form of the result.  For XYZZ the two stored factors meet in
// one product, ZZ ZZZ 2^376, which is the internal form of d / 2^16; the group's inverse is multiplied once by 2^384
// (the internal form of 2^-8) and every x and y again comes out in gnark form.
#include <hip/hip_runtime.h>

#include "../../include/curdle_msm.h"
#include "fp28.h"
#include "invert28.h"
#include "msm_kernels.h"
#include "../host/knobs.h"

namespace curdle {

using d28::F28;

namespace {

// threads of a block: K = 1 four waves, as the other point kernels; K > 1 one wave (the LDS of its prefixes)
template <int K>
constexpr int block_threads() { return K == 1 ? 256 : 64; }

// the lane prefixes of a K > 1 block: [K - 1][14 limbs][64 lanes]
template <int K>
__device__ __forceinline__ u32* prefix_store() {
  __shared__ u32 sh[(K - 1) * d28::N * 64];
  return sh;
}

// 12 words of a coordinate at a multiple of 16, as the 14 limbs of the same integer; zero for a lane beyond n
__device__ __forceinline__ void load_raw(F28& r, const uint8_t* __restrict__ p, bool in_range) {
  u32 w[12];
#pragma unroll
  for (int k = 0; k < 12; k++) w[k] = 0;
  if (in_range) d28::load_words<12>(w, p);
  d28::unpack(r, w);
}

// The denominator of the record at `src` in internal form, below 2p: Z, or d / 2^16 for d = ZZ ZZZ.
template <int FORM>
__device__ __forceinline__ void denominator(F28& e, const uint8_t* __restrict__ src, bool in_range) {
  F28 a, b;
  load_raw(a, src + 96, in_range);
  if constexpr (FORM == kNormalizeJac) {
#pragma unroll
    for (int j = 0; j < d28::N; j++) b.l[j] = d28::kToInt(j);
  } else {
    load_raw(b, src + 144, in_range);
  }
  d28::mul(e, a, b);
}

}  // namespace

template <int FORM, int K>
__global__ void __launch_bounds__(block_threads<K>(), 2)
    k_g1_normalize(const uint8_t* __restrict__ in, u32 n, uint8_t* __restrict__ out) {
  static_assert(K >= 1 && K <= 8, "a lane walks at most 8 points");
  constexpr size_t kStride = FORM == kNormalizeJac ? 144 : 192;
  constexpr u32 kBlock = block_threads<K>();
  const u32 lane = threadIdx.x & 63u;
  const u32 base = ((blockIdx.x * kBlock + threadIdx.x) >> 6) * (64u * K);  // the wave's first point
  if (base >= n) return;  // whole waves leave together: every wave that stays has all 64 lanes in its scans

  // this lane's K denominators: run = e_0 .. e_{K-1}; prefix k = e_0 .. e_k
  F28 run;
  u32 finite = 0;
#pragma unroll
  for (int k = 0; k < K; k++) {
    const u32 i = base + 64u * k + lane;
    F28 e;
    denominator<FORM>(e, in + kStride * (size_t)i, i < n);
    if (d28::is_zero_lt2p(e))
      d28::set_one(e);
    else
      finite |= 1u << k;
    if (k == 0)
      run = e;
    else
      d28::mul(run, run, e);
    if constexpr (K > 1) {
      if (k < K - 1) {
        u32* pre = prefix_store<K>() + (k * d28::N) * 64 + lane;
#pragma unroll
        for (int j = 0; j < d28::N; j++) pre[64 * j] = run.l[j];
      }
    }
  }

  // pf: product of the lanes up to this one, sf: from this one up
  F28 pf = run, sf = run, a, b;
#pragma unroll 1
  for (u32 d = 1; d < 64; d <<= 1) {
#pragma unroll
    for (int j = 0; j < d28::N; j++) {
      const u32 up = __shfl_up(pf.l[j], d), down = __shfl_down(sf.l[j], d);
      a.l[j] = lane >= d ? up : d28::kOne(j);
      b.l[j] = lane + d < 64 ? down : d28::kOne(j);
    }
    d28::mul(pf, pf, a);
    d28::mul(sf, sf, b);
  }
  F28 total, inv;
#pragma unroll
  for (int j = 0; j < d28::N; j++) {
    const u32 up = __shfl_up(pf.l[j], 1), down = __shfl_down(sf.l[j], 1);
    a.l[j] = lane >= 1 ? up : d28::kOne(j);
    b.l[j] = lane < 63 ? down : d28::kOne(j);
    total.l[j] = __shfl(pf.l[j], 63);
  }
  d28::mul(run, a, b);  // the product of every OTHER lane
  invert(inv, total);   // no factor is 0 mod p and p is prime: neither is the product
  if constexpr (FORM == kNormalizeXyzz) {
#pragma unroll
    for (int j = 0; j < d28::N; j++) a.l[j] = d28::kToExt(j);
    d28::mul(inv, inv, a);
  }
  d28::mul(run, run, inv);  // 1 / (e_0 .. e_{K-1})

#pragma unroll
  for (int k = K - 1; k >= 0; k--) {
    const u32 i = base + 64u * k + lane;
    const bool in_range = i < n, fin = (finite >> k) & 1u;
    const uint8_t* src = in + kStride * (size_t)i;
    F28 ik = run;  // 1 / e_k
    if (k > 0) {
      F28 e;
      denominator<FORM>(e, src, in_range);
      if (!fin) d28::set_one(e);
      if constexpr (K > 1) {
        const u32* pre = prefix_store<K>() + ((k - 1) * d28::N) * 64 + lane;
        F28 pk;
#pragma unroll
        for (int j = 0; j < d28::N; j++) pk.l[j] = pre[64 * j];
        d28::mul(ik, run, pk);
      }
      d28::mul(run, run, e);
    }
    if constexpr (FORM == kNormalizeJac) {
      d28::sqr(a, ik);     // 1 / Z^2
      d28::mul(b, a, ik);  // 1 / Z^3
    } else {
      F28 t;
      load_raw(t, src + 144, in_range);
      d28::mul(a, ik, t);  // ZZZ / d = 1 / ZZ
      load_raw(t, src + 96, in_range);
      d28::mul(b, ik, t);  // ZZ / d = 1 / ZZZ
    }
    F28 t;
    u32 w[24];
    load_raw(t, src, in_range);
    d28::mul(a, t, a);
    d28::canonical_lt2p(a);
    d28::pack(w, a);
    load_raw(t, src + 48, in_range);
    d28::mul(b, t, b);
    d28::canonical_lt2p(b);
    d28::pack(w + 12, b);
    if (!fin) {
#pragma unroll
      for (int j = 0; j < 24; j++) w[j] = 0;
    }
    if (in_range) d28::store_words<24>(out + 96 * (size_t)i, w);
  }
}

static uint32_t normalize_lane_points(uint32_t n) {
  const long long forced = knobs::get(knobs::NORMALIZE_LANE_POINTS);
  if (forced == 1 || forced == 8) return (uint32_t)forced;
  return n > kNormalizeWideMin ? 8 : 1;
}

hipError_t launch_g1_normalize(const void* in, int form, uint32_t n, void* out, hipStream_t stream, uint32_t* groups) {
  if (groups) *groups = 0;
  if (n == 0) return hipSuccess;
  if (form != kNormalizeJac && form != kNormalizeXyzz) return hipErrorInvalidValue;
  const uint32_t K = normalize_lane_points(n), waves = (n + 64 * K - 1) / (64 * K);
  const uint32_t threads = K == 1 ? block_threads<1>() : block_threads<8>(), wpb = threads / 64;
  const dim3 grid((waves + wpb - 1) / wpb), block(threads);
  const uint8_t* src = (const uint8_t*)in;
  uint8_t* dst = (uint8_t*)out;
  if (form == kNormalizeJac && K == 1)
    hipLaunchKernelGGL((k_g1_normalize<kNormalizeJac, 1>), grid, block, 0, stream, src, n, dst);
  else if (form == kNormalizeJac)
    hipLaunchKernelGGL((k_g1_normalize<kNormalizeJac, 8>), grid, block, 0, stream, src, n, dst);
  else if (K == 1)
    hipLaunchKernelGGL((k_g1_normalize<kNormalizeXyzz, 1>), grid, block, 0, stream, src, n, dst);
  else
    hipLaunchKernelGGL((k_g1_normalize<kNormalizeXyzz, 8>), grid, block, 0, stream, src, n, dst);
  if (groups) *groups = waves;
  return hipGetLastError();
}

}  // namespace curdle
