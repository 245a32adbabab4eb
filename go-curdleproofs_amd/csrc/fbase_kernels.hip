// Fixed-base scalar multiplication in G1 on the GPU: out_i = (s_i * m_i mod r) * P for n scalars and ONE point P whose
// multiples are precomputed, table[w * 255 + d - 1] = d * 2^(8 w) * P for the 32 windows w of 8 bits and the digits
// d = 1..255 (curdle_host_fixed_base_table builds them, fbase_api.hip converts them once).  k * P is then at most 32
// mixed additions and NO doubling, against the 127 doublings and up to 127 additions of the GLV chain of
// k_scalar_mul_batch_quad (group_kernels.hip): what computeTracker / getKComm (whisk/whisk_test.go:98-109) need for
// every validator at once, tracker = (r G, k r G), commitment = k G -- every one a multiple of the generator.
//
// A throughput kernel of the kind k_accumulate is: ONE LANE per scalar, d28::madd<true> from a gathered table at ONE
// addition site.  A lane reads its scalar (a Montgomery fr.Element, 8 words), multiplies it by its multiplier in Fr if
// a multiplier array is given, takes the product out of Montgomery form (canonical, below r) and walks its 32 unsigned
// 8-bit digits from window 0 upward; the entry of the next non-skipped window is loaded before the addition of this
// one.  The result leaves as G1XYZZ in gnark limbs, all four coordinates zero for infinity (ZZ = 0 is what
// launch_g1_normalize and launch_g1_compress read), the form launch_scalar_mul_batch writes.
//
// The table is what launch_convert_points_raw makes of the affine multiples: records of d28::A28, kA28Bytes apart, on
// the curve the MSM's bases are mapped to (fp28.h from_gnark_iso; the XYZZ formulas for a = 0 never use the constant
// term), so the four coordinates leave through d28::to_gnark_msm like every MSM result.  8,160 records of one
// 128-byte line each, 1,044,480 bytes: inside one XCD's 4 MiB L2.
//
// Exactness.  The digits are unsigned, the scalar is canonical (k < r) and P is in the prime-order subgroup (checked
// when the table is made).  Before window w the accumulator is m P with m = k mod 2^(8 w) < 2^(8 w); the addend is
// d 2^(8 w) P with d >= 1.  So m < 2^(8 w) <= d 2^(8 w): the accumulator is never + the addend; and m + d 2^(8 w) <= k
// < r: it is never - the addend either (that would need m + d 2^(8 w) = 0 mod r).  The only exceptional step is the
// first addition, into infinity.  d28::madd handles every exceptional case anyway (equal points double, opposite points
// give infinity), and nothing here relies on the argument: it says what the tests' digit families can reach, and the
// big-integer model (tests/fbase_model.py) asserts it on every case it emits.
//
// Divergence.  A zero digit (1 in 256) skips its addition; the first non-zero digit takes madd's is_inf path, which is
// window 0 for all but one scalar in 256 and so uniform over a wave in practice.  Nothing is done against either.
//
// THE KERNEL READS TABLE ENTRIES AT ADDRESSES CHOSEN BY SCALAR DIGITS and skips zero digits: its memory access
// pattern and its running time depend on the scalars.  It is not a constant-time multiplication.
//
// Plain vector loads and stores, no LDS, no scratch.
#include <hip/hip_runtime.h>

#include "msm_kernels_common.h"

namespace curdle {

namespace {
__device__ __forceinline__ void load_fr(Fr& f, const uint4* __restrict__ src) {
  const uint4 lo = src[0], hi = src[1];
  f.l[0] = lo.x; f.l[1] = lo.y; f.l[2] = lo.z; f.l[3] = lo.w;
  f.l[4] = hi.x; f.l[5] = hi.y; f.l[6] = hi.z; f.l[7] = hi.w;
}
// the low digit of k, and k >> 8: every window is read from word 0, so no register is indexed by the window
__device__ __forceinline__ u32 next_digit(Fr& k) {
  const u32 d = k.l[0] & 0xffu;
#pragma unroll
  for (int j = 0; j < 7; j++) k.l[j] = (k.l[j] >> 8) | (k.l[j + 1] << 24);
  k.l[7] >>= 8;
  return d;
}
__device__ __forceinline__ void store12(G1XYZZ* dst, int role, const u32 w[12]) {
  uint4* d = reinterpret_cast<uint4*>(reinterpret_cast<u32*>(dst) + 12 * role);
#pragma unroll
  for (int i = 0; i < 3; i++) d[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
}
}  // namespace

__global__ void __launch_bounds__(kBlock, 2)
    k_fbase_mul(const A28* __restrict__ table, const uint4* __restrict__ scalars, const uint4* __restrict__ multipliers,
                u32 n, G1XYZZ* __restrict__ out) {
  const u32 i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  Fr k;
  {
    Fr s;
    load_fr(s, scalars + 2 * (size_t)i);
    if (multipliers) {
      Fr m;
      load_fr(m, multipliers + 2 * (size_t)i);
      f_mul_inl<FrParams>(s, s, m);
    }
    f_from_mont<FrParams>(k, s);
  }
  X28 acc;
  d28::set_inf(acc);
  // a zero digit loads entry 0 of its window (a valid address) and skips the addition
  u32 d_next = next_digit(k);
  A28 pt_next;
  d28::load(pt_next, a28_at(table, d_next ? d_next - 1 : 0));
#pragma unroll 1
  for (u32 w = 0; w < 32; w++) {
    const u32 d = d_next;
    const A28 pt = pt_next;
    if (w + 1 < 32) {
      d_next = next_digit(k);
      d28::load(pt_next, a28_at(table, (w + 1) * 255u + (d_next ? d_next - 1 : 0)));
    }
    if (d == 0) continue;
    d28::madd<true>(acc, pt.x, pt.y);
  }
  u32 w12[12];
  G1XYZZ* dst = out + i;
  if (d28::is_inf(acc)) {
#pragma unroll
    for (int j = 0; j < 12; j++) w12[j] = 0;
#pragma unroll
    for (int role = 0; role < 4; role++) store12(dst, role, w12);
    return;
  }
  d28::to_gnark_msm(w12, acc.x, 0);
  store12(dst, 0, w12);
  d28::to_gnark_msm(w12, acc.y, 1);
  store12(dst, 1, w12);
  d28::to_gnark_msm(w12, acc.zz, 2);
  store12(dst, 2, w12);
  d28::to_gnark_msm(w12, acc.zzz, 3);
  store12(dst, 3, w12);
}

hipError_t launch_fbase_mul(const void* table28, const void* scalars, const void* multipliers, uint32_t n, void* out_xyzz,
                            hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_fbase_mul, dim3(cdiv(n, kBlock)), dim3(kBlock), 0, stream, reinterpret_cast<const A28*>(table28),
                     (const uint4*)scalars, (const uint4*)multipliers, (u32)n, (G1XYZZ*)out_xyzz);
  return hipGetLastError();
}

}  // namespace curdle
