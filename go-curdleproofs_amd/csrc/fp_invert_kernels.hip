// Batched inversion in Fp, one lane per element: out[i] = in[i]^-1, 0 -> 0, with an instruction stream and an address
// stream that do not depend on the elements.  One kernel in four builds, k_fp_invert<Fermat, Raw>:
//
//   Fermat false   the division steps of invert_ds.h: 1,110 masked shift-and-add steps in batches of 30;
//   Fermat true    the fixed exponent chain of invert28.h (the exponent is p - 2 for every lane: its window switch is
//                  wave-uniform and public), the control: the same words out;
//   Raw false      items are gnark fp.Elements: 48 bytes, Montgomery radix 2^384, canonical in and out;
//   Raw true       items are the 14 u32 limbs of fp28.h (56 bytes, Montgomery radix 2^392): normalised and below 2p in,
//                  canonical out -- a diagnostic form that reaches invert_ds(F28&, const F28&) as the MSM's exit calls it.
//
// A lane loads its own item (an address made of the lane index), checks its range by a borrow chain -- at or above p; in
// the raw form at or above 2p, or a limb at or above 2^28 -- and ORs the verdict, with the violation word of the division
// steps, into ONE status word by an unconditional per-lane atomic OR of 0 or 1: no branch is taken on it.  An item out of
// range is inverted like any other (whatever comes out is stored; the host form never hands it on).  The lane reads its
// item before it writes it and touches no other: out may be in.
//
// Plain loads and stores, one atomic OR, no LDS, no inline assembly beyond the field layer's.
#include <hip/hip_runtime.h>

#include "msm_kernels_common.h"
#include "g1_exit_ct.h"
#include "invert_ds.h"

namespace curdle {

namespace {
// 2p on fp28.h's limbs
__device__ __forceinline__ u32 k2P28(int i) {
  constexpr u32 t[14] = {0xfff5556u, 0xfdfffffu, 0x7ffff73u, 0xfffd62au, 0xc483d57u, 0x41ed61eu, 0xece61a5u,
                         0xe70a257u, 0x8ee9709u, 0x9759aecu, 0x74f6c86u, 0xcd34963u, 0x3d472ffu, 0x0034022u};
  return t[i];
}
}  // namespace

template <bool Fermat, bool Raw>
__global__ void __launch_bounds__(kBlock) k_fp_invert(const void* __restrict__ in, u32 n, void* out, u32* status) {
  const u32 i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  u32 viol;
  if constexpr (Raw) {
    F28 a, y;
    const uint2* src = reinterpret_cast<const uint2*>(in) + 7 * (size_t)i;  // 56 bytes an item: 8-byte words
#pragma unroll
    for (int j = 0; j < 7; j++) {
      const uint2 v = src[j];
      a.l[2 * j] = v.x;
      a.l[2 * j + 1] = v.y;
    }
    u32 wide = 0, borrow = 0;
#pragma unroll
    for (int j = 0; j < d28::N; j++) {
      wide |= a.l[j] >> 28;
      borrow = (a.l[j] - k2P28(j) - borrow) >> 31;  // limbs below 2^28: bit 31 of the difference is the borrow
    }
    viol = ((wide | (0u - wide)) >> 31) | (borrow ^ 1u);  // a wide limb, or no borrow: at or above 2p
    if constexpr (Fermat)
      invert(y, a);
    else
      viol |= invert_ds(y, a);
    u32 c[d28::N];
    ds::canonical28_ct(c, y.l);
    uint2* dst = reinterpret_cast<uint2*>(out) + 7 * (size_t)i;
#pragma unroll
    for (int j = 0; j < 7; j++) dst[j] = make_uint2(c[2 * j], c[2 * j + 1]);
  } else {
    u32 w[12], o[12];
    d28::load_words<12>(w, reinterpret_cast<const uint4*>(in) + 3 * (size_t)i);
    u32 borrow = 0;
#pragma unroll
    for (int j = 0; j < 12; j++) {
      const u64 t = (u64)w[j] - FpParams::mod(j) - borrow;
      borrow = (u32)(t >> 32) & 1u;
    }
    viol = borrow ^ 1u;  // no borrow: at or above p
    if constexpr (Fermat) {
      F28 a, y;
      d28::from_gnark(a, w);
      invert(y, a);
      to_gnark_ct<d28::kToExt>(o, y);
    } else {
      viol |= invert_ds_gnark(o, w);
    }
    d28::store_words<12>(reinterpret_cast<uint4*>(out) + 3 * (size_t)i, o);
  }
  // Unconditional, 0 or 1.  The address is made of the lane index (i < 2^31: always word 0) so that it is a per-lane
  // atomic, as in msm_ct_lane.h.
  atomicOr(status + (i >> 31), viol);
}

hipError_t launch_fp_invert(const void* in, uint32_t n, void* out, int fermat, int raw, uint32_t* status, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  if (n > kFpInvertPass) return hipErrorInvalidValue;
  const dim3 grid(cdiv(n, kBlock)), block(kBlock);
  if (fermat && raw)
    hipLaunchKernelGGL((k_fp_invert<true, true>), grid, block, 0, stream, in, (u32)n, out, status);
  else if (fermat)
    hipLaunchKernelGGL((k_fp_invert<true, false>), grid, block, 0, stream, in, (u32)n, out, status);
  else if (raw)
    hipLaunchKernelGGL((k_fp_invert<false, true>), grid, block, 0, stream, in, (u32)n, out, status);
  else
    hipLaunchKernelGGL((k_fp_invert<false, false>), grid, block, 0, stream, in, (u32)n, out, status);
  return hipGetLastError();
}

}  // namespace curdle
