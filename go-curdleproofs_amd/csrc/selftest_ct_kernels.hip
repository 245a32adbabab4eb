// Self-test operation 16 (curdle_selftest_op): the constant-time G1 layer -- g1_walk_ct.h, g1_add_ct.h, g1_exit_ct.h,
// invert28.h and the fixed-base step of fbase_walk_ct.h -- on raw limbs.  The words a test writes are the words the
// primitive sees, and every selector calls the production function from its header.  Test code only: nothing here
// carries a secret, and the kernels may use scratch.
//
//   in  (116 words)  sel | arg0 | arg1 | pad | A (X28, 56 words) | B (X28, 56 words)
//   out ( 60 words)  an X28, or 24 gnark words, or 14 limbs, from word 0 (the rest zero) | 4 flag words from word 56
//
//   sel  0  zero_mask(A.x)                          flag 0
//        1  finite_mask(the first 24 words of A)    flag 0
//        2  equal_mod_p(A.x, A.y)                   flag 0        A.x < 2p, A.y < 10p
//        3  to_gnark_ct<kToExt>(A.x)                12 words
//        4  to_gnark_ct<kToExtX16>(A.x)             12 words
//        5  to_gnark_ct<kToExtY64>(A.x)             12 words
//        6  invert(A.x)                             14 limbs
//        7  affine_words_ct(A)                      24 words
//        8  madd_bit(A, B.x, B.y, arg0, arg1)       X28           arg0 = bit, arg1 = started: 0 or all ones
//        9  madd_select(A, B.x, B.y, arg0, arg1)    X28           arg0 = nz,  arg1 = started
//       10  add_ct(A, B)                            X28
//       11  walk_ct over arg0 steps                 X28 | started | over
//           (x2, y2) = (A.x, A.y), the scalar is the first eight words of B, canonical; it is shifted left by
//           256 - arg0 one bit a step, every bit shifted out OR-ed into `over`, exactly as k_msm_ct_walk does
//
// All elements of one call share a selector (the host refuses anything else), so each selector is a kernel of its own
// and nothing branches on it.  Every operand is loaded from memory: no product sees a limb the compiler knows (the
// multiply-accumulate trap of DESIGN.md section 0).
#include <hip/hip_runtime.h>

#include "msm_kernels_common.h"
#include "msm_kernels.h"
#include "g1_walk_ct.h"
#include "g1_add_ct.h"
#include "g1_exit_ct.h"
#include "fbase_walk_ct.h"

namespace curdle {

namespace {
constexpr u32 kInW = 116, kOutW = 60;
static_assert(kSelftestTable[16].in_words == kInW && kSelftestTable[16].out_words == kOutW && kSelftestTable[16].lanes == 1,
              "operation 16's row of the table");
}  // namespace

template <u32 Sel>
__global__ void __launch_bounds__(kBlock, 1) k_selftest_ct(const u32* __restrict__ in, size_t n, u32* __restrict__ out) {
  static_assert(Sel < kSelftestCtSels, "selector");
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const u32* src = in + i * kInW;
  u32* dst = out + i * kOutW;
  X28 a, b;
  u32* a32 = reinterpret_cast<u32*>(&a);
  u32* b32 = reinterpret_cast<u32*>(&b);
  for (int k = 0; k < 56; k++) {
    a32[k] = src[4 + k];
    b32[k] = src[60 + k];
  }
  const u32 arg0 = src[1], arg1 = src[2];
  u32 o[kOutW];
  for (u32 k = 0; k < kOutW; k++) o[k] = 0;
  if constexpr (Sel == 0) {
    o[56] = zero_mask(a.x);
  } else if constexpr (Sel == 1) {
    o[56] = finite_mask(a32);
  } else if constexpr (Sel == 2) {
    o[56] = equal_mod_p(a.x, a.y);
  } else if constexpr (Sel == 3) {
    to_gnark_ct<d28::kToExt>(o, a.x);
  } else if constexpr (Sel == 4) {
    to_gnark_ct<d28::kToExtX16>(o, a.x);
  } else if constexpr (Sel == 5) {
    to_gnark_ct<d28::kToExtY64>(o, a.x);
  } else if constexpr (Sel == 6) {
    F28 r;
    invert(r, a.x);
    for (int k = 0; k < d28::N; k++) o[k] = r.l[k];
  } else if constexpr (Sel == 7) {
    affine_words_ct(o, a);
  } else if constexpr (Sel == 8 || Sel == 9 || Sel == 10) {
    if constexpr (Sel == 8) madd_bit(a, b.x, b.y, arg0, arg1);
    else if constexpr (Sel == 9) madd_select(a, b.x, b.y, arg0, arg1);
    else add_ct(a, b);
    for (int k = 0; k < 56; k++) o[k] = a32[k];
  } else {
    Fr s;
    for (int k = 0; k < 8; k++) s.l[k] = b32[k];
    const F28 x2 = a.x, y2 = a.y;
    u32 over = 0;
#pragma unroll 1
    for (u32 t = arg0; t < 256; t++) over |= next_bit_msb(s);
    X28 acc;
    const u32 started = walk_ct(acc, s, x2, y2, arg0);
    const u32* c32 = reinterpret_cast<const u32*>(&acc);
    for (int k = 0; k < 56; k++) o[k] = c32[k];
    o[56] = started;
    o[57] = over;
  }
  for (u32 k = 0; k < kOutW; k++) dst[k] = o[k];
}

namespace {
template <u32 Sel>
void launch_one(const uint32_t* d_in, size_t n, uint32_t* d_out, hipStream_t stream) {
  hipLaunchKernelGGL(k_selftest_ct<Sel>, dim3(cdiv(n, kBlock)), dim3(kBlock), 0, stream, d_in, n, d_out);
}
}  // namespace

hipError_t launch_selftest_ct(uint32_t sel, const uint32_t* d_in, size_t n, uint32_t* d_out, hipStream_t stream) {
  if (sel >= kSelftestCtSels || !d_in || !d_out) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  switch (sel) {
    case 0: launch_one<0>(d_in, n, d_out, stream); break;
    case 1: launch_one<1>(d_in, n, d_out, stream); break;
    case 2: launch_one<2>(d_in, n, d_out, stream); break;
    case 3: launch_one<3>(d_in, n, d_out, stream); break;
    case 4: launch_one<4>(d_in, n, d_out, stream); break;
    case 5: launch_one<5>(d_in, n, d_out, stream); break;
    case 6: launch_one<6>(d_in, n, d_out, stream); break;
    case 7: launch_one<7>(d_in, n, d_out, stream); break;
    case 8: launch_one<8>(d_in, n, d_out, stream); break;
    case 9: launch_one<9>(d_in, n, d_out, stream); break;
    case 10: launch_one<10>(d_in, n, d_out, stream); break;
    default: launch_one<11>(d_in, n, d_out, stream); break;
  }
  return hipGetLastError();
}

}  // namespace curdle
