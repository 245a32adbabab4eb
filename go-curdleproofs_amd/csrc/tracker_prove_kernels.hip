// The small kernels of the batched Whisk tracker-proof generator (tracker_api.hip): k calls of
// GenerateWhiskTrackerProof (the reference's whisk/whisk.go:149-175) in one.  The three scalar multiplications of a
// member, kG = k G, A = b G and B = b rG (:156-159), run as 3 n pairs of ONE launch_scalar_mul_batch and leave as
// bytes through launch_g1_compress; the transcript (:161-169) is the verifier's tape on launch_transcript_batch.
// What is left is movement and one Fr product per member:
//   k_tracker_prove_pairs  lays the 3 n (point, scalar) pairs out for the scalar multiplication;
//   k_tracker_prove_rows   writes the transcript rows in the layout k_tracker_gather defines;
//   k_tracker_response     s = b - c k (:171-172) and the 128 bytes A | B | s of every member.
#include <hip/hip_runtime.h>

#include "../../include/curdle_msm.h"
#include "bls12_381.h"
#include "msm_kernels.h"

namespace curdle {

static constexpr int kBlock = 256;

namespace {
constexpr u32 kRowWords = 38;  // transcript::TapeRowWords(6 * 48)
}

// Pair j < 2 n has the generator as its point; pair 2 n + i has rG_i, the decoded record 2 i (all zero = infinity
// where it did not decode or is infinity: b * inf = inf).  Eight lanes per pair: six move the point's 16-byte words,
// two copy b_i from the second third of the scalars to the last.
__global__ void __launch_bounds__(kBlock)
    k_tracker_prove_pairs(const uint4* __restrict__ decoded, G1Affine gen, u32 n, uint4* __restrict__ points,
                          uint4* __restrict__ scalars) {
  const u32 t = blockIdx.x * kBlock + threadIdx.x;
  const u32 j = t >> 3, w = t & 7u;
  if (j >= 3 * n) return;
  if (w < 6) {
    uint4 v = make_uint4(0, 0, 0, 0);
    if (j < 2 * n) {
#pragma unroll
      for (u32 q = 0; q < 3; q++) {
        if (w == q) v = make_uint4(gen.x.l[4 * q], gen.x.l[4 * q + 1], gen.x.l[4 * q + 2], gen.x.l[4 * q + 3]);
        if (w == q + 3) v = make_uint4(gen.y.l[4 * q], gen.y.l[4 * q + 1], gen.y.l[4 * q + 2], gen.y.l[4 * q + 3]);
      }
    } else {
      v = decoded[12 * (size_t)(j - 2 * n) + w];
    }
    points[6 * (size_t)j + w] = v;
  } else if (j >= 2 * n) {
    scalars[2 * (size_t)j + (w - 6)] = scalars[2 * (size_t)(j - n) + (w - 6)];
  }
}

__global__ void __launch_bounds__(kBlock)
    k_tracker_prove_rows(const uint64_t* __restrict__ trackers, const uint64_t* __restrict__ comp,
                         const uint64_t* __restrict__ gen, u32 n, uint64_t* __restrict__ rows) {
  const u32 t = blockIdx.x * kBlock + threadIdx.x;
  const u32 i = t / kRowWords, w = t % kRowWords;
  if (i >= n) return;
  uint64_t v = 0;
  if (w >= 1 && w <= 36) {
    const u32 u = w - 1;  // six words each of kG, g1Gen, krG, rG, A, B
    if (u < 6) v = comp[6 * (size_t)i + u];
    else if (u < 12) v = gen[u - 6];
    else if (u < 18) v = trackers[12 * (size_t)i + 6 + (u - 12)];
    else if (u < 24) v = trackers[12 * (size_t)i + (u - 18)];
    else if (u < 30) v = comp[6 * ((size_t)n + i) + (u - 24)];
    else v = comp[6 * (2 * (size_t)n + i) + (u - 30)];
  }
  rows[kRowWords * (size_t)i + w] = v;
}

// One lane per member.  c arrives canonical (the transcript kernel's 32 big-endian bytes, < r) and k in Montgomery
// form, so ONE Montgomery product gives c k canonical; b leaves Montgomery form and s = b - c k is written big-endian
// (fr.Element.Bytes, types.go:126).
__global__ void __launch_bounds__(kBlock)
    k_tracker_response(const uint4* __restrict__ comp, const u32* __restrict__ challenges,
                       const uint4* __restrict__ scalars, const uint8_t* __restrict__ status,
                       const uint8_t* __restrict__ sub, u32 n, uint4* __restrict__ proofs) {
  const u32 i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  uint4* out = proofs + 8 * (size_t)i;
  bool bad = false;
#pragma unroll
  for (u32 j = 2 * i; j < 2 * i + 2; j++)
    bad |= status[j] > CURDLE_DECODE_INFINITY || (status[j] == CURDLE_DECODE_OK && !sub[j]);
  if (bad) {
#pragma unroll
    for (int q = 0; q < 8; q++) out[q] = make_uint4(0, 0, 0, 0);
    return;
  }
  auto load = [](Fr& f, const uint4* src) {
    const uint4 lo = src[0], hi = src[1];
    f.l[0] = lo.x; f.l[1] = lo.y; f.l[2] = lo.z; f.l[3] = lo.w;
    f.l[4] = hi.x; f.l[5] = hi.y; f.l[6] = hi.z; f.l[7] = hi.w;
  };
  Fr k, b, c, ck, bc, s;
  load(k, scalars + 2 * (size_t)i);
  load(b, scalars + 2 * ((size_t)n + i));
#pragma unroll
  for (int w = 0; w < 8; w++) c.l[w] = __builtin_bswap32(challenges[8 * (size_t)i + 7 - w]);
  f_mul_inl<FrParams>(ck, c, k);
  f_from_mont<FrParams>(bc, b);
  f_sub<FrParams>(s, bc, ck);
  const uint4* A = comp + 3 * ((size_t)n + i);
  const uint4* B = comp + 3 * (2 * (size_t)n + i);
#pragma unroll
  for (int q = 0; q < 3; q++) {
    out[q] = A[q];
    out[3 + q] = B[q];
  }
  out[6] = make_uint4(__builtin_bswap32(s.l[7]), __builtin_bswap32(s.l[6]), __builtin_bswap32(s.l[5]), __builtin_bswap32(s.l[4]));
  out[7] = make_uint4(__builtin_bswap32(s.l[3]), __builtin_bswap32(s.l[2]), __builtin_bswap32(s.l[1]), __builtin_bswap32(s.l[0]));
}

hipError_t launch_tracker_prove_pairs(const void* decoded, const G1Affine& gen, uint32_t n, void* points, void* scalars,
                                      hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_tracker_prove_pairs, dim3((unsigned)(((uint64_t)24 * n + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream,
                     (const uint4*)decoded, gen, (u32)n, (uint4*)points, (uint4*)scalars);
  return hipGetLastError();
}

hipError_t launch_tracker_prove_rows(const void* trackers, const void* comp, const void* gen, uint32_t n, void* rows,
                                     hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_tracker_prove_rows, dim3((unsigned)(((uint64_t)kRowWords * n + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                     stream, (const uint64_t*)trackers, (const uint64_t*)comp, (const uint64_t*)gen, (u32)n, (uint64_t*)rows);
  return hipGetLastError();
}

hipError_t launch_tracker_response(const void* comp, const void* challenges, const void* scalars, const uint8_t* status,
                                   const uint8_t* sub, uint32_t n, void* proofs, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_tracker_response, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, (const uint4*)comp,
                     (const u32*)challenges, (const uint4*)scalars, status, sub, (u32)n, (uint4*)proofs);
  return hipGetLastError();
}

}  // namespace curdle
