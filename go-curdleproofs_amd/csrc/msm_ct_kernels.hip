// Constant-time multi-scalar multiplication: sum_i k_i P_i with an instruction stream and an address stream that do
// not depend on the scalars.  The twin of the bucket MSM (msm_sort_kernels.hip, msm_accumulate_kernel.hip), whose sort,
// bucket addresses and large-bucket queue are all functions of the scalars, in the manner of k_g1_mul_ct
// (g1_mul_ct_kernels.hip).  Seven kernels and two second builds of the finish; the rule of what may depend on a secret is the one of g1_walk_ct.h.
//
// k_msm_ct_walk.  One lane per (base, scalar) pair; behind the scalar's load the lane is msm_ct_lane (msm_ct_lane.h),
// shared with k_msm_ct_walk_rows.  The walk of g1_walk_ct.h with a PUBLIC step count `bits` (1...255,
// a kernel argument): the scalar is first shifted left by 256 - bits, one bit a step in a rolled loop whose trip count
// is the argument alone, and every bit shifted out is OR-ed into the lane's violation word; then walk_ct over `bits`
// steps.  The exactness argument of g1_walk_ct.h holds for every prefix of a scalar
// below r, so it holds for the low `bits` bits walked here.  The scalar is a gnark Montgomery fr.Element (32 bytes,
// f_from_mont in the lane) or a plain uint32 (the shuffle's permutation, so that the host does no field arithmetic on
// it): a kernel argument says which, and both loads are at addresses made of the lane index.  The violation word goes
// into ONE status word by an unconditional per-lane atomic OR of 0 or 1: no branch is taken on it.  The lane writes its term, an
// X28 record (224 bytes, not normalised), to term[i]: all-zero words when nothing was added (k = 0) or the base is
// infinity, which is public.  Nothing is normalised here: the terms never leave the workspace.
//
// k_g1_sum_ct.  One level of the FIXED fold-in-half order over the m terms: h = ceil(m / 2) and
// term[i] = add_ct(term[i], term[i + h]) for i < m - h, one lane per i; the host launches level after level with
// m <- h while m > kSumTail.  A level reads term[i + h] with i + h >= h and writes term[i] with i < m - h <= h: no lane
// reads what another writes.  Addresses and trip counts are functions of m alone.
//
// k_msm_ct_finish.  ONE block: the remaining levels (m <= kSumTail, so at most one addition per lane and level) with a
// barrier between them, then lane 0 normalises term[0] as k_g1_mul_ct does -- affine_words_ct of g1_exit_ct.h: one
// inversion, the masked canonical step -- and writes the 18 words curdle_msm_g1 returns, canonical (x, y, 1) or (1, 1, 0)
// for infinity, chosen by a mask on zz, and the status word behind them.
//
// k_g1_permute_ct.  out[i] = in[perm[i]] over 96-byte records with perm secret: lane i loads its own perm[i] (an
// address made of the lane index) and walks j = 0 ... n - 1, a public trip count with the address of in[j] made of j,
// accumulating in[j] & mask(perm[i] == j): n^2 record reads and no address made of perm.  `halves` record arrays of n
// records lie behind each other and are permuted alike (the shuffle's Ts | Us).
//
// k_fr_permute_ct.  The same gather over 32-byte records (Prove's permuted challenges; the records are bytes to it, not
// field elements): both kernels are instantiations of ONE body, gather_ct<W>, W the record's size in 16-byte words.
//
// k_permute_ct_seg<RecordBytes>.  k gathers of one n in one launch, over the same body: block (x, j) serves member j, whose
// records, entries and outputs are the j-th run of n in each array.  Lane i < n loads perm[j n + i] and walks
// t = 0 ... n - 1 over in[j n + t]: t is the same on every lane of a wave and j is the block's, so a record's address is
// wave-uniform and made of public values alone.  The mask is made of perm ^ t with t < n INSIDE the member's segment: an
// entry at or above n matches no t and gives a zero record, never a neighbour's.  One wave per block (kPermuteSegBlock):
// the gather is a chain of n dependent-free loads per lane and what it needs is waves on many CUs, not lanes per block --
// k members of n <= 64 are k waves on k CUs' SIMDs, where blocks of kBlock would leave three waves in four empty.
//
// k_g1_sum_ct_seg, k_msm_ct_finish_seg.  The same sum over k segments of ONE term array (the batched call: one walk over
// the concatenated pairs of k MSMs): MSM j owns term[begin_j, begin_j + count_j) and a PUBLIC table of (begin, count)
// says so.  Block (x, j) of k_g1_sum_ct_seg reads its entry at a wave-uniform address, derives the segment's size at
// this level from count_j and the level's number alone (m <- ceil(m / 2) once per earlier level, while m > kSumTail)
// and, if that is still above kSumTail, runs k_g1_sum_ct's level on the segment; the host launches levels while any
// segment is above kSumTail.  Block j of k_msm_ct_finish_seg recomputes where the levels left its segment
// (while m > kSumTail: m <- ceil(m / 2)), runs k_msm_ct_finish's tail on it and writes result j, 36 words, at
// out + 36 j; an empty segment (public) gives the infinity encoding; the status word follows the k results.  Per
// segment the order of additions is exactly k_g1_sum_ct's and k_msm_ct_finish's on that segment alone.
//
// k_msm_ct_finish_ds, k_msm_ct_finish_seg_ds.  The two finish kernels with the exit's inversion by division steps
// (invert_ds.h) in place of the Fermat chain: ONE body each with its Fermat twin (finish_block, finish_seg_block), ONE
// sum_tail and ONE write_result, the inversion a template parameter; the words out are the same.  The launchers take
// them under knob CT_FINISH_DIVSTEPS (finish_on_divsteps below).
//
// Plain loads and stores, one atomic OR, no LDS, no inline assembly beyond the field layer's.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../host/knobs.h"
#include "msm_kernels_common.h"
#include "g1_walk_ct.h"
#include "g1_add_ct.h"
#include "g1_exit_ct.h"
#include "msm_ct_lane.h"

namespace curdle {

__global__ void __launch_bounds__(kBlock, 2)
    k_msm_ct_walk(const uint4* __restrict__ points, const void* __restrict__ scalars, u32 form, u32 bits, u32 n,
                  X28* __restrict__ term, u32* status) {
  const u32 i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  Fr k;
  if (form == kMsmCtScalarU32) {  // a kernel argument: wave-uniform and public
#pragma unroll
    for (int j = 1; j < 8; j++) k.l[j] = 0;
    k.l[0] = static_cast<const u32*>(scalars)[i];  // an address made of the lane index: a vector load
  } else {
    Fr s;
    load_fr_lane(s, static_cast<const uint4*>(scalars) + 2 * (size_t)i);
    f_from_mont<FrParams>(k, s);
  }
  // all `bits` bits in one walk; the status word's address is made of the lane index (i < 2^31: always word 0)
  msm_ct_lane(points + 6 * (size_t)i, k, bits, 0, bits, reinterpret_cast<uint4*>(term + i), status + (i >> 31));
}

namespace {
// One level of the fold on one lane: term[i] = add_ct(term[i], term[i + h]).
__device__ __forceinline__ void sum_pair(X28* term, u32 i, u32 h) {
  X28 a, b;
  d28::load(a, term + i);
  d28::load(b, term + i + h);
  add_ct(a, b);
  d28::store(term + i, a);
}
}  // namespace

__global__ void __launch_bounds__(kBlock, 1) k_g1_sum_ct(X28* term, u32 m) {
  const u32 h = (m + 1) / 2;
  const u32 i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= m - h) return;
  sum_pair(term, i, h);
}

namespace {
// The levels one block runs, m <= kSumTail terms at `term`, with a barrier between them: every lane of the block.
__device__ __forceinline__ void sum_tail(X28* term, u32 m) {
#pragma unroll 1
  while (m > 1) {
    const u32 h = (m + 1) / 2;
#pragma unroll 1
    for (u32 i = threadIdx.x; i < m - h; i += kBlock) sum_pair(term, i, h);
    __threadfence_block();
    __syncthreads();
    m = h;
  }
}

// One lane: *term normalised into the 36 words curdle_msm_g1 returns.  Inv: the exit's inversion (g1_exit_ct.h).
template <class Inv>
__device__ __forceinline__ void write_result(const X28* term, u32* out) {
  X28 acc;
  d28::load(acc, term);
  const u32 fin = ~zero_mask(acc.zz);
  u32 w[24];
  affine_words_ct<Inv>(w, acc);  // infinity inverts 0 (which gives 0) and is masked away
#pragma unroll
  for (int j = 0; j < 12; j++) {
    const u32 one = FpParams::one(j);  // gnark's Montgomery 1
    out[j] = (w[j] & fin) | (one & ~fin);
    out[12 + j] = (w[12 + j] & fin) | (one & ~fin);
    out[24 + j] = one & fin;
  }
}
// The block of k_msm_ct_finish and of k_msm_ct_finish_ds: the tail, then lane 0 writes the result and the status word.
template <class Inv>
__device__ __forceinline__ void finish_block(X28* term, u32 m, const u32* status, u32* out) {
  sum_tail(term, m);
  if (threadIdx.x != 0) return;
  write_result<Inv>(term, out);
  out[36] = *status;
}

// Block j of k_msm_ct_finish_seg and of k_msm_ct_finish_seg_ds.
template <class Inv>
__device__ __forceinline__ void finish_seg_block(X28* term, const uint2* __restrict__ seg, const u32* status, u32* out) {
  const uint2 s = seg[blockIdx.x];  // a wave-uniform address
  u32* res = out + 36 * (size_t)blockIdx.x;
  if (blockIdx.x == 0 && threadIdx.x == 0) out[36 * (size_t)gridDim.x] = *status;
  if (s.y == 0) {  // an empty MSM: public
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int j = 0; j < 12; j++) {
      res[j] = res[12 + j] = FpParams::one(j);
      res[24 + j] = 0;
    }
    return;
  }
  u32 m = s.y;
#pragma unroll 1
  while (m > kMsmCtSumTail) m = (m + 1) / 2;  // where the level launches left the segment
  sum_tail(term + s.x, m);
  if (threadIdx.x != 0) return;
  write_result<Inv>(term + s.x, res);
}
}  // namespace

__global__ void __launch_bounds__(kBlock, 1) k_msm_ct_finish(X28* term, u32 m, const u32* status, u32* out) {
  finish_block<InvertFermat>(term, m, status, out);
}

// The same block with the division-step exit (invert_ds.h): the same words out.
__global__ void __launch_bounds__(kBlock, 1) k_msm_ct_finish_ds(X28* term, u32 m, const u32* status, u32* out) {
  finish_block<InvertDivsteps>(term, m, status, out);
}

// seg[j] = (begin_j, count_j), public.  `level` counts the launches before this one.
__global__ void __launch_bounds__(kBlock, 1) k_g1_sum_ct_seg(X28* term, const uint2* __restrict__ seg, u32 level) {
  const uint2 s = seg[blockIdx.y];  // a wave-uniform address
  u32 m = s.y;
#pragma unroll 1
  for (u32 l = 0; l < level && m > kMsmCtSumTail; l++) m = (m + 1) / 2;
  if (m <= kMsmCtSumTail) return;
  const u32 h = (m + 1) / 2;
  const u32 i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= m - h) return;
  sum_pair(term + s.x, i, h);
}

__global__ void __launch_bounds__(kBlock, 1)
    k_msm_ct_finish_seg(X28* term, const uint2* __restrict__ seg, const u32* status, u32* out) {
  finish_seg_block<InvertFermat>(term, seg, status, out);
}

__global__ void __launch_bounds__(kBlock, 1)
    k_msm_ct_finish_seg_ds(X28* term, const uint2* __restrict__ seg, const u32* status, u32* out) {
  finish_seg_block<InvertDivsteps>(term, seg, status, out);
}

namespace {
// The oblivious gather on one lane, over records of W 16-byte words: *dst = src[p] for p < n, a zero record otherwise.
// The lane walks j = 0 ... n - 1 (a public trip count), reads record j at an address made of j and keeps it under a
// mask made of p ^ j: p, the secret, reaches nothing but that mask.
template <int W>
__device__ __forceinline__ void gather_ct(const uint4* __restrict__ src, u32 p, u32 n, uint4* __restrict__ dst) {
  u32 acc[4 * W];
#pragma unroll
  for (int w = 0; w < 4 * W; w++) acc[w] = 0;
#pragma unroll 1
  for (u32 j = 0; j < n; j++) {
    const u32 d = p ^ j;
    const u32 m = ((d | (0u - d)) >> 31) - 1u;  // all ones iff p == j
#pragma unroll
    for (int q = 0; q < W; q++) {
      const uint4 v = src[W * (size_t)j + q];  // an address made of j
      acc[4 * q] |= v.x & m;
      acc[4 * q + 1] |= v.y & m;
      acc[4 * q + 2] |= v.z & m;
      acc[4 * q + 3] |= v.w & m;
    }
  }
#pragma unroll
  for (int q = 0; q < W; q++) dst[q] = make_uint4(acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]);
}
}  // namespace

__global__ void __launch_bounds__(kBlock)
    k_g1_permute_ct(const uint4* __restrict__ in, const u32* __restrict__ perm, u32 n, u32 halves, uint4* __restrict__ out) {
  const u32 g = blockIdx.x * kBlock + threadIdx.x;
  if (g >= n * halves) return;
  const u32 half = g / n, i = g - half * n;  // public
  const u32 p = perm[i];                     // an address made of the lane index
  gather_ct<6>(in + 6 * (size_t)half * n, p, n, out + 6 * (size_t)g);
}

__global__ void __launch_bounds__(kBlock)
    k_fr_permute_ct(const uint4* __restrict__ in, const u32* __restrict__ perm, u32 n, uint4* __restrict__ out) {
  const u32 i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const u32 p = perm[i];  // an address made of the lane index
  gather_ct<2>(in, p, n, out + 2 * (size_t)i);
}

static constexpr u32 kPermuteSegBlock = 64;

template <int RecordBytes>
__global__ void __launch_bounds__(kPermuteSegBlock)
    k_permute_ct_seg(const uint4* __restrict__ in, const u32* __restrict__ perm, u32 n, uint4* __restrict__ out) {
  static_assert(RecordBytes % 16 == 0, "records are whole 16-byte words");
  constexpr int W = RecordBytes / 16;
  const u32 i = blockIdx.x * kPermuteSegBlock + threadIdx.x;
  if (i >= n) return;                          // public
  const size_t base = (size_t)blockIdx.y * n;  // the member's segment: public, the block's
  const u32 p = perm[base + i];                // an address made of the lane index
  gather_ct<W>(in + W * base, p, n, out + W * (base + i));
}

hipError_t launch_msm_ct_walk(const void* points, const void* scalars, int scalar_form, uint32_t bits, uint32_t n, void* term,
                              uint32_t* status, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  if (n > (1u << 31) || bits < 1 || bits > 255 || (scalar_form != kMsmCtScalarFr && scalar_form != kMsmCtScalarU32)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_msm_ct_walk, dim3(cdiv(n, kBlock)), dim3(kBlock), 0, stream, (const uint4*)points, scalars,
                     (u32)scalar_form, (u32)bits, (u32)n, (X28*)term, status);
  return hipGetLastError();
}

namespace {
// finish launches on division steps | on Fermat
std::atomic<unsigned long long> g_finish_launches[2];

// Which build a finish launcher takes, counted as a launch of that build.  Knob CT_FINISH_DIVSTEPS: 1 always the _ds kernels, 0 never; unset: the
// library's rule, which is kCtFinishDivstepsDefault (msm_kernels.h) for every shape.
bool finish_on_divsteps() {
  const long long knob = knobs::get(knobs::CT_FINISH_DIVSTEPS);
  const bool ds = knob < 0 ? kCtFinishDivstepsDefault : knob != 0;
  g_finish_launches[ds ? 0 : 1].fetch_add(1, std::memory_order_relaxed);
  return ds;
}
}  // namespace

void msm_ct_finish_launches(unsigned long long out[2]) {
  out[0] = g_finish_launches[0].load(std::memory_order_relaxed);
  out[1] = g_finish_launches[1].load(std::memory_order_relaxed);
}

hipError_t launch_msm_ct_sum(void* term, uint32_t m, const uint32_t* status, void* out40, hipStream_t stream) {
  if (m == 0) return hipErrorInvalidValue;
  while (m > kMsmCtSumTail) {
    const u32 h = (m + 1) / 2;
    hipLaunchKernelGGL(k_g1_sum_ct, dim3(cdiv(m - h, kBlock)), dim3(kBlock), 0, stream, (X28*)term, (u32)m);
    if (hipError_t e = hipGetLastError()) return e;
    m = h;
  }
  if (finish_on_divsteps())
    hipLaunchKernelGGL(k_msm_ct_finish_ds, dim3(1), dim3(kBlock), 0, stream, (X28*)term, (u32)m, status, (u32*)out40);
  else
    hipLaunchKernelGGL(k_msm_ct_finish, dim3(1), dim3(kBlock), 0, stream, (X28*)term, (u32)m, status, (u32*)out40);
  return hipGetLastError();
}

hipError_t launch_msm_ct_sum_seg(void* term, const void* seg, const uint32_t* counts, uint32_t k, const uint32_t* status,
                                 void* out, uint32_t* levels, hipStream_t stream) {
  if (k == 0 || k > 65535) return hipErrorInvalidValue;
  u32 level = 0;
  for (;; level++) {
    // the widest addition count of this level, by the kernel's own rule
    u32 widest = 0;
    for (u32 j = 0; j < k; j++) {
      u32 m = counts[j];
      for (u32 l = 0; l < level && m > kMsmCtSumTail; l++) m = (m + 1) / 2;
      if (m > kMsmCtSumTail) widest = std::max(widest, m - (m + 1) / 2);
    }
    if (widest == 0) break;
    hipLaunchKernelGGL(k_g1_sum_ct_seg, dim3(cdiv(widest, kBlock), k), dim3(kBlock), 0, stream, (X28*)term, (const uint2*)seg, level);
    if (hipError_t e = hipGetLastError()) return e;
  }
  if (levels) *levels = level;
  if (finish_on_divsteps())
    hipLaunchKernelGGL(k_msm_ct_finish_seg_ds, dim3(k), dim3(kBlock), 0, stream, (X28*)term, (const uint2*)seg, status, (u32*)out);
  else
    hipLaunchKernelGGL(k_msm_ct_finish_seg, dim3(k), dim3(kBlock), 0, stream, (X28*)term, (const uint2*)seg, status, (u32*)out);
  return hipGetLastError();
}

hipError_t launch_g1_permute_ct(const void* in, const uint32_t* perm, uint32_t n, uint32_t halves, void* out, hipStream_t stream) {
  if (n == 0 || halves == 0) return hipSuccess;
  if ((u64)n * halves > ((u64)1 << 31)) return hipErrorInvalidValue;  // the lane index is 32 bits
  hipLaunchKernelGGL(k_g1_permute_ct, dim3(cdiv((u64)n * halves, kBlock)), dim3(kBlock), 0, stream, (const uint4*)in, perm,
                     (u32)n, (u32)halves, (uint4*)out);
  return hipGetLastError();
}

hipError_t launch_fr_permute_ct(const void* in, const uint32_t* perm, uint32_t n, void* out, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  if (n > (1u << 31)) return hipErrorInvalidValue;  // the lane index is 32 bits
  hipLaunchKernelGGL(k_fr_permute_ct, dim3(cdiv(n, kBlock)), dim3(kBlock), 0, stream, (const uint4*)in, perm, (u32)n, (uint4*)out);
  return hipGetLastError();
}

hipError_t launch_permute_ct_seg(const void* in, const uint32_t* perm, uint32_t n, uint32_t k, uint32_t record_bytes, void* out,
                                 hipStream_t stream) {
  if (n == 0 || k == 0) return hipSuccess;
  if (n > 65535 || k > 65535) return hipErrorInvalidValue;  // k is the grid's y
  const dim3 grid(cdiv(n, kPermuteSegBlock), k);
  if (record_bytes == 32)
    hipLaunchKernelGGL(k_permute_ct_seg<32>, grid, dim3(kPermuteSegBlock), 0, stream, (const uint4*)in, perm, (u32)n, (uint4*)out);
  else if (record_bytes == 96)
    hipLaunchKernelGGL(k_permute_ct_seg<96>, grid, dim3(kPermuteSegBlock), 0, stream, (const uint4*)in, perm, (u32)n, (uint4*)out);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace curdle
