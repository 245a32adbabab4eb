// The constant-time MSM over a RESIDENT, PUBLIC base set with the walk split into chunks (msm_ct_bases_api.hip).
// k = sum_j 2^(c j) d_j with c-bit digits d_j, so k P = sum_j d_j (2^(c j) P): the points 2^(c j) P are public arithmetic
// on public bases, made once (k_ct_bases_shift) and kept; lane (pair, j) then walks only the c bits of d_j over its own
// table point (k_msm_ct_walk_rows) and the terms go through the fold and the finish of msm_ct_kernels.hip unchanged.  The
// chain of a call is c steps instead of scalar_bits.  Two kernels; the rule of what may depend on a secret is the one
// of g1_walk_ct.h.
//
// k_ct_bases_shift.  One lane per base P_i (a gnark G1Affine record, (0, 0) = infinity): the accumulator starts as
// (x, y, 1, 1) -- zz = zzz = 0 for infinity, which d28::dbl keeps -- and takes c doublings between stores, for
// j = 1 ... C - 1, of 2^(c j) P_i as a gnark-form G1XYZZ record (192 bytes, what k_g1_normalize's XYZZ form reads) at
// staging[(j - 1) n + i].  d28::dbl has no exceptional arm and 2^(c j) P is never infinity for P of odd order.  PUBLIC
// arithmetic: no masks, and a branch on infinity is a branch on a public value.  The loops stay rolled (the
// multiply-accumulate trap of g1_walk_ct.h: the initial zz and zzz are constants).
//
// k_msm_ct_walk_rows.  The grid is (ceil(n / kBlock), Cb), Cb = ceil(bits / c) the chunks a scalar below 2^bits has;
// blockIdx.y = j is the chunk: block-uniform and public.  The ONE walk kernel of the family: the call's base sets -- up
// to four tables at one c, set s covering the indices [first_s, first_s + size_s) -- arrive by value (CtRowSets), and a
// call over one handle is the one-set case.  Lane p loads rows[p] (a PUBLIC index list the host checked against the
// sets' total), finds its set by three compares against the public first_s (selects, no indexed read of the argument;
// an empty set shares its first index with the next one and is never chosen) and loads the record
// table_s[j size_s + rows[p] - first_s] -- addresses made of public values only -- and its
// scalar at an address made of the lane index; the rest is msm_ct_lane (msm_ct_lane.h), the lane k_msm_ct_walk runs
// too.  The bits at or above `bits` are shifted out into the violation word
// with k_msm_ct_walk's loop (every chunk's lane of a pair ORs the same word), then the bits between the chunk's top and
// `bits` are shifted out by the same rolled loop, whose trip count is a function of j, c and bits alone; walk_ct over
// the chunk's step count -- c, or bits - c (Cb - 1) for the top chunk -- leaves d_j (2^(c j) P) and the lane stores it
// under started & finite at term[p Cb + j].  With that layout the terms of pair p are the run [p Cb, (p + 1) Cb) and
// those of pairs [begin, begin + count) the run [begin Cb, (begin + count) Cb): the (segmented) sum runs on it as it is.
//
// Exactness.  Q = 2^(c j) P has order r whenever P has (2 is invertible mod r), and the walk over Q is g1_walk_ct.h's
// walk of the scalar d_j < 2^c <= 2^64 < r: every kept sum is 2m Q + Q with 1 < 2m + 1 <= d_j < r, and since 2m + 1
// never reaches r not even a DISCARDED sum is exceptional.  The terms of one pair are multiples of one another and may
// be equal or opposite (d_0 = 2^c - 1, d_1 = 1, ...): the fold stays the complete add_ct.
//
// Plain loads and stores, one atomic OR, no LDS, no inline assembly beyond the field layer's.
#include <hip/hip_runtime.h>

#include "msm_kernels_common.h"
#include "g1_walk_ct.h"
#include "g1_add_ct.h"  // finite_mask
#include "msm_ct_lane.h"

namespace curdle {

__global__ void __launch_bounds__(kBlock, 2)
    k_ct_bases_shift(const uint4* __restrict__ points, u32 n, u32 c, u32 chunks, G1XYZZ* __restrict__ staging) {
  const u32 i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  u32 pw[24];
  d28::load_words<24>(pw, points + 6 * (size_t)i);
  const u32 finite = finite_mask(pw);  // public
  X28 acc;
  d28::from_gnark(acc.x, pw);
  d28::from_gnark(acc.y, pw + 12);
#pragma unroll
  for (int l = 0; l < d28::N; l++) acc.zz.l[l] = acc.zzz.l[l] = d28::kOne(l) & finite;
#pragma unroll 1
  for (u32 j = 1; j < chunks; j++) {
#pragma unroll 1
    for (u32 s = 0; s < c; s++) d28::dbl(acc);
    G1XYZZ g;
    d28::to_gnark(g, acc);
    d28::store_words<48>(staging + ((size_t)(j - 1) * n + i), reinterpret_cast<const u32*>(&g));
  }
}

__global__ void __launch_bounds__(kBlock, 2)
    k_msm_ct_walk_rows(const CtRowSets sets, const u32* __restrict__ rows, const uint4* __restrict__ scalars, u32 c, u32 bits, u32 n,
                       X28* __restrict__ term, u32* status) {
  const u32 p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= n) return;
  const u32 j = blockIdx.y, cb = gridDim.y;                 // the chunk and the chunk count: public
  const u32 steps = j + 1 < cb ? c : bits - c * (cb - 1);   // the top chunk is the short one
  const u32 skip = bits - (c * j + steps);                  // the bits between the chunk's top and `bits`
  // the lane's set: the last one whose first index is not above the row -- public values, three compares
  const u32 row = rows[p];
  const uint4* table = static_cast<const uint4*>(sets.table[0]);
  u32 size = sets.size[0], first = sets.first[0];
#pragma unroll
  for (int s = 1; s < kCtRowSetsMax; s++) {
    const bool in = row >= sets.first[s];
    table = in ? static_cast<const uint4*>(sets.table[s]) : table;
    size = in ? sets.size[s] : size;
    first = in ? sets.first[s] : first;
  }
  Fr k;
  {
    Fr s;
    load_fr_lane(s, scalars + 2 * (size_t)p);  // an address made of the lane index
    f_from_mont<FrParams>(k, s);
  }
  // the record's address is made of public values; the status word's of the lane index (p < 2^31: always word 0)
  msm_ct_lane(table + 6 * ((size_t)j * size + (row - first)), k, bits, skip, steps, reinterpret_cast<uint4*>(term + ((size_t)p * cb + j)),
              status + (p >> 31));
}

hipError_t launch_ct_bases_shift(const void* points, uint32_t n, uint32_t chunk_bits, uint32_t chunks, void* staging_xyzz,
                                 hipStream_t stream) {
  if (n == 0 || chunks < 2) return hipSuccess;
  if (chunk_bits < 1 || chunk_bits > 64 || (u64)n * chunks > ((u64)1 << 31)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_ct_bases_shift, dim3(cdiv(n, kBlock)), dim3(kBlock), 0, stream, (const uint4*)points, (u32)n,
                     (u32)chunk_bits, (u32)chunks, (G1XYZZ*)staging_xyzz);
  return hipGetLastError();
}

hipError_t launch_msm_ct_walk_rows(const CtRowSets& sets, const uint32_t* rows, const void* scalars, uint32_t chunk_bits,
                                   uint32_t bits, uint32_t n, void* term, uint32_t* status, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  if (bits < 1 || bits > 255 || chunk_bits < 1 || chunk_bits > 64) return hipErrorInvalidValue;
  const u32 cb = (bits + chunk_bits - 1) / chunk_bits;
  if ((u64)n * cb > ((u64)1 << 31)) return hipErrorInvalidValue;  // the term index is 32 bits
  for (int s = 0; s < kCtRowSetsMax; s++) {  // the ranges lie behind each other and a set with records has a table
    if (sets.first[s] != (s ? sets.first[s - 1] + sets.size[s - 1] : 0) || (sets.size[s] && !sets.table[s])) return hipErrorInvalidValue;
  }
  hipLaunchKernelGGL(k_msm_ct_walk_rows, dim3(cdiv(n, kBlock), cb), dim3(kBlock), 0, stream, sets, rows, (const uint4*)scalars,
                     (u32)chunk_bits, (u32)bits, (u32)n, (X28*)term, status);
  return hipGetLastError();
}

}  // namespace curdle
