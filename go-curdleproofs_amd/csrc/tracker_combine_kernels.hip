// The scalars of the combined tracker check (curdle_whisk_is_valid_tracker_proof_batch_combined, tracker_api.hip).
// The two equations of IsValidWhiskTrackerProof (whisk.go:136-144) of every member i of a pass, weighted by two
// 128-bit coefficients and summed, are ONE multi-scalar multiplication over the 5 n decoded records and G:
//
//     sum_i  rho_i (s_i G + c_i kG_i - A_i)  +  sigma_i (s_i rG_i + c_i krG_i - B_i)   ==  infinity
//
// k_tracker_combine, one lane per member, writes that MSM's scalars as Montgomery fr.Elements in the records' order
//     rG: sigma s     krG: sigma c     kG: rho c     A: -rho     B: -sigma
// and reduces rho s over its block: the generator's share of the block is ONE extra pair (G, sum) behind the 5 n
// records.  The coefficients come from one Keccak permutation per member (keccak_dev.h):
//     SHAKE256("curdle/tracker-combine/v1" | seed | le64(index of the member in the call))[0:32] = rho | sigma,
// 65 bytes, one rate block.  An excluded member (S >= r or a transcript without a challenge: skip; a record that did
// not decode; a decoded record outside the subgroup) gets five ZERO scalars and adds nothing to the block's sum, so
// none of its records reaches a bucket of the MSM.
#include <hip/hip_runtime.h>

#include "../../include/curdle_msm.h"
#include "bls12_381.h"
#include "keccak_dev.h"
#include "msm_kernels.h"

namespace curdle {

namespace {
constexpr int kCombineBlock = 256;

__device__ __forceinline__ void load_fr(Fr& f, const uint4* __restrict__ src) {
  const uint4 lo = src[0], hi = src[1];
  f.l[0] = lo.x; f.l[1] = lo.y; f.l[2] = lo.z; f.l[3] = lo.w;
  f.l[4] = hi.x; f.l[5] = hi.y; f.l[6] = hi.z; f.l[7] = hi.w;
}
__device__ __forceinline__ void store_fr(uint4* __restrict__ dst, const Fr& f) {
  dst[0] = make_uint4(f.l[0], f.l[1], f.l[2], f.l[3]);
  dst[1] = make_uint4(f.l[4], f.l[5], f.l[6], f.l[7]);
}
// Hides what the compiler knows about f's limbs.  The multiply-accumulate statements of mac_gfx950.inc take their
// carry word as a plain read-write operand ("+v", no early clobber) and write it before they have read every factor,
// so a factor limb the compiler KNOWS to equal the carry word's start value, zero, may be given the carry word's own
// register: the upper limbs of a 128-bit coefficient were, and a carry out of an earlier product then changed the
// factor (wrong scalars for about three coefficients in eight).  Limbs read from memory or left by a product are
// never known constants; the coefficients' limbs go through here.
__device__ __forceinline__ void opaque(Fr& f) {
#pragma unroll
  for (int i = 0; i < 8; i++) asm volatile("" : "+v"(f.l[i]));
}
// canonical (< r) -> Montgomery: times R^2 mod r (host_math.h fr_to_mont)
__device__ __forceinline__ void to_mont(Fr& r, const Fr& canonical) {
  constexpr u32 kR2[8] = {0xf3f29c6du, 0xc999e990u, 0x87925c23u, 0x2b6cedcbu, 0x7254398fu, 0x05d31496u, 0x9f59ff11u, 0x0748d9d9u};
  Fr rr;
#pragma unroll
  for (int i = 0; i < 8; i++) rr.l[i] = kR2[i];
  fr_mul(r, canonical, rr);
}
}  // namespace

// status, sub: the 5 n records' CURDLE_DECODE_* bytes and subgroup verdicts; sc: s then c per member, canonical,
// eight little-endian words each (k_tracker_challenge's layout); skip[i] != 0: S was refused or the transcript gave
// no challenge.  first: the index in the call of the pass's member 0.  scalars: 5 n + gridDim.x fr.Elements,
// points: the decoded records, of which only records 5 n + block (the generator) are written here.
__global__ void __launch_bounds__(kCombineBlock)
    k_tracker_combine(const uint8_t* __restrict__ status, const uint8_t* __restrict__ sub, const uint4* __restrict__ sc,
                      const uint8_t* __restrict__ skip, TrackerCombineSeed seed, uint64_t first, u32 n, G1Affine gen,
                      uint4* __restrict__ scalars, uint4* __restrict__ points) {
  __shared__ u32 part[8][kCombineBlock];  // limb-major: lane t reads and writes bank t mod 64
  const u32 tid = threadIdx.x;
  const u32 i = blockIdx.x * kCombineBlock + tid;
  Fr rs;
  f_zero(rs);
  if (i < n) {
    bool excluded = skip[i] != 0;
#pragma unroll
    for (u32 j = 0; j < 5; j++) {
      const u32 st = status[5 * (size_t)i + j];
      excluded |= st > CURDLE_DECODE_INFINITY || (st == CURDLE_DECODE_OK && sub[5 * (size_t)i + j] == 0);
    }
    Fr out[5];
#pragma unroll
    for (int j = 0; j < 5; j++) f_zero(out[j]);
    if (!excluded) {
      // one rate block of SHAKE256: the host has laid out prefix | seed | le64(0) | 0x1f; the index enters at bytes 57..64
      uint64_t a[25];
      const uint64_t idx = first + i;
#pragma unroll
      for (int w = 0; w < 9; w++) a[w] = seed.w[w];
#pragma unroll
      for (int w = 9; w < 25; w++) a[w] = 0;
      a[7] ^= idx << 8;
      a[8] ^= idx >> 56;
      a[16] ^= 0x8000000000000000ull;  // the last byte of the 136-byte rate
      keccak_f1600_dev(a);
      Fr rho, sigma, s, c;
      f_zero(rho);
      f_zero(sigma);
      rho.l[0] = (u32)a[0]; rho.l[1] = (u32)(a[0] >> 32); rho.l[2] = (u32)a[1]; rho.l[3] = (u32)(a[1] >> 32);
      sigma.l[0] = (u32)a[2]; sigma.l[1] = (u32)(a[2] >> 32); sigma.l[2] = (u32)a[3]; sigma.l[3] = (u32)(a[3] >> 32);
      opaque(rho);
      opaque(sigma);
      load_fr(s, sc + 4 * (size_t)i);
      load_fr(c, sc + 4 * (size_t)i + 2);
      to_mont(rho, rho);
      to_mont(sigma, sigma);
      to_mont(s, s);
      to_mont(c, c);
      fr_mul(out[0], sigma, s);
      fr_mul(out[1], sigma, c);
      fr_mul(out[2], rho, c);
      f_neg<FrParams>(out[3], rho);
      f_neg<FrParams>(out[4], sigma);
      fr_mul(rs, rho, s);
    }
    uint4* dst = scalars + 10 * (size_t)i;
#pragma unroll
    for (int j = 0; j < 5; j++) store_fr(dst + 2 * j, out[j]);
  }
  // the block's sum of rho s, mod r: a tree over LDS (every lane of the block arrives here)
#pragma unroll
  for (int w = 0; w < 8; w++) part[w][tid] = rs.l[w];
  __syncthreads();
  for (u32 stride = kCombineBlock / 2; stride > 0; stride >>= 1) {
    if (tid < stride) {
      Fr x, y;
#pragma unroll
      for (int w = 0; w < 8; w++) {
        x.l[w] = part[w][tid];
        y.l[w] = part[w][tid + stride];
      }
      fr_add(x, x, y);
#pragma unroll
      for (int w = 0; w < 8; w++) part[w][tid] = x.l[w];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const size_t pair = 5 * (size_t)n + blockIdx.x;
    scalars[2 * pair] = make_uint4(part[0][0], part[1][0], part[2][0], part[3][0]);
    scalars[2 * pair + 1] = make_uint4(part[4][0], part[5][0], part[6][0], part[7][0]);
#pragma unroll
    for (int q = 0; q < 3; q++) {
      points[6 * pair + q] = make_uint4(gen.x.l[4 * q], gen.x.l[4 * q + 1], gen.x.l[4 * q + 2], gen.x.l[4 * q + 3]);
      points[6 * pair + 3 + q] = make_uint4(gen.y.l[4 * q], gen.y.l[4 * q + 1], gen.y.l[4 * q + 2], gen.y.l[4 * q + 3]);
    }
  }
}

uint32_t tracker_combine_blocks(uint32_t n) { return (n + kCombineBlock - 1) / kCombineBlock; }

hipError_t launch_tracker_combine(const uint8_t* status, const uint8_t* sub, const void* sc, const uint8_t* skip,
                                  const TrackerCombineSeed& seed, uint64_t first, uint32_t n, const G1Affine& gen,
                                  void* scalars, void* points, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_tracker_combine, dim3(tracker_combine_blocks(n)), dim3(kCombineBlock), 0, stream, status, sub,
                     (const uint4*)sc, skip, seed, first, (u32)n, gen, (uint4*)scalars, (uint4*)points);
  return hipGetLastError();
}

}  // namespace curdle
