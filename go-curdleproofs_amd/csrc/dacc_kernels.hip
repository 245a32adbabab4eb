// Scalar side of the device-resident accumulator (include/curdle_msm.h "Accumulator on the
// device").
//
// The reference's msmaccumulator keeps `map[G1Affine]fr.Element` and does
// `map[v_i] += alpha * x_i` per check (msmaccumulator/msmaccumulator.go:38-43), with the
// verifier's x vectors computed by O(n log n) host loops
// (innerproductargument/innerproductargument.go:223-234,
// samemultiscalarargument/samemultiscalarargument.go:267-277).  Here the map is an array of
// scalar slots indexed by base (CRS slots, then instance slots); ONE lane per slot walks the
// checks, finds the segments that cover its slot, evaluates the element of x it needs from
// the check's description and accumulates -- no hashing, no atomics, and the output array is
// what k_digits reads.  256-bit modular integer arithmetic, latency-trivial (a few hundred
// Fr products per lane).
#include <hip/hip_runtime.h>

#include "../../include/curdle_msm.h"
#include "msm_kernels.h"
#include "dacc_eval.h"

#include <atomic>

namespace curdle {

// The evaluation itself lives in dacc_eval.h (shared with k_dacc_front, msm_sort_kernels.hip).
static constexpr u32 kDaccLdsBudget = 120 * 1024;  // of the CU's 160 KiB (opt-in beyond 64 KiB, per device)

template <bool LDS>
__global__ void __launch_bounds__(dacc::kBlock)
    k_dacc_scalars(const curdle_dacc_check* __restrict__ checks_g, u32 n_checks, const uint4* __restrict__ pool_g, u32 pool_len,
                   u32 n_crs, u32 n_inst, uint4* __restrict__ out) {
  extern __shared__ uint4 lds_stage[];
  const dacc::View vw = dacc::setup(lds_stage, checks_g, n_checks, pool_g, pool_len, LDS, threadIdx.x, dacc::kBlock);
  const u32 slot = blockIdx.x * dacc::kBlock + threadIdx.x;
  if (slot >= n_crs + n_inst) return;
  const Fr acc = dacc::eval_slot(vw, slot, n_crs);
  dacc::store_fr(out, slot, acc);
}

// The member build (curdle_dacc_run_members): one row of n_tot = n_crs + n_inst + n_extra scalars per member of a batch group,
// rows back to back -- the scalar vectors of ONE batched MSM whose members share the resident bases.  The checks arrive
// grouped by member (first[j] .. first[j + 1] are member j's); lane (slot, member j) walks that run only, so a check is
// evaluated once per slot it covers, into its own member's row, by the element rules of every other build (eval_slot_range).
// The slots behind the resident ones are the loose pairs: loose pair e carries its scalar in its member's row and zero in
// every other.  A block whose member has no checks writes its zeros without staging anything.
template <bool LDS>
__global__ void __launch_bounds__(dacc::kBlock)
    k_dacc_scalars_members(const curdle_dacc_check* __restrict__ checks_g, u32 n_checks, const u32* __restrict__ first,
                           const uint4* __restrict__ pool_g, u32 pool_len, u32 n_crs, u32 n_inst, u32 n_extra,
                           const uint4* __restrict__ extra_scalars, const u32* __restrict__ extra_member, uint4* __restrict__ out) {
  extern __shared__ uint4 lds_stage[];
  const u32 j = blockIdx.y, n_res = n_crs + n_inst, n_tot = n_res + n_extra;
  const u32 c0 = first[j], c1 = first[j + 1];
  const u32 slot = blockIdx.x * dacc::kBlock + threadIdx.x;
  uint4* row = out + 2 * (size_t)j * n_tot;
  Fr acc;
  f_zero(acc);
  if (c0 == c1) {  // block-uniform
    if (slot >= n_tot) return;
    if (slot >= n_res && extra_member[slot - n_res] == j) acc = dacc::load_fr(extra_scalars, slot - n_res);
    dacc::store_fr(row, slot, acc);
    return;
  }
  const dacc::View vw = dacc::setup(lds_stage, checks_g, n_checks, pool_g, pool_len, LDS, threadIdx.x, dacc::kBlock);
  if (slot >= n_tot) return;
  if (slot < n_res)
    acc = dacc::eval_slot_range(vw, slot, n_crs, c0, c1);
  else if (extra_member[slot - n_res] == j)
    acc = dacc::load_fr(extra_scalars, slot - n_res);
  dacc::store_fr(row, slot, acc);
}

static std::atomic<unsigned long long> g_dacc_builds[4];
void dacc_count_build(int which) { g_dacc_builds[which & 3].fetch_add(1, std::memory_order_relaxed); }

static hipError_t dacc_lds_optin() {
  static std::atomic<uint32_t> done{0};
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  const uint32_t bit = 1u << (dev & 31);
  if (done.load(std::memory_order_acquire) & bit) return hipSuccess;
  e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_dacc_scalars<true>), hipFuncAttributeMaxDynamicSharedMemorySize, kDaccLdsBudget);
  if (e == hipSuccess)
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_dacc_scalars_members<true>), hipFuncAttributeMaxDynamicSharedMemorySize, kDaccLdsBudget);
  if (e == hipSuccess) done.fetch_or(bit, std::memory_order_release);
  return e;
}

hipError_t launch_dacc_scalars(const void* d_checks, uint32_t n_checks, const void* d_pool, uint32_t pool_len, uint32_t n_crs,
                               uint32_t n_inst, void* d_out, hipStream_t stream) {
  const uint32_t n = n_crs + n_inst;
  if (n == 0) return hipSuccess;
  const size_t need = dacc::lds_bytes(pool_len, n_checks, kDaccLdsBudget);
  const dim3 grid((n + dacc::kBlock - 1) / dacc::kBlock), block(dacc::kBlock);
  if (need) {
    hipError_t e = dacc_lds_optin();
    if (e != hipSuccess) return e;
    dacc_count_build(2);
    hipLaunchKernelGGL(k_dacc_scalars<true>, grid, block, need, stream, reinterpret_cast<const curdle_dacc_check*>(d_checks), n_checks,
                       reinterpret_cast<const uint4*>(d_pool), pool_len, n_crs, n_inst, reinterpret_cast<uint4*>(d_out));
  } else {
    dacc_count_build(3);
    hipLaunchKernelGGL(k_dacc_scalars<false>, grid, block, 0, stream, reinterpret_cast<const curdle_dacc_check*>(d_checks), n_checks,
                       reinterpret_cast<const uint4*>(d_pool), pool_len, n_crs, n_inst, reinterpret_cast<uint4*>(d_out));
  }
  return hipGetLastError();
}

// (the member build is not one of curdle_stat_dacc_builds' four: curdle_stat_dacc_members counts its accumulations)
hipError_t launch_dacc_scalars_members(const DaccMembers& m, void* d_out, hipStream_t stream) {
  const uint32_t n_tot = m.n_crs + m.n_inst + m.n_extra;
  if (n_tot == 0 || m.n_members == 0) return hipSuccess;
  if (m.n_members > 65535) return hipErrorInvalidValue;  // grid.y
  const size_t need = dacc::lds_bytes(m.pool_len, m.n_checks, kDaccLdsBudget);
  const dim3 grid((n_tot + dacc::kBlock - 1) / dacc::kBlock, m.n_members), block(dacc::kBlock);
  const curdle_dacc_check* ck = reinterpret_cast<const curdle_dacc_check*>(m.d_checks);
  const uint32_t* first = reinterpret_cast<const uint32_t*>(m.d_member_first);
  const uint4* pool = reinterpret_cast<const uint4*>(m.d_pool);
  const uint4* xs = reinterpret_cast<const uint4*>(m.d_extra_scalars);
  const uint32_t* xm = reinterpret_cast<const uint32_t*>(m.d_extra_member);
  if (need) {
    hipError_t e = dacc_lds_optin();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_dacc_scalars_members<true>, grid, block, need, stream, ck, m.n_checks, first, pool, m.pool_len, m.n_crs,
                       m.n_inst, m.n_extra, xs, xm, reinterpret_cast<uint4*>(d_out));
  } else {
    hipLaunchKernelGGL(k_dacc_scalars_members<false>, grid, block, 0, stream, ck, m.n_checks, first, pool, m.pool_len, m.n_crs,
                       m.n_inst, m.n_extra, xs, xm, reinterpret_cast<uint4*>(d_out));
  }
  return hipGetLastError();
}

static std::atomic<unsigned long long> g_dacc_members[3];
void dacc_count_members(int which, unsigned long long by) { g_dacc_members[which % 3].fetch_add(by, std::memory_order_relaxed); }

}  // namespace curdle

extern "C" int curdle_stat_dacc_members(unsigned long long out[3]) {
  if (!out) return CURDLE_EINVAL;
  for (int i = 0; i < 3; i++) out[i] = curdle::g_dacc_members[i].load(std::memory_order_relaxed);
  return CURDLE_OK;
}

extern "C" int curdle_stat_dacc_builds(unsigned long long out[4]) {
  if (!out) return CURDLE_EINVAL;
  for (int i = 0; i < 4; i++) out[i] = curdle::g_dacc_builds[i].load(std::memory_order_relaxed);
  return CURDLE_OK;
}
