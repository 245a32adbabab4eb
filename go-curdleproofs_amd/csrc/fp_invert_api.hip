// C ABI of the batched field inversion (fp_invert_kernels.hip): curdle_fp_invert_batch / _device and
// curdle_stat_fp_invert.  out[i] = in[i]^-1 in Fp, 0 -> 0, one lane per element, by the division steps of invert_ds.h or,
// under CURDLE_FP_INVERT_FERMAT, by the exponent chain of invert28.h -- the control: the same words.
//
// A call takes ONE MSM slot, held by a SlotHold (api_helpers.h), for its stream and -- the host form -- its buffers.  The
// elements are treated as secrets.  The host form uploads them in passes of kFpInvertPass through the slot's pinned
// staging into ONE device buffer of the call's size, which the launches invert in place, one per pass; only when every
// pass is done and the status word is clean do the results come back, through the second pinned staging, so that `out`
// stays untouched on CURDLE_EINVAL (and may be `in`).  The device buffer and both stagings are on the call's WipeList,
// overwritten on the stream that used them on every way out.  The resident form reads and writes the caller's arrays
// where they are and copies nothing but the status word.  No stream is made here and nothing is allocated once the
// slot's buffers have grown.
#include "api_helpers.h"

#include <algorithm>

namespace {
constexpr unsigned kKnownFlags = CURDLE_FP_INVERT_FERMAT | CURDLE_FP_INVERT_RAW28;
constexpr size_t kFpInvertMax = (size_t)1 << 24;

// calls | elements; completed calls that ran on a device only
std::atomic<unsigned long long> g_fp_invert_stat[2];

size_t item_bytes(unsigned flags) { return flags & CURDLE_FP_INVERT_RAW28 ? 56 : 48; }

// What both forms refuse before any device work, in the header's order (misalignment is the resident form's, behind it).
int check(const void* in, size_t n, const void* out, unsigned flags) {
  if (flags & ~kKnownFlags) return fail(CURDLE_EINVAL, "unknown flag bits 0x%x", flags & ~kKnownFlags);
  if (n && (!in || !out)) return fail(CURDLE_EINVAL, "null argument");
  if (n > kFpInvertMax) return fail(CURDLE_EINVAL, "n = %zu exceeds the supported 2^24 elements", n);
  return CURDLE_OK;
}

int refuse_range(unsigned flags) {
  return flags & CURDLE_FP_INVERT_RAW28 ? fail(CURDLE_EINVAL, "an element is not below 2p on normalised limbs")
                                        : fail(CURDLE_EINVAL, "an element is not below p");
}

// One launch per pass over n items at d_in -> d_out; the status word at d_status was zeroed on st.
int launch_passes(const uint8_t* d_in, uint8_t* d_out, size_t n, unsigned flags, uint32_t* d_status, hipStream_t st) {
  const size_t item = item_bytes(flags);
  for (size_t lo = 0; lo < n; lo += kFpInvertPass) {
    const size_t cnt = std::min<size_t>(kFpInvertPass, n - lo);
    HIP_TRY(launch_fp_invert(d_in + item * lo, (uint32_t)cnt, d_out + item * lo, (flags & CURDLE_FP_INVERT_FERMAT) != 0,
                             (flags & CURDLE_FP_INVERT_RAW28) != 0, d_status, st));
  }
  return CURDLE_OK;
}

void count_call(size_t n) {
  g_fp_invert_stat[0].fetch_add(1, std::memory_order_relaxed);
  g_fp_invert_stat[1].fetch_add(n, std::memory_order_relaxed);
}
}  // namespace

extern "C" int curdle_fp_invert_batch(const uint64_t* in, size_t n, uint64_t* out, unsigned flags) {
  if (int rc = check(in, n, out, flags)) return rc;
  if (n == 0) return CURDLE_OK;
  SlotHold H(cur(), true, nullptr);
  WipeList W(H.stream());
  H.wipe_on_exit(&W, "field inversion: clearing the elements and their inverses");
  return H.run([&]() -> int {
    Slot& S = H.slot();
    const hipStream_t st = H.stream();
    const size_t item = item_bytes(flags), pass = std::min<size_t>(n, kFpInvertPass);
    int r;
    if ((r = ensure(S.points, n * item))) return r;  // the elements, inverted in place
    if ((r = ensure(S.results, 16))) return r;       // the status word
    if ((r = ensure_pinned(S, 0, pass * item))) return r;
    if ((r = ensure_pinned(S, 1, pass * item + 16))) return r;  // a pass of results | the status word
    W.note_device(S.points.p, n * item);
    W.note_host(S.h_stage[0], pass * item);
    W.note_host(S.h_stage[1], pass * item);
    uint8_t* d = static_cast<uint8_t*>(S.points.p);
    uint32_t* d_status = static_cast<uint32_t*>(S.results.p);
    uint8_t* h_back = static_cast<uint8_t*>(S.h_stage[1]);
    const uint8_t* src = reinterpret_cast<const uint8_t*>(in);
    HIP_TRY(hipMemsetAsync(d_status, 0, 16, st));
    for (size_t lo = 0; lo < n; lo += pass) {
      const size_t cnt = std::min(pass, n - lo);
      memcpy(S.h_stage[0], src + item * lo, item * cnt);
      HIP_TRY(hipMemcpyAsync(d + item * lo, S.h_stage[0], item * cnt, hipMemcpyHostToDevice, st));
      if ((r = launch_passes(d + item * lo, d + item * lo, cnt, flags, d_status, st))) return r;
      HIP_TRY(hipStreamSynchronize(st));  // the staging is free again
    }
    HIP_TRY(hipMemcpyAsync(h_back + pass * item, d_status, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    uint32_t verdict;
    memcpy(&verdict, h_back + pass * item, 4);
    if (verdict) return refuse_range(flags);
    uint8_t* dst = reinterpret_cast<uint8_t*>(out);
    for (size_t lo = 0; lo < n; lo += pass) {
      const size_t cnt = std::min(pass, n - lo);
      HIP_TRY(hipMemcpyAsync(h_back, d + item * lo, item * cnt, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      memcpy(dst + item * lo, h_back, item * cnt);
    }
    count_call(n);
    return CURDLE_OK;
  });
}

extern "C" int curdle_fp_invert_batch_device(const void* d_in, size_t n, void* d_out, unsigned flags, void* stream) {
  if (int rc = check(d_in, n, d_out, flags)) return rc;
  if (!aligned16(d_in) || !aligned16(d_out)) return fail(CURDLE_EINVAL, "device pointers must be multiples of 16");
  if (n == 0) return CURDLE_OK;
  SlotHold H(cur(), true, stream);
  return H.run([&]() -> int {
    Slot& S = H.slot();
    const hipStream_t st = H.stream();
    int r;
    if ((r = ensure(S.results, 16))) return r;
    if ((r = ensure_pinned(S, 1, 16))) return r;
    uint32_t* d_status = static_cast<uint32_t*>(S.results.p);
    HIP_TRY(hipMemsetAsync(d_status, 0, 16, st));
    // a lane reads its item before it writes it and touches no other: d_out may be d_in
    if ((r = launch_passes(static_cast<const uint8_t*>(d_in), static_cast<uint8_t*>(d_out), n, flags, d_status, st))) return r;
    HIP_TRY(hipMemcpyAsync(S.h_stage[1], d_status, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    uint32_t verdict;
    memcpy(&verdict, S.h_stage[1], 4);
    if (verdict) return refuse_range(flags);
    count_call(n);
    return CURDLE_OK;
  });
}

extern "C" int curdle_stat_fp_invert(unsigned long long out[4]) {
  if (int rc = read_stats(out, g_fp_invert_stat, 2)) return rc;
  msm_ct_finish_launches(out + 2);  // the finish of the constant-time MSM: launches on division steps | on Fermat
  return CURDLE_OK;
}
