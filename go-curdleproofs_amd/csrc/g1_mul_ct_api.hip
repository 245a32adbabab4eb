// C ABI of the constant-time variable-base multiplication (g1_mul_ct_kernels.hip): curdle_g1_scalar_mul_batch_ex /
// _device_ex, the flagged forms of curdle_g1_scalar_mul_batch / _device, and curdle_stat_g1_mul_ct.  flags = 0 IS the
// call without flags (decode_api.hip, normalize_api.hip): these entry points hand it over untouched.
//
// CURDLE_G1_MUL_CONSTANT_TIME: out[i] = scalars[i or 0] * points[i] by k_g1_mul_ct, in passes of at most G1_MUL_CT_PASS
// pairs, one launch each, and NOTHING else on the device: the kernel normalises in the lane, so no pass runs
// k_g1_normalize and none moves curdle_stat_normalize.  Addends are refused: a final addition addend + k P can be
// exceptional depending on the secret.  A call takes ONE MSM slot, held by a SlotHold (api_helpers.h), for its stream
// and -- the host form -- its buffers: the scalars go through the slot's pinned staging and a device buffer, and both
// are on the call's WipeList, overwritten on the stream that used them on every way out.  The resident form reads the
// caller's scalars where they are and copies nothing.  No stream is made here and nothing is allocated once the slot's
// buffers have grown.
#include "api_helpers.h"

#include <algorithm>

namespace {
constexpr unsigned kKnownFlags = CURDLE_G1_MUL_CONSTANT_TIME;
constexpr size_t kMulCtMax = (size_t)1 << 24;
constexpr size_t kMulCtPassDefault = (size_t)1 << 20;

// scalars multiplied by k_g1_mul_ct | its launches; completed passes only
std::atomic<unsigned long long> g_mul_ct_stat[2];

size_t pass_size() {
  const long long knob = knobs::get(knobs::G1_MUL_CT_PASS);
  const size_t v = knob < 0 ? kMulCtPassDefault : (size_t)knob;
  return std::max<size_t>(256, v / 256 * 256);
}

int check_flags(unsigned flags) {
  if (flags & ~kKnownFlags) return fail(CURDLE_EINVAL, "unknown flag bits 0x%x", flags & ~kKnownFlags);
  return CURDLE_OK;
}

int refuse_addends(const void* addends) {
  if (addends) return fail(CURDLE_EINVAL, "CURDLE_G1_MUL_CONSTANT_TIME takes no addends");
  return CURDLE_OK;
}
}  // namespace

namespace curdle_api {
void count_g1_mul_ct_pass(size_t n) {
  g_mul_ct_stat[0].fetch_add(n, std::memory_order_relaxed);
  g_mul_ct_stat[1].fetch_add(1, std::memory_order_relaxed);
}
}  // namespace curdle_api

extern "C" int curdle_g1_scalar_mul_batch_ex(const uint64_t* points, const uint64_t* scalars, size_t n_scalars,
                                             const uint64_t* addends, size_t n, unsigned flags, uint64_t* out_affine) {
  if (int rc = check_flags(flags)) return rc;
  if (!flags) return curdle_g1_scalar_mul_batch(points, scalars, n_scalars, addends, n, out_affine);
  if (n && (!points || !scalars || !out_affine)) return fail(CURDLE_EINVAL, "null argument");
  if (n == 0) return CURDLE_OK;
  if (n_scalars != n && n_scalars != 1) return fail(CURDLE_EINVAL, "n_scalars must be n or 1");
  if (n > kMulCtMax) return fail(CURDLE_EINVAL, "n = %zu exceeds the supported 2^24 points", n);
  if (int rc = refuse_addends(addends)) return rc;
  SlotHold H(cur(), true, nullptr);
  WipeList W(H.stream());
  H.wipe_on_exit(&W, "constant-time multiplication: clearing the scalars");  // nothing of the scalars stays
  return H.run([&]() -> int {
    Slot& S = H.slot();
    const hipStream_t st = H.stream();
    const bool shared = n_scalars == 1;
    const size_t pass = pass_size(), cap = std::min(n, pass), scap = shared ? 1 : cap;
    int r;
    if ((r = ensure(S.points, cap * 96))) return r;    // the records, multiplied in place
    if ((r = ensure(S.scalars, scap * 32))) return r;
    if ((r = ensure_pinned(S, 0, scap * 32 + cap * 96))) return r;  // scalars | points
    if ((r = ensure_pinned(S, 1, cap * 96))) return r;
    W.note_device(S.scalars.p, scap * 32);
    W.note_host(S.h_stage[0], scap * 32);
    uint8_t* h_sc = static_cast<uint8_t*>(S.h_stage[0]);
    uint8_t* h_pt = h_sc + scap * 32;
    for (size_t lo = 0; lo < n; lo += pass) {
      const size_t cnt = std::min(pass, n - lo);
      if (!shared || lo == 0) {
        const size_t ns = shared ? 1 : cnt;
        memcpy(h_sc, scalars + 4 * (shared ? 0 : lo), 32 * ns);
        HIP_TRY(hipMemcpyAsync(S.scalars.p, h_sc, 32 * ns, hipMemcpyHostToDevice, st));
      }
      memcpy(h_pt, points + 12 * lo, 96 * cnt);
      HIP_TRY(hipMemcpyAsync(S.points.p, h_pt, 96 * cnt, hipMemcpyHostToDevice, st));
      HIP_TRY(launch_g1_mul_ct(S.points.p, 1, S.scalars.p, shared ? 1 : 0, (uint32_t)cnt, S.points.p, st));
      HIP_TRY(hipMemcpyAsync(S.h_stage[1], S.points.p, 96 * cnt, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      memcpy(out_affine + 12 * lo, S.h_stage[1], 96 * cnt);
      count_g1_mul_ct_pass(cnt);
    }
    return CURDLE_OK;
  });
}

extern "C" int curdle_g1_scalar_mul_batch_device_ex(const void* d_points, const void* d_scalars, size_t n_scalars,
                                                    const void* d_addends, size_t n, unsigned flags, void* d_out_affine,
                                                    void* stream) {
  if (int rc = check_flags(flags)) return rc;
  if (!flags) return curdle_g1_scalar_mul_batch_device(d_points, d_scalars, n_scalars, d_addends, n, d_out_affine, stream);
  if (n == 0) return CURDLE_OK;
  if (!d_points || !d_scalars || !d_out_affine) return fail(CURDLE_EINVAL, "null argument");
  if (n_scalars != n && n_scalars != 1) return fail(CURDLE_EINVAL, "n_scalars must be n or 1");
  if (n > kMulCtMax) return fail(CURDLE_EINVAL, "n = %zu exceeds the supported 2^24 points", n);
  if (!aligned16(d_points) || !aligned16(d_scalars) || !aligned16(d_addends) || !aligned16(d_out_affine))
    return fail(CURDLE_EINVAL, "device pointers must be multiples of 16");
  if (int rc = refuse_addends(d_addends)) return rc;
  SlotHold H(cur(), true, stream);
  return H.run([&]() -> int {
    const hipStream_t st = H.stream();
    const bool shared = n_scalars == 1;
    const size_t pass = pass_size();
    const uint8_t* p = static_cast<const uint8_t*>(d_points);
    const uint8_t* s = static_cast<const uint8_t*>(d_scalars);
    uint8_t* o = static_cast<uint8_t*>(d_out_affine);
    // a lane reads its record before it writes it and touches no other: d_out_affine may be d_points
    for (size_t lo = 0; lo < n; lo += pass) {
      const size_t cnt = std::min(pass, n - lo);
      HIP_TRY(launch_g1_mul_ct(p + 96 * lo, 1, s + (shared ? 0 : 32 * lo), shared ? 1 : 0, (uint32_t)cnt, o + 96 * lo, st));
      HIP_TRY(hipStreamSynchronize(st));
      count_g1_mul_ct_pass(cnt);
    }
    return CURDLE_OK;
  });
}

extern "C" int curdle_stat_g1_mul_ct(unsigned long long out[2]) { return read_stats(out, g_mul_ct_stat, 2); }
