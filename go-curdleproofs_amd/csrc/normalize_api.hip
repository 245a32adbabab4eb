// C ABI of the batched G1 normalisation (normalize_kernels.hip): curdle_g1_normalize_batch / _device, gnark's
// BatchJacobianToAffineG1 on the GPU, and curdle_g1_scalar_mul_batch_device, the resident form of
// curdle_g1_scalar_mul_batch whose results stay on the device as affine points -- the layout every base array of
// this library has, so a device result can be the next call's device input.  All three run through an MSM slot held
// by a SlotHold (api_helpers.h): the slot lends its stream, the host form its buffers and pinned staging in
// passes of kNormalizePass points, the scalar multiplications their XYZZ workspace.  No stream is made here and
// nothing is allocated once the slot's buffers have grown.
#include "api_helpers.h"

#include <algorithm>

namespace {
static_assert(kNormalizeJac == CURDLE_G1_FORM_JAC && kNormalizeXyzz == CURDLE_G1_FORM_XYZZ, "the public forms are the kernel's");
constexpr size_t kNormalizeMax = (size_t)1 << 24;
constexpr size_t kNormalizePass = (size_t)1 << 20;  // up to 192 MB of points, 96 MB of results per pass

std::atomic<unsigned long long> g_nz_stat[2];  // points normalised on the device | inversion groups run

size_t record_bytes(int form) { return form == CURDLE_G1_FORM_JAC ? 144 : 192; }

// one launch of k_g1_normalize and its two counters
int normalize_launch(const void* d_in, int form, size_t n, void* d_out, hipStream_t st) {
  uint32_t groups = 0;
  HIP_TRY(launch_g1_normalize(d_in, form, (uint32_t)n, d_out, st, &groups));
  g_nz_stat[0].fetch_add(n, std::memory_order_relaxed);
  g_nz_stat[1].fetch_add(groups, std::memory_order_relaxed);
  return CURDLE_OK;
}

// Host points (d_in null: `points` is copied up and the records come back to `out`) or resident ones (d_in -> d_out,
// both device memory), on the slot's stream or the caller's.  The stream is synchronised before the slot is released.
int normalize_through_slot(Ctx& cx, const uint64_t* points, const void* d_in, int form, size_t n, uint64_t* out, void* d_out,
                           void* user_stream) {
  const size_t rec = record_bytes(form);
  SlotHold H(cx, true, user_stream);
  return H.run([&]() -> int {
    Slot& S = H.slot();
    const hipStream_t st = H.stream();
    int r;
    if (d_in) {
      if ((r = normalize_launch(d_in, form, n, d_out, st))) return r;
      HIP_TRY(hipStreamSynchronize(st));
      return CURDLE_OK;
    }
    const size_t cap = std::min(n, kNormalizePass);
    if ((r = ensure(S.points, cap * rec))) return r;
    if ((r = ensure(S.scalars, cap * 96))) return r;
    if ((r = ensure_pinned(S, 0, cap * rec))) return r;
    if ((r = ensure_pinned(S, 1, cap * 96))) return r;
    for (size_t lo = 0; lo < n; lo += kNormalizePass) {
      const size_t m = std::min(kNormalizePass, n - lo);
      // through the slot's pinned staging, not straight from the caller's pageable memory (decode_api.hip)
      memcpy(S.h_stage[0], reinterpret_cast<const uint8_t*>(points) + rec * lo, m * rec);
      HIP_TRY(hipMemcpyAsync(S.points.p, S.h_stage[0], m * rec, hipMemcpyHostToDevice, st));
      if ((r = normalize_launch(S.points.p, form, m, S.scalars.p, st))) return r;
      HIP_TRY(hipMemcpyAsync(S.h_stage[1], S.scalars.p, m * 96, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      memcpy(out + 12 * lo, S.h_stage[1], m * 96);
    }
    return CURDLE_OK;
  });
}

int check_form_and_count(int form, size_t n) {
  if (form != CURDLE_G1_FORM_JAC && form != CURDLE_G1_FORM_XYZZ) return fail(CURDLE_EINVAL, "unknown point form %d", form);
  if (n > kNormalizeMax) return fail(CURDLE_EINVAL, "n = %zu exceeds the supported 2^24 points", n);
  return CURDLE_OK;
}
}  // namespace

extern "C" int curdle_g1_normalize_batch(const uint64_t* points, int form, size_t n, uint64_t* out_affine) {
  if (n == 0) return CURDLE_OK;
  if (!points || !out_affine) return fail(CURDLE_EINVAL, "null argument");
  if (int rc = check_form_and_count(form, n)) return rc;
  return normalize_through_slot(cur(), points, nullptr, form, n, out_affine, nullptr, nullptr);
}

extern "C" int curdle_g1_normalize_batch_device(const void* d_points, int form, size_t n, void* d_out_affine, void* stream) {
  if (n == 0) return CURDLE_OK;
  if (!d_points || !d_out_affine) return fail(CURDLE_EINVAL, "null argument");
  if (int rc = check_form_and_count(form, n)) return rc;
  if (!aligned16(d_points) || !aligned16(d_out_affine)) return fail(CURDLE_EINVAL, "device pointers must be multiples of 16");
  return normalize_through_slot(cur(), nullptr, d_points, form, n, nullptr, d_out_affine, stream);
}

extern "C" int curdle_g1_scalar_mul_batch_device(const void* d_points, const void* d_scalars, size_t n_scalars,
                                                 const void* d_addends, size_t n, void* d_out_affine, void* stream) {
  if (n == 0) return CURDLE_OK;
  if (!d_points || !d_scalars || !d_out_affine) return fail(CURDLE_EINVAL, "null argument");
  if (n_scalars != n && n_scalars != 1) return fail(CURDLE_EINVAL, "n_scalars must be n or 1");
  if (n > kNormalizeMax) return fail(CURDLE_EINVAL, "n = %zu exceeds the supported 2^24 points", n);
  if (!aligned16(d_points) || !aligned16(d_scalars) || !aligned16(d_addends) || !aligned16(d_out_affine))
    return fail(CURDLE_EINVAL, "device pointers must be multiples of 16");
  SlotHold H(cur(), true, stream);
  return H.run([&]() -> int {
    Slot& S = H.slot();
    const hipStream_t st = H.stream();
    int r;
    // every result is in the slot's workspace before the first record is written: the output may be d_points or d_addends
    if ((r = ensure(S.sorted, n * sizeof(G1XYZZ)))) return r;
    HIP_TRY(launch_scalar_mul_batch(d_points, d_scalars, n_scalars == 1 ? 1 : 0, d_addends, (uint32_t)n, S.sorted.p, st));
    if ((r = normalize_launch(S.sorted.p, CURDLE_G1_FORM_XYZZ, n, d_out_affine, st))) return r;
    HIP_TRY(hipStreamSynchronize(st));
    return CURDLE_OK;
  });
}

extern "C" int curdle_stat_normalize(unsigned long long out[2]) { return read_stats(out, g_nz_stat, 2); }
