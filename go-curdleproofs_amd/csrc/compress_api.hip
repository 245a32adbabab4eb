// C ABI of the batched G1 compression (compress_kernels.hip): curdle_g1_compress_batch / _device, n calls of
// curdle_g1_compress (gnark's G1Affine.Bytes of a G1Jac) in one -- the counterpart of curdle_g1_decompress_batch.
// Both run through an MSM slot held by a SlotHold (api_helpers.h): the slot lends its stream, and the host
// form its buffers and pinned staging, in passes of kCompressPass points so that the staging stays bounded.  No
// stream is made here and nothing is allocated once the slot's buffers have grown to a pass.
#include "api_helpers.h"

#include <algorithm>

namespace {
constexpr size_t kCompressMax = (size_t)1 << 27;
constexpr size_t kCompressPass = (size_t)1 << 20;  // 144 MB of points, 48 MB of encodings per pass

// Host points (d_in null: `jac` is copied up and the bytes come back to `out`) or resident ones (d_in -> d_out, both
// device memory), on the slot's stream or the caller's.  The stream is synchronised before the slot is released.
int compress_through_slot(Ctx& cx, const uint64_t* jac, const void* d_in, size_t n, uint8_t* out, void* d_out, void* user_stream) {
  SlotHold H(cx, true, user_stream);
  return H.run([&]() -> int {
    Slot& S = H.slot();
    const hipStream_t st = H.stream();
    if (d_in) {
      HIP_TRY(launch_g1_compress(d_in, kCompressJac, (uint32_t)n, static_cast<uint8_t*>(d_out), st));
      HIP_TRY(hipStreamSynchronize(st));
      return CURDLE_OK;
    }
    const size_t cap = std::min(n, kCompressPass);
    int r;
    if ((r = ensure(S.points, cap * 144))) return r;
    if ((r = ensure(S.scalars, cap * 48))) return r;
    if ((r = ensure_pinned(S, 0, cap * 144))) return r;
    if ((r = ensure_pinned(S, 1, cap * 48))) return r;
    for (size_t lo = 0; lo < n; lo += kCompressPass) {
      const size_t m = std::min(kCompressPass, n - lo);
      // through the slot's pinned staging, not straight from the caller's pageable memory (decode_api.hip)
      memcpy(S.h_stage[0], jac + 18 * lo, m * 144);
      HIP_TRY(hipMemcpyAsync(S.points.p, S.h_stage[0], m * 144, hipMemcpyHostToDevice, st));
      HIP_TRY(launch_g1_compress(S.points.p, kCompressJac, (uint32_t)m, static_cast<uint8_t*>(S.scalars.p), st));
      HIP_TRY(hipMemcpyAsync(S.h_stage[1], S.scalars.p, m * 48, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      memcpy(out + 48 * lo, S.h_stage[1], m * 48);
    }
    return CURDLE_OK;
  });
}
}  // namespace

extern "C" int curdle_g1_compress_batch(const uint64_t* jac_points, size_t n, uint8_t* out) {
  if (n && (!jac_points || !out)) return fail(CURDLE_EINVAL, "null argument");
  if (n == 0) return CURDLE_OK;
  if (n > kCompressMax) return fail(CURDLE_EINVAL, "n = %zu exceeds the supported 2^27 points", n);
  return compress_through_slot(cur(), jac_points, nullptr, n, out, nullptr, nullptr);
}

extern "C" int curdle_g1_compress_batch_device(const void* d_jac_points, size_t n, void* d_out, void* stream) {
  if (n && (!d_jac_points || !d_out)) return fail(CURDLE_EINVAL, "null argument");
  if (n == 0) return CURDLE_OK;
  if (n > kCompressMax) return fail(CURDLE_EINVAL, "n = %zu exceeds the supported 2^27 points", n);
  return compress_through_slot(cur(), nullptr, d_jac_points, n, nullptr, d_out, stream);
}
