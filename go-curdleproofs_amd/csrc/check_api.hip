// C ABI of the membership check for G1 points that arrive in memory (check_kernels.hip), and the verifier entry
// points that run it on the instance points: curdleproof.Verify takes []G1Affine from its caller unchecked
// (curdleproof.go:199-207), and every fast path of this library needs its bases in the prime-order subgroup.
// The checked verifier lives here, with the backend, and calls the exported curdle_verify*: nothing under host/
// refers to these symbols, so the host-only build (tests/hostbuild) links as before.  The checked BATCH verifier
// (curdle_verify_batch_checked, at the end) hands the host layer its per-chunk check as a callback (host/batch_check.h).
#include "api_helpers.h"
#include "../host/batch_check.h"

namespace {
// checks begun on a decode context | run to the end through an MSM slot (the four batch calls below always are)
std::atomic<unsigned long long> g_check_paths[2];

constexpr size_t kCheckMax = (size_t)1 << 27;

// n points at `src` (device memory) -> n status bytes in `h_status` (pinned) on `stream`, which is synchronised
int check_on_stream(const void* d_points, size_t n, bool jac, int subgroup_check, void* d_status, void* h_status, hipStream_t stream) {
  HIP_TRY((jac ? launch_g1_check_jac : launch_g1_check_affine)((const uint32_t*)d_points, (uint32_t)n, subgroup_check, (uint8_t*)d_status, stream));
  HIP_TRY(hipMemcpyAsync(h_status, d_status, n, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return CURDLE_OK;
}

// The whole check through an MSM slot: host vectors (d_points null) or a resident array, of affine points (96 bytes)
// or, with `jac`, of Jacobian ones (144).
int check_through_slot(Ctx& cx, const uint64_t* const* vecs, const size_t* lens, int nvec, const void* d_points, size_t n,
                       int subgroup_check, uint8_t* status, void* user_stream, bool jac = false) {
  const size_t size = jac ? 144 : 96;
  SlotHold H(cx, true, user_stream);
  return H.run([&]() -> int {
    Slot& S = H.slot();
    const hipStream_t st = H.stream();
    int r;
    if ((r = ensure(S.counts, n))) return r;
    if ((r = ensure_pinned(S, 1, n))) return r;
    if (!d_points) {
      // through the slot's pinned staging, not straight from the caller's pageable memory (decode_api.hip)
      if ((r = ensure(S.points, n * size))) return r;
      if ((r = ensure_pinned(S, 0, n * size))) return r;
      uint8_t* h = static_cast<uint8_t*>(S.h_stage[0]);
      for (int v = 0; v < nvec; h += lens[v] * size, v++)
        if (lens[v]) memcpy(h, vecs[v], lens[v] * size);
      HIP_TRY(hipMemcpyAsync(S.points.p, S.h_stage[0], n * size, hipMemcpyHostToDevice, st));
      d_points = S.points.p;
    }
    if ((r = check_on_stream(d_points, n, jac, subgroup_check, S.counts.p, S.h_stage[1], st))) return r;
    memcpy(status, S.h_stage[1], n);
    return CURDLE_OK;
  });
}

// A decode context's pinned staging, grown to `in_bytes` of input and `out_bytes` of what comes back.
int ensure_dslot_staging(DSlot& D, size_t in_bytes, size_t out_bytes) {
  if (D.h_in_cap < in_bytes) {
    if (D.h_in) HIP_TRY(hipHostFree(D.h_in));
    D.h_in = nullptr;
    D.h_in_cap = 0;
    HIP_TRY(hipHostMalloc(&D.h_in, grow_size(in_bytes), hipHostMallocDefault));
    D.h_in_cap = grow_size(in_bytes);
  }
  if (D.h_out_cap < out_bytes) {
    if (D.h_out) HIP_TRY(hipHostFree(D.h_out));
    D.h_out = nullptr;
    D.h_out_cap = 0;
    HIP_TRY(hipHostMalloc(&D.h_out, grow_size(out_bytes), hipHostMallocDefault));
    D.h_out_cap = grow_size(out_bytes);
  }
  return CURDLE_OK;
}

const char* status_text(uint8_t st) {
  switch (st) {
    case CURDLE_DECODE_BAD_ENCODING: return "not a field element (a coordinate is not below p)";
    case CURDLE_DECODE_NOT_ON_CURVE: return "not on the curve";
    case CURDLE_DECODE_NOT_IN_SUBGROUP: return "not in the prime-order subgroup";
    default: return "invalid point";
  }
}

// One Jacobian point on the host: Z = 0 is infinity; a coordinate >= p; Y^2 = X^3 + 4 Z^6; the subgroup.
uint8_t check_jac_host(const uint64_t M[18]) {
  G1Jac j;
  memcpy(&j, M, sizeof(j));
  if (f_is_zero(j.z)) return CURDLE_DECODE_INFINITY;
  for (const Fp* c : {&j.x, &j.y, &j.z}) {
    int ge = 1;  // c >= p so far (equal)
    for (int i = 0; i < 12; i++) ge = c->l[i] > FpParams::mod(i) ? 1 : (c->l[i] < FpParams::mod(i) ? 0 : ge);
    if (ge) return CURDLE_DECODE_BAD_ENCODING;
  }
  Fp lhs, rhs, z2, z6, four;
  fp_sqr(lhs, j.y);
  fp_sqr(rhs, j.x);
  fp_mul(rhs, rhs, j.x);
  fp_sqr(z2, j.z);
  fp_sqr(z6, z2);
  fp_mul(z6, z6, z2);
  f_one(four);
  fp_dbl(four, four);
  fp_dbl(four, four);
  fp_mul(z6, z6, four);
  fp_add(rhs, rhs, z6);
  if (!f_eq(lhs, rhs)) return CURDLE_DECODE_NOT_ON_CURVE;
  G1XYZZ p;
  g1_from_jac(p, j);
  return g1_in_subgroup(p) ? CURDLE_DECODE_OK : CURDLE_DECODE_NOT_IN_SUBGROUP;
}
}  // namespace

namespace curdle_api {
int check_start(CheckJob& job, const uint64_t* const* vecs, const size_t* lens, int nvec, int subgroup_check) {
  Ctx& cx = cur();
  size_t n = 0;
  for (int v = 0; v < nvec; v++) {
    if (lens[v] && !vecs[v]) return fail(CURDLE_EINVAL, "null argument");
    if (lens[v] > kCheckMax) return fail(CURDLE_EINVAL, "n = %zu exceeds the supported 2^27 points", lens[v]);
    n += lens[v];
  }
  if (n > kCheckMax) return fail(CURDLE_EINVAL, "n = %zu exceeds the supported 2^27 points", n);
  job.cx = &cx;
  job.dslot = -1;
  job.status.assign(n, 0);
  if (n == 0) return CURDLE_OK;
  int idx = -1;
  {
    std::unique_lock<std::mutex> g(cx.mu);
    int rc = init_default_locked(cx);
    if (rc) return rc;
    for (int i = 0; i < kMaxDeferred && idx < 0; i++)
      if (!cx.dslots[i].busy) idx = i;
    if (idx >= 0) {
      cx.dslots[idx].busy = true;
      cx.dslots[idx].claimed = true;  // no decode ticket names this hold
      cx.dslots[idx].gen++;
    }
  }
  if (idx < 0) {
    // Every decode context is taken.  The caller will call MSM entry points next, so it may not HOLD an MSM slot
    // meanwhile: the check runs to its end through one, which is free again when this returns.
    g_check_paths[1].fetch_add(1, std::memory_order_relaxed);
    return check_through_slot(cx, vecs, lens, nvec, nullptr, n, subgroup_check, job.status.data(), nullptr);
  }
  g_check_paths[0].fetch_add(1, std::memory_order_relaxed);
  DSlot& D = cx.dslots[idx];
  auto body = [&]() -> int {
    HIP_TRY(hipSetDevice(cx.device));
    D.n = (uint32_t)n;
    int r;
    if ((r = ensure_dslot_streams(cx))) return r;
    if ((r = ensure(D.out, n * 96))) return r;
    if ((r = ensure(D.status, n))) return r;
    // pinned staging: the copy must not block the caller, who verifies meanwhile
    if ((r = ensure_dslot_staging(D, n * 96, n))) return r;
    uint8_t* h = static_cast<uint8_t*>(D.h_in);
    for (int v = 0; v < nvec; h += lens[v] * 96, v++)
      if (lens[v]) memcpy(h, vecs[v], lens[v] * 96);
    HIP_TRY(hipMemcpyAsync(D.out.p, D.h_in, n * 96, hipMemcpyHostToDevice, D.stream));
    HIP_TRY(launch_g1_check_affine((const uint32_t*)D.out.p, (uint32_t)n, subgroup_check, (uint8_t*)D.status.p, D.stream));
    HIP_TRY(hipMemcpyAsync(D.h_out, D.status.p, n, hipMemcpyDeviceToHost, D.stream));
    return CURDLE_OK;
  };
  int rc = body();
  if (rc) {
    if (D.stream) (void)hipStreamSynchronize(D.stream);
    std::lock_guard<std::mutex> g(cx.mu);
    D.busy = false;
    return rc;
  }
  job.dslot = idx;
  return CURDLE_OK;
}

int check_collect(CheckJob& job) {
  if (job.dslot < 0) return CURDLE_OK;
  Ctx& cx = *job.cx;
  DSlot& D = cx.dslots[job.dslot];
  int rc = CURDLE_OK;
  hipError_t he = hipSetDevice(cx.device);
  if (he == hipSuccess) he = hipStreamSynchronize(D.stream);
  if (he != hipSuccess) rc = fail(CURDLE_EHIP, "collecting the point check: %s", hipGetErrorString(he));
  if (rc == CURDLE_OK) memcpy(job.status.data(), D.h_out, job.status.size());
  {
    std::lock_guard<std::mutex> g(cx.mu);
    D.busy = false;
  }
  job.dslot = -1;
  return rc;
}
}  // namespace curdle_api

extern "C" int curdle_g1_check_batch(const uint64_t* points, size_t n, int subgroup_check, uint8_t* status) {
  if (n && (!points || !status)) return fail(CURDLE_EINVAL, "null argument");
  if (n == 0) return CURDLE_OK;
  if (n > kCheckMax) return fail(CURDLE_EINVAL, "n = %zu exceeds the supported 2^27 points", n);
  g_check_paths[1].fetch_add(1, std::memory_order_relaxed);
  return check_through_slot(cur(), &points, &n, 1, nullptr, n, subgroup_check, status, nullptr);
}

extern "C" int curdle_g1_check_batch_device(const void* d_points, size_t n, int subgroup_check, uint8_t* status, void* stream) {
  if (n && (!d_points || !status)) return fail(CURDLE_EINVAL, "null argument");
  if (n == 0) return CURDLE_OK;
  if (n > kCheckMax) return fail(CURDLE_EINVAL, "n = %zu exceeds the supported 2^27 points", n);
  g_check_paths[1].fetch_add(1, std::memory_order_relaxed);
  return check_through_slot(cur(), nullptr, nullptr, 0, d_points, n, subgroup_check, status, stream);
}

extern "C" int curdle_g1_check_jac_batch(const uint64_t* jac_points, size_t n, int subgroup_check, uint8_t* status) {
  if (n && (!jac_points || !status)) return fail(CURDLE_EINVAL, "null argument");
  if (n == 0) return CURDLE_OK;
  if (n > kCheckMax) return fail(CURDLE_EINVAL, "n = %zu exceeds the supported 2^27 points", n);
  g_check_paths[1].fetch_add(1, std::memory_order_relaxed);
  return check_through_slot(cur(), &jac_points, &n, 1, nullptr, n, subgroup_check, status, nullptr, true);
}

extern "C" int curdle_g1_check_jac_batch_device(const void* d_jac_points, size_t n, int subgroup_check, uint8_t* status, void* stream) {
  if (n && (!d_jac_points || !status)) return fail(CURDLE_EINVAL, "null argument");
  if (n == 0) return CURDLE_OK;
  if (n > kCheckMax) return fail(CURDLE_EINVAL, "n = %zu exceeds the supported 2^27 points", n);
  g_check_paths[1].fetch_add(1, std::memory_order_relaxed);
  return check_through_slot(cur(), nullptr, nullptr, 0, d_jac_points, n, subgroup_check, status, stream, true);
}

extern "C" int curdle_stat_check_paths(unsigned long long out[2]) { return read_stats(out, g_check_paths, 2); }

namespace {
// verify(&ok) is the unchecked call.  The check of the 4 ell instance points is started before it, on a decode
// context's stream, and collected after it and before anything is reported; M is checked on the host meanwhile.
template <class Verify>
int verify_checked(const uint64_t* Rs, const uint64_t* Ss, const uint64_t* Ts, const uint64_t* Us, size_t ell,
                   const uint64_t M[18], int* ok, Verify verify) {
  static const char* const kNames[4] = {"Rs", "Ss", "Ts", "Us"};
  const uint64_t* vecs[4] = {Rs, Ss, Ts, Us};
  const size_t lens[4] = {ell, ell, ell, ell};
  CheckJob job;
  int rc = check_start(job, vecs, lens, 4, 1);
  if (rc) return rc;
  const uint8_t m_status = check_jac_host(M);
  int vok = 0;
  const int vrc = verify(&vok);
  char verr[sizeof(g_err)];
  snprintf(verr, sizeof(verr), "%s", g_err);
  *ok = 0;
  if ((rc = check_collect(job))) return rc;
  for (int v = 0; v < 4; v++)
    for (size_t i = 0; i < ell; i++) {
      const uint8_t st = job.status[(size_t)v * ell + i];
      if (st != CURDLE_DECODE_OK && st != CURDLE_DECODE_INFINITY)  // infinity: gnark and the MSM accept it
        return fail(CURDLE_EINVAL, "%s[%zu]: %s", kNames[v], i, status_text(st));
    }
  if (m_status != CURDLE_DECODE_OK && m_status != CURDLE_DECODE_INFINITY) return fail(CURDLE_EINVAL, "M: %s", status_text(m_status));
  if (vrc) return fail(vrc, "%s", verr);
  *ok = vok;
  return CURDLE_OK;
}
}  // namespace

extern "C" int curdle_verify_checked(const curdle_crs* crs, const uint8_t* proof, size_t proof_len, const uint64_t* Rs,
                                     const uint64_t* Ss, const uint64_t* Ts, const uint64_t* Us, size_t ell,
                                     const uint64_t M[18], curdle_rand* rand, int* ok) {
  if (!crs || !proof || !Rs || !Ss || !Ts || !Us || !M || !rand || !ok) return fail(CURDLE_EINVAL, "null argument");
  *ok = 0;
  if (ell != curdle_crs_size(crs)) return fail(CURDLE_EINVAL, "ell does not match the CRS");
  return verify_checked(Rs, Ss, Ts, Us, ell, M, ok,
                        [&](int* v) { return curdle_verify(crs, proof, proof_len, Rs, Ss, Ts, Us, ell, M, rand, v); });
}

extern "C" int curdle_verify_proof_checked(const curdle_crs* crs, const curdle_proof* proof, const uint64_t* Rs,
                                           const uint64_t* Ss, const uint64_t* Ts, const uint64_t* Us, size_t ell,
                                           const uint64_t M[18], curdle_rand* rand, int* ok) {
  if (!crs || !proof || !Rs || !Ss || !Ts || !Us || !M || !rand || !ok) return fail(CURDLE_EINVAL, "null argument");
  *ok = 0;
  if (ell != curdle_crs_size(crs)) return fail(CURDLE_EINVAL, "ell does not match the CRS");
  return verify_checked(Rs, Ss, Ts, Us, ell, M, ok,
                        [&](int* v) { return curdle_verify_proof(crs, proof, Rs, Ss, Ts, Us, ell, M, rand, v); });
}

namespace {
std::atomic<unsigned long long> g_batch_checked[3];  // checked batches | members the check rejected | chunks checked

// One chunk of a checked batch, to the end: `na` affine vectors back to back, then `nj` Jacobian points, gathered into
// pinned staging; ONE upload, ONE affine and ONE Jacobian launch, the status bytes back.  On a decode context when one
// is free and through an MSM slot otherwise -- check_start's rule.  The caller is a producer thread of the batch
// (proto::CheckAhead) that holds nothing else meanwhile.
int check_chunk(const uint64_t* const* avecs, const size_t* alens, size_t na, const uint64_t* const* jpts, size_t nj,
                uint8_t* st_a, uint8_t* st_j) {
  Ctx& cx = cur();
  size_t n_aff = 0;
  for (size_t v = 0; v < na; v++) {
    if (alens[v] && !avecs[v]) return fail(CURDLE_EINVAL, "null argument");
    if (alens[v] > kCheckMax) return fail(CURDLE_EINVAL, "n = %zu exceeds the supported 2^27 points", alens[v]);
    n_aff += alens[v];
  }
  for (size_t j = 0; j < nj; j++)
    if (!jpts[j]) return fail(CURDLE_EINVAL, "null argument");
  const size_t n = n_aff + nj;
  if (n > kCheckMax) return fail(CURDLE_EINVAL, "n = %zu exceeds the supported 2^27 points", n);
  if (n == 0) return CURDLE_OK;
  const size_t bytes = n_aff * 96 + nj * 144;
  // d_in: `bytes` of device memory, d_st: n status bytes; h_in / h_st their pinned staging
  auto run = [&](void* d_in, void* d_st, void* h_in, void* h_st, hipStream_t stream) -> int {
    uint8_t* h = static_cast<uint8_t*>(h_in);
    for (size_t v = 0; v < na; h += alens[v] * 96, v++)
      if (alens[v]) memcpy(h, avecs[v], alens[v] * 96);
    for (size_t j = 0; j < nj; j++, h += 144) memcpy(h, jpts[j], 144);
    HIP_TRY(hipMemcpyAsync(d_in, h_in, bytes, hipMemcpyHostToDevice, stream));
    HIP_TRY(launch_g1_check_affine((const uint32_t*)d_in, (uint32_t)n_aff, 1, (uint8_t*)d_st, stream));
    HIP_TRY(launch_g1_check_jac((const uint32_t*)((const uint8_t*)d_in + n_aff * 96), (uint32_t)nj, 1, (uint8_t*)d_st + n_aff, stream));
    HIP_TRY(hipMemcpyAsync(h_st, d_st, n, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (n_aff) memcpy(st_a, h_st, n_aff);
    if (nj) memcpy(st_j, static_cast<uint8_t*>(h_st) + n_aff, nj);
    return CURDLE_OK;
  };
  int idx = -1;
  {
    std::unique_lock<std::mutex> g(cx.mu);
    int rc = init_default_locked(cx);
    if (rc) return rc;
    for (int i = 0; i < kMaxDeferred && idx < 0; i++)
      if (!cx.dslots[i].busy) idx = i;
    if (idx >= 0) {
      cx.dslots[idx].busy = true;
      cx.dslots[idx].claimed = true;  // no decode ticket names this hold
      cx.dslots[idx].gen++;
    }
  }
  if (idx >= 0) {
    DSlot& D = cx.dslots[idx];
    auto body = [&]() -> int {
      HIP_TRY(hipSetDevice(cx.device));
      D.n = (uint32_t)n;
      int r;
      if ((r = ensure_dslot_streams(cx))) return r;
      if ((r = ensure(D.out, bytes))) return r;
      if ((r = ensure(D.status, n))) return r;
      if ((r = ensure_dslot_staging(D, bytes, n))) return r;
      return run(D.out.p, D.status.p, D.h_in, D.h_out, D.stream);
    };
    int rc = body();
    if (rc && D.stream) (void)hipStreamSynchronize(D.stream);
    std::lock_guard<std::mutex> g(cx.mu);
    D.busy = false;
    return rc;
  }
  SlotHold H(cx, true, nullptr);
  return H.run([&]() -> int {
    Slot& S = H.slot();
    int r;
    if ((r = ensure(S.counts, n))) return r;
    if ((r = ensure_pinned(S, 1, n))) return r;
    if ((r = ensure(S.points, bytes))) return r;
    if ((r = ensure_pinned(S, 0, bytes))) return r;
    return run(S.points.p, S.counts.p, S.h_stage[0], S.h_stage[1], S.stream);
  });
}
}  // namespace

extern "C" int curdle_verify_batch_checked(const curdle_crs* crs, size_t k, const uint8_t* const* proofs, const size_t* proof_lens,
                                           const uint64_t* const* Rs, const uint64_t* const* Ss, const uint64_t* const* Ts,
                                           const uint64_t* const* Us, size_t ell, const uint64_t* Ms, curdle_rand* rand,
                                           int nthreads, int* oks, curdle_point_fault* faults) {
  // nothing reads as a verdict after a refusal either
  for (size_t i = 0; i < k; i++) {
    if (oks) oks[i] = 0;
    if (faults) faults[i] = curdle_point_fault{0xff, 0, 0, 0};
  }
  if (!crs || !rand || !oks || (k && (!proofs || !proof_lens || !Rs || !Ss || !Ts || !Us || !Ms)))
    return fail(CURDLE_EINVAL, "null argument");
  if (ell != curdle_crs_size(crs)) return fail(CURDLE_EINVAL, "ell does not match the CRS");
  if (k == 0) return CURDLE_OK;
  g_batch_checked[0].fetch_add(1, std::memory_order_relaxed);
  unsigned long long stats[2] = {0, 0};
  const int rc = curdle_verify_batch_checked_with(crs, k, proofs, proof_lens, Rs, Ss, Ts, Us, ell, Ms, rand, nthreads, oks, faults,
                                                  check_chunk, stats);
  g_batch_checked[1].fetch_add(stats[0], std::memory_order_relaxed);
  g_batch_checked[2].fetch_add(stats[1], std::memory_order_relaxed);
  return rc;
}

extern "C" int curdle_stat_batch_checked(unsigned long long out[3]) { return read_stats(out, g_batch_checked, 3); }
