// C ABI of the constant-time MSM (msm_ct_kernels.hip): curdle_msm_g1_ct / _device, curdle_stat_msm_ct, the batched forms
// (curdle_msm_g1_ct_batch / _batch_device / _multi, curdle_stat_msm_ct_batch), the oblivious gathers and the flagged
// shuffle step (curdle_shuffle_permute_commit_ex), the MSM's first user; that call's host part -- the range check of the
// permutation and the draw of the blinders -- is in host/proto_api.cpp.  The unit also holds the definitions of
// msm_ct_call.h: what these calls share with the MSM over a resident base set (msm_ct_bases_api.hip).
//
// A call takes ONE MSM slot, held by a SlotHold (api_helpers.h), for its stream and its buffers.  The terms k_i P_i live
// in the slot's `partials` buffer, 224 bytes each, and never leave the device.  The host and the resident form of a call
// are ONE function with a `resident` flag: single() and batch() behind the extern "C" forwards.  The term workspace is
// on the call's WipeList in both forms; the host form's scalars go through the slot's pinned staging and a device
// buffer, both on the list too (stage_scalars); the resident form reads the caller's arrays where they are and notes
// nothing of them.  Everything runs on one stream, the caller's if it gave one.  No stream is made here and nothing is
// allocated once the slot's buffers have grown.
//
// The single call and the shuffle step: k_msm_ct_walk, launch_msm_ct_sum, and the ONLY device-to-host copy of the MSM
// is the 160-byte block k_msm_ct_finish wrote (the 18 words of the result and the violation word).
//
// The batched forms: k MSMs (curdle_msm_g1_ct_batch / _device), or one scalar vector against k base sets
// (curdle_msm_g1_ct_multi), in ONE launch of k_msm_ct_walk over the concatenated pairs, the segmented sum
// (k_g1_sum_ct_seg per level, k_msm_ct_finish_seg) and ONE copy back of 144 k + 4 bytes: the k results and the violation
// word.  That is seg_walk_sum_fetch below, the body the resident-base form runs too with its own walk; the layout of
// the slot's small buffer and of the second pinned staging is stated at its declaration.  The (begin, count) table is
// made of `offsets`: public.
#include "msm_ct_call.h"

#include <algorithm>

namespace {
constexpr size_t kShuffleCtMax = 4096;    // the oblivious gather is quadratic
constexpr size_t kOutBytes = 160;         // 36 words of result, the violation word, three words of padding
constexpr size_t kStatusOffset = 192;     // the walks' status word, in the same small buffer behind the block

// pairs walked | walk launches | sums finished; completed calls only
std::atomic<unsigned long long> g_msm_ct_stat[3];
// batched calls | MSMs in them | level launches (k_g1_sum_ct_seg); completed calls that ran on a device only
std::atomic<unsigned long long> g_msm_ct_batch_stat[3];

void count_msm_ct(size_t pairs, unsigned walks, size_t sums = 1) {
  g_msm_ct_stat[0].fetch_add(pairs, std::memory_order_relaxed);
  g_msm_ct_stat[1].fetch_add(walks, std::memory_order_relaxed);
  g_msm_ct_stat[2].fetch_add(sums, std::memory_order_relaxed);
}

size_t round16(size_t v) { return (v + 15) / 16 * 16; }
}  // namespace

namespace curdle_api {
int check_scalar_bits(unsigned bits) {
  if (bits < 1 || bits > 255) return fail(CURDLE_EINVAL, "scalar_bits = %u is not in 1...255", bits);
  return CURDLE_OK;
}

int refuse_scalar_range() { return fail(CURDLE_EINVAL, "a scalar is not below 2^scalar_bits"); }

void count_msm_ct_batch(size_t msms, unsigned levels) {
  g_msm_ct_batch_stat[0].fetch_add(1, std::memory_order_relaxed);
  g_msm_ct_batch_stat[1].fetch_add(msms, std::memory_order_relaxed);
  g_msm_ct_batch_stat[2].fetch_add(levels, std::memory_order_relaxed);
}

int seg_shape(const size_t* offsets, size_t k, unsigned bits, unsigned stride, TotalText text, SegShape* sh) {
  if (int rc = check_scalar_bits(bits)) return rc;
  if (k > kMsmCtMaxBatch) return fail(CURDLE_EINVAL, "k = %zu exceeds the supported 4,096 MSMs of one call", k);
  for (size_t j = 0; j < k; j++)
    if (offsets[j + 1] < offsets[j]) return fail(CURDLE_EINVAL, "offsets decrease at %zu", j);
  sh->k = k;
  sh->stride = stride;
  sh->lo = k ? offsets[0] : 0;
  sh->total = k ? offsets[k] - offsets[0] : 0;
  if (sh->total > kMsmCtMaxTerms / stride)
    return text == TotalText::kPairs
               ? fail(CURDLE_EINVAL, "%zu pairs in all exceed the supported 65,536 pairs", sh->total)
               : fail(CURDLE_EINVAL, "n Cb = %zu x %u exceeds the supported 65,536 terms of one call", sh->total, stride);
  sh->seg.resize(2 * k);
  sh->counts.resize(k);
  for (size_t j = 0; j < k; j++) {
    sh->seg[2 * j] = (uint32_t)((offsets[j] - sh->lo) * stride);
    sh->seg[2 * j + 1] = sh->counts[j] = (uint32_t)((offsets[j + 1] - offsets[j]) * stride);
    sh->nonempty += offsets[j + 1] != offsets[j];
  }
  return CURDLE_OK;
}

int note_terms(Slot& S, WipeList& W, size_t terms) {
  if (int r = ensure(S.partials, terms * kMsmCtTermBytes)) return r;
  W.note_device(S.partials.p, terms * kMsmCtTermBytes);
  return CURDLE_OK;
}

int stage_scalars(Slot& S, WipeList& W, const void* scalars, size_t n, size_t copies, size_t behind, hipStream_t st) {
  const size_t run = n * 32, bytes = run * copies;
  int r;
  if ((r = ensure(S.scalars, bytes))) return r;
  if ((r = ensure_pinned(S, 0, bytes + behind))) return r;
  W.note_device(S.scalars.p, bytes);
  W.note_host(S.h_stage[0], bytes);
  for (size_t j = 0; j < copies; j++) memcpy(static_cast<uint8_t*>(S.h_stage[0]) + j * run, scalars, run);
  HIP_TRY(hipMemcpyAsync(S.scalars.p, S.h_stage[0], bytes, hipMemcpyHostToDevice, st));
  return CURDLE_OK;
}

int seg_walk_sum_fetch(SlotHold& H, const SegShape& sh, size_t extra_bytes, uint64_t* out_jac, unsigned* levels, const SegWalk& walk) {
  Slot& S = H.slot();
  const hipStream_t st = H.stream();
  const size_t k = sh.k, back = 144 * k + 4, status_off = round16(back), table_bytes = 8 * k;
  const size_t extra_off = round16(status_off + table_bytes);
  int r;
  if ((r = ensure(S.results, status_off + 16))) return r;
  if ((r = ensure(S.offsets, table_bytes))) return r;
  if ((r = ensure_pinned(S, 1, extra_off + extra_bytes))) return r;  // what comes back | the table | the family's: public
  uint8_t* h_block = static_cast<uint8_t*>(S.h_stage[1]);
  uint8_t* d_res = static_cast<uint8_t*>(S.results.p);
  uint32_t* d_status = reinterpret_cast<uint32_t*>(d_res + status_off);
  memcpy(h_block + status_off, sh.seg.data(), table_bytes);
  HIP_TRY(hipMemsetAsync(d_status, 0, 16, st));
  HIP_TRY(hipMemcpyAsync(S.offsets.p, h_block + status_off, table_bytes, hipMemcpyHostToDevice, st));
  if ((r = walk(d_status, h_block + extra_off, st))) return r;
  uint32_t lv = 0;
  HIP_TRY(launch_msm_ct_sum_seg(S.partials.p, S.offsets.p, sh.counts.data(), (uint32_t)k, d_status, d_res, &lv, st));
  HIP_TRY(hipMemcpyAsync(h_block, d_res, back, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  uint32_t verdict;
  memcpy(&verdict, h_block + 144 * k, 4);
  if (verdict) return refuse_scalar_range();
  memcpy(out_jac, h_block, 144 * k);
  *levels = lv;
  return CURDLE_OK;
}
}  // namespace curdle_api

namespace {
// the slot's small buffer in the single call's layout: zeroes the status word on st
int prepare_out(Slot& S, hipStream_t st) {
  if (int r = ensure(S.results, 256)) return r;
  HIP_TRY(hipMemsetAsync(static_cast<uint8_t*>(S.results.p) + kStatusOffset, 0, 16, st));
  return CURDLE_OK;
}
uint32_t* status_word(Slot& S) { return reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(S.results.p) + kStatusOffset); }

// Behind the walks: the sum over m terms, the block's copy (the call's only copy of anything the terms made), the wait,
// the verdict.  h_out: pinned, kOutBytes.
int sum_and_fetch(Slot& S, size_t m, void* h_out, uint64_t out_jac[18], hipStream_t st) {
  HIP_TRY(launch_msm_ct_sum(S.partials.p, (uint32_t)m, status_word(S), S.results.p, st));
  HIP_TRY(hipMemcpyAsync(h_out, S.results.p, kOutBytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (static_cast<const uint32_t*>(h_out)[36]) return refuse_scalar_range();
  memcpy(out_jac, h_out, 144);
  return CURDLE_OK;
}

// The host forms' pairs on their way to the device: `copies` runs of the n scalars (stage_scalars) and, behind them in
// the same pinned staging, the n x copies points (96 bytes each) that `fill` writes; the term workspace; the two uploads
// on st.  Behind it S.scalars and S.points hold the pairs.
template <class Fill>
int stage_pairs(Slot& S, WipeList& W, const void* scalars, size_t n, size_t copies, hipStream_t st, Fill&& fill) {
  const size_t m = n * copies;
  int r;
  if ((r = ensure(S.points, m * 96))) return r;
  if ((r = stage_scalars(S, W, scalars, n, copies, m * 96, st))) return r;
  if ((r = note_terms(S, W, m))) return r;
  uint8_t* h_pt = static_cast<uint8_t*>(S.h_stage[0]) + m * 32;
  fill(h_pt);
  HIP_TRY(hipMemcpyAsync(S.points.p, h_pt, m * 96, hipMemcpyHostToDevice, st));
  return CURDLE_OK;
}

unsigned bit_length(size_t v) {
  unsigned b = 0;
  for (; v; v >>= 1) b++;
  return b;
}

// curdle_msm_g1_ct (resident false: the pairs are staged and the scalars' copies wiped) and _device (the caller's arrays
// are read where they are: nothing of them is copied).
int single(const void* points, const void* scalars, bool resident, size_t n, unsigned bits, uint64_t out_jac[18], void* stream) {
  if (!out_jac || (n && (!points || !scalars))) return fail(CURDLE_EINVAL, "null argument");
  if (int rc = check_scalar_bits(bits)) return rc;
  if (n > kMsmCtMaxTerms) return fail(CURDLE_EINVAL, "n = %zu exceeds the supported 65,536 pairs", n);
  if (n == 0) {
    set_out_infinity(out_jac);
    return CURDLE_OK;
  }
  if (resident && (!aligned16(points) || !aligned16(scalars))) return fail(CURDLE_EINVAL, "device pointers must be multiples of 16");
  SlotHold H(cur(), true, stream);
  WipeList W(H.stream());
  H.wipe_on_exit(&W, resident ? "constant-time MSM: clearing the terms" : "constant-time MSM: clearing the scalars and the terms");
  return H.run([&]() -> int {
    Slot& S = H.slot();
    const hipStream_t st = H.stream();
    int r;
    if (resident) {
      if ((r = note_terms(S, W, n))) return r;
    } else {
      if ((r = stage_pairs(S, W, scalars, n, 1, st, [&](uint8_t* h_pt) { memcpy(h_pt, points, n * 96); }))) return r;
      points = S.points.p;
      scalars = S.scalars.p;
    }
    if ((r = ensure_pinned(S, 1, kOutBytes))) return r;
    if ((r = prepare_out(S, st))) return r;
    HIP_TRY(launch_msm_ct_walk(points, scalars, kMsmCtScalarFr, bits, (uint32_t)n, S.partials.p, status_word(S), st));
    if ((r = sum_and_fetch(S, n, S.h_stage[1], out_jac, st))) return r;
    count_msm_ct(n, 1);
    return CURDLE_OK;
  });
}

// One batched call behind its checks, sh.total > 0: the slot, the wipe, `stage` (a host form's stage_pairs, a resident
// form's note_terms), the shared body with ONE k_msm_ct_walk over all pairs, the counters.  d_points, d_scalars: the
// call's first pair in the caller's device arrays, or null for what `stage` left in S.points and S.scalars.
template <class Stage>
int batch_run(const SegShape& sh, unsigned bits, uint64_t* out_jac, const char* what, void* stream, const void* d_points,
              const void* d_scalars, Stage&& stage) {
  SlotHold H(cur(), true, stream);
  WipeList W(H.stream());
  H.wipe_on_exit(&W, what);
  return H.run([&]() -> int {
    Slot& S = H.slot();
    int r;
    if ((r = stage(S, W, H.stream()))) return r;
    if (!d_points) d_points = S.points.p, d_scalars = S.scalars.p;
    unsigned levels = 0;
    if ((r = seg_walk_sum_fetch(H, sh, 0, out_jac, &levels, [&](uint32_t* d_status, uint8_t*, hipStream_t st) -> int {
          HIP_TRY(launch_msm_ct_walk(d_points, d_scalars, kMsmCtScalarFr, bits, (uint32_t)sh.total, S.partials.p, d_status, st));
          return CURDLE_OK;
        })))
      return r;
    count_msm_ct(sh.total, 1, sh.nonempty);
    count_msm_ct_batch(sh.k, levels);
    return CURDLE_OK;
  });
}

// curdle_msm_g1_ct_batch (resident false) and _batch_device.
int batch(const void* points, const void* scalars, bool resident, const size_t* offsets, size_t k, unsigned bits, uint64_t* out_jac,
          void* stream) {
  if (!offsets || (k && (!out_jac || !points || !scalars))) return fail(CURDLE_EINVAL, "null argument");
  SegShape sh;
  if (int rc = seg_shape(offsets, k, bits, 1, TotalText::kPairs, &sh)) return rc;
  if (k == 0) return CURDLE_OK;
  if (resident && (!aligned16(points) || !aligned16(scalars))) return fail(CURDLE_EINVAL, "device pointers must be multiples of 16");
  if (sh.total == 0) {
    for (size_t j = 0; j < k; j++) set_out_infinity(out_jac + 18 * j);
    return CURDLE_OK;
  }
  // the call's first pair (96 and 32 bytes a record keep the alignment)
  const uint8_t* pts = static_cast<const uint8_t*>(points) + 96 * sh.lo;
  const uint8_t* sc = static_cast<const uint8_t*>(scalars) + 32 * sh.lo;
  if (resident)  // the caller's arrays are read where they are
    return batch_run(sh, bits, out_jac, "batched constant-time MSM: clearing the terms", stream, pts, sc,
                     [&](Slot& S, WipeList& W, hipStream_t) { return note_terms(S, W, sh.total); });
  return batch_run(sh, bits, out_jac, "batched constant-time MSM: clearing the scalars and the terms", nullptr, nullptr, nullptr,
                   [&](Slot& S, WipeList& W, hipStream_t st) {
                     return stage_pairs(S, W, sc, sh.total, 1, st, [&](uint8_t* h_pt) { memcpy(h_pt, pts, sh.total * 96); });
                   });
}
}  // namespace

extern "C" int curdle_msm_g1_ct(const uint64_t* points, const uint64_t* scalars, size_t n, unsigned scalar_bits,
                                uint64_t out_jac[18]) {
  return single(points, scalars, false, n, scalar_bits, out_jac, nullptr);
}

extern "C" int curdle_msm_g1_ct_device(const void* d_points, const void* d_scalars, size_t n, unsigned scalar_bits,
                                       uint64_t out_jac[18], void* stream) {
  return single(d_points, d_scalars, true, n, scalar_bits, out_jac, stream);
}

extern "C" int curdle_stat_msm_ct(unsigned long long out[3]) { return read_stats(out, g_msm_ct_stat, 3); }

extern "C" int curdle_msm_g1_ct_batch(const uint64_t* points, const uint64_t* scalars, const size_t* offsets, size_t k,
                                      unsigned scalar_bits, uint64_t* out_jac) {
  return batch(points, scalars, false, offsets, k, scalar_bits, out_jac, nullptr);
}

extern "C" int curdle_msm_g1_ct_batch_device(const void* d_points, const void* d_scalars, const size_t* offsets, size_t k,
                                             unsigned scalar_bits, uint64_t* out_jac, void* stream) {
  return batch(d_points, d_scalars, true, offsets, k, scalar_bits, out_jac, stream);
}

// One scalar vector against k base sets: the vector is replicated k times in the pinned staging (a host copy of public
// length) and the call is the batch of k MSMs of n pairs; the replicas are the staging's scalars and are wiped with it.
extern "C" int curdle_msm_g1_ct_multi(const uint64_t* const* points_sets, size_t k, const uint64_t* scalars, size_t n,
                                      unsigned scalar_bits, uint64_t* out_jac) {
  if (k && (!out_jac || !points_sets || (n && !scalars))) return fail(CURDLE_EINVAL, "null argument");
  if (int rc = check_scalar_bits(scalar_bits)) return rc;
  if (k > kMsmCtMaxBatch) return fail(CURDLE_EINVAL, "k = %zu exceeds the supported 4,096 MSMs of one call", k);
  if (k == 0) return CURDLE_OK;
  if (n > kMsmCtMaxTerms / k) return fail(CURDLE_EINVAL, "k n = %zu x %zu exceeds the supported 65,536 pairs", k, n);
  if (n == 0) {
    for (size_t j = 0; j < k; j++) set_out_infinity(out_jac + 18 * j);
    return CURDLE_OK;
  }
  for (size_t j = 0; j < k; j++)
    if (!points_sets[j]) return fail(CURDLE_EINVAL, "null argument: base set %zu", j);
  std::vector<size_t> offsets(k + 1);
  for (size_t j = 0; j <= k; j++) offsets[j] = j * n;
  SegShape sh;
  if (int rc = seg_shape(offsets.data(), k, scalar_bits, 1, TotalText::kPairs, &sh)) return rc;
  return batch_run(sh, scalar_bits, out_jac, "constant-time MSM over k base sets: clearing the replicated scalars and the terms",
                   nullptr, nullptr, nullptr, [&](Slot& S, WipeList& W, hipStream_t st) {
                     return stage_pairs(S, W, scalars, n, k, st, [&](uint8_t* h_pt) {
                       for (size_t j = 0; j < k; j++) memcpy(h_pt + j * n * 96, points_sets[j], n * 96);
                     });
                   });
}

extern "C" int curdle_stat_msm_ct_batch(unsigned long long out[3]) { return read_stats(out, g_msm_ct_batch_stat, 3); }

// The oblivious gather of the flagged shuffle step on its own, resident: d_out[i] = d_in[d_perm[i]], 96-byte records.
extern "C" int curdle_g1_permute_ct_device(const void* d_in, const void* d_perm, size_t n, void* d_out, void* stream) {
  if (n == 0) return CURDLE_OK;
  if (!d_in || !d_perm || !d_out) return fail(CURDLE_EINVAL, "null argument");
  if (n > kShuffleCtMax) return fail(CURDLE_EINVAL, "n = %zu exceeds the supported 4,096 records", n);
  if (!aligned16(d_in) || !aligned16(d_out) || ((uintptr_t)d_perm & 3u))
    return fail(CURDLE_EINVAL, "record pointers must be multiples of 16, the permutation's of 4");
  SlotHold H(cur(), true, stream);
  return H.run([&]() -> int {
    HIP_TRY(launch_g1_permute_ct(d_in, static_cast<const uint32_t*>(d_perm), (uint32_t)n, 1, d_out, H.stream()));
    HIP_TRY(hipStreamSynchronize(H.stream()));
    return CURDLE_OK;
  });
}

// ---------------------------------------------------------------------------------------------------------------------
// The oblivious gather over 32-byte records (k_fr_permute_ct): out[i] = in[perm[i]] with perm secret, what Prove's two
// permutations of the challenges become under curdle_prove_ct (alg::PermuteSecret, host/algebra.cpp).  The host form
// stages perm | in through the first pinned staging and the output through the second; perm's two copies and the output's
// two copies are on the WipeList (the input is not: in Prove it is the public challenge vector, and a caller whose input
// is secret wipes its own).  The _device form reads and writes the caller's arrays where they are.
// ---------------------------------------------------------------------------------------------------------------------
namespace {
// records gathered | launches; completed calls only
std::atomic<unsigned long long> g_fr_permute_ct_stat[2];

void count_fr_permute_ct(size_t n) {
  g_fr_permute_ct_stat[0].fetch_add(n, std::memory_order_relaxed);
  g_fr_permute_ct_stat[1].fetch_add(1, std::memory_order_relaxed);
}

// What both forms refuse first: a null argument, then n.
int fr_permute_check(const void* in, const void* perm, size_t n, const void* out) {
  if (!in || !perm || !out) return fail(CURDLE_EINVAL, "null argument");
  if (n > kShuffleCtMax) return fail(CURDLE_EINVAL, "n = %zu exceeds the supported 4,096 records", n);
  return CURDLE_OK;
}

// The host form of the single gather (m = n) and of the batched one (m = k n): perm | in staged through the first pinned
// staging, `launch` (the form's own kernel) on the slot's copies, the output back through the second, the counter by
// (m, 1).  perm's two copies and the output's two copies are always wiped, the input's two only under wipe_input.
template <class Launch>
int fr_permute_from_host(const uint64_t* in, const uint32_t* perm, size_t m, bool wipe_input, const char* what, uint64_t* out,
                         Launch&& launch) {
  SlotHold H(cur(), true, nullptr);
  WipeList W(H.stream());
  H.wipe_on_exit(&W, what);
  return H.run([&]() -> int {
    Slot& S = H.slot();
    const hipStream_t st = H.stream();
    const size_t rec = m * 32, perm_pad = (4 * m + 15) / 16 * 16;
    int r;
    if ((r = ensure(S.tmp, perm_pad))) return r;    // perm
    if ((r = ensure(S.scalars, rec))) return r;     // in
    if ((r = ensure(S.sorted, rec))) return r;      // out
    if ((r = ensure_pinned(S, 0, perm_pad + rec))) return r;  // perm | in
    if ((r = ensure_pinned(S, 1, rec))) return r;             // out
    W.note_device(S.tmp.p, perm_pad);
    if (wipe_input) W.note_device(S.scalars.p, rec);
    W.note_device(S.sorted.p, rec);
    W.note_host(S.h_stage[0], wipe_input ? perm_pad + rec : perm_pad);
    W.note_host(S.h_stage[1], rec);
    uint8_t* h = static_cast<uint8_t*>(S.h_stage[0]);
    memcpy(h, perm, 4 * m);
    memcpy(h + perm_pad, in, rec);
    HIP_TRY(hipMemcpyAsync(S.tmp.p, h, 4 * m, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(S.scalars.p, h + perm_pad, rec, hipMemcpyHostToDevice, st));
    HIP_TRY(launch(S.scalars.p, static_cast<const uint32_t*>(S.tmp.p), S.sorted.p, st));
    HIP_TRY(hipMemcpyAsync(S.h_stage[1], S.sorted.p, rec, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    memcpy(out, S.h_stage[1], rec);
    count_fr_permute_ct(m);
    return CURDLE_OK;
  });
}
}  // namespace

extern "C" int curdle_fr_permute_ct(const uint64_t* in, const uint32_t* perm, size_t n, uint64_t* out) {
  if (n == 0) return CURDLE_OK;
  if (int rc = fr_permute_check(in, perm, n, out)) return rc;
  return fr_permute_from_host(in, perm, n, false, "constant-time scalar gather: clearing the permutation and the gathered records",
                              out, [&](const void* d_in, const uint32_t* d_perm, void* d_out, hipStream_t st) {
                                return launch_fr_permute_ct(d_in, d_perm, (uint32_t)n, d_out, st);
                              });
}

extern "C" int curdle_fr_permute_ct_device(const void* d_in, const void* d_perm, size_t n, void* d_out, void* stream) {
  if (n == 0) return CURDLE_OK;
  if (int rc = fr_permute_check(d_in, d_perm, n, d_out)) return rc;
  const uintptr_t a = (uintptr_t)d_in, b = (uintptr_t)d_out;
  if (!aligned16(d_in) || !aligned16(d_out) || (a < b + 32 * n && b < a + 32 * n) || ((uintptr_t)d_perm & 3u))
    return fail(CURDLE_EINVAL, "record pointers must be multiples of 16 and must not overlap, the permutation's a multiple of 4");
  SlotHold H(cur(), true, stream);
  return H.run([&]() -> int {
    HIP_TRY(launch_fr_permute_ct(d_in, static_cast<const uint32_t*>(d_perm), (uint32_t)n, d_out, H.stream()));
    HIP_TRY(hipStreamSynchronize(H.stream()));
    count_fr_permute_ct(n);
    return CURDLE_OK;
  });
}

// The batched gather (k_permute_ct_seg): k members of one n in ONE launch, member j's records, entries and outputs the
// j-th run of n in each array -- what a lockstep group's k PermuteSecret calls become (alg::Lockstep, host/algebra.cpp).
// Staging, wiping and the slot hold are curdle_fr_permute_ct's over k n records, and the host form wipes the INPUT's two
// staging copies as well; the counter moves by (k n, 1).
namespace {
constexpr size_t kPermuteBatchMaxK = 4096;
constexpr size_t kPermuteBatchMaxRecords = (size_t)1 << 20;

// null, n, k, k n: the single call's order with k behind n
int permute_batch_check(const void* in, const void* perm, size_t n, size_t k, const void* out) {
  if (int rc = fr_permute_check(in, perm, n, out)) return rc;
  if (k > kPermuteBatchMaxK) return fail(CURDLE_EINVAL, "k = %zu exceeds the supported 4,096 members", k);
  if (k * n > kPermuteBatchMaxRecords) return fail(CURDLE_EINVAL, "k n = %zu exceeds the supported 2^20 records", k * n);
  return CURDLE_OK;
}

int permute_batch_device(const void* d_in, const void* d_perm, size_t n, size_t k, size_t record, void* d_out, void* stream) {
  if (n == 0 || k == 0) return CURDLE_OK;
  if (int rc = permute_batch_check(d_in, d_perm, n, k, d_out)) return rc;
  const uintptr_t a = (uintptr_t)d_in, b = (uintptr_t)d_out;
  const size_t bytes = record * k * n;
  if (!aligned16(d_in) || !aligned16(d_out) || (a < b + bytes && b < a + bytes) || ((uintptr_t)d_perm & 3u))
    return fail(CURDLE_EINVAL, "record pointers must be multiples of 16 and must not overlap, the permutation's a multiple of 4");
  SlotHold H(cur(), true, stream);
  return H.run([&]() -> int {
    HIP_TRY(launch_permute_ct_seg(d_in, static_cast<const uint32_t*>(d_perm), (uint32_t)n, (uint32_t)k, (uint32_t)record, d_out,
                                  H.stream()));
    HIP_TRY(hipStreamSynchronize(H.stream()));
    if (record == 32) count_fr_permute_ct(k * n);
    return CURDLE_OK;
  });
}
}  // namespace

extern "C" int curdle_fr_permute_ct_batch(const uint64_t* in, const uint32_t* perm, size_t n, size_t k, uint64_t* out) {
  if (n == 0 || k == 0) return CURDLE_OK;
  if (int rc = permute_batch_check(in, perm, n, k, out)) return rc;
  // unlike the single call, the input is wiped: a group's input may be secret (the shuffle step's unpermuted records)
  return fr_permute_from_host(in, perm, k * n, true,
                              "constant-time scalar gather batch: clearing the permutations and the gathered records", out,
                              [&](const void* d_in, const uint32_t* d_perm, void* d_out, hipStream_t st) {
                                return launch_permute_ct_seg(d_in, d_perm, (uint32_t)n, (uint32_t)k, 32, d_out, st);
                              });
}

extern "C" int curdle_fr_permute_ct_batch_device(const void* d_in, const void* d_perm, size_t n, size_t k, void* d_out, void* stream) {
  return permute_batch_device(d_in, d_perm, n, k, 32, d_out, stream);
}

extern "C" int curdle_g1_permute_ct_batch_device(const void* d_in, const void* d_perm, size_t n, size_t k, void* d_out, void* stream) {
  return permute_batch_device(d_in, d_perm, n, k, 96, d_out, stream);
}

extern "C" int curdle_stat_fr_permute_ct(unsigned long long out[2]) { return read_stats(out, g_fr_permute_ct_stat, 2); }

// The device work of curdle_shuffle_permute_commit_ex under CURDLE_SHUFFLE_CONSTANT_TIME (the entry point below checked the
// arguments; host/proto_api.cpp the permutation's range, and drew rs_m):
//   Ts | Us   one k_g1_mul_ct with the shared scalar k over the 2 ell records Rs | Ss, in place, then ONE
//             k_g1_permute_ct over both halves with the same perm;
//   M         k_msm_ct_walk over Gs with the permutation as plain uint32 scalars at bit_length(ell - 1) steps (public, at
//             least 1), a second walk over Hs with rs_m at 255 steps into the same workspace behind the first, ONE sum
//             over the ell + 4 terms and the finish.  M1 = sum perm[i] Gs[i] exists nowhere: not as a term, not on the host.
// The only device-to-host copies are Ts | Us and the 160-byte block (M and the violation word).  k, perm and rs_m go
// through the slot's pinned staging into ONE device buffer; that buffer, the staging, the unpermuted k R_i | k S_i and
// the term workspace are wiped on every way out.  Both walks run on the call's one stream: they are 5 ms chains of one
// and of ell / 64 waves, so a second stream would buy the shorter walk's length; not built, not measured.
static int shuffle_commit_ct(const uint64_t* Gs, const uint64_t* Hs, const uint64_t* Rs, const uint64_t* Ss, size_t ell,
                             const uint32_t* perm, const uint64_t k[4], const uint64_t rs_m[16], uint64_t* Ts_out,
                             uint64_t* Us_out, uint64_t M_out[18]) {
  SlotHold H(cur(), true, nullptr);
  WipeList W(H.stream());
  H.wipe_on_exit(&W, "constant-time shuffle step: clearing k, the permutation, the blinders and the terms");
  return H.run([&]() -> int {
    Slot& S = H.slot();
    const hipStream_t st = H.stream();
    const size_t m = ell + 4, sec = 32 + 128 + 4 * ell, sec_pad = (sec + 15) / 16 * 16, rec = 2 * ell * 96;
    int r;
    if ((r = ensure(S.points, rec))) return r;      // Rs | Ss, multiplied in place
    if ((r = ensure(S.sorted, rec))) return r;      // Ts | Us
    if ((r = ensure(S.tmp, m * 96))) return r;      // Gs | Hs
    if ((r = ensure(S.scalars, sec_pad))) return r; // k | rs_m | perm
    if ((r = ensure(S.partials, m * kMsmCtTermBytes))) return r;
    if ((r = ensure_pinned(S, 0, sec_pad + rec + m * 96))) return r;
    if ((r = ensure_pinned(S, 1, rec + kOutBytes))) return r;
    W.note_device(S.scalars.p, sec_pad);
    W.note_device(S.points.p, rec);
    W.note_device(S.partials.p, m * kMsmCtTermBytes);
    W.note_host(S.h_stage[0], sec_pad);
    uint8_t* h = static_cast<uint8_t*>(S.h_stage[0]);
    memcpy(h, k, 32);
    memcpy(h + 32, rs_m, 128);
    memcpy(h + 160, perm, 4 * ell);
    uint8_t* h_pub = h + sec_pad;
    memcpy(h_pub, Rs, ell * 96);
    memcpy(h_pub + ell * 96, Ss, ell * 96);
    memcpy(h_pub + rec, Gs, ell * 96);
    memcpy(h_pub + rec + ell * 96, Hs, 4 * 96);
    uint8_t* d_sec = static_cast<uint8_t*>(S.scalars.p);
    uint8_t* d_term = static_cast<uint8_t*>(S.partials.p);
    uint8_t* h_out = static_cast<uint8_t*>(S.h_stage[1]);
    if ((r = prepare_out(S, st))) return r;
    HIP_TRY(hipMemcpyAsync(d_sec, h, sec, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(S.points.p, h_pub, rec, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(S.tmp.p, h_pub + rec, m * 96, hipMemcpyHostToDevice, st));
    HIP_TRY(launch_g1_mul_ct(S.points.p, 1, d_sec, 1, (uint32_t)(2 * ell), S.points.p, st));
    HIP_TRY(launch_g1_permute_ct(S.points.p, reinterpret_cast<const uint32_t*>(d_sec + 160), (uint32_t)ell, 2, S.sorted.p, st));
    const unsigned pbits = std::max(1u, bit_length(ell - 1));
    HIP_TRY(launch_msm_ct_walk(S.tmp.p, d_sec + 160, kMsmCtScalarU32, pbits, (uint32_t)ell, d_term, status_word(S), st));
    HIP_TRY(launch_msm_ct_walk(static_cast<uint8_t*>(S.tmp.p) + ell * 96, d_sec + 32, kMsmCtScalarFr, 255, 4,
                               d_term + ell * kMsmCtTermBytes, status_word(S), st));
    HIP_TRY(hipMemcpyAsync(h_out + kOutBytes, S.sorted.p, rec, hipMemcpyDeviceToHost, st));
    if ((r = sum_and_fetch(S, m, h_out, M_out, st))) return r;
    memcpy(Ts_out, h_out + kOutBytes, ell * 96);
    memcpy(Us_out, h_out + kOutBytes + ell * 96, ell * 96);
    count_g1_mul_ct_pass(2 * ell);
    count_msm_ct(m, 2);
    return CURDLE_OK;
  });
}

// host/proto_api.cpp
int curdle_shuffle_commit_ct_host_part(const curdle_crs* crs, size_t ell, const uint32_t* perm, curdle_rand* rand,
                                       const uint64_t** Gs, const uint64_t** Hs, uint64_t rs_m[16]);

extern "C" int curdle_shuffle_permute_commit_ex(const curdle_crs* crs, const uint64_t* Rs, const uint64_t* Ss, size_t ell,
                                                const uint32_t* perm, const uint64_t k[4], curdle_rand* rand, unsigned flags,
                                                uint64_t* Ts_out, uint64_t* Us_out, uint64_t M_out[18],
                                                uint64_t rs_m_out[16]) {
  if (flags & ~CURDLE_SHUFFLE_CONSTANT_TIME)
    return fail(CURDLE_EINVAL, "unknown flag bits 0x%x", flags & ~CURDLE_SHUFFLE_CONSTANT_TIME);
  if (!flags) return curdle_shuffle_permute_commit(crs, Rs, Ss, ell, perm, k, rand, Ts_out, Us_out, M_out, rs_m_out);
  if (!crs || !Rs || !Ss || !perm || !k || !rand || !Ts_out || !Us_out || !M_out || !rs_m_out)
    return fail(CURDLE_EINVAL, "null argument");
  if (ell == 0 || ell > kShuffleCtMax)
    return fail(CURDLE_EINVAL, "ell = %zu is not in 1...4,096 under CURDLE_SHUFFLE_CONSTANT_TIME", ell);
  const uint64_t *Gs = nullptr, *Hs = nullptr;
  uint64_t rs_m[16];
  int rc = curdle_shuffle_commit_ct_host_part(crs, ell, perm, rand, &Gs, &Hs, rs_m);
  if (rc == CURDLE_OK) rc = shuffle_commit_ct(Gs, Hs, Rs, Ss, ell, perm, k, rs_m, Ts_out, Us_out, M_out);
  if (rc == CURDLE_OK) memcpy(rs_m_out, rs_m, sizeof(rs_m));
  explicit_bzero(rs_m, sizeof(rs_m));
  return rc;
}
