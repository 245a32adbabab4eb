// C ABI of the constant-time MSM (msm_ct_kernels.hip): curdle_msm_g1_ct / _device, curdle_stat_msm_ct, the batched forms
// (curdle_msm_g1_ct_batch / _batch_device / _multi, curdle_stat_msm_ct_batch: further down, with their own notes) and the
// flagged shuffle step (curdle_shuffle_permute_commit_ex), its first user; that call's host part -- the range check of the
// permutation and the draw of the blinders -- is in host/proto_api.cpp.
//
// A call takes ONE MSM slot, held by a SlotHold (api_helpers.h), for its stream and its buffers.  The terms k_i P_i live
// in the slot's `partials` buffer, 224 bytes each, and never leave the device: the ONLY device-to-host copy of an MSM is
// the 160-byte block k_msm_ct_finish wrote (the 18 words of the result and the violation word).  The term workspace is
// on the call's WipeList in both forms; the host form's scalars go through the slot's pinned staging and a device
// buffer, both on the list too.  Everything runs on one stream, the caller's if it gave one.  No stream is made here and
// nothing is allocated once the slot's buffers have grown.
#include "api_helpers.h"

#include <algorithm>

namespace {
constexpr size_t kMsmCtMax = 65536;       // one pass: 256 blocks
constexpr size_t kShuffleCtMax = 4096;    // the oblivious gather is quadratic
constexpr size_t kOutBytes = 160;         // 36 words of result, the violation word, three words of padding
constexpr size_t kStatusOffset = 192;     // the walks' status word, in the same small buffer behind the block

// pairs walked | walk launches | sums finished; completed calls only
std::atomic<unsigned long long> g_msm_ct_stat[3];

void count_msm_ct(size_t pairs, unsigned walks) {
  g_msm_ct_stat[0].fetch_add(pairs, std::memory_order_relaxed);
  g_msm_ct_stat[1].fetch_add(walks, std::memory_order_relaxed);
  g_msm_ct_stat[2].fetch_add(1, std::memory_order_relaxed);
}

int check_scalar_bits(unsigned bits) {
  if (bits < 1 || bits > 255) return fail(CURDLE_EINVAL, "scalar_bits = %u is not in 1...255", bits);
  return CURDLE_OK;
}

int check_args(const void* points, const void* scalars, size_t n, unsigned bits, const void* out) {
  if (!out || (n && (!points || !scalars))) return fail(CURDLE_EINVAL, "null argument");
  if (int rc = check_scalar_bits(bits)) return rc;
  if (n > kMsmCtMax) return fail(CURDLE_EINVAL, "n = %zu exceeds the supported 65,536 pairs", n);
  return CURDLE_OK;
}

// the slot's small buffer: zeroes the status word on st
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
  if (static_cast<const uint32_t*>(h_out)[36]) return fail(CURDLE_EINVAL, "a scalar is not below 2^scalar_bits");
  memcpy(out_jac, h_out, 144);
  return CURDLE_OK;
}

// The host forms' n pairs on their way to the device: the slot's buffers, the notes on the WipeList (the scalars' two
// copies and the term workspace), `fill` writing the scalars (n records of 32 bytes) and then the points (96 bytes each)
// into the pinned staging it is handed, and the two uploads on st.  Behind it S.scalars and S.points hold the pairs.
template <class Fill>
int stage_pairs(Slot& S, WipeList& W, size_t n, hipStream_t st, Fill&& fill) {
  int r;
  if ((r = ensure(S.points, n * 96))) return r;
  if ((r = ensure(S.scalars, n * 32))) return r;
  if ((r = ensure(S.partials, n * kMsmCtTermBytes))) return r;
  if ((r = ensure_pinned(S, 0, n * 32 + n * 96))) return r;  // scalars | points
  W.note_device(S.scalars.p, n * 32);
  W.note_device(S.partials.p, n * kMsmCtTermBytes);
  W.note_host(S.h_stage[0], n * 32);
  uint8_t* h_sc = static_cast<uint8_t*>(S.h_stage[0]);
  uint8_t* h_pt = h_sc + n * 32;
  fill(h_sc, h_pt);
  HIP_TRY(hipMemcpyAsync(S.scalars.p, h_sc, n * 32, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(S.points.p, h_pt, n * 96, hipMemcpyHostToDevice, st));
  return CURDLE_OK;
}

unsigned bit_length(size_t v) {
  unsigned b = 0;
  for (; v; v >>= 1) b++;
  return b;
}
}  // namespace

extern "C" int curdle_msm_g1_ct(const uint64_t* points, const uint64_t* scalars, size_t n, unsigned scalar_bits,
                                uint64_t out_jac[18]) {
  if (int rc = check_args(points, scalars, n, scalar_bits, out_jac)) return rc;
  if (n == 0) {
    set_out_infinity(out_jac);
    return CURDLE_OK;
  }
  SlotHold H(cur(), true, nullptr);
  WipeList W(H.stream());
  H.wipe_on_exit(&W, "constant-time MSM: clearing the scalars and the terms");
  return H.run([&]() -> int {
    Slot& S = H.slot();
    const hipStream_t st = H.stream();
    int r;
    if ((r = stage_pairs(S, W, n, st, [&](uint8_t* h_sc, uint8_t* h_pt) {
          memcpy(h_sc, scalars, n * 32);
          memcpy(h_pt, points, n * 96);
        })))
      return r;
    if ((r = ensure_pinned(S, 1, kOutBytes))) return r;
    if ((r = prepare_out(S, st))) return r;
    HIP_TRY(launch_msm_ct_walk(S.points.p, S.scalars.p, kMsmCtScalarFr, scalar_bits, (uint32_t)n, S.partials.p, status_word(S), st));
    if ((r = sum_and_fetch(S, n, S.h_stage[1], out_jac, st))) return r;
    count_msm_ct(n, 1);
    return CURDLE_OK;
  });
}

extern "C" int curdle_msm_g1_ct_device(const void* d_points, const void* d_scalars, size_t n, unsigned scalar_bits,
                                       uint64_t out_jac[18], void* stream) {
  if (int rc = check_args(d_points, d_scalars, n, scalar_bits, out_jac)) return rc;
  if (n == 0) {
    set_out_infinity(out_jac);
    return CURDLE_OK;
  }
  if (!aligned16(d_points) || !aligned16(d_scalars)) return fail(CURDLE_EINVAL, "device pointers must be multiples of 16");
  SlotHold H(cur(), true, stream);
  WipeList W(H.stream());
  H.wipe_on_exit(&W, "constant-time MSM: clearing the terms");
  return H.run([&]() -> int {
    Slot& S = H.slot();
    const hipStream_t st = H.stream();
    int r;
    if ((r = ensure(S.partials, n * kMsmCtTermBytes))) return r;
    if ((r = ensure_pinned(S, 1, kOutBytes))) return r;
    W.note_device(S.partials.p, n * kMsmCtTermBytes);
    if ((r = prepare_out(S, st))) return r;
    // the caller's scalars are read where they are: nothing of them is copied
    HIP_TRY(launch_msm_ct_walk(d_points, d_scalars, kMsmCtScalarFr, scalar_bits, (uint32_t)n, S.partials.p, status_word(S), st));
    if ((r = sum_and_fetch(S, n, S.h_stage[1], out_jac, st))) return r;
    count_msm_ct(n, 1);
    return CURDLE_OK;
  });
}

extern "C" int curdle_stat_msm_ct(unsigned long long out[3]) { return read_stats(out, g_msm_ct_stat, 3); }

// ---------------------------------------------------------------------------------------------------------------------
// The batched forms: k MSMs (curdle_msm_g1_ct_batch / _device), or one scalar vector against k base sets
// (curdle_msm_g1_ct_multi), in ONE launch of k_msm_ct_walk over the concatenated pairs, the segmented sum
// (k_g1_sum_ct_seg per level, k_msm_ct_finish_seg) and ONE copy back of 144 k + 4 bytes: the k results and the violation
// word.  The slot's small buffer holds, in this order, the results, the word the finish kernel copies the violation word
// to, and -- from the next multiple of 16 -- the walk's status word; the table of (begin, count) goes through the second
// pinned staging (behind the block that comes back) into the slot's `offsets` buffer.  It is made of `offsets`: public.
// ---------------------------------------------------------------------------------------------------------------------
namespace {
constexpr size_t kMsmCtBatchMax = 4096;  // MSMs of one call

// batched calls | MSMs in them | level launches (k_g1_sum_ct_seg); completed calls that ran on a device only
std::atomic<unsigned long long> g_msm_ct_batch_stat[3];

struct BatchShape {
  size_t k = 0, lo = 0, total = 0;
  std::vector<uint32_t> seg;     // (begin, count) per MSM, begin relative to the call's first pair
  std::vector<uint32_t> counts;  // count per MSM
  size_t nonempty = 0;
};

// What the batch refuses after the null arguments: scalar_bits, k, offsets that decrease, the total.
int batch_shape(const size_t* offsets, size_t k, unsigned bits, BatchShape* sh) {
  if (int rc = check_scalar_bits(bits)) return rc;
  if (k > kMsmCtBatchMax) return fail(CURDLE_EINVAL, "k = %zu exceeds the supported 4,096 MSMs of one call", k);
  for (size_t j = 0; j < k; j++)
    if (offsets[j + 1] < offsets[j]) return fail(CURDLE_EINVAL, "offsets decrease at %zu", j);
  sh->k = k;
  sh->lo = k ? offsets[0] : 0;
  sh->total = k ? offsets[k] - offsets[0] : 0;
  if (sh->total > kMsmCtMax) return fail(CURDLE_EINVAL, "%zu pairs in all exceed the supported 65,536 pairs", sh->total);
  sh->seg.resize(2 * k);
  sh->counts.resize(k);
  for (size_t j = 0; j < k; j++) {
    sh->seg[2 * j] = (uint32_t)(offsets[j] - sh->lo);
    sh->seg[2 * j + 1] = sh->counts[j] = (uint32_t)(offsets[j + 1] - offsets[j]);
    sh->nonempty += offsets[j + 1] != offsets[j];
  }
  return CURDLE_OK;
}

}  // namespace
namespace curdle_api {
void count_msm_ct_batch(size_t msms, unsigned levels) {
  g_msm_ct_batch_stat[0].fetch_add(1, std::memory_order_relaxed);
  g_msm_ct_batch_stat[1].fetch_add(msms, std::memory_order_relaxed);
  g_msm_ct_batch_stat[2].fetch_add(levels, std::memory_order_relaxed);
}
}  // namespace curdle_api
namespace {
size_t batch_out_bytes(size_t k) { return 144 * k + 4; }                         // what comes back
size_t batch_status_offset(size_t k) { return (144 * k + 4 + 15) / 16 * 16; }    // the walk's status word

// On the call's stream, behind the scalars and the points: the status word, the table, the walk, the sum, the copy, the
// wait, the verdict.  h_block: pinned, batch_out_bytes(k) and the table behind it (from the next multiple of 16).
int batch_walk_sum_fetch(Slot& S, const BatchShape& sh, const void* d_points, const void* d_scalars, unsigned bits,
                         uint64_t* out_jac, hipStream_t st) {
  const size_t k = sh.k, status_off = batch_status_offset(k), table_bytes = 8 * k;
  int r;
  if ((r = ensure(S.results, status_off + 16))) return r;
  if ((r = ensure(S.offsets, table_bytes))) return r;
  if ((r = ensure_pinned(S, 1, status_off + table_bytes))) return r;
  uint8_t* h_block = static_cast<uint8_t*>(S.h_stage[1]);
  uint8_t* d_res = static_cast<uint8_t*>(S.results.p);
  uint32_t* d_status = reinterpret_cast<uint32_t*>(d_res + status_off);
  memcpy(h_block + status_off, sh.seg.data(), table_bytes);
  HIP_TRY(hipMemsetAsync(d_status, 0, 16, st));
  HIP_TRY(hipMemcpyAsync(S.offsets.p, h_block + status_off, table_bytes, hipMemcpyHostToDevice, st));
  HIP_TRY(launch_msm_ct_walk(d_points, d_scalars, kMsmCtScalarFr, bits, (uint32_t)sh.total, S.partials.p, d_status, st));
  uint32_t levels = 0;
  HIP_TRY(launch_msm_ct_sum_seg(S.partials.p, S.offsets.p, sh.counts.data(), (uint32_t)k, d_status, d_res, &levels, st));
  HIP_TRY(hipMemcpyAsync(h_block, d_res, batch_out_bytes(k), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  uint32_t verdict;
  memcpy(&verdict, h_block + 144 * k, 4);
  if (verdict) return fail(CURDLE_EINVAL, "a scalar is not below 2^scalar_bits");
  memcpy(out_jac, h_block, 144 * k);
  g_msm_ct_stat[0].fetch_add(sh.total, std::memory_order_relaxed);
  g_msm_ct_stat[1].fetch_add(1, std::memory_order_relaxed);
  g_msm_ct_stat[2].fetch_add(sh.nonempty, std::memory_order_relaxed);
  count_msm_ct_batch(k, levels);
  return CURDLE_OK;
}

// The host forms behind their checks: `fill` is stage_pairs' over the sh.total pairs.
template <class Fill>
int batch_from_host(const BatchShape& sh, unsigned bits, uint64_t* out_jac, const char* what, Fill&& fill) {
  SlotHold H(cur(), true, nullptr);
  WipeList W(H.stream());
  H.wipe_on_exit(&W, what);
  return H.run([&]() -> int {
    Slot& S = H.slot();
    const hipStream_t st = H.stream();
    if (int r = stage_pairs(S, W, sh.total, st, fill)) return r;
    return batch_walk_sum_fetch(S, sh, S.points.p, S.scalars.p, bits, out_jac, st);
  });
}
}  // namespace

extern "C" int curdle_msm_g1_ct_batch(const uint64_t* points, const uint64_t* scalars, const size_t* offsets, size_t k,
                                      unsigned scalar_bits, uint64_t* out_jac) {
  if (!offsets || (k && (!out_jac || !points || !scalars))) return fail(CURDLE_EINVAL, "null argument");
  BatchShape sh;
  if (int rc = batch_shape(offsets, k, scalar_bits, &sh)) return rc;
  if (k == 0) return CURDLE_OK;
  if (sh.total == 0) {
    for (size_t j = 0; j < k; j++) set_out_infinity(out_jac + 18 * j);
    return CURDLE_OK;
  }
  return batch_from_host(sh, scalar_bits, out_jac, "batched constant-time MSM: clearing the scalars and the terms",
                         [&](uint8_t* h_sc, uint8_t* h_pt) {
                           memcpy(h_sc, scalars + 4 * sh.lo, sh.total * 32);
                           memcpy(h_pt, points + 12 * sh.lo, sh.total * 96);
                         });
}

extern "C" int curdle_msm_g1_ct_batch_device(const void* d_points, const void* d_scalars, const size_t* offsets, size_t k,
                                             unsigned scalar_bits, uint64_t* out_jac, void* stream) {
  if (!offsets || (k && (!out_jac || !d_points || !d_scalars))) return fail(CURDLE_EINVAL, "null argument");
  BatchShape sh;
  if (int rc = batch_shape(offsets, k, scalar_bits, &sh)) return rc;
  if (k == 0) return CURDLE_OK;
  if (!aligned16(d_points) || !aligned16(d_scalars)) return fail(CURDLE_EINVAL, "device pointers must be multiples of 16");
  if (sh.total == 0) {
    for (size_t j = 0; j < k; j++) set_out_infinity(out_jac + 18 * j);
    return CURDLE_OK;
  }
  SlotHold H(cur(), true, stream);
  WipeList W(H.stream());
  H.wipe_on_exit(&W, "batched constant-time MSM: clearing the terms");
  return H.run([&]() -> int {
    Slot& S = H.slot();
    if (int r = ensure(S.partials, sh.total * kMsmCtTermBytes)) return r;
    W.note_device(S.partials.p, sh.total * kMsmCtTermBytes);
    // the caller's arrays are read where they are, from the call's first pair (96 and 32 bytes a record keep the alignment)
    return batch_walk_sum_fetch(S, sh, static_cast<const uint8_t*>(d_points) + 96 * sh.lo,
                                static_cast<const uint8_t*>(d_scalars) + 32 * sh.lo, scalar_bits, out_jac, H.stream());
  });
}

// One scalar vector against k base sets: the vector is replicated k times in the pinned staging (a host copy of public
// length) and the call is the batch of k MSMs of n pairs; the replicas are the staging's scalars and are wiped with it.
extern "C" int curdle_msm_g1_ct_multi(const uint64_t* const* points_sets, size_t k, const uint64_t* scalars, size_t n,
                                      unsigned scalar_bits, uint64_t* out_jac) {
  if (k && (!out_jac || !points_sets || (n && !scalars))) return fail(CURDLE_EINVAL, "null argument");
  if (int rc = check_scalar_bits(scalar_bits)) return rc;
  if (k > kMsmCtBatchMax) return fail(CURDLE_EINVAL, "k = %zu exceeds the supported 4,096 MSMs of one call", k);
  if (k == 0) return CURDLE_OK;
  if (n > kMsmCtMax / k) return fail(CURDLE_EINVAL, "k n = %zu x %zu exceeds the supported 65,536 pairs", k, n);
  if (n == 0) {
    for (size_t j = 0; j < k; j++) set_out_infinity(out_jac + 18 * j);
    return CURDLE_OK;
  }
  for (size_t j = 0; j < k; j++)
    if (!points_sets[j]) return fail(CURDLE_EINVAL, "null argument: base set %zu", j);
  std::vector<size_t> offsets(k + 1);
  for (size_t j = 0; j <= k; j++) offsets[j] = j * n;
  BatchShape sh;
  if (int rc = batch_shape(offsets.data(), k, scalar_bits, &sh)) return rc;
  return batch_from_host(sh, scalar_bits, out_jac,
                         "constant-time MSM over k base sets: clearing the replicated scalars and the terms",
                         [&](uint8_t* h_sc, uint8_t* h_pt) {
                           for (size_t j = 0; j < k; j++) {
                             memcpy(h_sc + j * n * 32, scalars, n * 32);
                             memcpy(h_pt + j * n * 96, points_sets[j], n * 96);
                           }
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
