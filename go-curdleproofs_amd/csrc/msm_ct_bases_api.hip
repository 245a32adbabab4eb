// C ABI of the constant-time MSM over a resident PUBLIC base set (msm_ct_bases_kernels.hip): curdle_ct_bases, the handle
// of a table of C = ceil(255 / c) rows 2^(c j) P_i; curdle_msm_g1_ct_bases / _device / _batch / _batch_device, the MSM
// whose lanes walk c-bit chunks of the scalars over that table; curdle_stat_msm_ct_bases.
//
// The handle.  Its device copies are a ResidentCopy (api_helpers.h), as a resident base set's and a fixed-base table's
// are: one per context, made on first use there and again after a curdle_shutdown; a free during a call is deferred to
// that call's end.  The FIRST copy is built on the device -- row 0 uploaded, k_ct_bases_shift into a staging of G1XYZZ
// records that lives for the build only, k_g1_normalize's XYZZ form into rows 1 ... C - 1 -- and the rows come back into
// the handle's host copy, which every later copy is an upload of and which curdle_ct_bases_export reads.  n C <= 65,536
// keeps the staging within the constant-time MSM's term workspace (65,536 records of no more than 224 bytes).  The
// table is PUBLIC: nothing of it is wiped.
//
// The MSM.  The single call is the batch of one MSM: ONE body (rows_walk_sum_fetch) behind the checks.  On the call's
// one stream: the public tables -- (begin Cb, count Cb) per MSM and the row indices -- go up through the second pinned
// staging, k_msm_ct_walk_rows writes the n Cb terms into the slot's `partials`, the segmented sum of msm_ct_kernels.hip
// folds and finishes each MSM's run and ONE block of 144 k + 4 bytes comes back: the results and the violation word.
// The host forms stage the scalars through the first pinned staging and a device buffer; both, and the term workspace
// in every form, are on the call's WipeList.
#include "api_helpers.h"

#include <algorithm>

struct curdle_ct_bases {
  size_t n = 0;
  unsigned c = 0, chunks = 0;  // chunk_bits and C = ceil(255 / c)
  std::vector<uint64_t> host;  // C rows of n gnark G1Affine records; rows 1 ... C - 1 valid once `built`
  bool built = false;          // written under copy.mu by the first upload, which curdle_ct_bases_create waits for
  ResidentCopy copy;           // per context: the C rows
};

namespace {
constexpr size_t kTermMax = 65536;   // terms of one call, and records of one table: one pass
constexpr size_t kBatchMax = 4096;   // MSMs of one call
// The library's choice for chunk_bits = 0.  Measured (profiles/r33_msm_ct_bases.json; 255 bits, c = 8 / 16 / 32 / 64):
// 256 pairs 1.26 / 1.34 / 1.61 / 2.11 ms, 2,048 pairs 1.97 / 1.71 / 1.79 / 2.25 ms against 5.7 ms for curdle_msm_g1_ct_device.
// 8 wins by less than 0.2 ms at small calls, loses at 2,048 pairs, doubles the table and halves the pairs one call may
// hold (4,096 pairs no longer fit the 65,536 terms); 32 and 64 are slower.  DESIGN.md section 0, round 33.
constexpr unsigned kDefaultChunkBits = 16;

// tables built on a device | calls | (pair, chunk) lanes walked | MSMs finished; completed calls that ran on a device only
std::atomic<unsigned long long> g_stat[4];

unsigned chunks_of(unsigned bits, unsigned c) { return (bits + c - 1) / c; }

int bases_acquire(Ctx& cx, curdle_ct_bases* b, void** d_table) {
  static const ResidentCopy::Text text = {"the constant-time base table was freed",
                                          "the context was shut down under a constant-time base table upload",
                                          "constant-time base table"};
  ResidentCopy::Upload upload;
  if (b->n)  // an empty set has nothing to upload: its copy stays null
    upload = [b](hipStream_t st, void** dst) {
      const size_t n = b->n, C = b->chunks, row = n * 96;
      uint8_t* h = reinterpret_cast<uint8_t*>(b->host.data());
      void* staging = nullptr;
      hipError_t e = hipMalloc(dst, C * row);
      if (b->built) {
        if (e == hipSuccess) e = hipMemcpyAsync(*dst, h, C * row, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        return e;
      }
      uint8_t* d = static_cast<uint8_t*>(*dst);
      if (e == hipSuccess) e = hipMalloc(&staging, (C - 1) * n * sizeof(G1XYZZ));
      if (e == hipSuccess) e = hipMemcpyAsync(d, h, row, hipMemcpyHostToDevice, st);
      if (e == hipSuccess) e = launch_ct_bases_shift(d, (uint32_t)n, b->c, (uint32_t)C, staging, st);
      if (e == hipSuccess) e = launch_g1_normalize(staging, kNormalizeXyzz, (uint32_t)((C - 1) * n), d + row, st, nullptr);
      if (e == hipSuccess) e = hipMemcpyAsync(h + row, d + row, (C - 1) * row, hipMemcpyDeviceToHost, st);
      if (e == hipSuccess) e = hipStreamSynchronize(st);
      if (staging) (void)hipFree(staging);
      if (e == hipSuccess) {
        b->built = true;
        g_stat[0].fetch_add(1, std::memory_order_relaxed);
      }
      return e;
    };
  return b->copy.acquire(cx, upload, text, d_table);
}

void bases_release(curdle_ct_bases* b) {
  if (b->copy.release()) delete b;
}

// What both creators refuse after the null arguments: chunk_bits, then n C.  *c: the chunk width taken.
int check_create(size_t n, unsigned chunk_bits, unsigned* c) {
  *c = chunk_bits ? chunk_bits : kDefaultChunkBits;
  if (*c != 8 && *c != 16 && *c != 32 && *c != 64)
    return fail(CURDLE_EINVAL, "chunk_bits = %u is not 8, 16, 32, 64 or 0 (the library's choice)", chunk_bits);
  if (n > kTermMax / chunks_of(255, *c))
    return fail(CURDLE_EINVAL, "n C = %zu x %u exceeds the supported 65,536 table records", n, chunks_of(255, *c));
  return CURDLE_OK;
}

// The handle over n points which `fill` writes into row 0 (on the calling thread's context when n > 0), built there.
template <class Fill>
int create(size_t n, unsigned c, curdle_ct_bases** out, Fill&& fill) {
  curdle_ct_bases* b = new (std::nothrow) curdle_ct_bases();
  if (!b) return fail(CURDLE_ENOMEM, "out of memory");
  b->n = n;
  b->c = c;
  b->chunks = chunks_of(255, c);
  try {
    b->host.resize(12 * n * b->chunks);
  } catch (const std::bad_alloc&) {
    delete b;
    return fail(CURDLE_ENOMEM, "out of memory");
  }
  int rc = CURDLE_OK;
  if (n) {
    // resident on the creating thread's context now (a failure here is the caller's to see); on every other context
    // when a call there first names the handle
    void* d = nullptr;
    if ((rc = fill(b->host.data())) == CURDLE_OK && (rc = bases_acquire(cur(), b, &d)) == CURDLE_OK) bases_release(b);
  }
  if (rc) {
    delete b;
    return rc;
  }
  *out = b;
  return CURDLE_OK;
}

// The shape of a call behind its null arguments, in the order the header states: scalar_bits, k, offsets that
// decrease, the term total, a row index out of range.  The single call is offsets = {0, n}, k = 1.
struct Shape {
  size_t k = 0, lo = 0, total = 0, nonempty = 0;
  unsigned cb = 0;               // chunks walked: ceil(scalar_bits / c)
  std::vector<uint32_t> seg;     // (begin Cb, count Cb) per MSM, begin relative to the call's first pair
  std::vector<uint32_t> counts;  // count Cb per MSM
};

int shape_of(const curdle_ct_bases* b, const uint32_t* rows, const size_t* offsets, size_t k, unsigned bits, bool batch, Shape* sh) {
  if (bits < 1 || bits > 255) return fail(CURDLE_EINVAL, "scalar_bits = %u is not in 1...255", bits);
  if (batch && k > kBatchMax) return fail(CURDLE_EINVAL, "k = %zu exceeds the supported 4,096 MSMs of one call", k);
  for (size_t j = 0; j < k; j++)
    if (offsets[j + 1] < offsets[j]) return fail(CURDLE_EINVAL, "offsets decrease at %zu", j);
  sh->k = k;
  sh->cb = chunks_of(bits, b->c);
  sh->lo = k ? offsets[0] : 0;
  const size_t hi = k ? offsets[k] : 0;
  sh->total = hi - sh->lo;
  if (sh->total > kTermMax / sh->cb)
    return fail(CURDLE_EINVAL, "n Cb = %zu x %u exceeds the supported 65,536 terms of one call", sh->total, sh->cb);
  if (rows) {
    for (size_t p = sh->lo; p < hi; p++)
      if (rows[p] >= b->n) return fail(CURDLE_EINVAL, "rows[%zu] = %u is not below the %zu resident bases", p, rows[p], b->n);
  } else if (sh->total && hi > b->n) {
    return fail(CURDLE_EINVAL, "rows is null and the pairs end at %zu, beyond the %zu resident bases", hi, b->n);
  }
  sh->seg.resize(2 * k);
  sh->counts.resize(k);
  for (size_t j = 0; j < k; j++) {
    sh->seg[2 * j] = (uint32_t)((offsets[j] - sh->lo) * sh->cb);
    sh->seg[2 * j + 1] = sh->counts[j] = (uint32_t)((offsets[j + 1] - offsets[j]) * sh->cb);
    sh->nonempty += offsets[j + 1] != offsets[j];
  }
  return CURDLE_OK;
}

size_t round16(size_t v) { return (v + 15) / 16 * 16; }

// One call behind its checks, sh.total > 0.  scalars: the call's FIRST pair's, in host memory (resident false: staged
// and wiped here) or in device memory (read where they are).  rows: the caller's array from index 0, or null.
int rows_walk_sum_fetch(const curdle_ct_bases* bases, const uint32_t* rows, const void* scalars, bool resident, const Shape& sh,
                        unsigned bits, bool batch, uint64_t* out_jac, void* stream) {
  Ctx& cx = cur();
  curdle_ct_bases* b = const_cast<curdle_ct_bases*>(bases);
  void* d_table = nullptr;
  if (int rc = bases_acquire(cx, b, &d_table)) return rc;  // this context's copy, made on first use
  SlotHold H(cx, true, stream);
  WipeList W(H.stream());
  H.wipe_on_exit(&W, resident ? "constant-time MSM over resident bases: clearing the terms"
                              : "constant-time MSM over resident bases: clearing the scalars and the terms");
  const int rc = H.run([&]() -> int {
    Slot& S = H.slot();
    const hipStream_t st = H.stream();
    const size_t k = sh.k, n = sh.total, terms = n * sh.cb;
    // the slot's small buffer: k results | the word the finish copies the verdict to | from the next 16: the status word
    const size_t status_off = round16(144 * k + 4), seg_bytes = 8 * k, rows_off = round16(status_off + seg_bytes);
    int r;
    if ((r = ensure(S.partials, terms * kMsmCtTermBytes))) return r;
    if ((r = ensure(S.results, status_off + 16))) return r;
    if ((r = ensure(S.offsets, seg_bytes))) return r;
    if ((r = ensure(S.tmp, 4 * n))) return r;
    if ((r = ensure_pinned(S, 1, rows_off + 4 * n))) return r;  // what comes back | the segments | the rows: public
    W.note_device(S.partials.p, terms * kMsmCtTermBytes);
    const void* d_scalars = scalars;
    if (!resident) {
      if ((r = ensure(S.scalars, n * 32))) return r;
      if ((r = ensure_pinned(S, 0, n * 32))) return r;
      W.note_device(S.scalars.p, n * 32);
      W.note_host(S.h_stage[0], n * 32);
      memcpy(S.h_stage[0], scalars, n * 32);
      HIP_TRY(hipMemcpyAsync(S.scalars.p, S.h_stage[0], n * 32, hipMemcpyHostToDevice, st));
      d_scalars = S.scalars.p;
    }
    uint8_t* h_block = static_cast<uint8_t*>(S.h_stage[1]);
    uint8_t* d_res = static_cast<uint8_t*>(S.results.p);
    uint32_t* d_status = reinterpret_cast<uint32_t*>(d_res + status_off);
    uint32_t* h_rows = reinterpret_cast<uint32_t*>(h_block + rows_off);
    memcpy(h_block + status_off, sh.seg.data(), seg_bytes);
    for (size_t p = 0; p < n; p++) h_rows[p] = rows ? rows[sh.lo + p] : (uint32_t)(sh.lo + p);
    HIP_TRY(hipMemsetAsync(d_status, 0, 16, st));
    HIP_TRY(hipMemcpyAsync(S.offsets.p, h_block + status_off, seg_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(S.tmp.p, h_rows, 4 * n, hipMemcpyHostToDevice, st));
    HIP_TRY(launch_msm_ct_walk_rows(d_table, (uint32_t)b->n, static_cast<const uint32_t*>(S.tmp.p), d_scalars, b->c, bits,
                                    (uint32_t)n, S.partials.p, d_status, st));
    uint32_t levels = 0;
    HIP_TRY(launch_msm_ct_sum_seg(S.partials.p, S.offsets.p, sh.counts.data(), (uint32_t)k, d_status, d_res, &levels, st));
    HIP_TRY(hipMemcpyAsync(h_block, d_res, 144 * k + 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    uint32_t verdict;
    memcpy(&verdict, h_block + 144 * k, 4);
    if (verdict) return fail(CURDLE_EINVAL, "a scalar is not below 2^scalar_bits");
    memcpy(out_jac, h_block, 144 * k);
    g_stat[1].fetch_add(1, std::memory_order_relaxed);
    g_stat[2].fetch_add(terms, std::memory_order_relaxed);
    g_stat[3].fetch_add(sh.nonempty, std::memory_order_relaxed);
    if (batch) count_msm_ct_batch(k, levels);
    return CURDLE_OK;
  });
  bases_release(b);
  return rc;
}

int single(const curdle_ct_bases* b, const uint32_t* rows, const void* scalars, bool resident, size_t n, unsigned bits,
           uint64_t out_jac[18], void* stream) {
  if (!b || !out_jac || (n && !scalars)) return fail(CURDLE_EINVAL, "null argument");
  const size_t offsets[2] = {0, n};
  Shape sh;
  if (int rc = shape_of(b, rows, offsets, 1, bits, false, &sh)) return rc;
  if (n == 0) {
    set_out_infinity(out_jac);
    return CURDLE_OK;
  }
  if (resident && !aligned16(scalars)) return fail(CURDLE_EINVAL, "device pointers must be multiples of 16");
  return rows_walk_sum_fetch(b, rows, scalars, resident, sh, bits, false, out_jac, stream);
}

int batch(const curdle_ct_bases* b, const uint32_t* rows, const void* scalars, bool resident, const size_t* offsets, size_t k,
          unsigned bits, uint64_t* out_jac, void* stream) {
  if (!b || !offsets || (k && (!out_jac || !scalars))) return fail(CURDLE_EINVAL, "null argument");
  Shape sh;
  if (int rc = shape_of(b, rows, offsets, k, bits, true, &sh)) return rc;
  if (k == 0) return CURDLE_OK;
  if (resident && !aligned16(scalars)) return fail(CURDLE_EINVAL, "device pointers must be multiples of 16");
  if (sh.total == 0) {
    for (size_t j = 0; j < k; j++) set_out_infinity(out_jac + 18 * j);
    return CURDLE_OK;
  }
  // the call's first pair (32 bytes a record keep the alignment)
  return rows_walk_sum_fetch(b, rows, static_cast<const uint8_t*>(scalars) + 32 * sh.lo, resident, sh, bits, true, out_jac, stream);
}
}  // namespace

extern "C" int curdle_ct_bases_create(const uint64_t* points, size_t n, unsigned chunk_bits, curdle_ct_bases** out) {
  if (out) *out = nullptr;
  if (!out || (n && !points)) return fail(CURDLE_EINVAL, "null argument");
  unsigned c;
  if (int rc = check_create(n, chunk_bits, &c)) return rc;
  return create(n, c, out, [&](uint64_t* row0) {
    memcpy(row0, points, n * 96);
    return CURDLE_OK;
  });
}

extern "C" int curdle_ct_bases_create_device(const void* d_points, size_t n, unsigned chunk_bits, curdle_ct_bases** out, void* stream) {
  if (out) *out = nullptr;
  if (!out || (n && !d_points)) return fail(CURDLE_EINVAL, "null argument");
  unsigned c;
  if (int rc = check_create(n, chunk_bits, &c)) return rc;
  if (n && !aligned16(d_points)) return fail(CURDLE_EINVAL, "device pointers must be multiples of 16");
  // the points come down into the handle's host copy (behind what the caller queued on `stream`) and the handle is
  // then built like the host form's: one path, and the host copy is what every other context is made from anyway
  return create(n, c, out, [&](uint64_t* row0) -> int {
    Ctx& cx = cur();
    hipStream_t st = (hipStream_t)stream;
    {
      std::lock_guard<std::mutex> g(cx.mu);
      if (int rc = init_default_locked(cx)) return rc;
      if (!st) st = cx.util_stream;
    }
    HIP_TRY(hipSetDevice(cx.device));
    HIP_TRY(hipMemcpyAsync(row0, d_points, n * 96, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return CURDLE_OK;
  });
}

extern "C" void curdle_ct_bases_free(curdle_ct_bases* b) {
  if (b && b->copy.free_or_defer()) delete b;
}

extern "C" size_t curdle_ct_bases_size(const curdle_ct_bases* b) { return b ? b->n : 0; }
extern "C" unsigned curdle_ct_bases_chunk_bits(const curdle_ct_bases* b) { return b ? b->c : 0; }

extern "C" int curdle_ct_bases_export(const curdle_ct_bases* b, unsigned chunk, uint64_t* rows_out) {
  if (!b || (b->n && !rows_out)) return fail(CURDLE_EINVAL, "null argument");
  if (chunk >= b->chunks) return fail(CURDLE_EINVAL, "chunk = %u is not below the table's %u rows", chunk, b->chunks);
  if (b->n) memcpy(rows_out, b->host.data() + 12 * b->n * chunk, b->n * 96);
  return CURDLE_OK;
}

extern "C" int curdle_msm_g1_ct_bases(const curdle_ct_bases* b, const uint32_t* rows, const uint64_t* scalars, size_t n,
                                      unsigned scalar_bits, uint64_t out_jac[18]) {
  return single(b, rows, scalars, false, n, scalar_bits, out_jac, nullptr);
}

extern "C" int curdle_msm_g1_ct_bases_device(const curdle_ct_bases* b, const uint32_t* rows, const void* d_scalars, size_t n,
                                             unsigned scalar_bits, uint64_t out_jac[18], void* stream) {
  return single(b, rows, d_scalars, true, n, scalar_bits, out_jac, stream);
}

extern "C" int curdle_msm_g1_ct_bases_batch(const curdle_ct_bases* b, const uint32_t* rows, const uint64_t* scalars,
                                            const size_t* offsets, size_t k, unsigned scalar_bits, uint64_t* out_jac) {
  return batch(b, rows, scalars, false, offsets, k, scalar_bits, out_jac, nullptr);
}

extern "C" int curdle_msm_g1_ct_bases_batch_device(const curdle_ct_bases* b, const uint32_t* rows, const void* d_scalars,
                                                   const size_t* offsets, size_t k, unsigned scalar_bits, uint64_t* out_jac,
                                                   void* stream) {
  return batch(b, rows, d_scalars, true, offsets, k, scalar_bits, out_jac, stream);
}

extern "C" int curdle_stat_msm_ct_bases(unsigned long long out[4]) { return read_stats(out, g_stat, 4); }
