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
// The MSM.  The single call is the batch of one MSM, and a call over one handle is the call over up to four sets
// (curdle_msm_g1_ct_bases_sets_batch: the prover's funnel calls mix CRS points and instance points) with one set: ONE
// body (rows_call) behind the checks, and that body is the
// segmented call of msm_ct_call.h (seg_walk_sum_fetch, which curdle_msm_g1_ct_batch runs too) with this family's walk.
// The sets reach the walk as a kernel argument (CtRowSets: table, size and first index of each); every handle of a call
// is acquired before the device work and released behind it (SetsHold).
// On the call's one stream: the public tables -- (begin Cb, count Cb) per MSM and, behind it, the row indices -- go up
// through the second pinned staging, k_msm_ct_walk_rows writes the n Cb terms into the slot's `partials`, the segmented
// sum of msm_ct_kernels.hip folds and finishes each MSM's run and ONE block of 144 k + 4 bytes comes back: the results
// and the violation word.  The host forms stage the scalars through the first pinned staging and a device buffer
// (stage_scalars); both, and the term workspace in every form, are on the call's WipeList.  The tables are public and
// are not.
#include "msm_ct_call.h"

#include <algorithm>

struct curdle_ct_bases {
  size_t n = 0;
  unsigned c = 0, chunks = 0;  // chunk_bits and C = ceil(255 / c)
  std::vector<uint64_t> host;  // C rows of n gnark G1Affine records; rows 1 ... C - 1 valid once `built`
  bool built = false;          // written under copy.mu by the first upload, which curdle_ct_bases_create waits for
  ResidentCopy copy;           // per context: the C rows
};

namespace {
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
  if (n > kMsmCtMaxTerms / chunks_of(255, *c))
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
// seg_shape (msm_ct_call.h) runs all but the last with a pair counting Cb = ceil(scalar_bits / c) terms.
// n: the records the call's sets hold in all, c: their one chunk width.
int shape_of(size_t n, unsigned c, const uint32_t* rows, const size_t* offsets, size_t k, unsigned bits, SegShape* sh) {
  // (a scalar_bits out of range is refused before the stride is looked at)
  if (int rc = seg_shape(offsets, k, bits, chunks_of(bits, c), TotalText::kTerms, sh)) return rc;
  const size_t hi = sh->lo + sh->total;
  if (rows) {
    for (size_t p = sh->lo; p < hi; p++)
      if (rows[p] >= n) return fail(CURDLE_EINVAL, "rows[%zu] = %u is not below the %zu resident bases", p, rows[p], n);
  } else if (sh->total && hi > n) {
    return fail(CURDLE_EINVAL, "rows is null and the pairs end at %zu, beyond the %zu resident bases", hi, n);
  }
  return CURDLE_OK;
}

// The handles of one call, each a user of its ResidentCopy from acquire() until this dies: every set is acquired before
// the call's device work and released behind it on every way out, so a free during the call is deferred for each.
struct SetsHold {
  curdle_ct_bases* held[kCtRowSetsMax] = {};
  size_t n_held = 0;
  CtRowSets desc = {};
  // This context's copies, made on first use; an empty set has none and covers no index.
  int acquire(Ctx& cx, const curdle_ct_bases* const* sets, size_t n_sets) {
    uint32_t first = 0;
    for (size_t s = 0; s < (size_t)kCtRowSetsMax; s++) {
      desc.first[s] = first;
      if (s >= n_sets) continue;
      curdle_ct_bases* b = const_cast<curdle_ct_bases*>(sets[s]);
      void* d_table = nullptr;
      if (int rc = bases_acquire(cx, b, &d_table)) return rc;
      held[n_held++] = b;
      desc.table[s] = d_table;
      desc.size[s] = (uint32_t)b->n;
      first += (uint32_t)b->n;
    }
    return CURDLE_OK;
  }
  ~SetsHold() {
    while (n_held) bases_release(held[--n_held]);
  }
};

// One call behind its checks, sh.total > 0, over n_sets handles at one chunk width (the single-handle calls: one set).
// scalars: the call's FIRST pair's, in host memory (resident false: staged and wiped here) or in device memory (read
// where they are).  rows: the caller's array from index 0, or null.
int rows_call(const curdle_ct_bases* const* sets, size_t n_sets, const uint32_t* rows, const void* scalars, bool resident,
              const SegShape& sh, unsigned bits, bool batch, uint64_t* out_jac, void* stream) {
  Ctx& cx = cur();
  const unsigned c = sets[0]->c;
  SetsHold held;
  if (int rc = held.acquire(cx, sets, n_sets)) return rc;
  SlotHold H(cx, true, stream);
  WipeList W(H.stream());
  H.wipe_on_exit(&W, resident ? "constant-time MSM over resident bases: clearing the terms"
                              : "constant-time MSM over resident bases: clearing the scalars and the terms");
  const int rc = H.run([&]() -> int {
    Slot& S = H.slot();
    const size_t n = sh.total;
    int r;
    if ((r = note_terms(S, W, sh.terms()))) return r;
    if ((r = ensure(S.tmp, 4 * n))) return r;  // the rows on the device
    const void* d_scalars = scalars;
    if (!resident) {
      if ((r = stage_scalars(S, W, scalars, n, 1, 0, H.stream()))) return r;
      d_scalars = S.scalars.p;
    }
    unsigned levels = 0;
    // this family's part: the row list (public, not wiped) through the pinned bytes behind the table, and the walk
    if ((r = seg_walk_sum_fetch(H, sh, 4 * n, out_jac, &levels, [&](uint32_t* d_status, uint8_t* h_extra, hipStream_t st) -> int {
          uint32_t* h_rows = reinterpret_cast<uint32_t*>(h_extra);
          for (size_t p = 0; p < n; p++) h_rows[p] = rows ? rows[sh.lo + p] : (uint32_t)(sh.lo + p);
          HIP_TRY(hipMemcpyAsync(S.tmp.p, h_rows, 4 * n, hipMemcpyHostToDevice, st));
          HIP_TRY(launch_msm_ct_walk_rows(held.desc, static_cast<const uint32_t*>(S.tmp.p), d_scalars, c, bits, (uint32_t)n,
                                          S.partials.p, d_status, st));
          return CURDLE_OK;
        })))
      return r;
    g_stat[1].fetch_add(1, std::memory_order_relaxed);
    g_stat[2].fetch_add(sh.terms(), std::memory_order_relaxed);
    g_stat[3].fetch_add(sh.nonempty, std::memory_order_relaxed);
    if (batch) count_msm_ct_batch(sh.k, levels);
    return CURDLE_OK;
  });
  return rc;
}

int single(const curdle_ct_bases* b, const uint32_t* rows, const void* scalars, bool resident, size_t n, unsigned bits,
           uint64_t out_jac[18], void* stream) {
  if (!b || !out_jac || (n && !scalars)) return fail(CURDLE_EINVAL, "null argument");
  const size_t offsets[2] = {0, n};
  SegShape sh;
  if (int rc = shape_of(b->n, b->c, rows, offsets, 1, bits, &sh)) return rc;
  if (n == 0) {
    set_out_infinity(out_jac);
    return CURDLE_OK;
  }
  if (resident && !aligned16(scalars)) return fail(CURDLE_EINVAL, "device pointers must be multiples of 16");
  return rows_call(&b, 1, rows, scalars, resident, sh, bits, false, out_jac, stream);
}

// The batch behind the null checks of its handles, over n_sets of them at one chunk width: what the single-handle batch
// and the batch over several sets share from the shape on.  A call with pairs needs `rows` when it has several sets.
int batch_over(const curdle_ct_bases* const* sets, size_t n_sets, const uint32_t* rows, const void* scalars, bool resident,
               const size_t* offsets, size_t k, unsigned bits, uint64_t* out_jac, void* stream) {
  size_t n = 0;
  for (size_t s = 0; s < n_sets; s++) n += sets[s]->n;
  SegShape sh;
  if (int rc = shape_of(n, sets[0]->c, rows, offsets, k, bits, &sh)) return rc;
  if (k == 0) return CURDLE_OK;
  if (resident && !aligned16(scalars)) return fail(CURDLE_EINVAL, "device pointers must be multiples of 16");
  if (sh.total == 0) {
    for (size_t j = 0; j < k; j++) set_out_infinity(out_jac + 18 * j);
    return CURDLE_OK;
  }
  // the call's first pair (32 bytes a record keep the alignment)
  return rows_call(sets, n_sets, rows, static_cast<const uint8_t*>(scalars) + 32 * sh.lo, resident, sh, bits, true, out_jac, stream);
}

int batch(const curdle_ct_bases* b, const uint32_t* rows, const void* scalars, bool resident, const size_t* offsets, size_t k,
          unsigned bits, uint64_t* out_jac, void* stream) {
  if (!b || !offsets || (k && (!out_jac || !scalars))) return fail(CURDLE_EINVAL, "null argument");
  return batch_over(&b, 1, rows, scalars, resident, offsets, k, bits, out_jac, stream);
}

// curdle_msm_g1_ct_bases_sets_batch / _device: the null arguments (a null set is looked for among the first four only:
// nothing beyond CURDLE_CT_BASES_MAX_SETS is read), the set count, one chunk width, then the single-handle batch's order.
// rows: needed as soon as a pair would be read, i.e. when the offsets span any.
int sets_batch(const curdle_ct_bases* const* sets, size_t n_sets, const uint32_t* rows, const void* scalars, bool resident,
               const size_t* offsets, size_t k, unsigned bits, uint64_t* out_jac, void* stream) {
  if (!sets || !offsets || (k && (!out_jac || !scalars))) return fail(CURDLE_EINVAL, "null argument");
  for (size_t s = 0; s < std::min<size_t>(n_sets, CURDLE_CT_BASES_MAX_SETS); s++)
    if (!sets[s]) return fail(CURDLE_EINVAL, "null argument: sets[%zu]", s);
  if (k && k <= kMsmCtMaxBatch && !rows && offsets[k] > offsets[0]) return fail(CURDLE_EINVAL, "null argument: rows, and the call has pairs");
  if (n_sets < 1 || n_sets > CURDLE_CT_BASES_MAX_SETS)
    return fail(CURDLE_EINVAL, "n_sets = %zu is not in 1...%d", n_sets, CURDLE_CT_BASES_MAX_SETS);
  for (size_t s = 1; s < n_sets; s++)
    if (sets[s]->c != sets[0]->c)
      return fail(CURDLE_EINVAL, "the sets' chunk_bits differ: sets[%zu] has %u, sets[0] has %u", s, sets[s]->c, sets[0]->c);
  return batch_over(sets, n_sets, rows, scalars, resident, offsets, k, bits, out_jac, stream);
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

extern "C" int curdle_msm_g1_ct_bases_sets_batch(const curdle_ct_bases* const* sets, size_t n_sets, const uint32_t* rows,
                                                 const uint64_t* scalars, const size_t* offsets, size_t k, unsigned scalar_bits,
                                                 uint64_t* out_jac) {
  return sets_batch(sets, n_sets, rows, scalars, false, offsets, k, scalar_bits, out_jac, nullptr);
}

extern "C" int curdle_msm_g1_ct_bases_sets_batch_device(const curdle_ct_bases* const* sets, size_t n_sets, const uint32_t* rows,
                                                        const void* d_scalars, const size_t* offsets, size_t k,
                                                        unsigned scalar_bits, uint64_t* out_jac, void* stream) {
  return sets_batch(sets, n_sets, rows, d_scalars, true, offsets, k, scalar_bits, out_jac, stream);
}

extern "C" int curdle_stat_msm_ct_bases(unsigned long long out[4]) { return read_stats(out, g_stat, 4); }
