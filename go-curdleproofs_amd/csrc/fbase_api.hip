// C ABI of the fixed-base scalar multiplication (fbase_kernels.hip): curdle_fbase, the handle of one point's table of
// 8,160 multiples on the device; curdle_g1_fixed_base_mul_batch / _device, out[i] = (scalars[i] * multipliers[i]) * P
// as affine records or compressed bytes; and curdle_whisk_compute_trackers_batch, computeTracker and getKComm
// (whisk/whisk_test.go:98-109) for n validators in one call -- one launch of k_fbase_mul over 3 m scalars per pass.
//
// A call takes ONE MSM slot for its buffers and its stream, held by a SlotHold (api_helpers.h); no stream is
// made here and nothing is allocated once the slot's buffers have grown.  Per pass of at most FBASE_PASS scalars:
//   1. the scalars (and multipliers) go up through the slot's pinned staging, or are read where the caller keeps them;
//   2. k_fbase_mul writes G1XYZZ results into the slot's workspace;
//   3. k_g1_normalize makes affine records of them with ONE inversion per wave, straight into the caller's array
//      (resident, affine) or into the slot's;
//   4. compressed output: k_g1_compress<kCompressAffine> encodes the records -- nothing is inverted per point.
// A table belongs to a handle and has one copy per context, made on first use there: a ResidentCopy (api_helpers.h),
// as a resident base set's is; the generator's handle is the library's own and is never freed.
//
// THE KERNEL READS TABLE ENTRIES AT ADDRESSES CHOSEN BY SCALAR DIGITS and skips zero digits: memory access pattern and
// running time depend on the scalars.  What the library itself holds of them is overwritten on every way out: the call's
// WipeList (api_helpers.h).
//
// The _ex entry points take flags.  CURDLE_FBASE_CONSTANT_TIME puts k_fbase_mul_ct (fbase_ct_kernels.hip) in k_fbase_mul's
// place inside fb_launches and nothing else: same table, same passes, same slot hold and wipes, counters of its own
// (curdle_stat_fbase_ct).  The entry points without flags call the _ex ones with 0.
#include "api_helpers.h"
#include "../host/host_ops.h"

#include <algorithm>

struct curdle_fbase {
  std::vector<uint64_t> host;  // the 8,160 gnark affine multiples: a context that has not used the table yet converts its own copy
  ResidentCopy copy;           // per context: kFbaseEntries records of d28::A28, kA28Bytes apart
};

namespace {
constexpr size_t kFbMax = (size_t)1 << 24;
constexpr size_t kFbMaxMembers = (size_t)1 << 22;
constexpr size_t kFbPassDefault = (size_t)1 << 20;

// scalars multiplied on the device | launches of k_fbase_mul | tables built; completed passes only
std::atomic<unsigned long long> g_fb_stat[3];
// scalars multiplied by k_fbase_mul_ct | its launches; completed passes only
std::atomic<unsigned long long> g_fb_ct_stat[2];
constexpr unsigned kFbKnownFlags = CURDLE_FBASE_CONSTANT_TIME;

size_t pass_size() {
  const long long knob = knobs::get(knobs::FBASE_PASS);
  const size_t v = knob < 0 ? kFbPassDefault : (size_t)knob;
  return std::max<size_t>(256, v / 256 * 256);
}

// The table's copy on context cx, uploaded and converted on first use (and again after a shutdown); takes a user
// reference that fbase_release gives back.
int fbase_acquire(Ctx& cx, curdle_fbase* b, void** d28) {
  static const ResidentCopy::Text text = {"the fixed-base table was freed", "the context was shut down under a fixed-base table upload",
                                          "fixed-base table"};
  return b->copy.acquire(cx, [b](hipStream_t st, void** dst) {
    const size_t n = kFbaseEntries;
    void *raw = nullptr, *both = nullptr;
    hipError_t e = hipMalloc(dst, n * kA28Bytes);
    if (e == hipSuccess) e = hipMalloc(&raw, n * 96);
    if (e == hipSuccess) e = hipMalloc(&both, 2 * n * kA28Bytes);  // P and phi(P) per entry (launch_convert_points_raw)
    if (e == hipSuccess) e = hipMemcpyAsync(raw, b->host.data(), n * 96, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = launch_convert_points_raw(raw, (uint32_t)n, both, st);
    // the kernel gathers P's records only: kept dense, one 128-byte line each, so the table is half the L2 footprint
    if (e == hipSuccess) e = hipMemcpy2DAsync(*dst, kA28Bytes, both, 2 * kA28Bytes, kA28Bytes, n, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (raw) (void)hipFree(raw);
    if (both) (void)hipFree(both);
    if (e == hipSuccess) g_fb_stat[2].fetch_add(1, std::memory_order_relaxed);
    return e;
  }, text, d28);
}

void fbase_release(curdle_fbase* b) {
  if (b->copy.release()) delete b;
}

curdle_fbase* fbase_new(const G1Affine& p) {
  curdle_fbase* b = new (std::nothrow) curdle_fbase();
  if (!b) return nullptr;
  try {
    b->host.resize(12 * (size_t)kFbaseEntries);
  } catch (const std::bad_alloc&) {
    delete b;
    return nullptr;
  }
  curdle_host_fixed_base_table(b->host.data(), &p);
  return b;
}

// The generator's handle: made once per process (the initialisation of a local static is the race's referee), its
// device copies once per context like any other handle's (under the handle's mutex).  Never freed.
curdle_fbase* generator_base() {
  static curdle_fbase* g = [] {
    G1Affine gen;
    g1_generator(gen);
    return fbase_new(gen);
  }();
  return g;
}

// One gnark G1Affine on the host: infinity, a coordinate >= p, y^2 = x^3 + 4, the subgroup.  Null: the point is good.
const char* check_affine_host(const G1Affine& a) {
  if (g1_affine_is_inf(a)) return "the point is infinity";
  for (const Fp* c : {&a.x, &a.y}) {
    int ge = 1;
    for (int i = 0; i < 12; i++) ge = c->l[i] > FpParams::mod(i) ? 1 : (c->l[i] < FpParams::mod(i) ? 0 : ge);
    if (ge) return "a coordinate is not below p";
  }
  Fp lhs, rhs, four;
  fp_sqr(lhs, a.y);
  fp_sqr(rhs, a.x);
  fp_mul(rhs, rhs, a.x);
  f_one(four);
  fp_dbl(four, four);
  fp_dbl(four, four);
  fp_add(rhs, rhs, four);
  if (!f_eq(lhs, rhs)) return "the point is not on the curve";
  G1XYZZ p;
  g1_from_affine(p, a);
  if (!g1_in_subgroup(p)) return "the point is not in the prime-order subgroup";
  return nullptr;
}

// The slot and the stream of a call, and what it holds of the secrets: the library's device copy of scalars and
// multipliers, the pinned staging they went through and the unnormalised results (S.sorted).  The caller's arrays are
// never wiped; the kernel keeps the scalar and its digits in registers only.
struct FbCall {
  SlotHold& H;
  WipeList W;
  bool ct;  // CURDLE_FBASE_CONSTANT_TIME: which launcher fb_launches takes and which counters a pass moves
  Slot& slot() { return H.slot(); }
  hipStream_t stream() { return H.stream(); }
};

// The launches of one pass over resident scalars: cnt products -> XYZZ (S.sorted) -> affine records at d_affine (16-byte
// aligned) -> if d_comp, their encodings there (any alignment).
int fb_launches(FbCall& C, const void* d_table, const void* d_scalars, const void* d_mults, size_t cnt, void* d_affine,
                uint8_t* d_comp) {
  HIP_TRY((C.ct ? launch_fbase_mul_ct : launch_fbase_mul)(d_table, d_scalars, d_mults, (uint32_t)cnt, C.slot().sorted.p, C.stream()));
  HIP_TRY(launch_g1_normalize(C.slot().sorted.p, kNormalizeXyzz, (uint32_t)cnt, d_affine, C.stream(), nullptr));
  if (d_comp) HIP_TRY(launch_g1_compress(d_affine, kCompressAffine, (uint32_t)cnt, d_comp, C.stream()));
  return CURDLE_OK;
}

void count_pass(const FbCall& C, size_t cnt) {
  std::atomic<unsigned long long>* stat = C.ct ? g_fb_ct_stat : g_fb_stat;
  stat[0].fetch_add(cnt, std::memory_order_relaxed);
  stat[1].fetch_add(1, std::memory_order_relaxed);
}

// scalars / multipliers / out: host memory (resident false) or device memory.
int fb_run(FbCall& C, const void* d_table, const uint8_t* scalars, const uint8_t* mults, size_t n, bool resident, int out_form,
           uint8_t* out) {
  Slot& S = C.slot();
  const size_t pass = pass_size(), cap = std::min(n, pass);
  const bool comp = out_form == CURDLE_G1_OUT_COMPRESSED;
  const size_t rec = comp ? 48 : 96;
  int r;
  if ((r = ensure(S.sorted, cap * sizeof(G1XYZZ)))) return r;
  C.W.note_device(S.sorted.p, cap * sizeof(G1XYZZ));
  if (comp || !resident)
    if ((r = ensure(S.points, cap * 96))) return r;  // affine records
  if (!resident) {
    if (comp && (r = ensure(S.digits, cap * 48))) return r;    // encodings
    if ((r = ensure(S.scalars, cap * 64))) return r;           // scalars | multipliers
    if ((r = ensure_pinned(S, 0, cap * 64))) return r;
    if ((r = ensure_pinned(S, 1, cap * rec))) return r;
    C.W.note_device(S.scalars.p, cap * 64);
    C.W.note_host(S.h_stage[0], cap * 64);
  }
  for (size_t lo = 0; lo < n; lo += pass) {
    const size_t cnt = std::min(pass, n - lo);
    if (resident) {
      const void* dm = mults ? mults + 32 * lo : nullptr;
      if (comp)
        r = fb_launches(C, d_table, scalars + 32 * lo, dm, cnt, S.points.p, out + 48 * lo);
      else
        r = fb_launches(C, d_table, scalars + 32 * lo, dm, cnt, out + 96 * lo, nullptr);
      if (r) return r;
    } else {
      uint8_t* h = static_cast<uint8_t*>(S.h_stage[0]);
      uint8_t* d = static_cast<uint8_t*>(S.scalars.p);
      memcpy(h, scalars + 32 * lo, 32 * cnt);
      if (mults) memcpy(h + 32 * cnt, mults + 32 * lo, 32 * cnt);
      HIP_TRY(hipMemcpyAsync(d, h, (mults ? 64 : 32) * cnt, hipMemcpyHostToDevice, C.stream()));
      if ((r = fb_launches(C, d_table, d, mults ? d + 32 * cnt : nullptr, cnt, S.points.p,
                           comp ? static_cast<uint8_t*>(S.digits.p) : nullptr)))
        return r;
      HIP_TRY(hipMemcpyAsync(S.h_stage[1], comp ? S.digits.p : S.points.p, rec * cnt, hipMemcpyDeviceToHost, C.stream()));
    }
    HIP_TRY(hipStreamSynchronize(C.stream()));
    if (!resident) memcpy(out + rec * lo, S.h_stage[1], rec * cnt);
    count_pass(C, cnt);
  }
  return CURDLE_OK;
}

// One call through the table's copy on the calling thread's context and an MSM slot: run(C, d_table) does the passes.
template <class Run>
int fb_through_slot(const curdle_fbase* base, void* user_stream, unsigned flags, Run run) {
  Ctx& cx = cur();
  curdle_fbase* b = base ? const_cast<curdle_fbase*>(base) : generator_base();
  if (!b) return fail(CURDLE_ENOMEM, "out of memory");
  void* d_table = nullptr;
  int rc = fbase_acquire(cx, b, &d_table);
  if (rc) return rc;
  SlotHold H(cx, true, user_stream);
  FbCall C{H, WipeList(H.stream()), (flags & CURDLE_FBASE_CONSTANT_TIME) != 0};
  H.wipe_on_exit(&C.W, "fixed-base multiplication: clearing the scalars");  // nothing of the scalars stays
  rc = H.run([&]() -> int { return run(C, d_table); });
  fbase_release(b);
  return rc;
}

int check_flags(unsigned flags) {
  if (flags & ~kFbKnownFlags) return fail(CURDLE_EINVAL, "unknown flag bits 0x%x", flags & ~kFbKnownFlags);
  return CURDLE_OK;
}

int check_args(const void* scalars, size_t n, int out_form, const void* out) {
  if (!scalars || !out) return fail(CURDLE_EINVAL, "null argument");
  if (out_form != CURDLE_G1_OUT_AFFINE && out_form != CURDLE_G1_OUT_COMPRESSED)
    return fail(CURDLE_EINVAL, "unknown output form %d", out_form);
  if (n > kFbMax) return fail(CURDLE_EINVAL, "n = %zu exceeds the supported 2^24 scalars", n);
  return CURDLE_OK;
}

// The tracker batch: members [lo, lo + m) per pass with 3 m (2 m without commitments) scalars <= FBASE_PASS.  The pinned
// block of a pass is ones | r | k (| ones), 32 m bytes each; on the device the scalars start at its second part and the
// multipliers at its first, so the lanes see (r, 1), (k, r) and (1, k): r G, k r G and k G in ONE launch, no copy between.
int trackers_run(FbCall& C, const void* d_table, const uint64_t* ks, const uint64_t* rs, size_t n, uint8_t* trackers_out,
                 uint8_t* kcomm_out) {
  Slot& S = C.slot();
  const size_t cols = kcomm_out ? 3 : 2;
  const size_t mp = std::max<size_t>(1, pass_size() / cols), cap = std::min(n, mp);
  int r;
  if ((r = ensure(S.sorted, cols * cap * sizeof(G1XYZZ)))) return r;
  C.W.note_device(S.sorted.p, cols * cap * sizeof(G1XYZZ));
  if ((r = ensure(S.points, cols * cap * 96))) return r;     // affine records, column by column
  if ((r = ensure(S.digits, cols * cap * 48))) return r;     // their encodings
  if ((r = ensure(S.counts, 96 * cap))) return r;            // the trackers: r G | k r G member by member
  if ((r = ensure(S.scalars, (cols + 1) * cap * 32))) return r;
  if ((r = ensure_pinned(S, 0, (cols + 1) * cap * 32))) return r;
  if ((r = ensure_pinned(S, 1, cols * cap * 48))) return r;
  C.W.note_device(S.scalars.p, (cols + 1) * cap * 32);
  C.W.note_host(S.h_stage[0], (cols + 1) * cap * 32);
  Fr one;
  f_one(one);
  for (size_t lo = 0; lo < n; lo += mp) {
    const size_t m = std::min(mp, n - lo);
    uint8_t* h = static_cast<uint8_t*>(S.h_stage[0]);
    uint8_t* d = static_cast<uint8_t*>(S.scalars.p);
    for (size_t i = 0; i < m; i++) memcpy(h + 32 * i, &one, 32);
    if (rs)
      memcpy(h + 32 * m, rs + 4 * lo, 32 * m);
    else
      memcpy(h + 32 * m, h, 32 * m);  // r = 1: the fork's initial trackers (G, k G)
    memcpy(h + 64 * m, ks + 4 * lo, 32 * m);
    if (kcomm_out) memcpy(h + 96 * m, h, 32 * m);
    HIP_TRY(hipMemcpyAsync(d, h, (cols + 1) * m * 32, hipMemcpyHostToDevice, C.stream()));
    uint8_t* comp = static_cast<uint8_t*>(S.digits.p);
    if ((r = fb_launches(C, d_table, d + 32 * m, d, cols * m, S.points.p, comp))) return r;
    // the two tracker columns member by member
    HIP_TRY(hipMemcpy2DAsync(S.counts.p, 96, comp, 48, 48, m, hipMemcpyDeviceToDevice, C.stream()));
    HIP_TRY(hipMemcpy2DAsync(static_cast<uint8_t*>(S.counts.p) + 48, 96, comp + 48 * m, 48, 48, m, hipMemcpyDeviceToDevice, C.stream()));
    uint8_t* ho = static_cast<uint8_t*>(S.h_stage[1]);
    HIP_TRY(hipMemcpyAsync(ho, S.counts.p, 96 * m, hipMemcpyDeviceToHost, C.stream()));
    if (kcomm_out) HIP_TRY(hipMemcpyAsync(ho + 96 * m, comp + 96 * m, 48 * m, hipMemcpyDeviceToHost, C.stream()));
    HIP_TRY(hipStreamSynchronize(C.stream()));
    memcpy(trackers_out + 96 * lo, ho, 96 * m);
    if (kcomm_out) memcpy(kcomm_out + 48 * lo, ho + 96 * m, 48 * m);
    count_pass(C, cols * m);
  }
  return CURDLE_OK;
}
}  // namespace

namespace curdle_api {
int generator_table_acquire(Ctx& cx, void** d_table) {
  curdle_fbase* b = generator_base();
  if (!b) return fail(CURDLE_ENOMEM, "out of memory");
  return fbase_acquire(cx, b, d_table);
}
void generator_table_release() { fbase_release(generator_base()); }
void count_fbase_ct_pass(size_t n) {
  g_fb_ct_stat[0].fetch_add(n, std::memory_order_relaxed);
  g_fb_ct_stat[1].fetch_add(1, std::memory_order_relaxed);
}
}  // namespace curdle_api

extern "C" int curdle_fbase_create(const uint64_t point_affine[12], curdle_fbase** out) {
  if (!out || !point_affine) return fail(CURDLE_EINVAL, "null argument");
  *out = nullptr;
  G1Affine p;
  memcpy(&p, point_affine, sizeof(p));
  if (const char* why = check_affine_host(p)) return fail(CURDLE_EINVAL, "fixed base: %s", why);
  curdle_fbase* b = fbase_new(p);
  if (!b) return fail(CURDLE_ENOMEM, "out of memory");
  // resident on the creating thread's context now (a failure here is the caller's to see); on every other context when
  // a call there first names the handle
  void* d = nullptr;
  int rc = fbase_acquire(cur(), b, &d);
  if (rc) {
    delete b;
    return rc;
  }
  fbase_release(b);
  *out = b;
  return CURDLE_OK;
}

extern "C" void curdle_fbase_free(curdle_fbase* b) {
  if (b && b->copy.free_or_defer()) delete b;
}

extern "C" int curdle_g1_fixed_base_mul_batch_ex(const curdle_fbase* base, const uint64_t* scalars, const uint64_t* multipliers,
                                                 size_t n, int out_form, unsigned flags, void* out) {
  if (int rc = check_flags(flags)) return rc;
  if (n == 0) return CURDLE_OK;
  if (int rc = check_args(scalars, n, out_form, out)) return rc;
  return fb_through_slot(base, nullptr, flags, [&](FbCall& C, const void* d_table) {
    return fb_run(C, d_table, reinterpret_cast<const uint8_t*>(scalars), reinterpret_cast<const uint8_t*>(multipliers), n, false,
                  out_form, static_cast<uint8_t*>(out));
  });
}

extern "C" int curdle_g1_fixed_base_mul_batch(const curdle_fbase* base, const uint64_t* scalars, const uint64_t* multipliers,
                                              size_t n, int out_form, void* out) {
  return curdle_g1_fixed_base_mul_batch_ex(base, scalars, multipliers, n, out_form, 0, out);
}

extern "C" int curdle_g1_fixed_base_mul_batch_device_ex(const curdle_fbase* base, const void* d_scalars, const void* d_multipliers,
                                                        size_t n, int out_form, unsigned flags, void* d_out, void* stream) {
  if (int rc = check_flags(flags)) return rc;
  if (n == 0) return CURDLE_OK;
  if (int rc = check_args(d_scalars, n, out_form, d_out)) return rc;
  if (!aligned16(d_scalars) || !aligned16(d_multipliers) || (out_form == CURDLE_G1_OUT_AFFINE && !aligned16(d_out)))
    return fail(CURDLE_EINVAL, "device pointers must be multiples of 16 (a compressed d_out may have any alignment)");
  return fb_through_slot(base, stream, flags, [&](FbCall& C, const void* d_table) {
    return fb_run(C, d_table, static_cast<const uint8_t*>(d_scalars), static_cast<const uint8_t*>(d_multipliers), n, true,
                  out_form, static_cast<uint8_t*>(d_out));
  });
}

extern "C" int curdle_g1_fixed_base_mul_batch_device(const curdle_fbase* base, const void* d_scalars, const void* d_multipliers,
                                                     size_t n, int out_form, void* d_out, void* stream) {
  return curdle_g1_fixed_base_mul_batch_device_ex(base, d_scalars, d_multipliers, n, out_form, 0, d_out, stream);
}

extern "C" int curdle_whisk_compute_trackers_batch_ex(const uint64_t* ks, const uint64_t* rs, size_t n, unsigned flags,
                                                      uint8_t* trackers_out, uint8_t* k_commitments_out) {
  if (int rc = check_flags(flags)) return rc;  // like a count beyond the limit: refused without touching the outputs
  if (n == 0) return CURDLE_OK;
  if (n > kFbMaxMembers) return fail(CURDLE_EINVAL, "n = %zu exceeds the supported 2^22 trackers", n);
  int rc;
  if (!ks || !trackers_out)
    rc = fail(CURDLE_EINVAL, "null argument");
  else
    rc = fb_through_slot(nullptr, nullptr, flags, [&](FbCall& C, const void* d_table) {
      return trackers_run(C, d_table, ks, rs, n, trackers_out, k_commitments_out);
    });
  if (rc != CURDLE_OK) {  // a failed call leaves nothing that reads as a tracker
    if (trackers_out) memset(trackers_out, 0, 96 * n);
    if (k_commitments_out) memset(k_commitments_out, 0, 48 * n);
  }
  return rc;
}

extern "C" int curdle_whisk_compute_trackers_batch(const uint64_t* ks, const uint64_t* rs, size_t n, uint8_t* trackers_out,
                                                   uint8_t* k_commitments_out) {
  return curdle_whisk_compute_trackers_batch_ex(ks, rs, n, 0, trackers_out, k_commitments_out);
}

extern "C" int curdle_stat_fbase(unsigned long long out[3]) { return read_stats(out, g_fb_stat, 3); }
extern "C" int curdle_stat_fbase_ct(unsigned long long out[2]) { return read_stats(out, g_fb_ct_stat, 2); }
