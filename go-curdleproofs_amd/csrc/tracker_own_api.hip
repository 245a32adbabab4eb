// C ABI of the ownership search over Whisk trackers (tracker_own_kernels.hip): curdle_whisk_find_own_trackers /
// _device, owned[j * n + i] = does key j own tracker i, for m keys and n trackers in one call.  (The single form,
// curdle_whisk_is_own_tracker, is host code: host/proto_api.cpp.)
//
// The call takes ONE MSM slot for its buffers and its stream, held by a SlotHold (api_helpers.h); no stream is
// made here and nothing is allocated once the slot's buffers have grown.  Per pass of at most kOwnPass trackers:
//   1. the pass's 2 x 48-byte records ARE the decoder's input: they go up as they are (or are read where the caller
//      keeps them: _device) and are decoded ONCE, subgroup test included (launch_g1_decompress), for all keys;
//   2. k_tracker_own runs over the (key, tracker) grid in launches of at most TRACKER_OWN_PAIRS quads, back to back
//      on the one stream (own_launches below is the rule);
//   3. the verdict bytes of the pass come back once (host form), with the 2 x status bytes that count the bad pairs.
// The keys are secrets: the library's copies of them are on the call's WipeList (api_helpers.h) and are overwritten on
// every way out; the kernel keeps the keys and their split halves in registers only.
//
// The _ex forms take a flags word.  flags = 0 IS the path above (the entry points without flags pass 0).  Under
// CURDLE_TRACKER_OWN_CONSTANT_TIME everything above stays -- limits, refusals, the one decode per pass, the slot hold,
// the staging, the WipeList -- and step 2 alone changes: k_tracker_own_ct (tracker_own_ct_kernels.hip), one lane per
// pair, under the second launch rule (own_rule_ct below), counted by curdle_stat_tracker_own_ct and nowhere else.
#include "api_helpers.h"

#include <algorithm>

namespace {
constexpr size_t kOwnMaxTrackers = (size_t)1 << 20;
constexpr size_t kOwnMaxKeys = 65535;
constexpr size_t kOwnMaxPairs = (size_t)1 << 24;
constexpr size_t kOwnPass = (size_t)1 << 17;  // trackers per pass: 262,144 records, 25 MB of decoded points
constexpr size_t kOwnWave = 16;               // quads of a wave
// Quads per launch where the knob says nothing.  A full launch of 2^18 quads was measured at 12.3 ms (DESIGN.md
// section 0, profiles/r16_tracker_own.json), so no single launch holds a shared GPU for long.
constexpr size_t kOwnPairsDefault = (size_t)1 << 18;

constexpr unsigned kKnownFlags = CURDLE_TRACKER_OWN_CONSTANT_TIME;
constexpr size_t kOwnCtBlock = 256;  // lanes of a block of k_tracker_own_ct: one pair each

// pairs answered on the device | launches | those of the pairs answered BAD; completed passes only.  [0]: k_tracker_own,
// [1]: k_tracker_own_ct -- a pass moves one of them, never both
std::atomic<unsigned long long> g_own_stat[2][3];

size_t pairs_per_launch() {
  const long long knob = knobs::get(knobs::TRACKER_OWN_PAIRS);
  const size_t v = knob < 0 ? kOwnPairsDefault : (size_t)knob;
  return std::max(kOwnWave, v / kOwnWave * kOwnWave);  // whole waves, at least one
}

// The launch rule of one pass of `cnt` trackers and m keys, with at most `pairs` quads a launch.  Every key's trackers
// are padded to whole waves: w = 16 ceil(cnt / 16) quads.  The tracker dimension is cut into chunks of tc = min(w,
// pairs) quads, and a launch takes one chunk of min(65,535, pairs / tc) keys (at least one).
struct OwnRule {
  size_t tc, keys;
};
OwnRule own_rule(size_t cnt, size_t pairs) {
  const size_t w = (cnt + kOwnWave - 1) / kOwnWave * kOwnWave;
  OwnRule r;
  r.tc = std::min(w, pairs);
  r.keys = std::min<size_t>(kOwnMaxKeys, std::max<size_t>(1, pairs / r.tc));
  return r;
}

// The second rule, of k_tracker_own_ct: one LANE per pair and nothing padded.  P = max(256, knob / 256 * 256) pairs a
// launch, 2^18 where the knob says nothing: 18.4 ms of k_g1_mul_ct's walk, under the
// 0.1 s the default was chosen against.  tc = min(cnt, P) trackers and max(1, P / tc) keys a launch.
OwnRule own_rule_ct(size_t cnt) {
  const long long knob = knobs::get(knobs::TRACKER_OWN_PAIRS);
  const size_t v = knob < 0 ? kOwnPairsDefault : (size_t)knob;
  const size_t pairs = std::max(kOwnCtBlock, v / kOwnCtBlock * kOwnCtBlock);
  OwnRule r;
  r.tc = std::min(cnt, pairs);
  r.keys = std::max<size_t>(1, pairs / r.tc);
  return r;
}

// The launches of one pass over decoded records; *launches: how many.
int own_launches(const void* d_points, const uint8_t* d_status, const void* d_keys, size_t cnt, size_t m, uint8_t* d_out,
                 size_t stride, hipStream_t st, bool ct, unsigned long long* launches) {
  const OwnRule rule = ct ? own_rule_ct(cnt) : own_rule(cnt, pairs_per_launch());
  *launches = 0;
  for (size_t t0 = 0; t0 < cnt; t0 += rule.tc)
    for (size_t k0 = 0; k0 < m; k0 += rule.keys) {
      const uint32_t tc = (uint32_t)std::min(rule.tc, cnt - t0), kc = (uint32_t)std::min(rule.keys, m - k0);
      if (ct)
        HIP_TRY(launch_tracker_own_ct(d_points, d_status, d_keys, (uint32_t)t0, tc, (uint32_t)k0, kc, d_out, stride, st));
      else
        HIP_TRY(launch_tracker_own(d_points, d_status, d_keys, (uint32_t)t0, tc, (uint32_t)k0, kc, d_out, stride, st));
      ++*launches;
    }
  return CURDLE_OK;
}

// trackers / ks: host memory (resident false) or device memory; owned likewise.  W: the library's copies of the keys
// (the caller's own d_ks is never one of them).
int own_run(Slot& S, hipStream_t st, WipeList& W, const uint8_t* trackers, size_t n, const uint64_t* ks, size_t m,
            bool resident, bool ct, uint8_t* owned) {
  const size_t cap = std::min(n, kOwnPass);
  int r;
  if ((r = ensure(S.points, 192 * cap))) return r;  // decoded records
  if ((r = ensure(S.counts, 2 * cap))) return r;    // their statuses
  if ((r = ensure_pinned(S, 1, 2 * cap + (resident ? 0 : m * cap)))) return r;  // statuses | verdicts
  uint8_t* h_status = static_cast<uint8_t*>(S.h_stage[1]);
  uint8_t* h_owned = h_status + 2 * cap;
  uint8_t* d_status = static_cast<uint8_t*>(S.counts.p);
  const void* d_keys = ks;
  uint8_t* h_trk = nullptr;
  if (!resident) {
    if ((r = ensure(S.scalars, 96 * cap))) return r;  // compressed records
    if ((r = ensure(S.digits, 32 * m))) return r;     // keys
    if ((r = ensure(S.sorted, m * cap))) return r;    // verdicts of a pass, one row of the pass's trackers per key
    const size_t keys_at = (96 * cap + 255) / 256 * 256;  // trackers | keys
    if ((r = ensure_pinned(S, 0, keys_at + 32 * m))) return r;
    h_trk = static_cast<uint8_t*>(S.h_stage[0]);
    uint8_t* h_keys = h_trk + keys_at;
    W.note_host(h_keys, 32 * m);
    memcpy(h_keys, ks, 32 * m);
    W.note_device(S.digits.p, 32 * m);
    HIP_TRY(hipMemcpyAsync(S.digits.p, h_keys, 32 * m, hipMemcpyHostToDevice, st));
    d_keys = S.digits.p;
  }
  for (size_t lo = 0; lo < n; lo += kOwnPass) {
    const size_t cnt = std::min(kOwnPass, n - lo);
    const uint8_t* d_rec = trackers + 96 * lo;
    if (!resident) {
      memcpy(h_trk, trackers + 96 * lo, 96 * cnt);
      HIP_TRY(hipMemcpyAsync(S.scalars.p, h_trk, 96 * cnt, hipMemcpyHostToDevice, st));
      d_rec = static_cast<const uint8_t*>(S.scalars.p);
    }
    HIP_TRY(launch_g1_decompress(d_rec, (uint32_t)(2 * cnt), 1, (uint32_t*)S.points.p, d_status, st));
    unsigned long long launches = 0;
    if (resident) {
      if ((r = own_launches(S.points.p, d_status, d_keys, cnt, m, owned + lo, n, st, ct, &launches))) return r;
    } else {
      if ((r = own_launches(S.points.p, d_status, d_keys, cnt, m, static_cast<uint8_t*>(S.sorted.p), cnt, st, ct, &launches))) return r;
      HIP_TRY(hipMemcpyAsync(h_owned, S.sorted.p, m * cnt, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipMemcpyAsync(h_status, d_status, 2 * cnt, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (!resident)
      for (size_t j = 0; j < m; j++) memcpy(owned + j * n + lo, h_owned + j * cnt, cnt);
    unsigned long long bad = 0;
    for (size_t i = 0; i < cnt; i++)
      bad += h_status[2 * i] > CURDLE_DECODE_INFINITY || h_status[2 * i + 1] > CURDLE_DECODE_INFINITY;
    std::atomic<unsigned long long>* stat = g_own_stat[ct ? 1 : 0];
    stat[0].fetch_add(cnt * m, std::memory_order_relaxed);  // the pass is complete: its three counters move together
    stat[1].fetch_add(launches, std::memory_order_relaxed);
    stat[2].fetch_add(bad * m, std::memory_order_relaxed);
  }
  return CURDLE_OK;
}

int own_through_slot(const uint8_t* trackers, size_t n, const uint64_t* ks, size_t m, bool resident, bool ct,
                     uint8_t* owned, void* user_stream) {
  SlotHold H(cur(), true, user_stream);
  WipeList W(H.stream());
  H.wipe_on_exit(&W, "own trackers: clearing the keys");  // nothing of the keys stays, however the call ends
  return H.run([&]() -> int { return own_run(H.slot(), H.stream(), W, trackers, n, ks, m, resident, ct, owned); });
}

int check_counts(size_t n, size_t m) {
  if (n > kOwnMaxTrackers) return fail(CURDLE_EINVAL, "n = %zu exceeds the supported 2^20 trackers", n);
  if (m > kOwnMaxKeys) return fail(CURDLE_EINVAL, "m = %zu exceeds the supported 65,535 keys", m);
  if (m * n > kOwnMaxPairs) return fail(CURDLE_EINVAL, "m * n = %zu exceeds the supported 2^24 pairs", m * n);
  return CURDLE_OK;
}

int check_flags(unsigned flags) {
  if (flags & ~kKnownFlags) return fail(CURDLE_EINVAL, "unknown flag bits 0x%x", flags & ~kKnownFlags);
  return CURDLE_OK;
}
}  // namespace

extern "C" int curdle_whisk_find_own_trackers_ex(const uint8_t* trackers, size_t n, const uint64_t* ks, size_t m,
                                                 uint8_t* owned, unsigned flags) {
  int rc = check_flags(flags);  // before anything else is looked at
  if (rc == CURDLE_OK) {
    if (n == 0 || m == 0) return CURDLE_OK;
    if (!trackers || !ks || !owned)
      rc = fail(CURDLE_EINVAL, "null argument");
    else if ((rc = check_counts(n, m)) == CURDLE_OK)
      rc = own_through_slot(trackers, n, ks, m, false, (flags & CURDLE_TRACKER_OWN_CONSTANT_TIME) != 0, owned, nullptr);
  }
  size_t bytes;
  if (rc != CURDLE_OK && owned && !__builtin_mul_overflow(m, n, &bytes))  // "could not compute" never reads as a verdict
    memset(owned, CURDLE_TRACKER_UNKNOWN, bytes);
  return rc;
}

extern "C" int curdle_whisk_find_own_trackers_device_ex(const void* d_trackers, size_t n, const void* d_ks, size_t m,
                                                        void* d_owned, void* stream, unsigned flags) {
  if (int rc = check_flags(flags)) return rc;
  if (n == 0 || m == 0) return CURDLE_OK;
  if (!d_trackers || !d_ks || !d_owned) return fail(CURDLE_EINVAL, "null argument");
  if (int rc = check_counts(n, m)) return rc;
  if (!aligned16(d_trackers) || !aligned16(d_ks)) return fail(CURDLE_EINVAL, "d_trackers and d_ks must be multiples of 16");
  return own_through_slot(static_cast<const uint8_t*>(d_trackers), n, static_cast<const uint64_t*>(d_ks), m, true,
                          (flags & CURDLE_TRACKER_OWN_CONSTANT_TIME) != 0, static_cast<uint8_t*>(d_owned), stream);
}

extern "C" int curdle_whisk_find_own_trackers(const uint8_t* trackers, size_t n, const uint64_t* ks, size_t m,
                                              uint8_t* owned) {
  return curdle_whisk_find_own_trackers_ex(trackers, n, ks, m, owned, 0);
}

extern "C" int curdle_whisk_find_own_trackers_device(const void* d_trackers, size_t n, const void* d_ks, size_t m,
                                                     void* d_owned, void* stream) {
  return curdle_whisk_find_own_trackers_device_ex(d_trackers, n, d_ks, m, d_owned, stream, 0);
}

extern "C" int curdle_stat_tracker_own(unsigned long long out[3]) { return read_stats(out, g_own_stat[0], 3); }
extern "C" int curdle_stat_tracker_own_ct(unsigned long long out[3]) { return read_stats(out, g_own_stat[1], 3); }
