// C ABI of the batched Merlin transcripts on the device (include/curdle_msm.h, "Batched Merlin transcripts"): the
// call is checked and its program compiled into a tape on the host (host/transcript_batch.h, shared with the host
// twin curdle_transcript_batch_host in host/transcript.cpp), tape, start states and the members' rows go up in ONE
// copy, ONE kernel runs (transcript_kernels.hip), challenges, states and status bytes come back in ONE copy -- all on
// the context's transcript stream and buffers (TrCtx, msm_internal.h), never through an MSM slot or a decode context.
#include "api_helpers.h"
#include "../host/transcript.h"
#include "../host/transcript_batch.h"

namespace {
std::atomic<unsigned long long> g_tr_stat[2];  // members hashed on the device | handed back with a non-zero status

int ensure_host(void*& p, size_t& cap, size_t bytes) {
  if (cap >= bytes) return CURDLE_OK;
  if (p) HIP_TRY(hipHostFree(p));
  p = nullptr;
  cap = 0;
  HIP_TRY(hipHostMalloc(&p, grow_size(bytes), hipHostMallocDefault));
  cap = grow_size(bytes);
  return CURDLE_OK;
}

// Members per wave.  The call waits for a chain of dependent permutations, a wave's instructions cost the same with
// one lane active as with 64, and a wave repeats a challenge's try until ALL its members have an accepted draw (2.2
// tries for one member, ~7 for 64): few members per wave while the waves are few.  But the waves also share the
// tape and the rows' cache lines, and many of them slow each other down -- measured at ell = 124
// (profiles/r12_transcript_batch.json): 64 waves of one member 10.5 ms, 1,024 waves of one member 27.3 ms, 16 full
// waves 23.0 ms; 8,192 members as 2,048 waves of four 39.1 ms, as 128 full waves 21.1 ms.  So: at most 128 waves.
constexpr size_t kMaxWaves = 128;

uint32_t members_per_wave(size_t k) {
  const long long forced = knobs::get(knobs::TRANSCRIPT_LANES);
  if (forced >= 1 && forced <= 64) return (uint32_t)forced;
  uint32_t mpw = 1;
  while (mpw < 64 && (k + mpw - 1) / mpw > kMaxWaves) mpw *= 2;
  return mpw;
}

// Largest k for which an unset TRANSCRIPT_SHEET takes the sheet kernel (a state spread over lanes, two members per
// wave: transcript_sheet_kernels.hip).  The rule: the largest measured k at which the sheet kernel's wall time is
// below the lane kernel's by more than the larger of the two spreads of the repetitions; above it the lane kernel,
// whose 64 states per wave do far less work per member once the chip is full.  Measured on the prelude at ell = 124
// (profiles/r20_transcript_sheet.json, medians of 7, one lease; lane against sheet, wall ms, the larger spread in
// brackets): k = 1: 8.53 / 2.62 (1.83); 64: 10.84 / 3.43 (0.37); 256: 13.11 / 3.56 (0.60); 1,024: 19.45 / 5.31 (0.60);
// 4,096: 31.04 / 14.75 (0.78); 8,192: 37.82 / 27.67 (1.35) -- the kernels alone at 8,192: 21.0 / 11.4 ms.  The sheet
// kernel is ahead at every measured size, by less and less; 8,192 is the largest measured (65,536 members of that
// prelude exceed CURDLE_TRANSCRIPT_MAX_TOTAL), so nothing is claimed beyond it.  ell = 252 agrees: 78.97 / 58.85 (3.80)
// at 8,192.
constexpr size_t kSheetMaxMembers = 8192;
}  // namespace

// Which kernel hashes a batch of k members, and its geometry: the one rule for every caller of launch_transcript_batch
// (curdle_transcript_batch here, the tracker batches and the tracker prover in tracker_api.hip).  Knob
// TRANSCRIPT_SHEET decides when set; TRANSCRIPT_LANES alone is a statement about the lane kernel and selects it.
void curdle_api::choose_transcript_kernel(size_t k, TranscriptArgs* a) {
  const long long forced = knobs::get(knobs::TRANSCRIPT_SHEET);
  bool sheet;
  if (forced >= 0)
    sheet = forced != 0;
  else
    sheet = !knobs::is_set(knobs::TRANSCRIPT_LANES) && k <= kSheetMaxMembers;
  a->sheet = sheet ? 1 : 0;
  a->mpw = members_per_wave(k);
}

extern "C" int curdle_transcript_batch(const char* transcript_label, const uint8_t* init_states,
                                       const curdle_transcript_step* steps, size_t n_steps, const uint8_t* data,
                                       size_t data_stride, size_t k, uint8_t* challenges, uint8_t* states, uint8_t* status) {
  using namespace curdle::transcript;
  uint8_t start[3];
  std::string why;
  Tape tape;
  try {
    if (CheckBatchCall(transcript_label, init_states, steps, n_steps, data, data_stride, k, challenges, status, start, &why))
      return fail(CURDLE_EINVAL, "%s", why.c_str());
    if (k == 0) return CURDLE_OK;
    CompileTape(steps, n_steps, start, &tape);
  } catch (const std::bad_alloc&) {
    return fail(CURDLE_ENOMEM, "out of memory");
  }
  const size_t row_words = TapeRowWords(tape.consumed);
  if (k * row_words * 8 > CURDLE_TRANSCRIPT_MAX_TOTAL)
    return fail(CURDLE_EINVAL, "%zu members of %zu bytes exceed CURDLE_TRANSCRIPT_MAX_TOTAL", k, tape.consumed);
  const size_t n_ch = tape.n_challenges;
  // d_in: control list | block pool | start state(s) | rows;  d_out: challenges | states | status
  const size_t ctl_bytes = tape.ctl.size() * sizeof(TapeCtl), pool_bytes = tape.pool.size() * sizeof(TapeBlock);
  const size_t init_bytes = (init_states ? k : 1) * (size_t)CURDLE_TRANSCRIPT_STATE_SIZE, rows_bytes = k * row_words * 8;
  const size_t in_bytes = ctl_bytes + pool_bytes + init_bytes + rows_bytes;
  const size_t ch_bytes = k * n_ch * 32, st_bytes = states ? k * (size_t)CURDLE_TRANSCRIPT_STATE_SIZE : 0;
  const size_t out_bytes = ch_bytes + st_bytes + k;
  static_assert(sizeof(TapeCtl) % 8 == 0 && sizeof(TapeBlock) % 8 == 0 && CURDLE_TRANSCRIPT_STATE_SIZE % 8 == 0, "u64 alignment of d_in");

  Ctx& cx = cur();
  TrCtx& T = cx.tr;
  {
    std::unique_lock<std::mutex> g(cx.mu);
    int rc = init_default_locked(cx);
    if (rc) return rc;
    T.cv.wait(g, [&] { return !T.busy; });
    T.busy = true;
  }
  float kernel_ms = 0;
  auto body = [&]() -> int {
    HIP_TRY(hipSetDevice(cx.device));
    int r;
    if ((r = ensure_host(T.h_in, T.h_in_cap, in_bytes))) return r;
    if ((r = ensure_host(T.h_out, T.h_out_cap, out_bytes))) return r;
    if ((r = ensure(T.d_in, in_bytes))) return r;
    if ((r = ensure(T.d_out, out_bytes))) return r;
    uint8_t* h = static_cast<uint8_t*>(T.h_in);
    if (ctl_bytes) memcpy(h, tape.ctl.data(), ctl_bytes);
    if (pool_bytes) memcpy(h + ctl_bytes, tape.pool.data(), pool_bytes);
    uint8_t* h_init = h + ctl_bytes + pool_bytes;
    if (init_states)
      memcpy(h_init, init_states, init_bytes);
    else
      Transcript(std::string(transcript_label)).inner().Export(h_init);
    uint8_t* h_rows = h_init + init_bytes;
    for (size_t i = 0; i < k; i++) {  // 8 zero bytes | the member's bytes | zeros to the row's end (at least 8)
      uint8_t* row = h_rows + i * row_words * 8;
      memset(row, 0, 8);
      if (tape.consumed) memcpy(row + 8, data + i * data_stride, tape.consumed);
      memset(row + 8 + tape.consumed, 0, row_words * 8 - 8 - tape.consumed);
    }
    uint8_t* d_in = static_cast<uint8_t*>(T.d_in.p);
    uint8_t* d_out = static_cast<uint8_t*>(T.d_out.p);
    TranscriptArgs a;
    a.ctl = reinterpret_cast<const TapeCtl*>(d_in);
    a.pool = reinterpret_cast<const TapeBlock*>(d_in + ctl_bytes);
    a.init = reinterpret_cast<const uint64_t*>(d_in + ctl_bytes + pool_bytes);
    a.data = reinterpret_cast<const uint64_t*>(d_in + ctl_bytes + pool_bytes + init_bytes);
    a.challenges = reinterpret_cast<uint64_t*>(d_out);
    a.states = states ? reinterpret_cast<uint64_t*>(d_out + ch_bytes) : nullptr;
    a.status = d_out + ch_bytes + st_bytes;
    a.tail = (uint64_t)tape.pos | ((uint64_t)tape.pos_begin << 8) | ((uint64_t)tape.cur_flags << 16);
    a.n_ctl = (uint32_t)tape.ctl.size();
    a.row_words = (uint32_t)row_words;
    a.init_stride = init_states ? CURDLE_TRANSCRIPT_STATE_SIZE / 8 : 0;
    a.k = (uint32_t)k;
    choose_transcript_kernel(k, &a);
    a.n_challenges = (uint32_t)n_ch;
    HIP_TRY(hipMemcpyAsync(d_in, h, in_bytes, hipMemcpyHostToDevice, T.stream));
    HIP_TRY(hipEventRecord(T.ev[0], T.stream));
    HIP_TRY(launch_transcript_batch(a, T.stream));
    HIP_TRY(hipEventRecord(T.ev[1], T.stream));
    HIP_TRY(hipMemcpyAsync(T.h_out, d_out, out_bytes, hipMemcpyDeviceToHost, T.stream));
    HIP_TRY(hipStreamSynchronize(T.stream));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, T.ev[0], T.ev[1]));
    kernel_ms = ms;
    const uint8_t* ho = static_cast<const uint8_t*>(T.h_out);
    if (ch_bytes) memcpy(challenges, ho, ch_bytes);
    if (st_bytes) memcpy(states, ho + ch_bytes, st_bytes);
    memcpy(status, ho + ch_bytes + st_bytes, k);
    return CURDLE_OK;
  };
  int rc;
  try {
    rc = body();
  } catch (const std::bad_alloc&) {
    rc = fail(CURDLE_ENOMEM, "out of memory");
  }
  if (rc && T.stream) (void)hipStreamSynchronize(T.stream);  // nothing queued may outlive the hold
  {
    std::lock_guard<std::mutex> g(cx.mu);
    T.busy = false;
    if (!rc) T.last_ms = kernel_ms;
  }
  T.cv.notify_one();
  if (rc) return rc;
  unsigned long long handed_back = 0;
  for (size_t i = 0; i < k; i++) handed_back += status[i] != 0;
  g_tr_stat[0].fetch_add(k, std::memory_order_relaxed);
  g_tr_stat[1].fetch_add(handed_back, std::memory_order_relaxed);
  return CURDLE_OK;
}

extern "C" int curdle_stat_transcript(unsigned long long out[2]) { return read_stats(out, g_tr_stat, 2); }

extern "C" int curdle_stat_transcript_paths(unsigned long long out[2]) {
  if (!out) return CURDLE_EINVAL;
  transcript_path_counts(out);
  return CURDLE_OK;
}

// `reps` dependent permutations of n states by one of the two device forms of Keccak-f[1600]: a transcript call's
// stream, buffers and hold, one copy up, one kernel between the events, one copy back.
extern "C" int curdle_keccak_permute_batch(const uint64_t* states_in, size_t n, unsigned form, unsigned reps, uint64_t* states_out,
                                           double* kernel_ms) {
  if (!states_in || !states_out) return fail(CURDLE_EINVAL, "null argument");
  if (form > 1) return fail(CURDLE_EINVAL, "form %u: 0 is a state per lane, 1 a state spread over lanes", form);
  if (reps == 0 || reps > CURDLE_KECCAK_PERMUTE_MAX_REPS) return fail(CURDLE_EINVAL, "reps %u outside 1..%d", reps, CURDLE_KECCAK_PERMUTE_MAX_REPS);
  if (n > CURDLE_KECCAK_PERMUTE_MAX_STATES) return fail(CURDLE_EINVAL, "%zu states exceed CURDLE_KECCAK_PERMUTE_MAX_STATES", n);
  if (n == 0) {
    if (kernel_ms) *kernel_ms = 0;
    return CURDLE_OK;
  }
  const size_t bytes = n * 200;
  Ctx& cx = cur();
  TrCtx& T = cx.tr;
  {
    std::unique_lock<std::mutex> g(cx.mu);
    int rc = init_default_locked(cx);
    if (rc) return rc;
    T.cv.wait(g, [&] { return !T.busy; });
    T.busy = true;
  }
  float ms = 0;
  auto body = [&]() -> int {
    HIP_TRY(hipSetDevice(cx.device));
    int r;
    if ((r = ensure_host(T.h_in, T.h_in_cap, bytes))) return r;
    if ((r = ensure_host(T.h_out, T.h_out_cap, bytes))) return r;
    if ((r = ensure(T.d_in, bytes))) return r;
    if ((r = ensure(T.d_out, bytes))) return r;
    memcpy(T.h_in, states_in, bytes);
    HIP_TRY(hipMemcpyAsync(T.d_in.p, T.h_in, bytes, hipMemcpyHostToDevice, T.stream));
    HIP_TRY(hipEventRecord(T.ev[0], T.stream));
    HIP_TRY(launch_keccak_permute(static_cast<const uint64_t*>(T.d_in.p), static_cast<uint64_t*>(T.d_out.p), (uint32_t)n, reps, (int)form, T.stream));
    HIP_TRY(hipEventRecord(T.ev[1], T.stream));
    HIP_TRY(hipMemcpyAsync(T.h_out, T.d_out.p, bytes, hipMemcpyDeviceToHost, T.stream));
    HIP_TRY(hipStreamSynchronize(T.stream));
    HIP_TRY(hipEventElapsedTime(&ms, T.ev[0], T.ev[1]));
    memcpy(states_out, T.h_out, bytes);
    return CURDLE_OK;
  };
  int rc;
  try {
    rc = body();
  } catch (const std::bad_alloc&) {
    rc = fail(CURDLE_ENOMEM, "out of memory");
  }
  if (rc && T.stream) (void)hipStreamSynchronize(T.stream);  // nothing queued may outlive the hold
  {
    std::lock_guard<std::mutex> g(cx.mu);
    T.busy = false;
  }
  T.cv.notify_one();
  if (!rc && kernel_ms) *kernel_ms = ms;
  return rc;
}

extern "C" int curdle_transcript_last_kernel_ms(double* out) {
  if (!out) return fail(CURDLE_EINVAL, "null argument");
  Ctx& cx = cur();
  std::lock_guard<std::mutex> g(cx.mu);
  *out = cx.tr.last_ms;
  return CURDLE_OK;
}
