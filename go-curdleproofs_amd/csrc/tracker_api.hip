// C ABI of the batched Whisk tracker-proof check (tracker_kernels.hip): curdle_whisk_is_valid_tracker_proof_batch
// (_ex, _device), k calls of IsValidWhiskTrackerProof (the reference's whisk/whisk.go:116-147) in one -- and, in the
// second half of the file, of the batched generator curdle_whisk_generate_tracker_proof_batch (_blinders), k calls of
// GenerateWhiskTrackerProof (:149-175) in one, on the same tape and slots (tracker_prove_kernels.hip).
//
// Two forms.  HOST-HASHED (tracker_pass), per pass of at most kTrackerPass members, on the calling thread's context:
//   1. the 5 k records (rG, krG, kG, A, B per member) go up once; the square roots (launch_g1_decompress) run on
//      the held slot's stream and the subgroup test from the same bytes (launch_g1_subgroup_from_bytes) beside it
//      on a second slot's stream when one is free -- the two chains overlap, as in the two-step decoding;
//   2. meanwhile the host checks every S (< r) and hashes every member's transcript (whisk.go:131-134) from the
//      RAW records: every encoding the decoder accepts is the compressed form of the point it decodes to, so the
//      challenge is the one the single call computes (a member with a record that does not decode is an error
//      whatever was hashed);
//   3. s and c go up, k_tracker_check runs behind the square roots, and k + 10 k bytes come back: the verdicts,
//      the decoding statuses and the subgroup verdicts.
// DEVICE-HASHED (tracker_pass_device): from bytes to verdicts with no host arithmetic and no host thread.  The three
// arrays go up as they are (or are read where the caller keeps them: _device) behind the constant tape of the
// transcript program; k_tracker_gather writes the records, the transcript rows and S / skip; the transcript kernel
// (launch_transcript_batch, the tape compiled once per process) and the subgroup test run on the second slot's stream
// beside the square roots; k_tracker_challenge puts c next to s, k_tracker_check runs as above.  Tape, start state,
// rows and challenges live in the held slot's buffers: the transcript context (TrCtx) and its lock are not touched.
// COMBINED (tracker_pass_combined, curdle_whisk_is_valid_tracker_proof_batch_combined / _device): the device-hashed
// pass up to k_tracker_challenge, then ONE randomly weighted MSM over the decoded records settles the pass;
// k_tracker_check runs only when the sum is not infinity (the section before the generation half has the layout).
// No stream is made here and no device memory is allocated once the slots' buffers have grown to the batch.  Both
// halves hold their slot, and the second one when one is free, with a SlotHold (api_helpers.h).
#include "api_helpers.h"

#include <algorithm>
#include <exception>
#include <stdexcept>

#include "../host/algebra.h"
#include "../host/transcript.h"
#include "../host/transcript_batch.h"
#include "../host/whisk.h"

namespace {
std::atomic<unsigned long long> g_tk_stat[3];  // members hashed on the device | on the host | handed back to the host

constexpr size_t kRec = 48;                  // one compressed G1 record
constexpr size_t kTrackerPass = (size_t)1 << 16;  // members per pass: 327,680 records, 31 MB of decoded points
constexpr size_t kHashPerThread = 128;       // members' transcripts per host thread (one is ~2.7 us)
constexpr unsigned kMaxHashThreads = 16;

// The body of a batch: the constant tape is compiled on its first use and the host's share allocates, and neither may
// leave the C ABI as an exception.
template <class Body>
int guarded(const char* what, Body body) {
  try {
    return body();
  } catch (const std::logic_error& e) {  // the constant tape did not compile to the shape the kernels expect
    return fail(CURDLE_EHIP, "%s: internal error: %s", what, e.what());
  } catch (const std::exception& e) {
    return fail(CURDLE_ENOMEM, "%s: %s", what, e.what());
  }
}

// One member's challenge and response, in the kernel's layout (s then c, canonical, little-endian words);
// false if S is not canonical (< r), as TrackerProof.FromBytes requires (types.go:105-117).
bool member_scalars(const uint8_t* tracker, const uint8_t* k_comm, const uint8_t* proof, const uint8_t gen[kRec],
                    uint32_t sc[16]) {
  curdle::alg::Scalar s;
  if (!curdle::alg::Scalar::SetBytesCanonical(proof + 96, &s)) return false;
  s.Canonical(sc);
  uint8_t six[6 * kRec];  // kG, g1Gen, krG, rG, A, B
  memcpy(six, k_comm, kRec);
  memcpy(six + kRec, gen, kRec);
  memcpy(six + 2 * kRec, tracker + kRec, kRec);
  memcpy(six + 3 * kRec, tracker, kRec);
  memcpy(six + 4 * kRec, proof, 2 * kRec);
  curdle::transcript::Transcript tr("whisk_opening_proof");  // whisk.go:15-17
  tr.AppendCompressed("tracker_opening_proof", six, 6);
  tr.GetAndAppendChallenge("tracker_opening_proof_challenge").Canonical(sc + 8);
  return true;
}

struct Gen {
  uint8_t b[kRec];
  Gen() { curdle::alg::Point::Generator().Compressed(b); }
};

// scalars / skip of members [0, m) of the pass, on up to kMaxHashThreads host threads
void hash_members(const uint8_t* trackers, const uint8_t* k_comms, const uint8_t* proofs, size_t m, uint32_t* sc,
                  uint8_t* skip) {
  static const Gen gen;
  auto run = [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; i++) {
      const bool ok = member_scalars(trackers + 96 * i, k_comms + kRec * i, proofs + 128 * i, gen.b, sc + 16 * i);
      if (!ok) memset(sc + 16 * i, 0, 64);
      skip[i] = ok ? 0 : 1;
    }
  };
  const unsigned hw = std::max(1u, std::min(kMaxHashThreads, std::thread::hardware_concurrency()));
  const size_t nt = std::min<size_t>(hw, (m + kHashPerThread - 1) / kHashPerThread);
  if (nt <= 1) return run(0, m);
  std::vector<std::thread> th;
  std::exception_ptr err;
  std::mutex err_mu;
  const size_t per = (m + nt - 1) / nt;
  for (size_t t = 1; t < nt; t++)
    th.emplace_back([&, t] {
      try {
        run(std::min(m, t * per), std::min(m, (t + 1) * per));
      } catch (...) {
        std::lock_guard<std::mutex> g(err_mu);
        err = std::current_exception();
      }
    });
  try {
    run(0, std::min(m, per));
  } catch (...) {
    std::lock_guard<std::mutex> g(err_mu);
    err = std::current_exception();
  }
  for (auto& t : th) t.join();
  if (err) std::rethrow_exception(err);
}

// One pass: members [0, m) of the given arrays, verdicts into results.  A holds the buffers and runs the square
// roots and the check; B (may be null) runs the subgroup test.
int tracker_pass(Ctx& cx, Slot& A, Slot* B, const uint8_t* trackers, const uint8_t* k_comms, const uint8_t* proofs,
                 size_t m, int* results) {
  const size_t nrec = 5 * m;
  int r;
  if ((r = ensure(A.scalars, nrec * kRec))) return r;   // compressed records
  if ((r = ensure(A.points, nrec * 96))) return r;      // decoded records
  if ((r = ensure(A.counts, 2 * nrec + m))) return r;   // statuses | subgroup verdicts | member verdicts
  if ((r = ensure(A.digits, 64 * m + m))) return r;     // s, c | skip
  if ((r = ensure_pinned(A, 0, nrec * kRec + 65 * m))) return r;
  if ((r = ensure_pinned(A, 1, 2 * nrec + m))) return r;
  uint8_t* h_in = static_cast<uint8_t*>(A.h_stage[0]);
  uint8_t* h_sc = h_in + nrec * kRec;
  uint8_t* h_out = static_cast<uint8_t*>(A.h_stage[1]);
  uint8_t* d_rec = static_cast<uint8_t*>(A.scalars.p);
  uint8_t* d_status = static_cast<uint8_t*>(A.counts.p);
  uint8_t* d_sub = d_status + nrec;
  uint8_t* d_out = d_sub + nrec;
  uint8_t* d_sc = static_cast<uint8_t*>(A.digits.p);
  for (size_t i = 0; i < m; i++) {
    uint8_t* d = h_in + 5 * kRec * i;
    memcpy(d, trackers + 96 * i, 2 * kRec);          // rG, krG
    memcpy(d + 2 * kRec, k_comms + kRec * i, kRec);  // kG
    memcpy(d + 3 * kRec, proofs + 128 * i, 2 * kRec);  // A, B
  }
  HIP_TRY(hipMemcpyAsync(d_rec, h_in, nrec * kRec, hipMemcpyHostToDevice, A.stream));
  if (B) {
    HIP_TRY(hipEventRecord(A.pre_done, A.stream));
    HIP_TRY(hipStreamWaitEvent(B->stream, A.pre_done, 0));
    HIP_TRY(launch_g1_subgroup_from_bytes(d_rec, (uint32_t)nrec, d_sub, B->stream));
    HIP_TRY(hipEventRecord(B->acc_done, B->stream));
  }
  HIP_TRY(launch_g1_decompress(d_rec, (uint32_t)nrec, 0, (uint32_t*)A.points.p, d_status, A.stream));
  if (!B) HIP_TRY(launch_g1_subgroup_from_bytes(d_rec, (uint32_t)nrec, d_sub, A.stream));
  // the host's share, while the GPU decodes
  hash_members(trackers, k_comms, proofs, m, reinterpret_cast<uint32_t*>(h_sc), h_sc + 64 * m);
  HIP_TRY(hipMemcpyAsync(d_sc, h_sc, 65 * m, hipMemcpyHostToDevice, A.stream));
  G1Affine gen;
  g1_generator(gen);
  HIP_TRY(launch_tracker_check(A.points.p, d_status, d_sc, d_sc + 64 * m, gen, (uint32_t)m, d_out, A.stream));
  if (B) HIP_TRY(hipStreamWaitEvent(A.stream, B->acc_done, 0));
  HIP_TRY(hipMemcpyAsync(h_out, d_status, 2 * nrec + m, hipMemcpyDeviceToHost, A.stream));
  HIP_TRY(hipStreamSynchronize(A.stream));
  const uint8_t* st = h_out;
  const uint8_t* sub = h_out + nrec;
  const uint8_t* verdict = h_out + 2 * nrec;
  const uint8_t* skip = h_sc + 64 * m;
  for (size_t i = 0; i < m; i++) {
    bool err = skip[i] != 0;
    for (size_t j = 5 * i; j < 5 * i + 5; j++) err |= st[j] > CURDLE_DECODE_INFINITY || (st[j] == CURDLE_DECODE_OK && !sub[j]);
    if (err) {
      results[i] = CURDLE_EINVAL;
    } else if (verdict[i] == kTrackerAccept || verdict[i] == kTrackerReject) {
      results[i] = verdict[i];
    } else {
      return fail(CURDLE_EHIP, "tracker check: member %zu of a pass has no verdict", i);
    }
  }
  g_tk_stat[1].fetch_add(m, std::memory_order_relaxed);
  return CURDLE_OK;
}

// The constant part of the device-hashed form, compiled once per process: the tape of
//   Transcript("whisk_opening_proof"); AppendPoints("tracker_opening_proof", kG g1Gen krG rG A B);
//   GetAndAppendChallenge("tracker_opening_proof_challenge")                                  (whisk.go:15-17, 131-134)
// as one block of bytes, control list | block pool | start state | the generator's encoding, padded to 16.
struct TrackerTape {
  std::vector<uint8_t> bytes;
  size_t pool_off = 0, init_off = 0, gen_off = 0;
  uint32_t n_ctl = 0;
  uint64_t tail = 0;
  TrackerTape() {
    using namespace curdle::transcript;
    auto step = [](uint32_t op, uint32_t count, uint32_t len, const char* label) {
      curdle_transcript_step s = {};
      s.op = op, s.count = count, s.len = len, s.label_len = (uint32_t)strlen(label);
      memcpy(s.label, label, s.label_len);
      return s;
    };
    const curdle_transcript_step steps[2] = {step(CURDLE_TR_APPEND, 6, kRec, "tracker_opening_proof"),
                                             step(CURDLE_TR_CHALLENGES, 1, 0, "tracker_opening_proof_challenge")};
    uint8_t init[CURDLE_TRANSCRIPT_STATE_SIZE];
    Transcript("whisk_opening_proof").inner().Export(init);
    Tape tape;
    CompileTape(steps, 2, init + 200, &tape);
    if (tape.consumed != 6 * kRec || tape.n_challenges != 1) throw std::logic_error("tracker tape");
    const size_t ctl_bytes = tape.ctl.size() * sizeof(TapeCtl), pool_bytes = tape.pool.size() * sizeof(TapeBlock);
    pool_off = ctl_bytes;
    init_off = pool_off + pool_bytes;
    gen_off = init_off + sizeof(init);
    bytes.assign((gen_off + kRec + 15) / 16 * 16, 0);
    memcpy(bytes.data(), tape.ctl.data(), ctl_bytes);
    memcpy(bytes.data() + pool_off, tape.pool.data(), pool_bytes);
    memcpy(bytes.data() + init_off, init, sizeof(init));
    memcpy(bytes.data() + gen_off, Gen().b, kRec);
    n_ctl = (uint32_t)tape.ctl.size();
    tail = (uint64_t)tape.pos | ((uint64_t)tape.pos_begin << 8) | ((uint64_t)tape.cur_flags << 16);
  }
};
constexpr size_t kRowBytes = 8 * (2 + 6 * kRec / 8);  // transcript::TapeRowWords(288) words

// One device-hashed pass.  `resident`: the three arrays are device pointers, read where they are.  `sa` is the
// stream the pass runs on: the held slot's, or the caller's (then B is null and everything runs on that stream).
int tracker_pass_device(Ctx& cx, Slot& A, Slot* B, hipStream_t sa, const uint8_t* trackers, const uint8_t* k_comms,
                        const uint8_t* proofs, bool resident, size_t m, int* results) {
  static const TrackerTape T;
  const size_t nrec = 5 * m, tape_bytes = T.bytes.size(), raw_bytes = resident ? 0 : 272 * m;
  int r;
  if ((r = ensure(A.scalars, nrec * kRec))) return r;     // compressed records
  if ((r = ensure(A.points, nrec * 96))) return r;        // decoded records
  if ((r = ensure(A.counts, 2 * nrec + 2 * m))) return r;  // statuses | subgroup verdicts | member verdicts | transcript statuses
  if ((r = ensure(A.digits, 64 * m + m))) return r;       // s, c | skip
  if ((r = ensure(A.sorted, tape_bytes + raw_bytes + (kRowBytes + 32) * m))) return r;  // tape | the arrays | rows | challenges
  if ((r = ensure_pinned(A, 0, tape_bytes + raw_bytes))) return r;
  if ((r = ensure_pinned(A, 1, 2 * nrec + 2 * m))) return r;
  uint8_t* h_in = static_cast<uint8_t*>(A.h_stage[0]);
  uint8_t* h_out = static_cast<uint8_t*>(A.h_stage[1]);
  uint8_t* d_tape = static_cast<uint8_t*>(A.sorted.p);
  uint8_t* d_raw = d_tape + tape_bytes;
  uint8_t* d_rows = d_raw + raw_bytes;
  uint8_t* d_ch = d_rows + kRowBytes * m;
  uint8_t* d_rec = static_cast<uint8_t*>(A.scalars.p);
  uint8_t* d_status = static_cast<uint8_t*>(A.counts.p);
  uint8_t* d_sub = d_status + nrec;
  uint8_t* d_out = d_sub + nrec;
  uint8_t* d_trst = d_out + m;
  uint8_t* d_sc = static_cast<uint8_t*>(A.digits.p);
  memcpy(h_in, T.bytes.data(), tape_bytes);
  if (!resident) {  // as the caller laid them out: nothing is repacked
    memcpy(h_in + tape_bytes, trackers, 96 * m);
    memcpy(h_in + tape_bytes + 96 * m, k_comms, kRec * m);
    memcpy(h_in + tape_bytes + 144 * m, proofs, 128 * m);
    trackers = d_raw, k_comms = d_raw + 96 * m, proofs = d_raw + 144 * m;
  }
  HIP_TRY(hipMemcpyAsync(d_tape, h_in, tape_bytes + raw_bytes, hipMemcpyHostToDevice, sa));
  HIP_TRY(launch_tracker_gather(trackers, k_comms, proofs, d_tape + T.gen_off, (uint32_t)m, d_rec, d_rows, d_sc, d_sc + 64 * m, sa));
  TranscriptArgs ta = {};
  ta.ctl = reinterpret_cast<const curdle::transcript::TapeCtl*>(d_tape);
  ta.pool = reinterpret_cast<const curdle::transcript::TapeBlock*>(d_tape + T.pool_off);
  ta.data = reinterpret_cast<const uint64_t*>(d_rows);
  ta.init = reinterpret_cast<const uint64_t*>(d_tape + T.init_off);
  ta.challenges = reinterpret_cast<uint64_t*>(d_ch);
  ta.states = nullptr;
  ta.status = d_trst;
  ta.tail = T.tail;
  ta.n_ctl = T.n_ctl;
  ta.row_words = (uint32_t)(kRowBytes / 8);
  ta.init_stride = 0;
  ta.k = (uint32_t)m;
  choose_transcript_kernel(m, &ta);
  ta.n_challenges = 1;
  if (B) {  // transcripts, then the subgroup test, beside the square roots
    HIP_TRY(hipEventRecord(A.pre_done, sa));
    HIP_TRY(hipStreamWaitEvent(B->stream, A.pre_done, 0));
    HIP_TRY(launch_transcript_batch(ta, B->stream));
    HIP_TRY(hipEventRecord(B->pre_done, B->stream));
    HIP_TRY(launch_g1_subgroup_from_bytes(d_rec, (uint32_t)nrec, d_sub, B->stream));
    HIP_TRY(hipEventRecord(B->acc_done, B->stream));
  }
  HIP_TRY(launch_g1_decompress(d_rec, (uint32_t)nrec, 0, (uint32_t*)A.points.p, d_status, sa));
  if (B) {
    HIP_TRY(hipStreamWaitEvent(sa, B->pre_done, 0));
  } else {
    HIP_TRY(launch_transcript_batch(ta, sa));
    HIP_TRY(launch_g1_subgroup_from_bytes(d_rec, (uint32_t)nrec, d_sub, sa));
  }
  HIP_TRY(launch_tracker_challenge(d_ch, d_trst, (uint32_t)m, d_sc, d_sc + 64 * m, sa));
  G1Affine gen;
  g1_generator(gen);
  HIP_TRY(launch_tracker_check(A.points.p, d_status, d_sc, d_sc + 64 * m, gen, (uint32_t)m, d_out, sa));
  if (B) HIP_TRY(hipStreamWaitEvent(sa, B->acc_done, 0));
  HIP_TRY(hipMemcpyAsync(h_out, d_status, 2 * nrec + 2 * m, hipMemcpyDeviceToHost, sa));
  HIP_TRY(hipStreamSynchronize(sa));
  const uint8_t* st = h_out;
  const uint8_t* sub = h_out + nrec;
  const uint8_t* verdict = h_out + 2 * nrec;
  const uint8_t* trst = verdict + m;
  unsigned long long handed_back = 0;
  for (size_t i = 0; i < m; i++) {
    if (trst[i]) {  // 256 rejected draws (0.547^256): the single call settles the member on the host
      if (resident) return fail(CURDLE_EHIP, "tracker check: member %zu of a pass drew no canonical challenge", i);
      int ok = 0;
      const int rc = curdle_whisk_is_valid_tracker_proof(h_in + tape_bytes + 96 * i, h_in + tape_bytes + 96 * m + kRec * i,
                                                         h_in + tape_bytes + 144 * m + 128 * i, &ok);
      results[i] = rc ? rc : ok;
      handed_back++;
      continue;
    }
    bool err = verdict[i] == kTrackerError;  // S >= r, or a record that does not decode
    for (size_t j = 5 * i; j < 5 * i + 5; j++) err |= st[j] > CURDLE_DECODE_INFINITY || (st[j] == CURDLE_DECODE_OK && !sub[j]);
    if (err) {
      results[i] = CURDLE_EINVAL;
    } else if (verdict[i] == kTrackerAccept || verdict[i] == kTrackerReject) {
      results[i] = verdict[i];
    } else {
      return fail(CURDLE_EHIP, "tracker check: member %zu of a pass has no verdict", i);
    }
  }
  g_tk_stat[0].fetch_add(m - handed_back, std::memory_order_relaxed);
  g_tk_stat[2].fetch_add(handed_back, std::memory_order_relaxed);
  return CURDLE_OK;
}

// Smallest batch whose transcripts CURDLE_TRACKER_HASH_DEFAULT hashes on the device (knob TRACKER_DEVICE_HASH unset):
// the smallest measured k at which, on 16 CPUs, device hashing is not slower than the parent's host hashing by more
// than the spread of the repetitions -- and it holds at every larger measured size too (DESIGN.md section 0;
// profiles/r13_tracker_device_hash.json, default_rule_from_k).  Medians of 7, device against parent: k = 64 2.23
// against 2.23 ms, 1,024 2.60 against 2.29 ms (inside the parent's 19 % spread there, but 0.3 ms behind its median),
// 8,192 3.30 against 3.39 ms, 65,536 20.9 against 26.7 ms.
constexpr size_t kDeviceHashFrom = 64;

// The whole call: host arrays (hash_device chooses the form) or resident ones (always device-hashed).
int tracker_batch(const uint8_t* trackers, const uint8_t* k_comms, const uint8_t* proofs, size_t k, bool hash_device,
                  bool resident, void* user_stream, int* results) {
  int rc = CURDLE_OK;
  if (!trackers || !k_comms || !proofs || !results) {
    rc = fail(CURDLE_EINVAL, "null argument");
  } else {
    Ctx& cx = cur();
    SlotHold H(cx, true, user_stream);
    // a second slot only lends its stream (and two events) to the subgroup test and the transcripts; without one
    // they run behind the square roots.  A caller's stream carries the whole pass.
    Slot* B = user_stream ? nullptr : H.try_second();
    rc = H.run([&]() -> int {
      return guarded("tracker check", [&]() -> int {
        Slot& A = H.slot();
        const hipStream_t sa = H.stream();
        for (size_t lo = 0; lo < k; lo += kTrackerPass) {
          const size_t m = std::min(kTrackerPass, k - lo);
          const int r = hash_device ? tracker_pass_device(cx, A, B, sa, trackers + 96 * lo, k_comms + kRec * lo,
                                                          proofs + 128 * lo, resident, m, results + lo)
                                    : tracker_pass(cx, A, B, trackers + 96 * lo, k_comms + kRec * lo, proofs + 128 * lo, m,
                                                   results + lo);
          if (r) return r;
        }
        return CURDLE_OK;
      });
    });
  }
  if (rc != CURDLE_OK && results)  // "could not compute" must never read as a verdict
    for (size_t i = 0; i < k; i++) results[i] = rc;
  return rc;
}

// --- the combined form: a pass settled by ONE randomly weighted MSM -----------------------------------------------------
//
// curdle_whisk_is_valid_tracker_proof_batch_combined (_device).  A pass starts as tracker_pass_device does (upload,
// gather, transcripts and subgroup test beside the square roots, k_tracker_challenge); then k_tracker_combine
// (tracker_combine_kernels.hip) writes the 5 m scalars of the weighted sum of the members' 2 m equations and one
// (G, partial sum) pair per block, and the library's own MSM (enqueue_slot / finish_slot) runs over the decoded records
// on the pass's stream.  Infinity: every member that was not excluded is accepted.  Anything else: k_tracker_check
// runs as in the plain form and its verdicts are the answer.
//
// The MSM runs in the HELD slot, so the pass keeps nothing it needs afterwards in a buffer enqueue_slot writes
// (offsets, counts, starts, cursor, fragcnt, foff, small, digits, sorted, tmp, ccur, points28, frags, partials,
// winsums, winsums28, results, chain, mdone and the pinned h_buf).  enqueue_slot never touches `points` and `scalars`
// (they are the staging of the host-buffer MSM entry points, which hold their own slot), `tracker_keep` (this
// pass's alone) or the pinned h_stage pair, and that is where everything read after the MSM lives:
//   points        the 5 m decoded records | the blocks' generator points        (the MSM's bases; the fallback's input)
//   scalars       the 5 m compressed records | the 5 m + blocks MSM scalars
//   tracker_keep  statuses | subgroup verdicts | member verdicts | transcript statuses | skip | s, c
// `sorted` holds tape, arrays, rows and challenges as in the plain form: all of it is consumed by k_tracker_challenge,
// in stream order before the MSM's first kernel.  No second slot is waited for: B only lends its stream, as above, and
// on a caller's stream there is none and the whole pass, MSM included, runs on that stream.
std::atomic<unsigned long long> g_tc_stat[4];  // passes settled by the sum | fallen back | members accepted by a sum | excluded
std::atomic<float> g_tc_kernel_ms{0};          // k_tracker_combine in the last curdle_whisk_tracker_combined_scalars, by HIP events

void combine_seed_words(const uint8_t seed[32], TrackerCombineSeed* out) {
  static const char kDomain[] = "curdle/tracker-combine/v1";  // 25 bytes
  uint8_t block[72] = {0};
  memcpy(block, kDomain, 25);
  memcpy(block + 25, seed, 32);
  block[65] = 0x1f;  // SHAKE's domain bits and the first padding bit, behind the 65 bytes of input
  memcpy(out->w, block, 72);
}

struct CombineDiag {  // curdle_whisk_tracker_combined_scalars: the pass stops behind k_tracker_combine
  uint64_t* scalars_out;
  uint64_t* g_out;
};

int tracker_pass_combined(Ctx& cx, Slot& A, Slot* B, hipStream_t sa, const uint8_t* trackers, const uint8_t* k_comms,
                          const uint8_t* proofs, bool resident, size_t m, size_t first, const TrackerCombineSeed& seed,
                          int* results, const CombineDiag* diag) {
  static const TrackerTape T;
  const size_t nrec = 5 * m, tape_bytes = T.bytes.size(), raw_bytes = resident ? 0 : 272 * m;
  const size_t nblk = tracker_combine_blocks((uint32_t)m), npairs = nrec + nblk;
  const size_t bytes_out = 2 * nrec + 3 * m;          // statuses | subgroup verdicts | member verdicts | transcript statuses | skip
  const size_t sc_off = (bytes_out + 15) / 16 * 16;  // s, c behind them
  int r;
  if ((r = ensure(A.scalars, nrec * kRec + npairs * 32))) return r;
  if ((r = ensure(A.points, npairs * 96))) return r;
  if ((r = ensure(A.tracker_keep, sc_off + 64 * m))) return r;
  if ((r = ensure(A.sorted, tape_bytes + raw_bytes + (kRowBytes + 32) * m))) return r;  // tape | the arrays | rows | challenges
  if ((r = ensure_pinned(A, 0, tape_bytes + raw_bytes))) return r;
  if ((r = ensure_pinned(A, 1, bytes_out + (diag ? nblk * 32 : 0)))) return r;
  uint8_t* h_in = static_cast<uint8_t*>(A.h_stage[0]);
  uint8_t* h_out = static_cast<uint8_t*>(A.h_stage[1]);
  uint8_t* d_tape = static_cast<uint8_t*>(A.sorted.p);
  uint8_t* d_raw = d_tape + tape_bytes;
  uint8_t* d_rows = d_raw + raw_bytes;
  uint8_t* d_ch = d_rows + kRowBytes * m;
  uint8_t* d_rec = static_cast<uint8_t*>(A.scalars.p);
  uint8_t* d_msm_sc = d_rec + nrec * kRec;
  uint8_t* d_status = static_cast<uint8_t*>(A.tracker_keep.p);
  uint8_t* d_sub = d_status + nrec;
  uint8_t* d_out = d_sub + nrec;
  uint8_t* d_trst = d_out + m;
  uint8_t* d_skip = d_trst + m;
  uint8_t* d_sc = d_status + sc_off;
  memcpy(h_in, T.bytes.data(), tape_bytes);
  if (!resident) {
    memcpy(h_in + tape_bytes, trackers, 96 * m);
    memcpy(h_in + tape_bytes + 96 * m, k_comms, kRec * m);
    memcpy(h_in + tape_bytes + 144 * m, proofs, 128 * m);
    trackers = d_raw, k_comms = d_raw + 96 * m, proofs = d_raw + 144 * m;
  }
  HIP_TRY(hipMemcpyAsync(d_tape, h_in, tape_bytes + raw_bytes, hipMemcpyHostToDevice, sa));
  HIP_TRY(launch_tracker_gather(trackers, k_comms, proofs, d_tape + T.gen_off, (uint32_t)m, d_rec, d_rows, d_sc, d_skip, sa));
  TranscriptArgs ta = {};
  ta.ctl = reinterpret_cast<const curdle::transcript::TapeCtl*>(d_tape);
  ta.pool = reinterpret_cast<const curdle::transcript::TapeBlock*>(d_tape + T.pool_off);
  ta.data = reinterpret_cast<const uint64_t*>(d_rows);
  ta.init = reinterpret_cast<const uint64_t*>(d_tape + T.init_off);
  ta.challenges = reinterpret_cast<uint64_t*>(d_ch);
  ta.states = nullptr;
  ta.status = d_trst;
  ta.tail = T.tail;
  ta.n_ctl = T.n_ctl;
  ta.row_words = (uint32_t)(kRowBytes / 8);
  ta.init_stride = 0;
  ta.k = (uint32_t)m;
  choose_transcript_kernel(m, &ta);
  ta.n_challenges = 1;
  if (B) {  // transcripts, then the subgroup test, beside the square roots
    HIP_TRY(hipEventRecord(A.pre_done, sa));
    HIP_TRY(hipStreamWaitEvent(B->stream, A.pre_done, 0));
    HIP_TRY(launch_transcript_batch(ta, B->stream));
    HIP_TRY(hipEventRecord(B->pre_done, B->stream));
    HIP_TRY(launch_g1_subgroup_from_bytes(d_rec, (uint32_t)nrec, d_sub, B->stream));
    HIP_TRY(hipEventRecord(B->acc_done, B->stream));
  }
  HIP_TRY(launch_g1_decompress(d_rec, (uint32_t)nrec, 0, (uint32_t*)A.points.p, d_status, sa));
  if (B) {
    HIP_TRY(hipStreamWaitEvent(sa, B->pre_done, 0));
  } else {
    HIP_TRY(launch_transcript_batch(ta, sa));
    HIP_TRY(launch_g1_subgroup_from_bytes(d_rec, (uint32_t)nrec, d_sub, sa));
  }
  HIP_TRY(launch_tracker_challenge(d_ch, d_trst, (uint32_t)m, d_sc, d_skip, sa));
  // the scalars wait for the subgroup verdicts too: a record outside the subgroup must get a zero scalar
  if (B) HIP_TRY(hipStreamWaitEvent(sa, B->acc_done, 0));
  G1Affine gen;
  g1_generator(gen);
  if (diag) {  // the diagnostic brackets the kernel with the slot's profiling events (made on their first use, like Prof's)
    if (!A.ev_made) {
      for (auto& e : A.ev) HIP_TRY(hipEventCreate(&e));
      A.ev_made = true;
    }
    HIP_TRY(hipEventRecord(A.ev[0], sa));
  }
  HIP_TRY(launch_tracker_combine(d_status, d_sub, d_sc, d_skip, seed, (uint64_t)first, (uint32_t)m, gen, d_msm_sc, A.points.p, sa));
  if (diag) {
    HIP_TRY(hipEventRecord(A.ev[1], sa));
    HIP_TRY(hipMemcpyAsync(diag->scalars_out, d_msm_sc, nrec * 32, hipMemcpyDeviceToHost, sa));
    HIP_TRY(hipMemcpyAsync(h_out + bytes_out, d_msm_sc + nrec * 32, nblk * 32, hipMemcpyDeviceToHost, sa));
    HIP_TRY(hipStreamSynchronize(sa));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, A.ev[0], A.ev[1]));
    g_tc_kernel_ms.store(ms, std::memory_order_relaxed);
    Fr g;
    f_zero(g);
    for (size_t b = 0; b < nblk; b++) {
      Fr part;
      memcpy(part.l, h_out + bytes_out + 32 * b, 32);
      fr_add(g, g, part);
    }
    memcpy(diag->g_out, g.l, 32);
    return CURDLE_OK;
  }
  // everything but the chains' verdicts comes back behind the scalars, ahead of the MSM: finish_slot's wait covers it
  HIP_TRY(hipMemcpyAsync(h_out, d_status, bytes_out, hipMemcpyDeviceToHost, sa));
  const uint32_t off[2] = {0, (uint32_t)npairs};
  MsmCall call{off};
  MsmInputs in;
  in.points = A.points.p;
  in.scalars = d_msm_sc;
  uint64_t sum[18];
  if ((r = enqueue_slot(cx, A, call, in, {sa, sa, sa}))) return r;
  if ((r = finish_slot(cx, A, sum))) return r;
  bool settled = true;  // Z = 0: the weighted sum is the point at infinity
  for (int w = 12; w < 18; w++) settled &= sum[w] == 0;
  const uint8_t* st = h_out;
  const uint8_t* sub = h_out + nrec;
  const uint8_t* verdict = h_out + 2 * nrec;
  const uint8_t* trst = verdict + m;
  const uint8_t* skip = trst + m;
  if (!settled) {
    HIP_TRY(launch_tracker_check(A.points.p, d_status, d_sc, d_skip, gen, (uint32_t)m, d_out, sa));
    HIP_TRY(hipMemcpyAsync(h_out + 2 * nrec, d_out, m, hipMemcpyDeviceToHost, sa));
    HIP_TRY(hipStreamSynchronize(sa));
  }
  unsigned long long accepted = 0, excluded = 0;
  for (size_t i = 0; i < m; i++) {
    if (trst[i]) {  // 256 rejected draws (0.547^256): the single call settles the member on the host
      if (resident) return fail(CURDLE_EHIP, "tracker check: member %zu of a pass drew no canonical challenge", i);
      int ok = 0;
      const int rc = curdle_whisk_is_valid_tracker_proof(h_in + tape_bytes + 96 * i, h_in + tape_bytes + 96 * m + kRec * i,
                                                         h_in + tape_bytes + 144 * m + 128 * i, &ok);
      results[i] = rc ? rc : ok;
      excluded++;
      continue;
    }
    bool err = skip[i] != 0;  // S >= r
    for (size_t j = 5 * i; j < 5 * i + 5; j++) err |= st[j] > CURDLE_DECODE_INFINITY || (st[j] == CURDLE_DECODE_OK && !sub[j]);
    if (err) {
      results[i] = CURDLE_EINVAL;
      excluded++;
    } else if (settled) {
      results[i] = kTrackerAccept;
      accepted++;
    } else if (verdict[i] == kTrackerAccept || verdict[i] == kTrackerReject) {
      results[i] = verdict[i];
    } else {
      return fail(CURDLE_EHIP, "tracker check: member %zu of a pass has no verdict", i);
    }
  }
  g_tc_stat[settled ? 0 : 1].fetch_add(1, std::memory_order_relaxed);
  g_tc_stat[2].fetch_add(accepted, std::memory_order_relaxed);
  g_tc_stat[3].fetch_add(excluded, std::memory_order_relaxed);
  return CURDLE_OK;
}

// The whole combined call: host arrays or resident ones; with `diag`, one pass that stops behind the scalars.
int tracker_batch_combined(const uint8_t* trackers, const uint8_t* k_comms, const uint8_t* proofs, size_t k,
                           const uint8_t* seed, bool resident, void* user_stream, int* results, const CombineDiag* diag) {
  int rc = CURDLE_OK;
  if (!trackers || !k_comms || !proofs || !seed || (!diag && !results) || (diag && (!diag->scalars_out || !diag->g_out))) {
    rc = fail(CURDLE_EINVAL, "null argument");
  } else if (diag && k > kTrackerPass) {
    rc = fail(CURDLE_EINVAL, "the scalars of at most %zu members (one pass) can be read back", kTrackerPass);
  } else {
    TrackerCombineSeed words;
    combine_seed_words(seed, &words);
    Ctx& cx = cur();
    SlotHold H(cx, true, user_stream);
    Slot* B = user_stream ? nullptr : H.try_second();  // never waited for: it only lends its stream
    rc = H.run([&]() -> int {
      return guarded("combined tracker check", [&]() -> int {
        Slot& A = H.slot();
        const hipStream_t sa = H.stream();
        for (size_t lo = 0; lo < k; lo += kTrackerPass) {
          const size_t m = std::min(kTrackerPass, k - lo);
          const int r = tracker_pass_combined(cx, A, B, sa, trackers + 96 * lo, k_comms + kRec * lo, proofs + 128 * lo,
                                              resident, m, lo, words, results ? results + lo : nullptr, diag);
          if (r) {  // nothing queued may outlive the hold (the drain below knows neither a caller's stream nor B)
            (void)hipStreamSynchronize(sa);
            if (B) (void)hipStreamSynchronize(B->stream);
            return r;
          }
        }
        return CURDLE_OK;
      });
    }, SlotHold::kDrainSlot);
  }
  if (rc != CURDLE_OK && results)  // "could not compute" must never read as a verdict
    for (size_t i = 0; i < k; i++) results[i] = rc;
  return rc;
}

// --- generation: k calls of GenerateWhiskTrackerProof (whisk.go:149-175) in one ---------------------------------------
//
// Per pass of at most kTrackerPass members, on the held slot's stream (B, when a second slot is free, lends its stream
// to the subgroup test, which then runs beside the square roots and the scalar multiplications):
//   1. tape | trackers go up as they are, and k (with b, when the caller gives the blinders); the 2 m tracker records
//      are decoded (launch_g1_decompress + launch_g1_subgroup_from_bytes);
//   2. with a curdle_rand the 4 m status bytes come back, the host draws ONE GetFr per decodable member in member
//      order -- the single call decodes before it draws (host/whisk.cpp), so a member that fails to decode draws
//      nothing -- and b goes up;
//   3. k_tracker_prove_pairs, ONE launch_scalar_mul_batch over (G, k) | (G, b) | (rG, b), launch_g1_compress over the
//      3 m results, k_tracker_prove_rows, the verifier's tape on launch_transcript_batch, k_tracker_response;
//   4. 128 m + 5 m bytes come back; the buffers that held k, b and the XYZZ results are overwritten.
// A member whose transcript comes back with a status (256 rejected draws) is generated by the single path on the host.
// CURDLE_TRACKER_PROVE_CONSTANT_TIME (the _ex entry points; d_table is then the generator's fixed-base table) changes
// step 3 alone: launch_fbase_mul_ct over k | b (2 m scalars, XYZZ) and launch_g1_normalize put kG and A, launch_g1_mul_ct
// over the decoded rG records (every second record) and b puts B, as affine records where the pairs' points would lie,
// and launch_g1_compress encodes the 3 m of them as kCompressAffine; k_tracker_prove_pairs and the chain do not run.
std::atomic<unsigned long long> g_tp_stat[2];  // members generated on the device | handed to the host single path

struct ProvePass {
  Slot& A;
  hipStream_t sa;
  size_t m;
  WipeList W;  // the places a secret was written to in this pass; wiped on every way out of the pass
};

int prove_pass_run(Ctx& cx, ProvePass& P, Slot* B, const uint8_t* trackers, const uint64_t* ks, const uint64_t* blinders,
                   curdle_rand* rand, const void* d_table, uint8_t* proofs_out, int* results) {
  static const TrackerTape T;
  Slot& A = P.A;
  const hipStream_t sa = P.sa;
  const size_t m = P.m, nrec = 2 * m, tape_bytes = T.bytes.size();
  int r;
  if ((r = ensure(A.sorted, tape_bytes + 96 * m + (kRowBytes + 32) * m))) return r;  // tape | trackers | rows | challenges
  if ((r = ensure(A.points, (192 + 288 + 576) * m))) return r;  // decoded records | the pairs' points | XYZZ results
  if ((r = ensure(A.counts, 2 * nrec + m))) return r;           // statuses | subgroup verdicts | transcript statuses
  if ((r = ensure(A.digits, 96 * m))) return r;                 // k | b | b, Montgomery
  if ((r = ensure(A.scalars, (144 + 128) * m))) return r;       // kG | A | B compressed, the proofs
  if ((r = ensure_pinned(A, 0, tape_bytes + 96 * m + 64 * m))) return r;
  if ((r = ensure_pinned(A, 1, 128 * m + 2 * nrec + m))) return r;
  uint8_t* h_in = static_cast<uint8_t*>(A.h_stage[0]);
  uint8_t* h_k = h_in + tape_bytes + 96 * m;
  uint8_t* h_b = h_k + 32 * m;
  uint8_t* h_out = static_cast<uint8_t*>(A.h_stage[1]);
  uint8_t* h_st = h_out + 128 * m;
  uint8_t* d_tape = static_cast<uint8_t*>(A.sorted.p);
  uint8_t* d_trk = d_tape + tape_bytes;
  uint8_t* d_rows = d_trk + 96 * m;
  uint8_t* d_ch = d_rows + kRowBytes * m;
  uint8_t* d_dec = static_cast<uint8_t*>(A.points.p);
  uint8_t* d_pairs = d_dec + 192 * m;
  uint8_t* d_xyzz = d_pairs + 288 * m;
  uint8_t* d_status = static_cast<uint8_t*>(A.counts.p);
  uint8_t* d_sub = d_status + nrec;
  uint8_t* d_trst = d_sub + nrec;
  uint8_t* d_sc = static_cast<uint8_t*>(A.digits.p);
  uint8_t* d_comp = static_cast<uint8_t*>(A.scalars.p);
  uint8_t* d_proofs = d_comp + 144 * m;

  memcpy(h_in, T.bytes.data(), tape_bytes);
  memcpy(h_in + tape_bytes, trackers, 96 * m);
  P.W.note_host(h_k, 64 * m);
  memcpy(h_k, ks, 32 * m);
  if (blinders) memcpy(h_b, blinders, 32 * m);
  HIP_TRY(hipMemcpyAsync(d_tape, h_in, tape_bytes + 96 * m, hipMemcpyHostToDevice, sa));
  P.W.note_device(d_sc, 96 * m);
  HIP_TRY(hipMemcpyAsync(d_sc, h_k, (blinders ? 64 : 32) * m, hipMemcpyHostToDevice, sa));
  if (B) {
    HIP_TRY(hipEventRecord(A.pre_done, sa));
    HIP_TRY(hipStreamWaitEvent(B->stream, A.pre_done, 0));
    HIP_TRY(launch_g1_subgroup_from_bytes(d_trk, (uint32_t)nrec, d_sub, B->stream));
    HIP_TRY(hipEventRecord(B->acc_done, B->stream));
  }
  HIP_TRY(launch_g1_decompress(d_trk, (uint32_t)nrec, 0, (uint32_t*)d_dec, d_status, sa));
  if (!B) HIP_TRY(launch_g1_subgroup_from_bytes(d_trk, (uint32_t)nrec, d_sub, sa));
  auto bad_member = [&](size_t i) {
    bool bad = false;
    for (size_t j = 2 * i; j < 2 * i + 2; j++)
      bad |= h_st[j] > CURDLE_DECODE_INFINITY || (h_st[j] == CURDLE_DECODE_OK && !h_st[nrec + j]);
    return bad;
  };
  if (!blinders) {
    if (B) HIP_TRY(hipStreamWaitEvent(sa, B->acc_done, 0));
    HIP_TRY(hipMemcpyAsync(h_st, d_status, 2 * nrec, hipMemcpyDeviceToHost, sa));
    HIP_TRY(hipStreamSynchronize(sa));
    for (size_t i = 0; i < m; i++) {
      uint64_t b[4] = {0, 0, 0, 0};
      if (!bad_member(i) && (r = curdle_rand_get_fr(rand, b))) return r;
      memcpy(h_b + 32 * i, b, 32);
    }
    HIP_TRY(hipMemcpyAsync(d_sc + 32 * m, h_b, 32 * m, hipMemcpyHostToDevice, sa));
  }
  G1Affine gen;
  g1_generator(gen);
  P.W.note_device(d_xyzz, 576 * m);
  if (d_table) {  // kG | A | B as affine records at d_pairs: nothing unnormalised is made of b and rG
    HIP_TRY(launch_fbase_mul_ct(d_table, d_sc, nullptr, (uint32_t)(2 * m), d_xyzz, sa));
    HIP_TRY(launch_g1_normalize(d_xyzz, kNormalizeXyzz, (uint32_t)(2 * m), d_pairs, sa, nullptr));
    HIP_TRY(launch_g1_mul_ct(d_dec, 2, d_sc + 32 * m, 0, (uint32_t)m, d_pairs + 192 * m, sa));
    HIP_TRY(launch_g1_compress(d_pairs, kCompressAffine, (uint32_t)(3 * m), d_comp, sa));
  } else {
    HIP_TRY(launch_tracker_prove_pairs(d_dec, gen, (uint32_t)m, d_pairs, d_sc, sa));
    HIP_TRY(launch_scalar_mul_batch(d_pairs, d_sc, 0, nullptr, (uint32_t)(3 * m), d_xyzz, sa));
    HIP_TRY(launch_g1_compress(d_xyzz, kCompressXyzz, (uint32_t)(3 * m), d_comp, sa));
  }
  HIP_TRY(launch_tracker_prove_rows(d_trk, d_comp, d_tape + T.gen_off, (uint32_t)m, d_rows, sa));
  TranscriptArgs ta = {};
  ta.ctl = reinterpret_cast<const curdle::transcript::TapeCtl*>(d_tape);
  ta.pool = reinterpret_cast<const curdle::transcript::TapeBlock*>(d_tape + T.pool_off);
  ta.data = reinterpret_cast<const uint64_t*>(d_rows);
  ta.init = reinterpret_cast<const uint64_t*>(d_tape + T.init_off);
  ta.challenges = reinterpret_cast<uint64_t*>(d_ch);
  ta.states = nullptr;
  ta.status = d_trst;
  ta.tail = T.tail;
  ta.n_ctl = T.n_ctl;
  ta.row_words = (uint32_t)(kRowBytes / 8);
  ta.init_stride = 0;
  ta.k = (uint32_t)m;
  choose_transcript_kernel(m, &ta);
  ta.n_challenges = 1;
  HIP_TRY(launch_transcript_batch(ta, sa));
  if (B && blinders) HIP_TRY(hipStreamWaitEvent(sa, B->acc_done, 0));
  HIP_TRY(launch_tracker_response(d_comp, d_ch, d_sc, d_status, d_sub, (uint32_t)m, d_proofs, sa));
  HIP_TRY(hipMemcpyAsync(h_out, d_proofs, 128 * m, hipMemcpyDeviceToHost, sa));
  HIP_TRY(hipMemcpyAsync(h_st, d_status, 2 * nrec + m, hipMemcpyDeviceToHost, sa));
  HIP_TRY(hipStreamSynchronize(sa));
  const uint8_t* trst = h_st + 2 * nrec;
  unsigned long long handed = 0;
  for (size_t i = 0; i < m; i++) {
    uint8_t* out = proofs_out + 128 * i;
    if (bad_member(i)) {  // where the single call fails to set rG or krG
      memset(out, 0, 128);
      results[i] = CURDLE_EINVAL;
    } else if (trst[i]) {  // 256 rejected draws (0.547^256): the single path settles the member on the host
      curdle::whisk::WhiskTracker t;
      memcpy(&t, trackers + 96 * i, 96);
      try {
        curdle::whisk::GenerateWhiskTrackerProofWithBlinder(t, curdle::alg::Scalar::FromMont(ks + 4 * i),
                                                            curdle::alg::Scalar::FromMont(reinterpret_cast<const uint64_t*>(h_b + 32 * i)), out);
        results[i] = CURDLE_OK;
      } catch (const std::runtime_error&) {
        memset(out, 0, 128);
        results[i] = CURDLE_EINVAL;
      }
      handed++;
    } else {
      memcpy(out, h_out + 128 * i, 128);
      results[i] = CURDLE_OK;
    }
  }
  g_tp_stat[0].fetch_add(m - handed, std::memory_order_relaxed);
  g_tp_stat[1].fetch_add(handed, std::memory_order_relaxed);
  if (d_table) {  // a completed pass: one launch of each constant-time kernel
    count_fbase_ct_pass(2 * m);
    count_g1_mul_ct_pass(m);
  }
  return CURDLE_OK;
}

// The whole call; exactly one of blinders / rand is given.
int tracker_prove_batch(const uint8_t* trackers, const uint64_t* ks, const uint64_t* blinders, curdle_rand* rand, size_t k,
                        unsigned flags, uint8_t* proofs_out, int* results) {
  int rc = CURDLE_OK;
  void* d_table = nullptr;
  bool table_held = false;
  if (!trackers || !ks || (!blinders && !rand) || !proofs_out || !results) {
    rc = fail(CURDLE_EINVAL, "null argument");
  } else if ((flags & CURDLE_TRACKER_PROVE_CONSTANT_TIME) && (rc = generator_table_acquire(cur(), &d_table))) {
    // no device, or the table could not be made: rc says which
  } else {
    table_held = d_table != nullptr;
    Ctx& cx = cur();
    SlotHold H(cx, true, nullptr);
    Slot* B = H.try_second();  // a second slot only lends its stream and an event to the subgroup test
    rc = H.run([&]() -> int {
      return guarded("tracker proofs", [&]() -> int {
        for (size_t lo = 0; lo < k; lo += kTrackerPass) {
          ProvePass P{H.slot(), H.stream(), std::min(kTrackerPass, k - lo), WipeList(H.stream())};
          int r = prove_pass_run(cx, P, B, trackers + 96 * lo, ks + 4 * lo, blinders ? blinders + 4 * lo : nullptr, rand,
                                 d_table, proofs_out + 128 * lo, results + lo);
          if (r && B) (void)hipStreamSynchronize(B->stream);
          const int w = P.W.wipe("tracker proofs: clearing the secrets");  // nothing of k and b stays behind in the slot
          if (r || w) return r ? r : w;
        }
        return CURDLE_OK;
      });
    });
  }
  if (table_held) generator_table_release();
  if (rc != CURDLE_OK) {  // "could not compute" must never read as a proof
    if (results)
      for (size_t i = 0; i < k; i++) results[i] = rc;
    if (proofs_out) memset(proofs_out, 0, 128 * k);
  }
  return rc;
}

}  // namespace

extern "C" int curdle_whisk_is_valid_tracker_proof_batch_ex(const uint8_t* trackers, const uint8_t* k_commitments,
                                                            const uint8_t* proofs, size_t k, unsigned flags, int* results) {
  if (flags > CURDLE_TRACKER_HASH_DEVICE) {
    const int rc = fail(CURDLE_EINVAL, "unknown flags %u", flags);
    if (results)
      for (size_t i = 0; i < k; i++) results[i] = rc;
    return rc;
  }
  if (k == 0) return CURDLE_OK;
  bool device = flags == CURDLE_TRACKER_HASH_DEVICE;
  if (flags == CURDLE_TRACKER_HASH_DEFAULT) {
    const long long knob = knobs::get(knobs::TRACKER_DEVICE_HASH);
    device = knob < 0 ? k >= kDeviceHashFrom : knob != 0;
  }
  return tracker_batch(trackers, k_commitments, proofs, k, device, false, nullptr, results);
}

extern "C" int curdle_whisk_is_valid_tracker_proof_batch(const uint8_t* trackers, const uint8_t* k_commitments,
                                                         const uint8_t* proofs, size_t k, int* results) {
  return curdle_whisk_is_valid_tracker_proof_batch_ex(trackers, k_commitments, proofs, k, CURDLE_TRACKER_HASH_DEFAULT, results);
}

extern "C" int curdle_whisk_is_valid_tracker_proof_batch_device(const void* d_trackers, const void* d_k_commitments,
                                                                const void* d_proofs, size_t k, int* results, void* stream) {
  if (k == 0) return CURDLE_OK;
  return tracker_batch(static_cast<const uint8_t*>(d_trackers), static_cast<const uint8_t*>(d_k_commitments),
                       static_cast<const uint8_t*>(d_proofs), k, true, true, stream, results);
}

extern "C" int curdle_stat_tracker(unsigned long long out[3]) { return read_stats(out, g_tk_stat, 3); }

extern "C" int curdle_whisk_is_valid_tracker_proof_batch_combined(const uint8_t* trackers, const uint8_t* k_commitments,
                                                                  const uint8_t* proofs, size_t k, const uint8_t seed[32],
                                                                  int* results) {
  if (k == 0) return CURDLE_OK;
  return tracker_batch_combined(trackers, k_commitments, proofs, k, seed, false, nullptr, results, nullptr);
}

extern "C" int curdle_whisk_is_valid_tracker_proof_batch_combined_device(const void* d_trackers, const void* d_k_commitments,
                                                                         const void* d_proofs, size_t k, const uint8_t seed[32],
                                                                         int* results, void* stream) {
  if (k == 0) return CURDLE_OK;
  return tracker_batch_combined(static_cast<const uint8_t*>(d_trackers), static_cast<const uint8_t*>(d_k_commitments),
                                static_cast<const uint8_t*>(d_proofs), k, seed, true, stream, results, nullptr);
}

extern "C" int curdle_stat_tracker_combined(unsigned long long out[4]) { return read_stats(out, g_tc_stat, 4); }

extern "C" int curdle_tracker_combined_last_kernel_ms(double* out) {
  if (!out) return CURDLE_EINVAL;
  *out = g_tc_kernel_ms.load(std::memory_order_relaxed);
  return CURDLE_OK;
}

extern "C" int curdle_whisk_tracker_combined_scalars(const uint8_t* trackers, const uint8_t* k_commitments,
                                                     const uint8_t* proofs, size_t k, const uint8_t seed[32],
                                                     uint64_t* scalars_out, uint64_t g_out[4]) {
  if (k == 0) return CURDLE_OK;
  const CombineDiag diag{scalars_out, g_out};
  return tracker_batch_combined(trackers, k_commitments, proofs, k, seed, false, nullptr, nullptr, &diag);
}

extern "C" int curdle_whisk_generate_tracker_proof_batch_blinders_ex(const uint8_t* trackers, const uint64_t* ks,
                                                                     const uint64_t* blinders, size_t k, unsigned flags,
                                                                     uint8_t* proofs_out, int* results) {
  if (flags & ~CURDLE_TRACKER_PROVE_CONSTANT_TIME)  // refused without touching the outputs
    return fail(CURDLE_EINVAL, "unknown flag bits 0x%x", flags & ~CURDLE_TRACKER_PROVE_CONSTANT_TIME);
  if (k == 0) return CURDLE_OK;
  return tracker_prove_batch(trackers, ks, blinders, nullptr, k, flags, proofs_out, results);
}

extern "C" int curdle_whisk_generate_tracker_proof_batch_ex(const uint8_t* trackers, const uint64_t* ks, curdle_rand* rand,
                                                            size_t k, unsigned flags, uint8_t* proofs_out, int* results) {
  if (flags & ~CURDLE_TRACKER_PROVE_CONSTANT_TIME)
    return fail(CURDLE_EINVAL, "unknown flag bits 0x%x", flags & ~CURDLE_TRACKER_PROVE_CONSTANT_TIME);
  if (k == 0) return CURDLE_OK;
  return tracker_prove_batch(trackers, ks, nullptr, rand, k, flags, proofs_out, results);
}

extern "C" int curdle_whisk_generate_tracker_proof_batch_blinders(const uint8_t* trackers, const uint64_t* ks,
                                                                  const uint64_t* blinders, size_t k, uint8_t* proofs_out,
                                                                  int* results) {
  return curdle_whisk_generate_tracker_proof_batch_blinders_ex(trackers, ks, blinders, k, 0, proofs_out, results);
}

extern "C" int curdle_whisk_generate_tracker_proof_batch(const uint8_t* trackers, const uint64_t* ks, curdle_rand* rand,
                                                         size_t k, uint8_t* proofs_out, int* results) {
  return curdle_whisk_generate_tracker_proof_batch_ex(trackers, ks, rand, k, 0, proofs_out, results);
}

extern "C" int curdle_stat_tracker_prove(unsigned long long out[2]) { return read_stats(out, g_tp_stat, 2); }
