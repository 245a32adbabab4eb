// C ABI of the batched Whisk tracker-proof check (tracker_kernels.hip): curdle_whisk_is_valid_tracker_proof_batch
// (_ex, _device), k calls of IsValidWhiskTrackerProof (the reference's whisk/whisk.go:116-147) in one -- and, in the
// second half of the file, of the batched generator curdle_whisk_generate_tracker_proof_batch (_blinders), k calls of
// GenerateWhiskTrackerProof (:149-175) in one, on the same tape and slots (tracker_prove_kernels.hip).
//
// Three forms of the check, each per pass of at most kTrackerPass members, on the calling thread's context.
// HOST-HASHED (tracker_pass):
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
// (launch_transcript_batch over tracker_tape(), compiled once per process) and the subgroup test run on the second
// slot's stream beside the square roots; k_tracker_challenge puts c next to s -- all of that is hashed_prelude --
// and k_tracker_check runs as above.  Tape, start state, rows and challenges live in the held slot's buffers: the
// transcript context (TrCtx) and its lock are not touched.
// COMBINED (tracker_pass_combined, curdle_whisk_is_valid_tracker_proof_batch_combined / _device): hashed_prelude into
// buffers the MSM leaves alone, then ONE randomly weighted MSM over the decoded records settles the pass;
// k_tracker_check runs only when the sum is not infinity (the section before the generation half has the layout).
// What the forms share stands once: decode_beside (the square roots with the side chain beside them on the lent
// stream, or behind them when no slot was lent) and join_side, tracker_tape / tape_args, bad_records and settle_pass
// (a member's answer from the bytes that came back; hand_back where its transcript gave up), fill_results.
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

// The one instance.  Every caller stands inside guarded(...), where a tape that did not compile becomes CURDLE_EHIP.
const TrackerTape& tracker_tape() {
  static const TrackerTape T;
  return T;
}

// The transcript launch of an m-member pass over the copy of the tape at d_tape: rows in, challenges and one status
// byte per member out.
TranscriptArgs tape_args(const uint8_t* d_tape, const uint8_t* d_rows, uint8_t* d_ch, uint8_t* d_trst, size_t m) {
  const TrackerTape& T = tracker_tape();
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
  return ta;
}

// The side chain of a pass on stream st: the transcripts, where the pass hashes on the device (ta), then the subgroup
// test of the nrec records from their bytes.  On a lent slot's stream (B) that slot's events mark the two ends.
int side_chain(const TranscriptArgs* ta, const uint8_t* d_rec, size_t nrec, uint8_t* d_sub, Slot* B, hipStream_t st) {
  if (ta) {
    HIP_TRY(launch_transcript_batch(*ta, st));
    if (B) HIP_TRY(hipEventRecord(B->pre_done, st));
  }
  HIP_TRY(launch_g1_subgroup_from_bytes(d_rec, (uint32_t)nrec, d_sub, st));
  if (B) HIP_TRY(hipEventRecord(B->acc_done, st));
  return CURDLE_OK;
}

// The square roots of nrec records on sa with the side chain beside them: on the lent slot's stream, behind what sa
// holds so far -- or, when no slot was lent (B null), on sa behind the square roots.  With transcripts in the chain, sa
// waits for them (B->pre_done) before it goes on; the subgroup verdicts are waited for where the pass first reads
// them (join_side), which is a different place in every form and is the overlap the forms were measured with.
int decode_beside(Slot& A, Slot* B, hipStream_t sa, const uint8_t* d_rec, size_t nrec, void* d_points, uint8_t* d_status,
                  uint8_t* d_sub, const TranscriptArgs* ta) {
  int r;
  if (B) {
    HIP_TRY(hipEventRecord(A.pre_done, sa));
    HIP_TRY(hipStreamWaitEvent(B->stream, A.pre_done, 0));
    if ((r = side_chain(ta, d_rec, nrec, d_sub, B, B->stream))) return r;
  }
  HIP_TRY(launch_g1_decompress(d_rec, (uint32_t)nrec, 0, (uint32_t*)d_points, d_status, sa));
  if (!B) return side_chain(ta, d_rec, nrec, d_sub, nullptr, sa);
  if (ta) HIP_TRY(hipStreamWaitEvent(sa, B->pre_done, 0));
  return CURDLE_OK;
}

int join_side(Slot* B, hipStream_t sa) {
  if (B) HIP_TRY(hipStreamWaitEvent(sa, B->acc_done, 0));
  return CURDLE_OK;
}

// Where a device-hashed pass of m members keeps what its prelude reads and writes: device memory, but for h_raw.
struct HashedPass {
  size_t m;
  uint8_t *tape, *raw, *rows, *ch;  // the constant tape | the three arrays (host form) | transcript rows | challenges
  uint8_t* h_raw;                   // the three arrays as staged on the host; null in the resident form
  uint8_t* rec;                     // the 5 m compressed records ...
  void* points;                     // ... and decoded
  uint8_t *status, *sub, *trst;     // decoding statuses | subgroup verdicts (5 m each) | transcript statuses (m)
  uint8_t *sc, *skip;               // s, c (64 m) | S was not canonical (m)
};

// A record that does not decode, or decodes to a point outside the subgroup, among `count` records from `first`.
bool bad_records(const uint8_t* st, const uint8_t* sub, size_t first, size_t count) {
  bool bad = false;
  for (size_t j = first; j < first + count; j++) bad |= st[j] > CURDLE_DECODE_INFINITY || (st[j] == CURDLE_DECODE_OK && !sub[j]);
  return bad;
}

// Member i's transcript gave up (256 rejected draws, 0.547^256): the single call settles the member on the host, from
// the arrays as they were staged.  The resident form has no host copy and refuses.
int hand_back(const HashedPass& L, size_t i, int* result) {
  if (!L.h_raw) return fail(CURDLE_EHIP, "tracker check: member %zu of a pass drew no canonical challenge", i);
  int ok = 0;
  const int rc = curdle_whisk_is_valid_tracker_proof(L.h_raw + 96 * i, L.h_raw + 96 * L.m + kRec * i,
                                                     L.h_raw + 144 * L.m + 128 * i, &ok);
  *result = rc ? rc : ok;
  return CURDLE_OK;
}

// What came back from a pass of m members, on the host.
struct PassBytes {
  const uint8_t *st, *sub;  // decoding statuses and subgroup verdicts of the 5 m records
  const uint8_t* verdict;   // k_tracker_check's; not read where the sum settled the pass
  const uint8_t* skip;      // S >= r; null where verdict == kTrackerError says so (the plain device-hashed form)
  const uint8_t* trst;      // transcript statuses; null where the host hashed
  bool settled;             // the combined form's sum was the point at infinity: who is not an error is accepted
};
struct Settled {
  unsigned long long handed_back = 0, errors = 0;
};

// Every member's answer.  L: the staging of a device-hashed pass (for hand_back), null where the host hashed.
int settle_pass(const PassBytes& V, const HashedPass* L, size_t m, int* results, Settled* n) {
  int r;
  for (size_t i = 0; i < m; i++) {
    if (V.trst && V.trst[i]) {
      if ((r = hand_back(*L, i, &results[i]))) return r;
      n->handed_back++;
      continue;
    }
    const bool s_bad = V.skip ? V.skip[i] != 0 : V.verdict[i] == kTrackerError;  // the latter: or a record that does not decode
    if (s_bad || bad_records(V.st, V.sub, 5 * i, 5)) {
      results[i] = CURDLE_EINVAL;
      n->errors++;
    } else if (V.settled) {
      results[i] = kTrackerAccept;
    } else if (V.verdict[i] == kTrackerAccept || V.verdict[i] == kTrackerReject) {
      results[i] = V.verdict[i];
    } else {
      return fail(CURDLE_EHIP, "tracker check: member %zu of a pass has no verdict", i);
    }
  }
  return CURDLE_OK;
}

// "could not compute" must never read as a verdict, or as a proof's result
void fill_results(int* results, size_t k, int rc) {
  if (results)
    for (size_t i = 0; i < k; i++) results[i] = rc;
}

// One host-hashed pass: members [0, m) of the given arrays, verdicts into results.  A holds the buffers and runs the
// square roots and the check; B (may be null) lends its stream to the subgroup test.
int tracker_pass(Slot& A, Slot* B, const uint8_t* trackers, const uint8_t* k_comms, const uint8_t* proofs, size_t m,
                 int* results) {
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
  if ((r = decode_beside(A, B, A.stream, d_rec, nrec, A.points.p, d_status, d_sub, nullptr))) return r;
  // the host's share, while the GPU decodes
  hash_members(trackers, k_comms, proofs, m, reinterpret_cast<uint32_t*>(h_sc), h_sc + 64 * m);
  HIP_TRY(hipMemcpyAsync(d_sc, h_sc, 65 * m, hipMemcpyHostToDevice, A.stream));
  G1Affine gen;
  g1_generator(gen);
  HIP_TRY(launch_tracker_check(A.points.p, d_status, d_sc, d_sc + 64 * m, gen, (uint32_t)m, d_out, A.stream));
  if ((r = join_side(B, A.stream))) return r;  // behind the check, which does not read the subgroup verdicts
  HIP_TRY(hipMemcpyAsync(h_out, d_status, 2 * nrec + m, hipMemcpyDeviceToHost, A.stream));
  HIP_TRY(hipStreamSynchronize(A.stream));
  const PassBytes V{h_out, h_out + nrec, h_out + 2 * nrec, h_sc + 64 * m, nullptr, false};
  Settled n;
  if ((r = settle_pass(V, nullptr, m, results, &n))) return r;
  g_tk_stat[1].fetch_add(m, std::memory_order_relaxed);
  return CURDLE_OK;
}

// tape | the three arrays | rows | challenges in the held slot's `sorted`, tape | the arrays in its first pinned
// stage: the same in both device-hashed forms.  Grows the two and fills L's share of them.
int hashed_staging(Slot& A, bool resident, size_t m, HashedPass* L) {
  const size_t tape_bytes = tracker_tape().bytes.size(), raw_bytes = resident ? 0 : 272 * m;
  int r;
  if ((r = ensure(A.sorted, tape_bytes + raw_bytes + (kRowBytes + 32) * m))) return r;
  if ((r = ensure_pinned(A, 0, tape_bytes + raw_bytes))) return r;
  L->m = m;
  L->tape = static_cast<uint8_t*>(A.sorted.p);
  L->raw = L->tape + tape_bytes;
  L->rows = L->raw + raw_bytes;
  L->ch = L->rows + kRowBytes * m;
  L->h_raw = resident ? nullptr : static_cast<uint8_t*>(A.h_stage[0]) + tape_bytes;
  return CURDLE_OK;
}

// The device-hashed prelude on sa, from the three arrays (host memory, or resident: L.h_raw null) to s, c and skip:
// upload, gather, the transcripts and the subgroup test beside the square roots, the challenge.  The subgroup verdicts
// are not waited for: join_side, where the form first reads them.
int hashed_prelude(Slot& A, Slot* B, hipStream_t sa, const HashedPass& L, const uint8_t* trackers, const uint8_t* k_comms,
                   const uint8_t* proofs) {
  const TrackerTape& T = tracker_tape();
  const size_t m = L.m, tape_bytes = T.bytes.size();
  int r;
  memcpy(A.h_stage[0], T.bytes.data(), tape_bytes);
  if (L.h_raw) {  // as the caller laid them out: nothing is repacked
    memcpy(L.h_raw, trackers, 96 * m);
    memcpy(L.h_raw + 96 * m, k_comms, kRec * m);
    memcpy(L.h_raw + 144 * m, proofs, 128 * m);
    trackers = L.raw, k_comms = L.raw + 96 * m, proofs = L.raw + 144 * m;
  }
  HIP_TRY(hipMemcpyAsync(L.tape, A.h_stage[0], tape_bytes + (L.h_raw ? 272 * m : 0), hipMemcpyHostToDevice, sa));
  HIP_TRY(launch_tracker_gather(trackers, k_comms, proofs, L.tape + T.gen_off, (uint32_t)m, L.rec, L.rows, L.sc, L.skip, sa));
  const TranscriptArgs ta = tape_args(L.tape, L.rows, L.ch, L.trst, m);
  if ((r = decode_beside(A, B, sa, L.rec, 5 * m, L.points, L.status, L.sub, &ta))) return r;
  HIP_TRY(launch_tracker_challenge(L.ch, L.trst, (uint32_t)m, L.sc, L.skip, sa));
  return CURDLE_OK;
}

// One device-hashed pass.  `resident`: the three arrays are device pointers, read where they are.  `sa` is the
// stream the pass runs on: the held slot's, or the caller's (then B is null and everything runs on that stream).
int tracker_pass_device(Slot& A, Slot* B, hipStream_t sa, const uint8_t* trackers, const uint8_t* k_comms,
                        const uint8_t* proofs, bool resident, size_t m, int* results) {
  const size_t nrec = 5 * m;
  HashedPass L;
  int r;
  if ((r = ensure(A.scalars, nrec * kRec))) return r;     // compressed records
  if ((r = ensure(A.points, nrec * 96))) return r;        // decoded records
  if ((r = ensure(A.counts, 2 * nrec + 2 * m))) return r;  // statuses | subgroup verdicts | member verdicts | transcript statuses
  if ((r = ensure(A.digits, 64 * m + m))) return r;       // s, c | skip
  if ((r = hashed_staging(A, resident, m, &L))) return r;
  if ((r = ensure_pinned(A, 1, 2 * nrec + 2 * m))) return r;
  uint8_t* h_out = static_cast<uint8_t*>(A.h_stage[1]);
  L.rec = static_cast<uint8_t*>(A.scalars.p);
  L.points = A.points.p;
  L.status = static_cast<uint8_t*>(A.counts.p);
  L.sub = L.status + nrec;
  uint8_t* d_out = L.sub + nrec;
  L.trst = d_out + m;
  L.sc = static_cast<uint8_t*>(A.digits.p);
  L.skip = L.sc + 64 * m;
  if ((r = hashed_prelude(A, B, sa, L, trackers, k_comms, proofs))) return r;
  G1Affine gen;
  g1_generator(gen);
  HIP_TRY(launch_tracker_check(L.points, L.status, L.sc, L.skip, gen, (uint32_t)m, d_out, sa));
  if ((r = join_side(B, sa))) return r;  // behind the check, which does not read the subgroup verdicts
  HIP_TRY(hipMemcpyAsync(h_out, L.status, 2 * nrec + 2 * m, hipMemcpyDeviceToHost, sa));
  HIP_TRY(hipStreamSynchronize(sa));
  // skip stays on the device: k_tracker_check's kTrackerError covers S >= r
  const PassBytes V{h_out, h_out + nrec, h_out + 2 * nrec, nullptr, h_out + 2 * nrec + m, false};
  Settled n;
  if ((r = settle_pass(V, &L, m, results, &n))) return r;
  g_tk_stat[0].fetch_add(m - n.handed_back, std::memory_order_relaxed);
  g_tk_stat[2].fetch_add(n.handed_back, std::memory_order_relaxed);
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
          const int r = hash_device ? tracker_pass_device(A, B, sa, trackers + 96 * lo, k_comms + kRec * lo,
                                                          proofs + 128 * lo, resident, m, results + lo)
                                    : tracker_pass(A, B, trackers + 96 * lo, k_comms + kRec * lo, proofs + 128 * lo, m,
                                                   results + lo);
          if (r) return r;
        }
        return CURDLE_OK;
      });
    });
  }
  if (rc != CURDLE_OK) fill_results(results, k, rc);
  return rc;
}

// --- the combined form: a pass settled by ONE randomly weighted MSM -----------------------------------------------------
//
// curdle_whisk_is_valid_tracker_proof_batch_combined (_device).  A pass starts with hashed_prelude (upload, gather,
// transcripts and subgroup test beside the square roots, k_tracker_challenge); then k_tracker_combine
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
  const size_t nrec = 5 * m;
  const size_t nblk = tracker_combine_blocks((uint32_t)m), npairs = nrec + nblk;
  const size_t bytes_out = 2 * nrec + 3 * m;          // statuses | subgroup verdicts | member verdicts | transcript statuses | skip
  const size_t sc_off = (bytes_out + 15) / 16 * 16;  // s, c behind them
  HashedPass L;
  int r;
  if ((r = ensure(A.scalars, nrec * kRec + npairs * 32))) return r;
  if ((r = ensure(A.points, npairs * 96))) return r;
  if ((r = ensure(A.tracker_keep, sc_off + 64 * m))) return r;
  if ((r = hashed_staging(A, resident, m, &L))) return r;
  if ((r = ensure_pinned(A, 1, bytes_out + (diag ? nblk * 32 : 0)))) return r;
  uint8_t* h_out = static_cast<uint8_t*>(A.h_stage[1]);
  L.rec = static_cast<uint8_t*>(A.scalars.p);
  uint8_t* d_msm_sc = L.rec + nrec * kRec;
  L.points = A.points.p;
  L.status = static_cast<uint8_t*>(A.tracker_keep.p);
  L.sub = L.status + nrec;
  uint8_t* d_out = L.sub + nrec;
  L.trst = d_out + m;
  L.skip = L.trst + m;
  L.sc = L.status + sc_off;
  if ((r = hashed_prelude(A, B, sa, L, trackers, k_comms, proofs))) return r;
  // the scalars wait for the subgroup verdicts too: a record outside the subgroup must get a zero scalar
  if ((r = join_side(B, sa))) return r;
  G1Affine gen;
  g1_generator(gen);
  if (diag) {  // the diagnostic brackets the kernel with the slot's profiling events (made on their first use, like Prof's)
    if (!A.ev_made) {
      for (auto& e : A.ev) HIP_TRY(hipEventCreate(&e));
      A.ev_made = true;
    }
    HIP_TRY(hipEventRecord(A.ev[0], sa));
  }
  HIP_TRY(launch_tracker_combine(L.status, L.sub, L.sc, L.skip, seed, (uint64_t)first, (uint32_t)m, gen, d_msm_sc, L.points, sa));
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
  HIP_TRY(hipMemcpyAsync(h_out, L.status, bytes_out, hipMemcpyDeviceToHost, sa));
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
  if (!settled) {
    HIP_TRY(launch_tracker_check(L.points, L.status, L.sc, L.skip, gen, (uint32_t)m, d_out, sa));
    HIP_TRY(hipMemcpyAsync(h_out + 2 * nrec, d_out, m, hipMemcpyDeviceToHost, sa));
    HIP_TRY(hipStreamSynchronize(sa));
  }
  const PassBytes V{h_out, h_out + nrec, h_out + 2 * nrec, h_out + 2 * nrec + 2 * m, h_out + 2 * nrec + m, settled};
  Settled n;
  if ((r = settle_pass(V, &L, m, results, &n))) return r;
  const unsigned long long excluded = n.handed_back + n.errors;  // from the sum: handed to the host, or refused
  g_tc_stat[settled ? 0 : 1].fetch_add(1, std::memory_order_relaxed);
  g_tc_stat[2].fetch_add(settled ? m - excluded : 0, std::memory_order_relaxed);
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
  if (rc != CURDLE_OK) fill_results(results, k, rc);
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

int prove_pass_run(ProvePass& P, Slot* B, const uint8_t* trackers, const uint64_t* ks, const uint64_t* blinders,
                   curdle_rand* rand, const void* d_table, uint8_t* proofs_out, int* results) {
  const TrackerTape& T = tracker_tape();
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
  if ((r = decode_beside(A, B, sa, d_trk, nrec, d_dec, d_status, d_sub, nullptr))) return r;
  if (!blinders) {  // the draws need the subgroup verdicts now; with blinders they are first read by the response
    if ((r = join_side(B, sa))) return r;
    HIP_TRY(hipMemcpyAsync(h_st, d_status, 2 * nrec, hipMemcpyDeviceToHost, sa));
    HIP_TRY(hipStreamSynchronize(sa));
    for (size_t i = 0; i < m; i++) {
      uint64_t b[4] = {0, 0, 0, 0};
      if (!bad_records(h_st, h_st + nrec, 2 * i, 2) && (r = curdle_rand_get_fr(rand, b))) return r;
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
  HIP_TRY(launch_transcript_batch(tape_args(d_tape, d_rows, d_ch, d_trst, m), sa));
  if (blinders && (r = join_side(B, sa))) return r;
  HIP_TRY(launch_tracker_response(d_comp, d_ch, d_sc, d_status, d_sub, (uint32_t)m, d_proofs, sa));
  HIP_TRY(hipMemcpyAsync(h_out, d_proofs, 128 * m, hipMemcpyDeviceToHost, sa));
  HIP_TRY(hipMemcpyAsync(h_st, d_status, 2 * nrec + m, hipMemcpyDeviceToHost, sa));
  HIP_TRY(hipStreamSynchronize(sa));
  const uint8_t* trst = h_st + 2 * nrec;
  unsigned long long handed = 0;
  for (size_t i = 0; i < m; i++) {
    uint8_t* out = proofs_out + 128 * i;
    if (bad_records(h_st, h_st + nrec, 2 * i, 2)) {  // where the single call fails to set rG or krG
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
          int r = prove_pass_run(P, B, trackers + 96 * lo, ks + 4 * lo, blinders ? blinders + 4 * lo : nullptr, rand,
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
    fill_results(results, k, rc);
    if (proofs_out) memset(proofs_out, 0, 128 * k);
  }
  return rc;
}

}  // namespace

extern "C" int curdle_whisk_is_valid_tracker_proof_batch_ex(const uint8_t* trackers, const uint8_t* k_commitments,
                                                            const uint8_t* proofs, size_t k, unsigned flags, int* results) {
  if (flags > CURDLE_TRACKER_HASH_DEVICE) {
    const int rc = fail(CURDLE_EINVAL, "unknown flags %u", flags);
    fill_results(results, k, rc);
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
