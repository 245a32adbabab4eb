// C ABI of the batched Whisk tracker-proof check (tracker_kernels.hip): curdle_whisk_is_valid_tracker_proof_batch,
// k calls of IsValidWhiskTrackerProof (the reference's whisk/whisk.go:116-147) in one.
//
// Per pass of at most kTrackerPass members, on the calling thread's context:
//   1. the 5 k records (rG, krG, kG, A, B per member) go up once; the square roots (launch_g1_decompress) run on
//      the held slot's stream and the subgroup test from the same bytes (launch_g1_subgroup_from_bytes) beside it
//      on a second slot's stream when one is free -- the two chains overlap, as in the two-step decoding;
//   2. meanwhile the host checks every S (< r) and hashes every member's transcript (whisk.go:131-134) from the
//      RAW records: every encoding the decoder accepts is the compressed form of the point it decodes to, so the
//      challenge is the one the single call computes (a member with a record that does not decode is an error
//      whatever was hashed);
//   3. s and c go up, k_tracker_check runs behind the square roots, and k + 10 k bytes come back: the verdicts,
//      the decoding statuses and the subgroup verdicts.
// No stream is made here and no device memory is allocated once the slots' buffers have grown to the batch.
#include "msm_internal.h"

#include <algorithm>
#include <exception>

#include "../host/algebra.h"
#include "../host/transcript.h"

namespace {

constexpr size_t kRec = 48;                  // one compressed G1 record
constexpr size_t kTrackerPass = (size_t)1 << 16;  // members per pass: 327,680 records, 31 MB of decoded points
constexpr size_t kHashPerThread = 128;       // members' transcripts per host thread (one is ~2.7 us)
constexpr unsigned kMaxHashThreads = 16;

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

// scalars / skip of members [0, m) of the pass, on up to kMaxHashThreads host threads
void hash_members(const uint8_t* trackers, const uint8_t* k_comms, const uint8_t* proofs, size_t m, uint32_t* sc,
                  uint8_t* skip) {
  static const struct Gen {
    uint8_t b[kRec];
    Gen() { curdle::alg::Point::Generator().Compressed(b); }
  } gen;
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
  return CURDLE_OK;
}

}  // namespace

extern "C" int curdle_whisk_is_valid_tracker_proof_batch(const uint8_t* trackers, const uint8_t* k_commitments,
                                                         const uint8_t* proofs, size_t k, int* results) {
  if (k == 0) return CURDLE_OK;
  int rc = CURDLE_OK;
  if (!trackers || !k_commitments || !proofs || !results) {
    rc = fail(CURDLE_EINVAL, "null argument");
  } else {
    Ctx& cx = cur();
    int ia = -1, ib = -1;
    rc = acquire_slot(cx, true, &ia);
    if (rc == CURDLE_OK) {
      // a second slot only lends its stream to the subgroup test; without one the test runs behind the square roots
      {
        std::lock_guard<std::mutex> g(cx.mu);
        for (int i = 0; i < kSlots && ib < 0; i++)
          if (!cx.slots[i].busy) {
            cx.slots[i].busy = true;
            cx.slots[i].claimed = false;
            cx.slots[i].gen++;
            ib = i;
          }
      }
      Slot& A = cx.slots[ia];
      Slot* B = ib >= 0 ? &cx.slots[ib] : nullptr;
      auto body = [&]() -> int {
        HIP_TRY(hipSetDevice(cx.device));
        for (size_t lo = 0; lo < k; lo += kTrackerPass) {
          const size_t m = std::min(kTrackerPass, k - lo);
          const int r = tracker_pass(cx, A, B, trackers + 96 * lo, k_commitments + kRec * lo, proofs + 128 * lo, m,
                                     results + lo);
          if (r) return r;
        }
        return CURDLE_OK;
      };
      try {
        rc = body();
      } catch (const std::exception& e) {
        rc = fail(CURDLE_ENOMEM, "tracker check: %s", e.what());
      }
      if (rc) {  // nothing queued may outlive the slots' hold
        (void)hipStreamSynchronize(A.stream);
        if (B) (void)hipStreamSynchronize(B->stream);
      }
      if (B) release_slot(cx, ib);
      release_slot(cx, ia);
    }
  }
  if (rc != CURDLE_OK && results)  // "could not compute" must never read as a verdict
    for (size_t i = 0; i < k; i++) results[i] = rc;
  return rc;
}
