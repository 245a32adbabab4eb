// Host-side restatement of the reference's `whisk` package: the
// byte-level API the Ethereum Whisk SSLE spec consumes -- shuffle proofs over 124 trackers
// (curdleproof.Prove / Verify behind a fixed-size encoding) and the tracker opening proofs
// (a discrete-log-equality proof).  Same names, argument order and error behaviour as
// /root/reference/whisk/{whisk.go,types.go}; Go's (value, error) becomes a return value plus
// std::runtime_error for the error leg.  Every MSM underneath goes to the GPU.
#pragma once
#include <stdint.h>

#include <vector>

#include "curdleproofs.h"

namespace curdle {
namespace whisk {

static constexpr size_t G1POINT_SIZE = 48;                       // types.go:14
static constexpr size_t N = 128;                                 // :16
static constexpr size_t ELL = N - proto::N_BLINDERS;             // :17
static constexpr size_t TRACKER_PROOF_SIZE = 128;                // :19
static constexpr size_t WHISK_SHUFFLE_PROOF_SIZE = 4576;         // :20

struct WhiskTracker {  // types.go:73-76: the two points in gnark's compressed form
  uint8_t rG[G1POINT_SIZE];
  uint8_t krG[G1POINT_SIZE];
};
WhiskTracker NewWhiskTracker(const G1Affine& rG, const G1Affine& krG);  // :78

struct TrackerProof {  // types.go:99-103
  G1Affine A, B;
  alg::Scalar S;
  static TrackerProof FromBytes(const uint8_t buf[TRACKER_PROOF_SIZE]);  // :105
  void Serialize(uint8_t out[TRACKER_PROOF_SIZE]) const;                 // :119
};

// whisk.go:20 -- (true|false, nil) is the return value, (false, err) throws.
bool IsValidWhiskShuffleProof(const proto::CRS& crs, const std::vector<WhiskTracker>& preST,
                              const std::vector<WhiskTracker>& postST, const uint8_t proof[WHISK_SHUFFLE_PROOF_SIZE],
                              common::Rand& rand);
// Many shuffle proofs over one CRS at once (no reference counterpart; BASELINE config 5 is
// "1024 Whisk proofs"): every point of every proof and tracker set decoded by one GPU
// kernel, the proofs verified by proto::VerifyBatchCore (worker threads, one MSM per group
// of 32 proofs).  Returns the accept bits; a proof or tracker set that does not decode is
// rejected (bit 0) rather than raised.
struct ShuffleBatchItem {
  const WhiskTracker* preST;
  const WhiskTracker* postST;
  size_t n;
  const uint8_t* proof;  // WHISK_SHUFFLE_PROOF_SIZE bytes
};
std::vector<int> IsValidWhiskShuffleProofBatch(const proto::CRS& crs, const std::vector<ShuffleBatchItem>& items,
                                               common::Rand& rand, int nthreads);
// The steps of GenerateWhiskShuffleProof that handle nothing secret, shared with the constant-time form of the call
// (curdle_whisk_generate_shuffle_proof_ct, proto_api.cpp): the size rule (throws the reference's error unless n is ELL),
// the batched decoding of the 2n tracker points (throws getPoints' errors) and WhiskShuffleProof.Serialize (M, the
// serialised curdleproof, zero padding).
void CheckShuffleSize(size_t n);
void DecodeTrackers(const std::vector<WhiskTracker>& trackers, std::vector<G1Affine>* Rs, std::vector<G1Affine>* Ss);
void SerializeShuffleProof(const alg::Point& M, const uint8_t* body, size_t body_len, uint8_t proof_out[WHISK_SHUFFLE_PROOF_SIZE]);
// whisk.go:63 -- returns the post-shuffle trackers, writes the 4,576-byte proof.
std::vector<WhiskTracker> GenerateWhiskShuffleProof(const proto::CRS& crs, const std::vector<WhiskTracker>& preTrackers,
                                                    common::Rand& rand, uint8_t proof_out[WHISK_SHUFFLE_PROOF_SIZE]);
// GenerateWhiskShuffleProof for k pre-tracker arrays of one n, in lockstep (alg::Lockstep): per member the draws and their
// order are the single call's (GeneratePermutation, then GetFr, on the calling thread, member after member), all 2 n k
// tracker points go through ONE batched decode, then the members run the shuffle step, Prove and the serialisation on
// threads of their own, in groups of at most group_size, their device calls coalesced step by step.  With
// constant_time the members run under the two constant-time scopes and the step is proto::ShufflePermuteCommitSecret:
// curdle_whisk_generate_shuffle_proof_ct's results.  post_out: k n trackers; proofs_out: k proofs of
// WHISK_SHUFFLE_PROOF_SIZE.  Returns a code per member (CURDLE_OK; CURDLE_EINVAL for an n that is not ELL or a tracker that
// does not decode, nothing written for that member; a device call's code otherwise) and, in *what when it is given, the
// text of each failed member's error.  With constant_time and PROVER_FOLD_BASES set every member gets curdle_prove_ct's
// refusal where the single call meets it: behind the shuffle step and its draws, before any prover work.  Throws what
// the decode throws.
std::vector<int> GenerateWhiskShuffleProofBatch(const proto::CRS& crs, const std::vector<const WhiskTracker*>& preTrackers,
                                                size_t n, const std::vector<common::Rand*>& rands, bool constant_time,
                                                size_t group_size, WhiskTracker* post_out, uint8_t* proofs_out,
                                                alg::LockstepRun* run, std::vector<std::string>* what = nullptr);
// whisk.go:116
bool IsValidWhiskTrackerProof(const WhiskTracker& tracker, const uint8_t kComm[G1POINT_SIZE],
                              const uint8_t trackerProof[TRACKER_PROOF_SIZE]);
// whisk.go:149
void GenerateWhiskTrackerProof(const WhiskTracker& tracker, const alg::Scalar& k, common::Rand& rand,
                               uint8_t out[TRACKER_PROOF_SIZE]);
// ... with the blinder given instead of drawn: what the batched generator (csrc/tracker_api.hip) hands a
// member to whose transcript the device could not finish.  The same bytes as the call above for the same blinder.
void GenerateWhiskTrackerProofWithBlinder(const WhiskTracker& tracker, const alg::Scalar& k, const alg::Scalar& blinder,
                                          uint8_t out[TRACKER_PROOF_SIZE]);
// Does k own the tracker: k rG == krG as group elements, infinity included (computeTracker, whisk_test.go:98-104,
// read backwards).  Throws like GenerateWhiskTrackerProof if rG or krG does not decode (curve and subgroup).
bool IsOwnWhiskTracker(const WhiskTracker& tracker, const alg::Scalar& k);
// computeTracker, whisk_test.go:98-104: (r G, k r G), each a multiple of the generator from its FixedBase table.
WhiskTracker ComputeWhiskTracker(const alg::Scalar& k, const alg::Scalar& r);
// getKComm, whisk_test.go:106-109: k G in gnark's compressed form.
void WhiskKCommitment(const alg::Scalar& k, uint8_t out[G1POINT_SIZE]);

}  // namespace whisk
}  // namespace curdle
