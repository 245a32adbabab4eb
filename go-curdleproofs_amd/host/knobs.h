// The library's tunables ("knobs") in ONE table.  Every knob is read ONCE from the environment
// (CURDLE_<NAME>), the first time any knob is asked for -- in practice at curdle_init -- and never
// again: getenv beside a host program's setenv is not thread-safe, and a dozen of them on every MSM
// was what INTEGRATION.md said did not happen.  After that a value changes only through
// curdle_plan_override(name, value), the hook the tests and the measurement tools use to walk a
// knob through its range inside one process.
//
// Knobs whose experiments are closed were removed in round 4 (the measurements stay under
// profiles/): CURDLE_TWO_ROUNDS, CURDLE_TAIL_PRIO, CURDLE_SYNC_STREAMS, CURDLE_PRE_STREAMS,
// CURDLE_SEG_LEN_MIN, CURDLE_SORT_CHUNK, CURDLE_FUSE_SCAN_MAX, CURDLE_HOST_ONE_COPY (=
// CURDLE_HOST_CHUNKS=1), CURDLE_DECODE_PRIO, CURDLE_BATCH_EXTRA_PRODUCERS, CURDLE_NO_IFMA.
// Round 6, the same for the experiments rounds 4 and 5 closed: CURDLE_ROUND_LANES, CURDLE_SYNC_LANES, CURDLE_PIPE_LANES,
// CURDLE_REDUCE_BITS, CURDLE_GPU_COMBINE_MIN, CURDLE_SCAN (with k_scan_fused), CURDLE_FRONT, CURDLE_DIRECT_RESULTS,
// CURDLE_HOST_OVERLAP_MIN, CURDLE_HOST_SORT_STREAMS, CURDLE_HOST_GRADED, CURDLE_HOST_PATTERN.
#pragma once
#include <stddef.h>

namespace curdle {
namespace knobs {
enum Id {
  WINDOW_BITS,        // maximum window width c of every plan (4..16); unset: the size table
  SEG_LEN,            // sorted positions per accumulate lane
  REDUCE_SEG,         // buckets per bucket-reduce segment (power of two)
  SCATTER,            // 1: one-pass scatter, 2: two-pass wherever the shapes allow; unset: by size
  HOST_CHUNKS,        // chunks of a host-buffer MSM from 2^19 pairs (1..4)
  MAX_MSMS_PER_PASS,  // MSMs per pass of a batch beyond the bucket-slot limit
  MULTI_DEVICE_MIN,   // pairs from which curdle_msm_g1 spreads over the configured devices
  MAIN_STREAMS,       // accumulate streams of a context (1..4), read when the context is created
  TWO_KERNEL_MAX,     // one-shot decodings up to this many points take the two-kernel form
  QUAD_MAX_LANES,     // decode / scalar-multiplication kernels: quads up to this many lanes
  BATCH_CHUNK,        // batch verification: proofs per decode-ahead chunk
  BATCH_PRODUCERS,    // ... decode-ahead producer threads
  BATCH_GROUP,        // ... proofs settled per device accumulation
  DEVICE_ACC,         // 0: the verifier's accumulator on the host mirror
  HOST_DECODE,        // 1: point decoding on the host
  VERIFY_EAGER,       // 1: check points evaluated where the reference does
  VERIFY_TRACE,       // 1: per-phase timings of a verification on stderr
  PROVER_FOLD_BASES,  // 1: the prover folds its bases round by round like the reference
  ACC_PRIO,           // k_accumulate: the two waves of a SIMD take turns at high priority every 2^v x 10 ns (0: never; unset: 15 for synchronous calls from half a round of lanes)
  REDUCE_PRIO,        // wave priority (0..3) of k_reduce_segments / k_reduce_level; unset: 3 for pipelined calls, 0 for synchronous ones
  AUX_PRIO,           // wave priority (0..3) of the sort kernels, the conversion and the chunk fold; unset: 3 for pipelined calls, 0 for synchronous ones
  HOST_FOLD,          // 0: chunked host-buffer MSMs keep every chunk's fragments for the one reduction (no progressive folding)
  MAX_LARGE,          // test hook: caps the plan's large-bucket queue (max_large = min(plan, value), at least 1), so a test can overflow it
  BATCH_CHECKERS,     // checked batch verification: producer threads of the point check
  TRANSCRIPT_LANES,   // curdle_transcript_batch: members per wave (1..64); unset: by the batch's size
  GPU_PRELUDE,        // 1: the Whisk batch verifier takes its members' transcript preludes from curdle_transcript_batch, a chunk at a time; unset or 0: on the host
  TRACKER_DEVICE_HASH,  // the tracker batch's transcripts under CURDLE_TRACKER_HASH_DEFAULT: 1 hashed on the device, 0 on the host; unset: by the batch's size (tracker_api.hip)
  NORMALIZE_LANE_POINTS,  // k_g1_normalize: points per lane, 1 or 8 (any other value: as unset); unset: 8 beyond 65,536 points (normalize_kernels.hip)
  TRACKER_OWN_PAIRS,      // curdle_whisk_find_own_trackers: (key, tracker) quads per launch of k_tracker_own, rounded down to whole waves of 16, at least 16; unset: 2^18 (tracker_own_api.hip).  Under CURDLE_TRACKER_OWN_CONSTANT_TIME: (key, tracker) LANES per launch of k_tracker_own_ct, rounded down to a multiple of 256, at least 256; unset: 2^18
  FBASE_PASS,             // curdle_g1_fixed_base_mul_batch, curdle_whisk_compute_trackers_batch: scalars per pass (one launch of k_fbase_mul), rounded down to a multiple of 256, at least 256; unset: 2^20 (fbase_api.hip)
  TRANSCRIPT_SHEET,       // the batched transcripts' kernel: 1 always the sheet kernel (a state spread over lanes), 0 never; unset: the library's rule, and TRANSCRIPT_LANES set means the lane kernel (choose_transcript_kernel, transcript_api.hip)
  STREAM_PLAN,            // streams of pipelined MSMs, read when the context is created: 1 wide (a tail stream per slot), 2 compact (one tail stream: four busy streams); 0 or unset: compact below 16 hardware queues (GPU_MAX_HW_QUEUES), wide from there (stream_plan, msm_plan.hip)
  TRANSCRIPT_MAX_TRIES,   // test hook: lowers the batched transcripts' retry bound (draws of one challenge before the member is handed back with a status) to min(256, value) for value >= 1, so a test can reach the status byte; unset, 0 or above 256: 256.  The single calls ignore it (transcript_max_tries below)
  G1_MUL_CT_PASS,         // curdle_g1_scalar_mul_batch_ex / _device_ex under CURDLE_G1_MUL_CONSTANT_TIME: pairs per pass (one launch of k_g1_mul_ct), rounded down to a multiple of 256, at least 256; unset: 2^20 (g1_mul_ct_api.hip)
  PROVE_BATCH_GROUP,      // curdle_prove_batch, curdle_whisk_generate_shuffle_proof_batch: members proved in lockstep at a time, one thread each (1..64); unset, 0 or above 64: 64 (proto_api.cpp)
  PROVE_BATCH_PAIRS,      // test hook: lowers the (point, scalar) pairs or records from which a lockstep group's coalesced call is split by whole members, so a test can reach the split; unset or 0: the primitives' own limits (alg::Lockstep, algebra.cpp)
  PROVE_RESIDENT_TERMS,   // test hook: lowers the terms (pairs x chunks) up to which a funnel call under an alg::ResidentBasesScope goes to the resident tables, so a test can reach the old path beside the new one; unset, 0 or above 65,536: the primitive's own limit (algebra.cpp)
  CT_FINISH_DIVSTEPS,     // the finish of the constant-time MSM (k_msm_ct_finish / _seg): 1 always the builds whose exit inverts by division steps (k_msm_ct_finish_ds / _seg_ds, csrc/invert_ds.h), 0 never; unset: the library's rule (kCtFinishDivstepsDefault, csrc/msm_kernels.h).  The results are bit-identical either way
  COUNT
};
// The knob's value, or -1 if it is not set (every knob's valid values are >= 0).
long long get(Id id);
inline bool is_set(Id id) { return get(id) >= 0; }
// name: "WINDOW_BITS" or "CURDLE_WINDOW_BITS"; value < 0 unsets.  0 on success, -1 for an unknown name.
int set(const char* name, long long value);
const char* name(Id id);
// The retry bound of the batched transcripts under TRANSCRIPT_MAX_TRIES: what k_transcript_batch, k_transcript_sheet and
// curdle_transcript_batch_host compare a challenge's draws against (transcript::kMaxTries = 256 unless a test lowered it).
int transcript_max_tries();
}  // namespace knobs
}  // namespace curdle
