// Host-callable launchers of the gfx950 MSM kernels (msm_sort_kernels.hip, msm_accumulate_kernel.hip, msm_reduce_kernels.hip, msm_misc_kernels.hip).
// Internal to libcurdlemsm.so; the public surface is include/curdle_msm.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bls12_381.h"

namespace curdle {

static constexpr int kMaxWindows = 64;

// Pippenger decomposition shared by the k MSMs of one call (k = 1 for a single
// MSM).  The 255 scalar bits are cut into W windows of bits[w] bits each, as
// even as possible.  Windows below the top one are recoded into signed digits
// d in [-2^(b-1), 2^(b-1)] (2^(b-1) buckets: negating an affine point is free);
// the top window keeps its unsigned digit (2^b buckets), so no carry can leave
// it and no window is left with a handful of heavily loaded buckets.  Bucket
// slot `base[w] + m - 1` of an MSM holds the points whose |digit| in window w
// is m; the MSMs' slot ranges follow each other (NB slots each).
struct MsmPlan {
  uint32_t n;          // pairs of all MSMs of the call
  uint32_t k;          // scalar vectors (sorted MSMs) in the call
  uint32_t sets;       // base sets sharing every scalar vector's recoding and sort (1 but for curdle_msm_g1_multi)
  uint32_t kr;         // results = k * sets; result r = set * k + j
  uint32_t frag_stride;  // fragments reserved per base set
  uint32_t reduce_prio;  // s_setprio of the reduction kernels' waves (knob REDUCE_PRIO; 3 for pipelined calls)
  uint32_t aux_prio;     // s_setprio of the sort kernels' and the fold's waves (knob AUX_PRIO; experiment, 0 by default)
  uint32_t acc_prio;     // k_accumulate: log2 of the priority time slice in 10 ns ticks, 0 = no turns (knob ACC_PRIO)
  uint32_t n_max;      // pairs of the largest MSM
  int c;               // requested maximum window width
  int W;               // windows of the full decomposition
  int win_begin;       // windows [win_begin, win_end) are computed by this call
  int win_end;
  uint32_t NB;         // bucket slots per MSM over [win_begin, win_end)
  uint32_t NS;         // bucket-reduce segments per MSM = NB / seg
  uint32_t seg;        // buckets per running-sum segment
  uint32_t G;          // segment results tree-summed per partial = min(256, smallest nbkt / seg)
  uint32_t max_nbkt;   // largest nbkt[] in range
  uint32_t L;          // sorted positions per accumulate lane
  uint32_t max_small;  // buckets with more fragments than this are pre-merged by a block
  uint32_t max_large;  // capacity of the large-bucket queue
  uint32_t chunk;      // pairs per sort block
  uint32_t gpu_combine;  // 1: window sums combined on the GPU (large batches), 0: on the host
  uint32_t fuse_scan;    // the bucket-slot scans: 0 six launches (multi-block; L = 1 only), 2 k_scan_one (one block, up to 32,768 slots), 3 k_scan_chain (one launch, any size)
  uint32_t glv;          // 1: scalars split with the endomorphism (bases must be in G1); 0: 255-bit scalars whole, any curve point
  uint32_t two_level;    // 1: the scatter runs in two passes (coarse bins, then buckets): single large MSMs
  // 1: the k MSMs of the call have n / k terms each and share ONE base array of that many records (the device accumulator's
  // member form): the scatter writes a term's index inside its own MSM, which is the record every member gathers
  uint32_t shared_bases;
  // The bucket reduction without a scalar multiple (single MSMs; k_reduce_segments / k_reduce_groups):
  // a window's sum_b (b + 1) B_b leaves the GPU as `nout` points with bit positions, which the host's
  // Horner pass over the windows takes in like window sums.  Then G <= 16 (one wave's quads).
  uint32_t reduce_bits;  // 1: that form; 0: k_bucket_reduce_quad + window sums (batches, shared-scalar calls)
  uint32_t lg_seg;       // log2(seg)
  uint32_t lgG;          // log2(G)
  uint32_t NG;           // segment groups per MSM = NS / G
  uint32_t nout;         // points per window handed to the host = 2 + log2(max_nbkt / seg): sum S | - | X_0 ..
  uint8_t bits[kMaxWindows];    // width of window w
  uint16_t shift[kMaxWindows];  // bit offset of window w
  uint32_t nbkt[kMaxWindows];   // bucket slots of window w
  uint32_t base[kMaxWindows];   // first slot of window w inside an MSM's NB slots
  uint32_t merge_blocks;        // (host only, last so that no field the kernels read moves) k_merge_large's grid at most
};

// Sizes of the internal (fp28.h) point formats, for workspace allocation.
static constexpr size_t kX28Bytes = 224;
static constexpr size_t kA28Bytes = 128;  // stride of the internal point array: a 112-byte d28::A28 padded to one 128-byte line

// Device workspace, laid out by msm_enqueue.hip.  nb = k * NB bucket slots.
struct MsmWorkspace {
  const uint32_t* offsets;  // [k + 1]   first pair of each MSM (device)
  uint32_t* counts;   // [nb]      points per bucket
  uint32_t* starts;   // [nb + 1]  exclusive prefix of counts; [nb] = number of sorted entries
  uint32_t* cursor;   // [nb]      scatter cursors (copy of starts)
  uint32_t* fragcnt;  // [nb]      accumulation fragments per bucket
  uint32_t* foff;     // [nb + 1]  exclusive prefix of fragcnt
  uint32_t* blocksum; // [1024]    scan scratch
  uint32_t* large;    // [max_large] buckets queued for merge_large
  uint32_t* nlarge;   // [1]
  uint32_t* mdone;    // [sets][max_large] k_merge_large: finished chunks per queue entry (zero between calls)
  uint32_t* digits;   // [nw][n]   |digit| | sign<<31, window-major
  uint32_t* sorted;   // [nw * n]  pair index | sign<<31, grouped by bucket
  uint32_t* tmp;      // [nw * n]  two-level scatter: entries grouped by coarse bin (null otherwise)
  uint32_t* ccur;     // [coarse_words(nw)] two-level sort: the bins' cursors, their packed starts, and the copies of the coarse counts
  void* points28;     // [n]       input points in internal form (d28::A28, 112 B)
  void* frags;        // [nb + lanes + 1]  d28::X28 (224 B)
  void* partials;     // [k * NS / G]      d28::X28, one per group of G bucket-reduce lanes
  void* winsums28;    // [k][nw]           d28::X28 (large batches: combined on the GPU)
  G1XYZZ* winsums;    // [k][nw]   gnark-form XYZZ, canonical coordinates (host combine)
  G1XYZZ* results;    // [k]       XYZZ results of a batched call, gnark form (normalised by the host)
  // k_scan_chain (MsmPlan::fuse_scan == 3): the chain words [2][1024] (zero when allocated, never cleared again), the
  // ticket counter behind them, the count it stood at before this launch and this launch's epoch (never 0)
  unsigned long long* chain;
  uint32_t* chain_ticket;
  // a word of pinned host memory, set on every call: a kernel that cannot finish the call correctly raises it (a plain
  // store of one of the kErr codes below) and finish_slot fails the call
  uint32_t* host_err;
  uint32_t chain_base, chain_epoch;
};
static constexpr uint32_t kErrScanGaveUp = 1;     // k_scan_chain: a wait for an earlier tile gave up
static constexpr uint32_t kErrQueueOverflow = 2;  // k_merge_large: more buckets over max_small than the large-bucket queue holds
uint32_t scan_chain_tiles(uint32_t nb);  // blocks (= tickets) one k_scan_chain launch over nb slots takes
size_t scan_chain_bytes();               // bytes behind MsmWorkspace::chain (the ticket counter at the end)

// The fragment lists the bucket reduction folds in: one per CHUNK of an MSM whose pairs were
// accumulated in several pieces over the same plan (host-buffer calls: a piece is accumulated
// while the next one crosses PCIe; msm_host_chunks.hip run_host_chunked) -- the pieces share the bucket
// slots, so their fragments meet in ONE reduction instead of one reduction per piece.
static constexpr int kMaxFragSources = 4;
struct FragSources {
  const void* frags[kMaxFragSources];        // d28::X28
  const uint32_t* foff[kMaxFragSources];     // [nb + 1]
  const uint32_t* fragcnt[kMaxFragSources];  // [nb]
  uint32_t n;
};

// Words of MsmWorkspace::ccur for nw windows.  Its tail (the coarse counts) must be ZERO before a call's first launch;
// the kernels leave it zero again (msm_enqueue.hip clears the buffer when it is made and after a failed call).
size_t coarse_words(uint32_t nw);

// The device accumulator's job as the fused front of a small call sees it (launch_dacc_front): device pointers into the
// uploaded job (checks | pool | loose points | loose scalars) and the counts.
struct DaccFront {
  const void* d_checks;
  const void* d_pool;
  const void* d_extra_points;
  const void* d_extra_scalars;
  void* d_scalars_out;  // [n_crs + n_inst + n_extra] fr.Elements, or null
  uint32_t n_checks, pool_len, n_crs, n_inst, n_extra;
};

// The member form of the device accumulator's job (launch_dacc_scalars_members): device pointers into the uploaded job
// (checks grouped by member | pool | loose points | loose scalars | first check of each member, n_members + 1 words |
// member of each loose pair) and the counts.
struct DaccMembers {
  const void* d_checks;
  const void* d_member_first;
  const void* d_pool;
  const void* d_extra_scalars;
  const void* d_extra_member;
  uint32_t n_checks, pool_len, n_crs, n_inst, n_extra, n_members;
};

// Every launcher enqueues on `stream` and returns the launch status.
// n gnark affine points -> internal form at d_out28 (kA28Bytes apart), outside a plan: the device accumulator
// converts its resident base sets once and per-verification points as they arrive.
hipError_t launch_convert_points_raw(const void* d_points, uint32_t n, void* d_out28, hipStream_t stream, uint32_t prio = 0);
// chunked host-buffer calls: this chunk's fragments into the per-bucket running sums (sums: NB points, meta: 2 * NB words)
hipError_t launch_fold_fragments(const MsmPlan& p, const MsmWorkspace& ws, void* sums, void* meta, bool first, hipStream_t stream);
hipError_t launch_digits(const MsmPlan& p, const MsmWorkspace& ws, const void* d_scalars, hipStream_t stream);
// conversion of npts points into ws.points28 and the recoding in ONE launch (small calls; not for two-level plans)
hipError_t launch_front(const MsmPlan& p, const MsmWorkspace& ws, const void* d_points, uint32_t npts, const void* d_scalars,
                        hipStream_t stream);
// loose-base conversion + slot scalars + recoding in ONE launch (small device-accumulator calls; not two-level plans)
void dacc_count_build(int which);  // dacc_kernels.hip: 0 / 1 the fused front staged / not, 2 / 3 k_dacc_scalars<true> / <false>
hipError_t launch_dacc_front(const MsmPlan& p, const MsmWorkspace& ws, const DaccFront& f, hipStream_t stream);
hipError_t launch_hist(const MsmPlan& p, const MsmWorkspace& ws, hipStream_t stream);
hipError_t launch_scan(const MsmPlan& p, const MsmWorkspace& ws, hipStream_t stream);
hipError_t launch_scatter(const MsmPlan& p, const MsmWorkspace& ws, hipStream_t stream);
hipError_t launch_accumulate(const MsmPlan& p, const MsmWorkspace& ws, hipStream_t stream);
hipError_t launch_merge_large(const MsmPlan& p, const MsmWorkspace& ws, hipStream_t stream);
// extra: fragment lists of earlier chunks (same plan) to fold in besides ws's own; may be null
hipError_t launch_bucket_reduce(const MsmPlan& p, const MsmWorkspace& ws, hipStream_t stream, const FragSources* extra = nullptr);
hipError_t launch_window_sum(const MsmPlan& p, const MsmWorkspace& ws, hipStream_t stream);
// The reduce_bits form: segments -> groups (ws.partials, room for 2 x kr x NG x (2 + lgG) + 2 points), groups ->
// nout points per window (ws.winsums), in one or two levels.
hipError_t launch_reduce_segments(const MsmPlan& p, const MsmWorkspace& ws, hipStream_t stream, const FragSources* extra = nullptr);
hipError_t launch_reduce_groups(const MsmPlan& p, const MsmWorkspace& ws, hipStream_t stream);
// Bit position (relative to the window's shift) of output point `slot` of window w in the reduce_bits
// form, or -1 for a slot the window does not use (it holds infinity).  Host and device agree on this.
int reduce_bits_position(const MsmPlan& p, int w, uint32_t slot);
// Batched calls only: Horner over each MSM's window sums, one quad per MSM.
hipError_t launch_combine(const MsmPlan& p, const MsmWorkspace& ws, hipStream_t stream);

// P_i = p0 + i*Q for i < n (n <= 2^27); d_table holds 27 affine points 2^j * Q.
hipError_t launch_synth_walk(const G1Affine* d_table, const G1Affine& p0, uint32_t n, void* d_out, hipStream_t stream);

// Element-wise primitive test (curdle_selftest_op); all pointers are device memory.
// ONE table says what an operation reads and writes per element and how many lanes it takes: the host
// wrapper sizes its buffers from it, the launcher its grid, the kernel its indexing, and the Python
// binding asks for it (curdle_selftest_shape) -- an operation missing from any of the four used to
// fall through to another operation's widths (the r3a abort).
struct SelftestOp {
  uint32_t in_words;   // 32-bit words read per element
  uint32_t out_words;  // ... written per element
  uint32_t lanes;      // lanes per element: 4 for the lane-distributed (quad) operations
};
static constexpr int kSelftestOps = 17;
static constexpr SelftestOp kSelftestTable[kSelftestOps] = {
    {24, 12, 1}, {24, 12, 1}, {24, 12, 1}, {24, 12, 1},  // 0..3  Fp mul / add / sub / sqr
    {16, 8, 1},                                           // 4     Fr Montgomery -> canonical
    {96, 48, 1}, {96, 48, 1}, {96, 48, 1},                // 5..7  XYZZ madd / add / dbl, one lane
    {96, 48, 4}, {96, 48, 4}, {96, 48, 4},                // 8..10 add / dbl / small multiple on quads
    {8, 10, 1},                                           // 11    the GLV split
    {24, 26, 1},                                          // 12    a base into the MSM's curve and back (+ the two bound flags)
    {60, 16, 1},                                          // 13    fp28.h field operations on raw limbs
    {116, 56, 1},                                         // 14    fp28.h point operations on raw limbs, one lane
    {116, 56, 4},                                         // 15    quad28.h point operations on raw limbs
    {116, 60, 1},                                         // 16    the constant-time G1 layer on raw limbs (selftest_ct_kernels.hip)
};
// Operations 13..16 read and write the internal 14 x 28-bit limbs directly (no from_gnark / to_gnark on
// either side).  Word 0 of an element selects the primitive; a selector outside these counts is refused
// by the host before anything is copied or launched.  Operation 16 has a kernel per selector: all elements of
// one call share the selector, its mask words are 0 or all ones and its walk has 1..255 steps, or the host refuses.
static constexpr uint32_t kSelftestFieldSels = 26;  // op 13
static constexpr uint32_t kSelftestPointSels = 6;   // op 14
static constexpr uint32_t kSelftestQuadSels = 4;    // op 15
static constexpr uint32_t kSelftestCtSels = 12;     // op 16
// hipErrorInvalidValue for an op outside the table, and for op 16, which has its own launcher (nothing is launched).
hipError_t launch_selftest(int op, const uint32_t* d_in, size_t n, uint32_t* d_out, hipStream_t stream);
// selftest_ct_kernels.hip: op 16, the kernel of selector `sel` over n elements of the table's widths.
hipError_t launch_selftest_ct(uint32_t sel, const uint32_t* d_in, size_t n, uint32_t* d_out, hipStream_t stream);

// decode_kernels.hip: n compressed G1 points (48 B each) -> n gnark affine points (24 u32
// each) + one CURDLE_DECODE_* status byte per point.
hipError_t launch_g1_decompress(const uint8_t* in, uint32_t n, int subgroup_check, uint32_t* out, uint8_t* status,
                                hipStream_t stream);

// check_kernels.hip: n gnark affine points IN MEMORY (24 u32 each) -> one CURDLE_DECODE_* status byte per point:
// infinity (all words zero), a coordinate >= p, off the curve, and with subgroup_check outside the prime-order subgroup.
hipError_t launch_g1_check_affine(const uint32_t* pts, uint32_t n, int subgroup_check, uint8_t* status, hipStream_t stream);
hipError_t launch_g1_check_jac(const uint32_t* pts, uint32_t n, int subgroup_check, uint8_t* status, hipStream_t stream);

// transcript_kernels.hip: one compiled transcript program (host/transcript_batch.h) over k members, `mpw` members
// on the first lanes of every wave.  Device pointers; rows, states and challenges are 8-byte aligned.
namespace transcript {
struct TapeCtl;
struct TapeBlock;
}  // namespace transcript
struct TranscriptArgs {
  const transcript::TapeCtl* ctl;
  const transcript::TapeBlock* pool;
  const uint64_t* data;   // k rows of row_words u64 (transcript::TapeRowWords)
  const uint64_t* init;   // member m starts from init + m * init_stride: 25 state lanes
  uint64_t* challenges;   // k x n_challenges x 4
  uint64_t* states;       // k x 26, or null
  uint8_t* status;        // k
  uint64_t tail;          // pos | pos_begin << 8 | cur_flags << 16 after the program
  uint32_t n_ctl, row_words, init_stride, k, mpw, n_challenges;
  uint32_t sheet;         // 1: k_transcript_sheet (transcript_sheet_kernels.hip), two members per wave; `mpw` is then unused
  uint32_t max_tries;     // draws of one challenge before status 1; launch_transcript_batch fills it, never a caller
};
// Kernel and geometry (`sheet`, `mpw`) are the caller's, from choose_transcript_kernel (transcript_api.hip); the launch
// fills `max_tries` (knobs::transcript_max_tries: 256 unless test hook TRANSCRIPT_MAX_TRIES lowered it) and takes the
// kernels' build that reads it only then -- at 256 the build with the constant, the parent's code -- dispatches on
// `sheet` and counts the members each kernel hashed (transcript_path_counts: lane kernel | sheet kernel).
hipError_t launch_transcript_batch(const TranscriptArgs& args, hipStream_t stream);
hipError_t launch_transcript_sheet(const TranscriptArgs& args, hipStream_t stream);
void transcript_path_counts(unsigned long long out[2]);
// transcript_sheet_kernels.hip: `reps` dependent Keccak-f[1600] on each of n states of 25 u64 (device pointers), by
// keccak_f1600_dev with one state per wave (sheet = 0) or by sheet_keccak_f1600 with two (sheet = 1).
hipError_t launch_keccak_permute(const uint64_t* in, uint64_t* out, uint32_t n, uint32_t reps, int sheet, hipStream_t stream);

// The subgroup test straight from the n compressed records, without their square roots (so it
// can run beside launch_g1_decompress(..., subgroup_check = 0, ...)): sub[i] = 0 iff record i,
// if it decodes to a point at all, is not in the prime-order subgroup.
hipError_t launch_g1_subgroup_from_bytes(const uint8_t* in, uint32_t n, uint8_t* sub, hipStream_t stream);

// group_kernels.hip: out[i] = addends[i] + scalars[i or 0] * points[i] as gnark-format XYZZ
// (ZZ = 0 for infinity); points / addends gnark affine (addends may be null), scalars
// Montgomery fr.Elements.
// dacc_kernels.hip: the slot scalars of the device accumulator (checks: curdle_dacc_check[], pool: fr.Elements).
hipError_t launch_dacc_scalars(const void* d_checks, uint32_t n_checks, const void* d_pool, uint32_t pool_len, uint32_t n_crs,
                               uint32_t n_inst, void* d_out, hipStream_t stream);

// ... one row of n_crs + n_inst + n_extra scalars per member (d_out: n_members rows back to back), loose pairs included.
hipError_t launch_dacc_scalars_members(const DaccMembers& m, void* d_out, hipStream_t stream);
void dacc_count_members(int which, unsigned long long by);  // curdle_stat_dacc_members' three counters

hipError_t launch_scalar_mul_batch(const void* points, const void* scalars, int shared_scalar, const void* addends,
                                   uint32_t n, void* out_xyzz, hipStream_t stream);

// tracker_kernels.hip: the two equations of n Whisk tracker proofs (whisk.go:136-146), one byte
// per member.  points: 5 n gnark affine records (rG, krG, kG, A, B per member) with their
// CURDLE_DECODE_* status bytes; scalars: s, c per member, canonical, 8 little-endian words each;
// skip[i] != 0 marks a member not to check; gen: the G1 generator.
static constexpr uint8_t kTrackerReject = 0, kTrackerAccept = 1, kTrackerError = 2;  // error: a record did not decode, or skip
hipError_t launch_tracker_check(const void* points, const uint8_t* status, const void* scalars, const uint8_t* skip,
                                const G1Affine& gen, uint32_t n, uint8_t* out, hipStream_t stream);
// The device-hashed form's two small kernels.  Gather: n members of the caller's three arrays (96, 48 and 128 bytes
// each, any alignment) -> rec: 5 n compressed records (rG, krG, kG, A, B); rows: n transcript rows of
// TapeRowWords(288) u64 (8 zero bytes | kG g1Gen krG rG A B | 8 zero bytes; gen: the generator's 48-byte encoding,
// 8-byte aligned); scalars + 16 i: S as eight little-endian words (zero where S >= r) and skip[i] = (S >= r).
// Challenge: the transcript kernel's 32 big-endian bytes of member i -> scalars + 16 i + 8; a member with a
// non-zero tr_status gets zero scalars and skip[i] = 1.  rec, rows, scalars and challenges are 16-byte aligned.
hipError_t launch_tracker_gather(const uint8_t* trackers, const uint8_t* k_comms, const uint8_t* proofs, const void* gen,
                                 uint32_t n, void* rec, void* rows, void* scalars, uint8_t* skip, hipStream_t stream);
hipError_t launch_tracker_challenge(const void* challenges, const uint8_t* tr_status, uint32_t n, void* scalars,
                                    uint8_t* skip, hipStream_t stream);

// tracker_combine_kernels.hip: the scalars of the combined tracker check, one lane per member.  From the records'
// status bytes and subgroup verdicts, s | c at sc + 16 i (launch_tracker_challenge's layout) and skip, member i's five
// MSM scalars (Montgomery fr.Elements, for rG krG kG A B: sigma s, sigma c, rho c, -rho, -sigma; all zero for an
// excluded member) go to scalars + 40 i words, and block b's sum of rho s mod r to pair 5 n + b, whose point (the
// generator) the kernel writes to points + 96 (5 n + b) bytes.  scalars and points hold 5 n + tracker_combine_blocks(n)
// pairs, 16-byte aligned.  seed: the first nine words of the SHAKE256 rate block "curdle/tracker-combine/v1" | seed |
// le64(0) | 0x1f; `first` is the index in the call of the pass's member 0.
struct TrackerCombineSeed {
  uint64_t w[9];
};
uint32_t tracker_combine_blocks(uint32_t n);
hipError_t launch_tracker_combine(const uint8_t* status, const uint8_t* sub, const void* sc, const uint8_t* skip,
                                  const TrackerCombineSeed& seed, uint64_t first, uint32_t n, const G1Affine& gen,
                                  void* scalars, void* points, hipStream_t stream);

// tracker_own_kernels.hip: does key j own tracker t, one (key, tracker) pair per quad and 64 trackers of ONE key per
// block, so that every tested key bit is wave-uniform.  points: decoded records, rG_t at 2 t and krG_t at 2 t + 1, with
// their CURDLE_DECODE_* status bytes (subgroup test included); keys: Montgomery fr.Elements, 16-byte aligned.  One
// launch covers trackers [t0, t0 + cnt) of keys [key0, key0 + nkeys), nkeys <= 65,535 (a grid dimension), and writes
// out[key * stride + t] = CURDLE_TRACKER_NOT_OWNED / _OWNED / _BAD (a status beyond CURDLE_DECODE_INFINITY: no chain).
hipError_t launch_tracker_own(const void* points, const uint8_t* status, const void* keys, uint32_t t0, uint32_t cnt,
                              uint32_t key0, uint32_t nkeys, uint8_t* out, size_t stride, hipStream_t stream);
// tracker_own_ct_kernels.hip: the same verdicts over the same arguments by the constant-time twin, one LANE per (key,
// tracker) pair, flattened (lane g: key0 + g / tc, t0 + g % tc) so that the key's address is made of the lane index;
// 255 double-and-always-add steps on rG and a projective equality test against krG, no inversion.  One launch covers
// trackers [t0, t0 + tc) of keys [key0, key0 + kc), tc kc <= 2^31.  Neither the instruction stream nor the address
// stream depends on the keys.
hipError_t launch_tracker_own_ct(const void* points, const uint8_t* status, const void* keys, uint32_t t0, uint32_t tc,
                                 uint32_t key0, uint32_t kc, uint8_t* out, size_t stride, hipStream_t stream);

// compress_kernels.hip: n points in memory -> n x 48 bytes of gnark's compressed encoding (G1Affine.Bytes), one lane
// per point.  form kCompressJac: gnark G1Jac, 144 bytes each (Z = 0: infinity); kCompressXyzz: G1XYZZ in gnark limbs,
// 192 bytes each, as launch_scalar_mul_batch writes it (ZZ = 0: infinity).  `in` and `out` may have any alignment.
// kCompressAffine (internal: no public CURDLE_G1_FORM_* value): gnark G1Affine records, 96 bytes each, as
// launch_g1_normalize writes them (both coordinates zero: infinity); nothing is inverted.
static constexpr int kCompressJac = 0, kCompressXyzz = 1, kCompressAffine = 2;
hipError_t launch_g1_compress(const void* in, int form, uint32_t n, uint8_t* out, hipStream_t stream);

// fbase_kernels.hip: out[i] = (scalars[i] * multipliers[i] mod r) * P as G1XYZZ in gnark limbs (all zero for
// infinity), one lane per scalar, at most 32 mixed additions from table28: the 8,160 multiples d * 2^(8 w) * P of
// curdle_host_fixed_base_table, entry w * 255 + d - 1, as launch_convert_points_raw converts them but kA28Bytes apart
// (P's records only).  scalars / multipliers: Montgomery fr.Elements, multiples of 16; multipliers may be null.
// READS TABLE ENTRIES AT ADDRESSES CHOSEN BY SCALAR DIGITS.
static constexpr uint32_t kFbaseEntries = 32 * 255;
hipError_t launch_fbase_mul(const void* table28, const void* scalars, const void* multipliers, uint32_t n, void* out_xyzz,
                            hipStream_t stream);
// fbase_ct_kernels.hip: the same function of the same arguments over the same table, as 64 unsigned 4-bit windows:
// every window reads all 15 of its multiples (a subset of table28) at addresses made of the window alone, selects by
// mask and always adds.  Neither the instruction stream nor the address stream depends on scalars or multipliers.
hipError_t launch_fbase_mul_ct(const void* table28, const void* scalars, const void* multipliers, uint32_t n, void* out_xyzz,
                               hipStream_t stream);

// g1_mul_ct_kernels.hip: out_affine[i] = scalars[i or 0] * points[i * point_stride], the constant-time twin of
// launch_scalar_mul_batch without addends, one lane per pair and 255 double-and-always-add steps.  points: gnark
// G1Affine records ((0, 0): infinity), point_stride records apart; scalars: Montgomery fr.Elements below r; the result
// is n normalised gnark G1Affine records, 96 bytes apart (the lane inverts its own denominator), and out_affine may be
// points when point_stride is 1.  Every pointer is a multiple of 16.  Neither the instruction stream nor the address
// stream depends on the scalars.
hipError_t launch_g1_mul_ct(const void* points, uint32_t point_stride, const void* scalars, int shared_scalar, uint32_t n,
                            void* out_affine, hipStream_t stream);

// msm_ct_kernels.hip: the constant-time MSM, sum_i scalars[i] * points[i], in three steps over a workspace of X28 terms
// (kMsmCtTermBytes each, 16-byte aligned).  Neither the instruction stream nor the address stream of any of them
// depends on the scalars or on the terms.
//   launch_msm_ct_walk: term[i] = scalars[i] * points[i] for i < n by `bits` (1...255, public) double-and-always-add
//     steps, one lane per pair; scalars are Montgomery fr.Elements (kMsmCtScalarFr) or plain uint32 (kMsmCtScalarU32);
//     a scalar with a bit at or above `bits` ORs 1 into *status (which the caller zeroes first).
//   launch_msm_ct_sum: folds term[0, m) in place in the fixed fold-in-half order (h = ceil(m / 2), term[i] += term[i + h]
//     for i < m - h, m <- h), one launch per level above kMsmCtSumTail terms and one block for the rest, which then
//     normalises term[0] and writes out40: the 36 words of curdle_msm_g1's result, *status behind them, three words untouched.
//   launch_msm_ct_sum_seg: the same sum over k segments of one term array, 1 <= k <= 65,535.  seg: k device records
//     (begin, count), two uint32 each; counts: the same counts on the host, which decide how many level launches there
//     are (k_g1_sum_ct_seg, one per level while any segment is above kMsmCtSumTail; *levels receives the number).  One
//     block per segment then finishes it as launch_msm_ct_sum does and writes 36 words at out + 36 j (the infinity
//     encoding for an empty segment); *status follows the k results.  Per segment the order of additions is
//     launch_msm_ct_sum's on that segment alone.
//   launch_g1_permute_ct: out[h n + i] = in[h n + perm[i]] for i < n, h < halves, 96-byte records, perm secret: every
//     lane reads all n records of its half.  out must not overlap in.
//   launch_fr_permute_ct: out[i] = in[perm[i]] for i < n over 32-byte records by the same gather (an entry at or above n:
//     a zero record).  out must not overlap in.
//   launch_permute_ct_seg: k gathers of one n in ONE launch: out[j n + i] = in[j n + perm[j n + i]] for i < n, j < k, over
//     records of record_bytes = 32 or 96; an entry at or above n gives a zero record, never another member's.  n and k
//     at most 65,535 each.  out must not overlap in.
enum { kMsmCtScalarFr = 0, kMsmCtScalarU32 = 1 };
static constexpr uint32_t kMsmCtTermBytes = 224;
static constexpr uint32_t kMsmCtSumTail = 512;
hipError_t launch_msm_ct_walk(const void* points, const void* scalars, int scalar_form, uint32_t bits, uint32_t n, void* term,
                              uint32_t* status, hipStream_t stream);
hipError_t launch_msm_ct_sum(void* term, uint32_t m, const uint32_t* status, void* out40, hipStream_t stream);
hipError_t launch_msm_ct_sum_seg(void* term, const void* seg, const uint32_t* counts, uint32_t k, const uint32_t* status,
                                 void* out, uint32_t* levels, hipStream_t stream);
hipError_t launch_g1_permute_ct(const void* in, const uint32_t* perm, uint32_t n, uint32_t halves, void* out, hipStream_t stream);
hipError_t launch_fr_permute_ct(const void* in, const uint32_t* perm, uint32_t n, void* out, hipStream_t stream);
hipError_t launch_permute_ct_seg(const void* in, const uint32_t* perm, uint32_t n, uint32_t k, uint32_t record_bytes, void* out,
                                 hipStream_t stream);
// The finish of launch_msm_ct_sum and launch_msm_ct_sum_seg exists in two builds with the same words out: the exit's
// inversion on the Fermat chain (k_msm_ct_finish, k_msm_ct_finish_seg) or on division steps (k_msm_ct_finish_ds,
// k_msm_ct_finish_seg_ds).  Knob CT_FINISH_DIVSTEPS chooses (1 / 0); unset, the library's rule is this constant: true since
// the measurement of round 37 put the _ds finish below the Fermat one by more than the sum of both arms' spreads at 1 x 256
// and 4,096 x 16 terms and in a handle Prove at ell = 124 (profiles/r37_invert_ds.json).
// msm_ct_finish_launches: out[0] finish launches on division steps, out[1] on Fermat.
static constexpr bool kCtFinishDivstepsDefault = true;
void msm_ct_finish_launches(unsigned long long out[2]);

// fp_invert_kernels.hip: out[i] = in[i]^-1 in Fp for i < n <= kFpInvertPass, 0 -> 0, one lane per element, by division
// steps (invert_ds.h) or, fermat != 0, by the exponent chain of invert28.h: the same words.  Items are gnark fp.Elements
// (48 bytes, canonical in and out) or, raw != 0, the 14 limbs of fp28.h (56 bytes; normalised and below 2p in, canonical
// out).  An item out of range ORs 1 into *status (which the caller zeroes first) without a branch.  in and out are
// multiples of 16 and out may be in.  Neither the instruction stream nor the address stream depends on the elements.
static constexpr uint32_t kFpInvertPass = 1u << 20;
hipError_t launch_fp_invert(const void* in, uint32_t n, void* out, int fermat, int raw, uint32_t* status, hipStream_t stream);

// msm_ct_bases_kernels.hip: the constant-time MSM over a resident PUBLIC base set, the walk split into chunks of
// chunk_bits (1...64) bits.
//   launch_ct_bases_shift: staging_xyzz[(j - 1) n + i] = 2^(chunk_bits j) points[i] for 1 <= j < chunks as gnark-form
//     G1XYZZ records (192 bytes, ZZ = 0: infinity), what launch_g1_normalize's kNormalizeXyzz reads; points are gnark
//     G1Affine records.  Public arithmetic.
//   launch_msm_ct_walk_rows: term[p Cb + j] = (chunk j of scalars[p]) * table_s[j size_s + rows[p] - first_s] for p < n
//     and j < Cb = ceil(bits / chunk_bits), s the set whose range [first_s, first_s + size_s) holds rows[p]:
//     launch_msm_ct_walk's walk, status word and term records over chunk_bits steps (the top chunk:
//     bits - chunk_bits (Cb - 1)).  sets: up to four tables of Cb or more rows of size_s gnark G1Affine records each, all
//     at one chunk_bits, laid behind each other in the index space (CtRowSets: a kernel argument by value); rows: n
//     device uint32 below the sets' total (public; the caller checked them); scalars: Montgomery fr.Elements.
//     n Cb <= 2^31.
static constexpr int kCtRowSetsMax = 4;
struct CtRowSets {
  const void* table[kCtRowSetsMax];  // null for an empty set: never read
  uint32_t size[kCtRowSetsMax];      // records a row of the set's table holds
  uint32_t first[kCtRowSetsMax];     // B_s = size_0 + ... + size_(s-1); the total for s beyond the call's sets
};
hipError_t launch_ct_bases_shift(const void* points, uint32_t n, uint32_t chunk_bits, uint32_t chunks, void* staging_xyzz,
                                 hipStream_t stream);
hipError_t launch_msm_ct_walk_rows(const CtRowSets& sets, const uint32_t* rows, const void* scalars, uint32_t chunk_bits,
                                   uint32_t bits, uint32_t n, void* term, uint32_t* status, hipStream_t stream);

// normalize_kernels.hip: n points in memory -> n gnark G1Affine records (96 bytes; infinity: all zero), ONE inversion
// per wave of 64 lanes with 1 or 8 points each (Montgomery's trick over a wave scan).  The forms are those of
// launch_g1_compress; a denominator (Z, or ZZ ZZZ) that is 0 mod p is infinity.  `in` and `out` are multiples of 16
// and do not overlap.  *groups (may be null): the inversion groups (waves) of the launch.
static constexpr int kNormalizeJac = 0, kNormalizeXyzz = 1;
// Up to this many points every lane takes one (the launch is at most one wave per SIMD of the chip's 1,024 and the
// chain of ONE group is what the caller waits for); beyond it eight.  Knob NORMALIZE_LANE_POINTS (1 or 8) overrides.
static constexpr uint32_t kNormalizeWideMin = 65536;
hipError_t launch_g1_normalize(const void* in, int form, uint32_t n, void* out, hipStream_t stream, uint32_t* groups);

// tracker_prove_kernels.hip: the small kernels of the batched tracker-proof generator (tracker_api.hip), n members.
// Pairs: the 3 n (point, scalar) pairs of one launch_scalar_mul_batch, (G, k_i) | (G, b_i) | (rG_i, b_i): `decoded`
// holds the 2 n decoded tracker records (rG_i, krG_i; a record that did not decode is all zero, which the chain reads
// as infinity), scalars + 8 i the Montgomery k_i, scalars + 8 (n + i) the b_i, which are copied to 8 (2 n + i).
hipError_t launch_tracker_prove_pairs(const void* decoded, const G1Affine& gen, uint32_t n, void* points, void* scalars,
                                      hipStream_t stream);
// Rows: member i's transcript row, 8 zero bytes | kG g1Gen krG rG A B | 8 zero bytes (launch_tracker_gather's layout),
// from its tracker record (96 bytes: rG | krG) and the compressed results, kG_i at comp + 48 i, A_i at 48 (n + i),
// B_i at 48 (2 n + i).  Every pointer is 8-byte aligned.
hipError_t launch_tracker_prove_rows(const void* trackers, const void* comp, const void* gen, uint32_t n, void* rows,
                                     hipStream_t stream);
// Response: proofs + 128 i = A_i | B_i | s_i with s = b - c k in Fr, 32 big-endian bytes; c: the transcript kernel's
// 32 big-endian bytes per member.  A member with a record whose status is beyond CURDLE_DECODE_INFINITY, or which
// decoded outside the subgroup (sub = 0), gets 128 zero bytes.
hipError_t launch_tracker_response(const void* comp, const void* challenges, const void* scalars, const uint8_t* status,
                                   const uint8_t* sub, uint32_t n, void* proofs, hipStream_t stream);

}  // namespace curdle
