/*
 * curdle_msm.h -- C ABI of libcurdlemsm.so: BLS12-381 G1 multi-scalar
 * multiplication on MI355X (gfx950), the drop-in for the MSM path of
 * jsign/go-curdleproofs -- plus, further down, the entry points of the layers either side of
 * that path (batched point decoding, batched scalar multiplications, the protocol and Whisk
 * restatements that funnel every MSM into the GPU).
 *
 * Every entry point replaces one reference interface (paths relative to
 * /root/reference); INTEGRATION.md shows the cgo binding for each.
 *
 * Data layouts are gnark-crypto v0.11.0's in-memory layouts (go.mod:6), so Go
 * slices can be handed over with unsafe.Pointer(&s[0]) and no copy:
 *   fr.Element            = 4 x uint64, little-endian limbs, Montgomery (R = 2^256)
 *   fp.Element            = 6 x uint64, little-endian limbs, Montgomery (R = 2^384)
 *   bls12381.G1Affine     = {X, Y fp.Element}   = 12 x uint64; (0,0) is infinity
 *   bls12381.G1Jac        = {X, Y, Z fp.Element} = 18 x uint64; Z = 0 is infinity
 *
 * Results are returned as the canonical Jacobian representative: (x, y, 1) of
 * the affine result (Z = Montgomery one), or (1, 1, 0) for infinity.  The
 * reference never inspects Jacobian limbs (only Equal / AddAssign / to-affine,
 * e.g. msmaccumulator/msmaccumulator.go:63), so any representative is valid;
 * a canonical one makes results byte-comparable.
 *
 * All functions return CURDLE_OK (0) or a negative CURDLE_E* code; the text of
 * the last error on the calling thread is available from curdle_last_error().
 * No C++ exception crosses this boundary.  Calls are synchronous (no pointer
 * is retained after return -- the cgo rule) and thread-safe.  There is no CPU
 * fallback: if no gfx950 device is usable the MSM entry points fail with
 * CURDLE_ENODEV.
 */
#ifndef CURDLE_MSM_H
#define CURDLE_MSM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CURDLE_OK 0
#define CURDLE_EINVAL (-1) /* bad argument (null pointer, length mismatch)      */
#define CURDLE_ENODEV (-2) /* no usable HIP device / library not initialised    */
#define CURDLE_EHIP (-3)   /* a HIP runtime call failed                         */
#define CURDLE_ENOMEM (-4) /* device or host allocation failed                  */
#define CURDLE_EBUSY (-5)  /* every MSM slot is in flight (async API)              */
#define CURDLE_MSM_SLOTS 8 /* MSMs that can be in flight at once                   */

#define CURDLE_G1_AFFINE_U64 12
#define CURDLE_G1_JAC_U64 18
#define CURDLE_FR_U64 4

/* ------------------------------------------------------------------------- *
 * Library life cycle
 * ------------------------------------------------------------------------- */

/* Selects the HIP device this process computes on (one process per GPU) and
 * creates the stream + workspace.  Called implicitly with device 0 by the
 * first MSM call.  Replaces: common.MultiExpConf (common/util.go:14), the
 * reference's only configuration knob. */
int curdle_init(int device);
/* One process driving SEVERAL GPUs (the reference's caller is one
 * process making synchronous MultiExp calls, msmaccumulator/msmaccumulator.go:59): configures
 * one context per entry of devices[] (HIP device ids; an id may repeat, which puts two
 * contexts on one GPU -- how the multi-device code is tested on a one-GPU machine), each with
 * its own streams, workspace slots and one host worker thread.  After it
 *   - every entry point runs on the calling thread's CURRENT context: curdle_set_device(i)
 *     selects context i for this thread (default 0), like hipSetDevice; tickets and handles
 *     (curdle_dacc, decode tickets) remember their context; a curdle_dbases / curdle_crs is
 *     made resident lazily on every context that uses it;
 *   - curdle_msm_g1 splits a large host-buffer MSM by POINT RANGES over all contexts (each GPU
 *     copies and runs its own n / D pairs, the host thread of each device drives it, the D
 *     partial sums are added on the host with the code of curdle_g1_sum: no collective) --
 *     unless the calling thread has SELECTED a device with curdle_set_device: a thread pinned
 *     to a device (a batch shard, curdlemsm.OnDevice) keeps its MSM there;
 *   - curdle_msm_g1_replicated does the same for inputs the caller keeps resident on every
 *     GPU, by Pippenger windows (north_star's partition) or point ranges;
 *   - curdle_verify_batch and curdle_whisk_is_valid_shuffle_proof_batch shard their proofs
 *     over the contexts (BASELINE config 5: replicas, no data-path exchange).
 * n = 1 is curdle_init(devices[0]).  Fails with CURDLE_EINVAL if the library is already
 * initialised on a different list.  All or nothing: if one entry cannot be brought up (bad id,
 * out of memory), every context this call created is closed again and a retry starts clean.
 * The multi-device paths were exercised as two contexts on one GPU and under a logical-device
 * interposer (tools/logical_devices_shim.cpp), never on two physical GPUs: unmeasured there. */
#define CURDLE_MAX_DEVICES 16
int curdle_init_devices(const int* devices, int n);
int curdle_device_count(void);      /* contexts configured (1 unless curdle_init_devices said more) */
/* This thread's current context, 0 <= ordinal < curdle_device_count(); -1 = no selection (context
 * 0, and large host-buffer MSMs may spread over all devices again). */
int curdle_set_device(int ordinal);
int curdle_get_device(void);
/* The calling thread's SELECTION: the ordinal it passed to curdle_set_device, or -1 if it has made none (or
 * cleared it with -1).  What a binding that selects a device temporarily restores afterwards
 * (curdlemsm.OnDevice): restoring curdle_get_device()'s 0 would leave the thread pinned to device 0. */
int curdle_get_device_selection(void);
/* Diagnostics: host-buffer MSMs (curdle_msm_g1) that were spread over several devices since the library was loaded. */
unsigned long long curdle_stat_spread_calls(void);
/* Closes every context (streams, workspaces, host threads).  CURDLE_EBUSY while an MSM or a point
 * decoding is in flight on a slot, or a call that spans the devices' host threads is running.  Like every teardown of a library, it must not run
 * concurrently with other entry points: a call that has not taken its slot yet is not seen. */
int curdle_shutdown(void);
/* Copies the calling thread's last error text (NUL-terminated) into buf. */
int curdle_last_error(char* buf, size_t len);

/* Test / measurement hook: the library's tunables ("knobs", go-curdleproofs_amd/host/knobs.h: window
 * width, lane and segment lengths, chunk counts, ...) are read ONCE from the environment
 * (CURDLE_<NAME>), when the library is first used, and never again.  This call changes one
 * afterwards -- name with or without the CURDLE_ prefix, value < 0 = back to "not set" (the
 * library's own rule) -- so that a test can walk a knob through its range inside one process.
 * Not for production callers; CURDLE_EINVAL for a name the table does not have. */
int curdle_plan_override(const char* name, long long value);
/* 1 if a HIP device is visible to the library, else 0 (never fails). */
int curdle_device_available(void);

/* ------------------------------------------------------------------------- *
 * The hot path: (*G1Jac).MultiExp(points []G1Affine, scalars []fr.Element, cfg)
 *   gnark-crypto v0.11.0, called at msmaccumulator/msmaccumulator.go:59 and
 *   the 38 other sites listed in SURVEY.md section 8(a).
 * out_jac = sum_i scalars[i] * points[i].  n = 0 gives infinity and CURDLE_OK
 * (msmaccumulator_test.go:14 runs sizes 0..3).  Inputs are host memory and
 * are copied to the device on every call: the prover mutates bases in place
 * between calls (innerproductargument.go:155-166), so nothing is cached by
 * pointer.
 * PRECONDITION (differs from gnark): every base must lie in the prime-order subgroup G1 (or be
 * the point at infinity).  The kernels split every scalar as k P = k1 P + k2 phi(P) with the
 * curve endomorphism phi(x, y) = (beta x, y), which is multiplication by lambda only on G1;
 * gnark's MultiExp does not use the endomorphism and is defined for any curve point.  Every
 * base the reference feeds this path is in G1 (CRS points are multiples of the generator,
 * proof and tracker points pass gnark's Decoder / SetBytes subgroup check).  For an on-curve
 * point outside G1 -- e.g. one taken from curdle_g1_decompress with subgroup_check = 0, or from
 * the begin / points decoding steps before the subgroup verdict -- the result is the well-defined
 * but different point k1 P + k2 (beta x, y)
 * (tests/test_msm_gpu.py::test_bases_outside_the_prime_order_subgroup_...).  The same holds for
 * curdle_g1_scalar_mul_batch and the device accumulator.  Bases that come from outside and went through no
 * decoder can be checked first: curdle_g1_check_batch / curdle_g1_check_batch_device (range, curve equation,
 * subgroup), or curdle_verify_checked for the verifier's instance points.
 * ------------------------------------------------------------------------- */
int curdle_msm_g1(const uint64_t* points, const uint64_t* scalars, size_t n,
                  uint64_t out_jac[CURDLE_G1_JAC_U64]);

/* The same call with options (flags = 0 is curdle_msm_g1).
 *
 * CURDLE_MSM_ANY_CURVE_POINT -- the opt-out from the precondition above: gnark's contract.  The scalars are
 *   NOT split with the endomorphism; each is recoded whole (255 bits, twice the windows), so the result is
 *   k P for every point P of the curve y^2 = x^3 + 4, in the prime-order subgroup or not -- what
 *   (*G1Jac).MultiExp (go.mod:6) returns for such input.  Costs about twice the bucket reduction and a digit
 *   array of twice the needed size; the additions are the same.  For callers that take bases from outside
 *   without a subgroup check (curdleproof.Verify takes []G1Affine from its caller, curdleproof.go:199-207).
 * CURDLE_MSM_BASES_UNCHANGED (device-input entry points only) -- the caller promises that the n points at
 *   d_points have not changed since the previous call that named the same (d_points, n) with this flag on this
 *   context: the library keeps its converted copy of them (one per pointer and count, at most four per context,
 *   the least recently used idle one is replaced; 256 bytes per point) and converts nothing on later calls.
 *   This is the "explicit, caller-managed" form of caching SURVEY.md section 8b allows: without the flag nothing
 *   is ever cached by pointer (the prover mutates its bases in place between calls).  A rank of the multi-GPU
 *   window split passes the same resident bases on every call; msmaccumulator.Verify's bases are mostly the CRS.
 *   curdle_msm_forget_bases(d_points) drops the copy (before the memory is freed or rewritten). */
#define CURDLE_MSM_ANY_CURVE_POINT 1u
#define CURDLE_MSM_BASES_UNCHANGED 2u
int curdle_msm_g1_ex(const uint64_t* points, const uint64_t* scalars, size_t n, unsigned flags,
                     uint64_t out_jac[CURDLE_G1_JAC_U64]);

/* Same MSM with inputs already resident in device memory (HIP device
 * pointers, same layouts).  `stream` is a hipStream_t or NULL for the
 * library's own stream.  This is what bench.py times. */
int curdle_msm_g1_device(const void* d_points, const void* d_scalars, size_t n,
                         uint64_t out_jac[CURDLE_G1_JAC_U64], void* stream);
/* ... with the flags of curdle_msm_g1_ex (both apply to device inputs). */
int curdle_msm_g1_device_ex(const void* d_points, const void* d_scalars, size_t n, unsigned flags,
                            uint64_t out_jac[CURDLE_G1_JAC_U64], void* stream);
int curdle_msm_forget_bases(const void* d_points);

/* The same MSM over inputs the caller keeps resident on EVERY configured context:
 * d_points[i] / d_scalars[i] are device pointers on context i's GPU, each holding all n pairs
 * (curdle_device_count() entries).  split: 1 = Pippenger windows [w_i, w_i+1) per context
 * (north_star's partition: every GPU walks all n pairs for its windows), 2 = point ranges
 * (every GPU runs all windows over its n / D pairs), 0 = the library's choice (windows up to
 * 2^21 pairs, point ranges beyond: the per-rank step times of DESIGN.md section 5).  One host
 * thread per device; the D 144-byte partials are summed on the host. */
int curdle_msm_g1_replicated(const void* const* d_points, const void* const* d_scalars, size_t n, int split,
                             uint64_t out_jac[CURDLE_G1_JAC_U64]);

/* Asynchronous form of the device-resident MSM.  submit() enqueues every GPU phase
 * of one MSM (window range as below; window_bits = 0, win_begin = 0, win_end = -1 for
 * the whole MSM) on a free workspace slot and returns immediately with a ticket;
 * wait() blocks until that MSM is done, finishes it on the host and writes the
 * result.  Up to CURDLE_MSM_SLOTS MSMs can be in flight: the latency-bound tail of
 * one (bucket reduce, D2H, host combine) then overlaps the accumulation of the next.
 * The device inputs must stay valid and unchanged until wait() returns.  submit()
 * fails with CURDLE_EBUSY when every slot is in flight. */
int curdle_msm_g1_device_submit(const void* d_points, const void* d_scalars, size_t n,
                                int window_bits, int win_begin, int win_end, int* ticket);
int curdle_msm_g1_device_submit_ex(const void* d_points, const void* d_scalars, size_t n,
                                   int window_bits, int win_begin, int win_end, unsigned flags, int* ticket);
int curdle_msm_wait(int ticket, uint64_t out_jac[CURDLE_G1_JAC_U64]);
/* How many of the CURDLE_MSM_SLOTS workspace slots are free right now (a hint: other threads
 * take and release slots concurrently).  A caller that would hold a slot across host work of
 * its own (the verifier starts its accumulation before it hashes) uses it to decide whether
 * to take the slot early or late. */
int curdle_msm_free_slots(void);

/* Partial MSM over Pippenger windows [win_begin, win_end) of the
* decomposition the library would use for (n, window_bits); the partial is
 * already scaled by 2^(bit offset of window win_begin).  Summing the partials of a
 * partition of [0, curdle_msm_num_windows()) with curdle_g1_sum() gives the
 * full MSM.  This is the multi-GPU split of north_star: one rank per GPU, each
 * taking a window range, 144-byte partials all-gathered over RCCL.
 * window_bits = 0 lets the library choose. */
int curdle_msm_g1_device_windows(const void* d_points, const void* d_scalars, size_t n,
                                 int window_bits, int win_begin, int win_end,
                                 uint64_t out_jac[CURDLE_G1_JAC_U64], void* stream);
int curdle_msm_g1_device_windows_ex(const void* d_points, const void* d_scalars, size_t n,
                                    int window_bits, int win_begin, int win_end, unsigned flags,
                                    uint64_t out_jac[CURDLE_G1_JAC_U64], void* stream);
int curdle_msm_window_bits(size_t n);              /* the library's choice of c for n   */
int curdle_msm_num_windows(size_t n, int window_bits); /* W = ceil(127 / c) for that choice */
/* Widths of the W windows for (n, window_bits), lowest window first (sum = 127: the
 * library splits every scalar into two 127-bit halves, k P = k1 P + k2 phi(P), and a
 * window covers the same bits of both): the bits are spread as evenly as possible; all
 * windows but the top one are recoded into signed digits, the top one is unsigned.
 * Returns W. */
int curdle_msm_window_widths(size_t n, int window_bits, int widths[64]);
/* The same two for a call that passes `flags` (review of round 5): with CURDLE_MSM_ANY_CURVE_POINT the
 * plan recodes the whole 255-bit scalar, so it has W = ceil(255 / c) windows whose widths sum to 255,
 * and the window ranges of *_windows_ex / *_submit_ex are ranges over THOSE windows -- a caller that
 * partitions [0, curdle_msm_num_windows()) and passes the flag would cover the low half of every
 * scalar only, with no error.  flags = 0 (or CURDLE_MSM_BASES_UNCHANGED alone) gives the values above. */
int curdle_msm_num_windows_ex(size_t n, int window_bits, unsigned flags);
int curdle_msm_window_widths_ex(size_t n, int window_bits, unsigned flags, int widths[64]);

/* out = sum of k Jacobian points (host memory, any representatives).
 * Replaces the chain of G1Jac.AddAssign a caller would do on partials. */
int curdle_g1_sum(const uint64_t* jac_points, size_t k, uint64_t out_jac[CURDLE_G1_JAC_U64]);

/* k independent MSMs in one call (many
 * concurrent msmaccumulator.Verify calls).  MSM j covers pairs
 * [offsets[j], offsets[j+1]) of the concatenated points/scalars arrays;
 * offsets has k+1 entries.  out_jac holds k results. */
int curdle_msm_g1_batch(const uint64_t* points, const uint64_t* scalars,
                        const size_t* offsets, size_t k, uint64_t* out_jac);

/* The same with inputs resident in device memory (offsets stays a host array). */
int curdle_msm_g1_batch_device(const void* d_points, const void* d_scalars, const size_t* offsets,
                               size_t k, uint64_t* out_jac, void* stream);

/* k MSMs that share ONE scalar vector against k base sets of n points each
 * (samemultiscalarargument.go:64-70 and :206,218,231; curdleproof.go:110,114).
 * points_sets[j] points at n affine points. */
int curdle_msm_g1_multi(const uint64_t* const* points_sets, size_t k,
                        const uint64_t* scalars, size_t n, uint64_t* out_jac);

/* ------------------------------------------------------------------------- *
 * msmaccumulator (msmaccumulator/msmaccumulator.go:11-64), host-side mirror.
 * The Go package keeps its own map; these entry points exist so that the
 * C++/Python side of this repository can run the reference's accumulator
 * tests through the same library.  `rand` is a curdle_rand handle
 * (common/rand.go).
 * ------------------------------------------------------------------------- */
typedef struct curdle_acc curdle_acc;
typedef struct curdle_rand curdle_rand;

curdle_rand* curdle_rand_new(uint64_t seed);                  /* common.NewRand, rand.go:19        */
void curdle_rand_free(curdle_rand* r);
int curdle_rand_get_fr(curdle_rand* r, uint64_t out_fr[4]);   /* GetFr, rand.go:35 (Montgomery)    */
int curdle_rand_get_g1_affine(curdle_rand* r, uint64_t out_aff[12]); /* GetG1Affine, rand.go:72    */
int curdle_rand_permutation(curdle_rand* r, size_t n, uint32_t* out); /* GeneratePermutation :97   */

curdle_acc* curdle_acc_new(void);                             /* New, msmaccumulator.go:16         */
void curdle_acc_free(curdle_acc* a);
/* AccumulateCheck(C, x, v, rand), msmaccumulator.go:23.  len(x) != len(v) is
 * CURDLE_EINVAL ("x and v must have the same length"). */
int curdle_acc_accumulate_check(curdle_acc* a, const uint64_t C_jac[18],
                                const uint64_t* x, size_t x_len,
                                const uint64_t* v, size_t v_len, curdle_rand* rand);
/* The same check with C given as the linear combination it would have been computed
 * from, C = sum_j c_scalars[j] * c_points[j] (affine points, Montgomery scalars): alpha is
 * drawn exactly as in AccumulateCheck and the terms -alpha * c_scalars[j] join the base /
 * scalar map, so Verify()'s one MSM checks the reference's equation with alpha * C moved
 * to the other side -- no MSM for C and no alpha * C scalar multiplication now.  A_c is
 * left unchanged.  Same accept bit as accumulate_check(C) for every input. */
int curdle_acc_accumulate_check_deferred(curdle_acc* a, const uint64_t* c_scalars, const uint64_t* c_points,
                                         size_t c_len, const uint64_t* x, size_t x_len,
                                         const uint64_t* v, size_t v_len, curdle_rand* rand);
/* Verify(), msmaccumulator.go:49: *ok = 1 iff MSM(bases, scalars) == A_c.  The
 * MSM runs on the GPU through curdle_msm_g1. */
int curdle_acc_verify(curdle_acc* a, int* ok);
int curdle_acc_get_A_c(const curdle_acc* a, uint64_t out_jac[18]); /* exported field A_c, :12     */
size_t curdle_acc_num_bases(const curdle_acc* a);
/* Flattened map (bases then scalars), in insertion order. */
int curdle_acc_export(const curdle_acc* a, uint64_t* points, uint64_t* scalars);

/* ------------------------------------------------------------------------- *
 * Protocol layers around the hot path: a host-side
 * restatement of the reference's CRS, ShufflePermuteCommit, curdleproof.Prove and
 * curdleproof.Verify, so that a whole Verify (all sub-argument MSMs + the final
 * batched msmaccumulator MSM on the GPU) can be run without a Go toolchain.  The Go
 * package keeps its own protocol code; this is the caller either side of the MSM,
 * for end-to-end tests and the verifies/s measurement.  UNVERIFIED against
 * Go-produced proofs.
 * Points are gnark G1Affine arrays (ell x 12 u64), M a G1Jac, scalars fr.Elements.
 * ------------------------------------------------------------------------- */
/* BYTE COMPATIBILITY WITH THE GO IMPLEMENTATION IS UNVERIFIED for every entry point of this
 * section that produces or consumes serialised proofs (curdle_prove, curdle_verify,
 * curdle_proof_from_bytes, curdle_verify_batch, curdle_whisk_*): no Go toolchain and no
 * Go-produced proof exist in the build environment.  The transcript labels, challenge order,
 * gnark Encoder framing and verifier equations were checked against the reference source by
 * reading; what the tests pin is Merlin's published vector, the common.Rand known answers, the
 * reference's size constants (48 / 128 / 4576 bytes) and this implementation's own proof bytes
 * for fixed seeds (tests/golden/proof_vectors.npz).  The MSM entry points above do not depend
 * on any of this. */
typedef struct curdle_crs curdle_crs;
curdle_crs* curdle_crs_generate(size_t ell, curdle_rand* rand);   /* GenerateCRS, crs.go:20           */
void curdle_crs_free(curdle_crs* crs);
size_t curdle_crs_size(const curdle_crs* crs);
/* A CRS that no curdle_rand produced: the caller's points, or their bytes.  In the reference CRS is a struct of public
 * fields (crs.go:10-18) that the caller fills in and passes; a Whisk deployment uses one fixed, published CRS.  The
 * handle that comes out is indistinguishable from a generated one -- H, Gt and Gu stored with Z = 1 as GenerateCRS
 * leaves them, the fixed-base tables of Gsum and Hsum built from the stored sums, a fresh resident copy for the device
 * accumulator -- and goes to every entry point that takes a curdle_crs; curdle_crs_free and curdle_crs_size apply.
 *
 * WIRE FORM (curdle_crs_from_bytes / curdle_crs_to_bytes).  THE REFERENCE DEFINES NO CRS SERIALISATION (crs.go has
 * none): this form is THIS LIBRARY'S OWN.  It is the struct's fields in declaration order -- Gs, Hs, H, Gt, Gu, Gsum,
 * Hsum -- each point in gnark's 48-byte compressed encoding with nothing in between: 48 (ell + 9) bytes, and ell is
 * read from the length.
 *
 * A VALIDATED import (curdle_crs_from_bytes always; curdle_crs_from_points without CURDLE_CRS_TRUSTED) checks, in
 * this order:
 *   1. before any device work: a null argument (a null field of curdle_crs_points included), a flag bit that is not
 *      defined here, ell = 0 or ell > CURDLE_CRS_MAX_ELL; for bytes a len that is not 48 (ell + 9) for an ell in that
 *      range.  CURDLE_EINVAL, *out = NULL, *fault NOT written.
 *   2. every point ON THE GPU, with the subgroup test: from_points by one curdle_g1_check_batch over
 *      Gs | Hs | Gsum | Hsum and one curdle_g1_check_jac_batch over H | Gt | Gu, from_bytes by one
 *      curdle_g1_decompress_batch over all ell + 9 records.  The first status that is not CURDLE_DECODE_OK, in wire
 *      order, is the fault, with that CURDLE_DECODE_* code as its reason.  CURDLE_DECODE_INFINITY is a fault for Gs,
 *      Hs, H, Gt and Gu (a generator at infinity is no generator) and none, here, for Gsum and Hsum.  No host
 *      fallback: without a device CURDLE_ENODEV, as the check calls themselves answer.
 *   3. duplicates among Gs | Hs | H | Gt | Gu as group elements (H, Gt, Gu normalised on the host first): two equal
 *      points are a known relation between generators.  The fault names the LATER point in wire order, reason
 *      CURDLE_CRS_DUPLICATE; curdle_last_error names both.
 *   4. the sums: Gs and Hs summed as GenerateCRS sums them (crs.go:41-48) against Gsum, then Hsum, (0, 0) being
 *      infinity.  Reason CURDLE_CRS_SUM_MISMATCH, index 0.
 * On a fault: CURDLE_EINVAL, *out = NULL, *fault (if not null) filled, and curdle_last_error reads like the checked
 * verifier's texts -- "Gs[17]: not in the prime-order subgroup".  On success *out receives the handle and *fault (if
 * not null) is {-1, 0, 0}.
 *
 * CURDLE_CRS_TRUSTED (from_points only): only the refusals of step 1 apply.  The fields are taken as they are -- an
 * inconsistent Gsum included, which is what the reference does with a hand-filled struct --, nothing is sent to a
 * device, no counter moves, and the call works on a machine without a GPU.  That every point lies in G1 is then the
 * CALLER'S PRECONDITION, as it is for the bases of curdle_msm_g1.  For a caller who generated the CRS itself. */
#define CURDLE_CRS_N_BLINDERS 4
#define CURDLE_CRS_MAX_ELL ((size_t)1 << 20)
#define CURDLE_CRS_TRUSTED 1u           /* from_points only: take the fields as they are, check nothing, no device */
/* which field a fault names, in WIRE ORDER */
#define CURDLE_CRS_GS 0
#define CURDLE_CRS_HS 1
#define CURDLE_CRS_H 2
#define CURDLE_CRS_GT 3
#define CURDLE_CRS_GU 4
#define CURDLE_CRS_GSUM 5
#define CURDLE_CRS_HSUM 6
/* reasons beyond CURDLE_DECODE_* (1..4) */
#define CURDLE_CRS_DUPLICATE 16
#define CURDLE_CRS_SUM_MISMATCH 17
typedef struct {            /* gnark's in-memory layouts, unchanged: what cgo hands over */
  const uint64_t* Gs;       /* ell x 12, G1Affine */
  size_t ell;
  const uint64_t* Hs;       /* CURDLE_CRS_N_BLINDERS x 12 */
  const uint64_t* H;        /* 18, G1Jac, any Z */
  const uint64_t* Gt;       /* 18 */
  const uint64_t* Gu;       /* 18 */
  const uint64_t* Gsum;     /* 12 */
  const uint64_t* Hsum;     /* 12 */
} curdle_crs_points;
typedef struct {
  int field;                /* CURDLE_CRS_GS ... CURDLE_CRS_HSUM; -1: no fault */
  size_t index;             /* within Gs or Hs; 0 for the single points */
  int reason;               /* CURDLE_DECODE_* or CURDLE_CRS_DUPLICATE / CURDLE_CRS_SUM_MISMATCH */
} curdle_crs_fault;
int curdle_crs_from_points(const curdle_crs_points* in, unsigned flags, curdle_crs** out, curdle_crs_fault* fault);
int curdle_crs_from_bytes(const uint8_t* in, size_t len, curdle_crs** out, curdle_crs_fault* fault);
/* The handle's fields in the layouts of curdle_crs_points (Gs: curdle_crs_size(crs) x 12; H, Gt, Gu with Z = 1, or
 * (1, 1, 0) for infinity) and in the wire form.  Host code, no device needed; a null argument: CURDLE_EINVAL.
 * curdle_crs_to_bytes sets *len to the needed 48 (ell + 9) even when cap is too small (CURDLE_EINVAL then), as
 * curdle_prove does for its proof. */
int curdle_crs_export_points(const curdle_crs* crs, uint64_t* Gs, uint64_t* Hs, uint64_t H[18], uint64_t Gt[18],
                             uint64_t Gu[18], uint64_t Gsum[12], uint64_t Hsum[12]);
int curdle_crs_to_bytes(const curdle_crs* crs, uint8_t* out, size_t cap, size_t* len);
/* common.ShufflePermuteCommit, common/util.go:45 */
int curdle_shuffle_permute_commit(const curdle_crs* crs, const uint64_t* Rs, const uint64_t* Ss, size_t ell,
                                  const uint32_t* perm, const uint64_t k[4], curdle_rand* rand,
                                  uint64_t* Ts_out, uint64_t* Us_out, uint64_t M_out[18], uint64_t rs_m_out[16]);
/* curdleproof.Prove, curdleproof.go:38; the proof is returned serialised (Proof.Serialize, :358).
 * If cap is too small *proof_len still receives the needed size. */
int curdle_prove(const curdle_crs* crs, const uint64_t* Rs, const uint64_t* Ss, const uint64_t* Ts,
                 const uint64_t* Us, size_t ell, const uint64_t M[18], const uint32_t* perm,
                 const uint64_t k[4], const uint64_t rs_m[16], curdle_rand* rand,
                 uint8_t* proof_out, size_t cap, size_t* proof_len);
/* curdleproof.Verify, curdleproof.go:199, on a serialised proof (Proof.FromReader, :320):
 * returns CURDLE_OK with *ok = accept bit for (true|false, nil); a negative code for
 * (false, err) -- malformed proof, zero randomizer, device failure. */
int curdle_verify(const curdle_crs* crs, const uint8_t* proof, size_t proof_len, const uint64_t* Rs,
                  const uint64_t* Ss, const uint64_t* Ts, const uint64_t* Us, size_t ell,
                  const uint64_t M[18], curdle_rand* rand, int* ok);
/* The same split as the reference's API, where Verify takes a decoded `Proof` value
 * (curdleproof.go:199) and decoding is Proof.FromReader (:320): decode once -- curve and
 * subgroup checks on every point -- into a handle, verify the handle (this is what the
 * reference's BenchmarkVerifier times, curdleproof_test.go:210-237), free it. */
typedef struct curdle_proof curdle_proof;
int curdle_proof_from_bytes(const uint8_t* proof, size_t proof_len, curdle_proof** out);
void curdle_proof_free(curdle_proof* p);
int curdle_verify_proof(const curdle_crs* crs, const curdle_proof* proof, const uint64_t* Rs,
                        const uint64_t* Ss, const uint64_t* Ts, const uint64_t* Us, size_t ell,
                        const uint64_t M[18], curdle_rand* rand, int* ok);
/* Cross-proof batch verification (the reference verifies one proof
 * at a time): k proofs over the same CRS and the same ell.  The host part of each proof runs
 * on `nthreads` worker threads; all proofs' checks are folded into ONE accumulator (per-proof
 * randomness derived from `rand`; the CRS bases merge) and ONE MSM of ~k * (4 ell + 100) pairs
 * decides.  oks[i] receives each proof's accept bit: if a group's MSM fails, the group's
 * recorded checks are summed once more per member (curdle_dacc_run_members: one GPU pass, no
 * proof decoded or hashed again; with the host-mirror accumulator, or a group beyond that form's
 * limits, the members are verified one by one), so the bits are exact either way.  A malformed proof or a zero
 * randomizer counts as rejected here (curdle_verify reports those as errors).
 * proofs / Rs / Ss / Ts / Us: arrays of k pointers; Ms: k x 18 limbs. */
int curdle_verify_batch(const curdle_crs* crs, size_t k, const uint8_t* const* proofs, const size_t* proof_lens,
                        const uint64_t* const* Rs, const uint64_t* const* Ss, const uint64_t* const* Ts,
                        const uint64_t* const* Us, size_t ell, const uint64_t* Ms, curdle_rand* rand,
                        int nthreads, int* oks);
/* How curdle_verify evaluates the check points it hands to the accumulator.  0 (default):
 * deferred -- each is passed as the linear combination of proof / statement points it is,
 * so a verification is ONE MSM on the GPU.  1: eager -- evaluated where the reference
 * evaluates them (a MultiExp per argument, then AccumulateCheck's alpha * C on the host).
 * Identical accept bit; the eager mode exists for differential tests.  Initial value from
 * the environment variable CURDLE_VERIFY_EAGER.  Returns the previous setting. */
int curdle_verify_set_eager(int eager);
int curdle_proof_reencode(const uint8_t* proof, size_t proof_len, uint8_t* out, size_t cap, size_t* out_len);
/* The reference's `whisk` package (whisk/whisk.go, whisk/types.go): the byte-level API of the
 * Whisk SSLE spec.  A tracker is 96 bytes (rG || krG, gnark compressed points, types.go:73-76);
 * a shuffle proof is CURDLE_WHISK_SHUFFLE_PROOF_SIZE bytes (M, the curdleproof, zero padding,
 * types.go:53-71) over CURDLE_WHISK_ELL trackers; a tracker (opening) proof is 128 bytes (A, B, s).
 * Every decoded point is curve- and subgroup-checked, as gnark's Decoder / SetBytes do.
 * Return CURDLE_OK with *ok = the accept bit for (true|false, nil); negative for (false, err). */
#define CURDLE_WHISK_ELL 124
#define CURDLE_WHISK_TRACKER_SIZE 96
#define CURDLE_WHISK_TRACKER_PROOF_SIZE 128
#define CURDLE_WHISK_SHUFFLE_PROOF_SIZE 4576
/* IsValidWhiskShuffleProof, whisk.go:20 */
int curdle_whisk_is_valid_shuffle_proof(const curdle_crs* crs, const uint8_t* pre_trackers, const uint8_t* post_trackers,
                                        size_t n_pre, size_t n_post,
                                        const uint8_t proof[CURDLE_WHISK_SHUFFLE_PROOF_SIZE], curdle_rand* rand, int* ok);
/* k shuffle proofs over one CRS at once (no reference counterpart; BASELINE config 5): all
 * points of all proofs and tracker sets decoded by one GPU kernel, the proofs verified like
 * curdle_verify_batch.  pre / post: k pointers to n trackers each; proofs: k pointers to
 * CURDLE_WHISK_SHUFFLE_PROOF_SIZE bytes.  oks[i] = accept bit; what does not decode is rejected. */
int curdle_whisk_is_valid_shuffle_proof_batch(const curdle_crs* crs, size_t k, const uint8_t* const* pre_trackers,
                                              const uint8_t* const* post_trackers, size_t n,
                                              const uint8_t* const* proofs, curdle_rand* rand, int nthreads, int* oks);
/* GenerateWhiskShuffleProof, whisk.go:63: n must be CURDLE_WHISK_ELL (the permutation length is fixed there) */
int curdle_whisk_generate_shuffle_proof(const curdle_crs* crs, const uint8_t* pre_trackers, size_t n, curdle_rand* rand,
                                        uint8_t* post_trackers_out, uint8_t proof_out[CURDLE_WHISK_SHUFFLE_PROOF_SIZE]);
/* IsValidWhiskTrackerProof, whisk.go:116 (host only: four scalar multiplications) */
int curdle_whisk_is_valid_tracker_proof(const uint8_t tracker[CURDLE_WHISK_TRACKER_SIZE], const uint8_t k_commitment[48],
                                        const uint8_t proof[CURDLE_WHISK_TRACKER_PROOF_SIZE], int* ok);
/* k tracker proofs at once, each answered as curdle_whisk_is_valid_tracker_proof answers it
 * (IsValidWhiskTrackerProof, whisk.go:116).  trackers: k x 96 bytes, k_commitments: k x 48,
 * proofs: k x 128, back to back.  The 5 k points are decoded (curve and subgroup checked) and both
 * equations of every member are checked on the GPU; the transcripts are hashed where
 * CURDLE_TRACKER_HASH_DEFAULT says (below): this call is _ex with that flag.
 * results[i] = 1 (accept), 0 (reject: (false, nil)) or CURDLE_EINVAL where the single call
 * returns CURDLE_EINVAL ((false, err): a record that is not a point of the subgroup, S >= r).
 * k = 0: CURDLE_OK, nothing read or written, no device needed.  On a negative return every
 * results[i] holds that code: "could not compute" never reads as a verdict.  No host fallback:
 * without a device the call fails with CURDLE_ENODEV. */
int curdle_whisk_is_valid_tracker_proof_batch(const uint8_t* trackers, const uint8_t* k_commitments,
                                              const uint8_t* proofs, size_t k, int* results);
/* The same call with the place where the members' Merlin transcripts (whisk.go:131-134) are hashed.
 *   CURDLE_TRACKER_HASH_HOST    on the host, on up to 16 threads started inside the call, with the S < r checks
 *                               and the gathering of the 5 k records, while the GPU takes the square roots.
 *   CURDLE_TRACKER_HASH_DEVICE  on the GPU: the three arrays go up as they are, kernels gather the records, check
 *                               every S < r and hash the transcripts (the batched Merlin kernel of
 *                               curdle_transcript_batch, over a tape compiled once per process) beside the square
 *                               roots.  No host arithmetic and no host thread.  A member whose transcript draws
 *                               CURDLE_TRANSCRIPT_MAX_TRIES non-canonical challenges (probability 0.547^256) is
 *                               answered by the single call on the host.
 *   CURDLE_TRACKER_HASH_DEFAULT the library's rule: knob CURDLE_TRACKER_DEVICE_HASH = 1 device, 0 host, unset by
 *                               the batch's size: on the device from 64 members (DESIGN.md section 0 has the measurement).
 * The answers are the same under every flag.  Any other flag value: CURDLE_EINVAL, before anything is copied or
 * launched. */
#define CURDLE_TRACKER_HASH_DEFAULT 0u
#define CURDLE_TRACKER_HASH_HOST 1u
#define CURDLE_TRACKER_HASH_DEVICE 2u
int curdle_whisk_is_valid_tracker_proof_batch_ex(const uint8_t* trackers, const uint8_t* k_commitments,
                                                 const uint8_t* proofs, size_t k, unsigned flags, int* results);
/* The same check over arrays already resident in device memory (HIP device pointers to k x 96, k x 48 and
 * k x 128 bytes, any alignment); the transcripts are always hashed on the device.  `stream` is a hipStream_t or
 * NULL for the library's own stream, as in curdle_msm_g1_device: the arrays are read in that stream's order, so
 * they may have been written on it immediately before.  `results` is host memory and valid when the call returns.
 * A member whose transcript draws no canonical challenge fails the call (CURDLE_EHIP in every result). */
int curdle_whisk_is_valid_tracker_proof_batch_device(const void* d_trackers, const void* d_k_commitments,
                                                     const void* d_proofs, size_t k, int* results, void* stream);
/* Diagnostics: members of tracker batches since the library was loaded whose transcripts out[0] were hashed on the
 * device, out[1] on the host, out[2] handed back to the host after a non-zero transcript status. */
int curdle_stat_tracker(unsigned long long out[3]);
/* The COMBINED form of the tracker batch: per pass of at most 65,536 members, ONE randomly weighted multi-scalar
 * multiplication settles every member at once.  The 2 m equations of the pass's members (whisk.go:136-144) are
 * weighted by two 128-bit coefficients per member and summed over the 5 m decoded records and G:
 *     sum_i  rho_i (s_i G + c_i kG_i - A_i)  +  sigma_i (s_i rG_i + c_i krG_i - B_i)
 * If the sum is the point at infinity, every member of the pass that was not refused is answered 1.  If it is not,
 * the pass runs the per-member check of curdle_whisk_is_valid_tracker_proof_batch_ex and answers exactly as that call
 * does.  Refusals are exact in both cases: a member with S >= r, a record that does not decode or a record outside
 * the subgroup is answered CURDLE_EINVAL, takes no part in the sum (its scalars are zero, so its records reach no
 * bucket) and does not make a pass fall back.  A 0 is only ever the per-member check's answer.  The transcripts are
 * always hashed on the device (CURDLE_TRACKER_HASH_DEVICE).
 *
 * `seed` (32 bytes, host memory in both forms) is what the coefficients are derived from, on the device:
 *     SHAKE256("curdle/tracker-combine/v1" | seed | le64(i))[0:32] = rho_i | sigma_i   (two little-endian integers),
 * i the member's index in the call.  The seed MUST be unpredictable to whoever made the proofs and FRESH for every
 * call (32 bytes of the operating system's randomness): someone who knows the coefficients in advance can make
 * invalid proofs whose errors cancel in the sum.
 *
 * Error bound: an accept is wrong with probability at most 2^-128 per call.  The sum is a polynomial of degree 1 in
 * each coefficient over F_r whose coefficient on rho_i (sigma_i) is member i's error in its first (second) equation,
 * a multiple of G since every record that takes part is in the subgroup.  One invalid member leaves a non-zero
 * coefficient on its rho or its sigma; with all other coefficients fixed, at most one of that coefficient's 2^128
 * values makes the sum vanish.  (SHAKE256 is taken as a random function of the unpredictable seed.)
 *
 * Cost: a batch in which every member is valid or refused pays the MSM and no chains.  A batch with ONE rejected
 * member pays the combined pass PLUS the chains of that pass: more than the plain call.  Nothing routes to this
 * form automatically; the existing entry points never take it.
 *
 * Conventions are those of _ex / _device: results[i] = 1, 0 or CURDLE_EINVAL; k = 0: CURDLE_OK, no device needed; a
 * null pointer (the seed included) with k > 0: CURDLE_EINVAL before any device work; on a negative return every
 * results[i] holds that code.  _device: HIP device pointers of any alignment, `stream` a hipStream_t or NULL; on a
 * caller's stream the whole pass, the MSM included, runs on that stream.  A member whose transcript draws no
 * canonical challenge (CURDLE_TRANSCRIPT_MAX_TRIES rejected draws) takes no part in the sum and is answered by the
 * single call on the host; in the _device form, which has no host copy of it, it fails the call (CURDLE_EHIP in
 * every result), as in curdle_whisk_is_valid_tracker_proof_batch_device. */
int curdle_whisk_is_valid_tracker_proof_batch_combined(const uint8_t* trackers, const uint8_t* k_commitments,
                                                       const uint8_t* proofs, size_t k, const uint8_t seed[32], int* results);
int curdle_whisk_is_valid_tracker_proof_batch_combined_device(const void* d_trackers, const void* d_k_commitments,
                                                              const void* d_proofs, size_t k, const uint8_t seed[32],
                                                              int* results, void* stream);
/* Diagnostics of the combined form since the library was loaded: out[0] passes settled by the sum, out[1] passes that
 * fell back to the per-member chains, out[2] members accepted by a sum, out[3] members excluded from a sum (answered
 * CURDLE_EINVAL or handed back to the host), in either kind of pass. */
int curdle_stat_tracker_combined(unsigned long long out[4]);
/* Diagnostic (like curdle_selftest_op): the MSM scalars the combined form computes for k <= 65,536 members (one
 * pass; more: CURDLE_EINVAL), without the MSM.  scalars_out: k x 5 x 4 limbs, Montgomery fr.Elements, member i's
 * scalars for rG, krG, kG, A, B: sigma s, sigma c, rho c, -rho, -sigma, all zero for an excluded member.  g_out: the
 * generator's scalar, sum rho_i s_i mod r (Montgomery), added up on the host from the kernel's per-block sums.  The
 * fallback hides a broken sum behind correct answers; this call and the counters make the sum testable. */
int curdle_whisk_tracker_combined_scalars(const uint8_t* trackers, const uint8_t* k_commitments,
                                          const uint8_t* proofs, size_t k, const uint8_t seed[32], uint64_t* scalars_out, uint64_t g_out[4]);
/* Milliseconds k_tracker_combine took in the process's last successful curdle_whisk_tracker_combined_scalars, by HIP
 * events around the kernel alone (like curdle_transcript_last_kernel_ms); 0 before the first. */
int curdle_tracker_combined_last_kernel_ms(double* out);
/* GenerateWhiskTrackerProof, whisk.go:149 */
int curdle_whisk_generate_tracker_proof(const uint8_t tracker[CURDLE_WHISK_TRACKER_SIZE], const uint64_t k[4],
                                        curdle_rand* rand, uint8_t proof_out[CURDLE_WHISK_TRACKER_PROOF_SIZE]);
/* k tracker proofs generated at once ON THE GPU, member i as curdle_whisk_generate_tracker_proof(trackers + 96 i,
 * ks + 4 i) generates it with the blinder blinders + 4 i (GenerateWhiskTrackerProof, whisk.go:149-175): proofs_out + 128 i
 * holds byte for byte what the single call writes for the same tracker, k and blinder, and results[i] = CURDLE_OK.
 * Where the single call returns CURDLE_EINVAL (a tracker record that is not a point of the subgroup), results[i] =
 * CURDLE_EINVAL and the member's 128 bytes are zero; its neighbours are unaffected.  trackers: k x 96 bytes; ks,
 * blinders: k x 4 limbs, Montgomery fr.Elements; proofs_out: k x 128 bytes, back to back.
 * The 2 k tracker records are decoded, the 3 k scalar multiplications kG = k G, A = b G, B = b rG run in one launch,
 * their results are normalised and compressed (the kernel of curdle_g1_compress_batch), the transcripts are hashed
 * by the batched Merlin kernel and s = b - c k is computed in Fr, all on the device, in passes of 65,536 members.  A
 * member whose transcript draws CURDLE_TRANSCRIPT_MAX_TRIES non-canonical challenges (probability 0.547^256) is
 * generated by the single path on the host.
 * k = 0: CURDLE_OK, nothing read or written, no device needed.  Null pointers with k > 0: CURDLE_EINVAL.  On a
 * negative return every results[i] holds that code and proofs_out is zero.  No host fallback: without a device the
 * call fails with CURDLE_ENODEV.
 * SECRETS.  ks and blinders are secrets.  The device buffers and the pinned staging that held them, and the
 * unnormalised results of the scalar multiplications, are overwritten (on the stream that used them) before the call
 * returns on every path.  The scalar-multiplication chain BRANCHES ON SCALAR BITS, as the host path and gnark's
 * ScalarMultiplication do: its running time depends on k and b.  CURDLE_TRACKER_PROVE_CONSTANT_TIME on the _ex forms
 * below puts constant-time kernels in the chain's place. */
int curdle_whisk_generate_tracker_proof_batch_blinders(const uint8_t* trackers, const uint64_t* ks, const uint64_t* blinders,
                                                       size_t k, uint8_t* proofs_out, int* results);
/* The same, drawing the blinders from rand exactly as k successive single calls on that rand would: the single call
 * decodes its tracker before it draws, so a member that fails to decode draws nothing.  The call decodes, waits for the
 * 2 k verdicts, draws one GetFr per decodable member in member order on the host and continues; afterwards rand is in
 * the state the k single calls would have left it in. */
int curdle_whisk_generate_tracker_proof_batch(const uint8_t* trackers, const uint64_t* ks, curdle_rand* rand, size_t k,
                                              uint8_t* proofs_out, int* results);
/* Diagnostics: members of generated batches since the library was loaded, out[0] generated on the device, out[1]
 * handed to the host single path after a non-zero transcript status. */
int curdle_stat_tracker_prove(unsigned long long out[2]);
/* The two generators above with a flags word.  flags = 0 IS the call above: same kernels, same counters (the calls
 * above pass 0).  A bit that is not defined here: CURDLE_EINVAL before anything else is looked at, copied or launched,
 * also with k = 0, and WITHOUT touching proofs_out or results.  Everything else -- passes, k = 0, null pointers,
 * CURDLE_ENODEV, results, zeroed members, the wipes, the output byte for byte -- is as described above.
 *
 * CURDLE_TRACKER_PROVE_CONSTANT_TIME changes the three scalar multiplications of a pass and nothing else: kG = k G and
 * A = b G run through k_fbase_mul_ct over the generator's resident table (CURDLE_FBASE_CONSTANT_TIME's kernel, with
 * that flag's promise and its normalisation), B = b rG through k_g1_mul_ct over the decoded rG records
 * (CURDLE_G1_MUL_CONSTANT_TIME's kernel, below), and the 3 m results are encoded from AFFINE records, which inverts
 * nothing.  The GLV chain and the kernel that lays out its pairs do not run.  Decoding, transcript rows, the batched
 * Merlin kernel, s = b - c k, the hand-back of a member with a transcript status, results and wipes are unchanged.  A
 * flagged pass of m members moves curdle_stat_fbase_ct[0] by 2 m and curdle_stat_g1_mul_ct[0] by m, one launch each,
 * and neither curdle_stat_fbase[0..1] nor curdle_stat_normalize.
 * WHAT THE FLAG PROMISES: the instruction stream (every branch, every exec mask beyond the end-of-array guard, every
 * loop count) and the address stream (every load and store address) of k_fbase_mul_ct, k_g1_mul_ct and
 * k_tracker_response -- the three kernels that read ks or blinders -- are independent of the values of ks and
 * blinders.  The host only copies ks and blinders (into the pinned staging and the device buffer that are wiped on the
 * way out) and never looks at them.  What follows those kernels works on kG, A, B, the challenge and s, which are the
 * call's public output.
 * WHAT IT DOES NOT PROMISE: anything about data-dependent power draw and clock behaviour of the chip, which is not
 * addressed; and nothing about the default path, whose warning above stays true.
 * OUTSIDE THE PROMISE: the host's draw of the blinders in the rand form (curdle_rand_get_fr, one per decodable member),
 * and the member handed to the host single path after CURDLE_TRANSCRIPT_MAX_TRIES rejected draws (probability
 * 0.547^256), whose multiplications are the host's. */
#define CURDLE_TRACKER_PROVE_CONSTANT_TIME 1u
int curdle_whisk_generate_tracker_proof_batch_blinders_ex(const uint8_t* trackers, const uint64_t* ks, const uint64_t* blinders,
                                                          size_t k, unsigned flags, uint8_t* proofs_out, int* results);
int curdle_whisk_generate_tracker_proof_batch_ex(const uint8_t* trackers, const uint64_t* ks, curdle_rand* rand, size_t k,
                                                 unsigned flags, uint8_t* proofs_out, int* results);
/* Which trackers does a key own?  A tracker is (rG, krG) with krG = k rG (computeTracker, whisk_test.go:98-104); a
 * client that did not make the tracker learns whether it is its own by evaluating k rG == krG.
 * The single form, host only, no device needed: *owned = 1 iff k rG and krG are the same group element, infinity a
 * group element like any other (k = 0 owns exactly the trackers whose krG is infinity; a tracker with rG = infinity
 * is owned by every key iff its krG is infinity; krG = -(k rG) is not owned), else 0.  Both records are decoded as
 * gnark's SetBytes does (curve and subgroup, whisk/types.go:85-95): if either does not decode the call returns
 * CURDLE_EINVAL, as curdle_whisk_generate_tracker_proof does, and *owned is 0.  k: a Montgomery fr.Element. */
int curdle_whisk_is_own_tracker(const uint8_t tracker[CURDLE_WHISK_TRACKER_SIZE], const uint64_t k[4], int* owned);
/* m keys against n trackers ON THE GPU: owned[j * n + i], one byte, answers key j (ks + 4 j, Montgomery fr.Element)
 * and tracker i (trackers + 96 i) as the single form answers them: */
#define CURDLE_TRACKER_NOT_OWNED 0
#define CURDLE_TRACKER_OWNED 1
#define CURDLE_TRACKER_BAD 2       /* rG or krG is not the encoding of a point of the subgroup */
#define CURDLE_TRACKER_UNKNOWN 255 /* the call failed: never reads as a verdict */
/* A tracker with a record that does not decode has CURDLE_TRACKER_BAD in its byte for EVERY key; its neighbours are
 * unaffected.  The 2 n records are decoded once (curve and subgroup) for all keys, in passes of 131,072 trackers;
 * every (key, tracker) pair is one 255-bit scalar multiplication through the GLV split with an exact equality test
 * on the device, in launches of at most CURDLE_TRACKER_OWN_PAIRS pairs (knob; 262,144) back to back on one stream.
 * n = 0 or m = 0: CURDLE_OK, nothing read or written, no device needed.  Null pointers otherwise: CURDLE_EINVAL.
 * Limits: n <= 2^20, m <= 65,535, m n <= 2^24; beyond them CURDLE_EINVAL with the limit named in curdle_last_error,
 * before anything is copied or launched.  On a negative return `owned` is filled with CURDLE_TRACKER_UNKNOWN.  No
 * host fallback: without a device the call fails with CURDLE_ENODEV.  The call takes one MSM slot for its buffers.
 * SECRETS.  ks are secrets.  The device buffer and the pinned staging that held them are overwritten (on the stream
 * that used them) before the call returns on every path; the kernel keeps a key and the two halves of its split in
 * registers only.  The scalar-multiplication chain BRANCHES ON KEY BITS, as the host path and gnark's
 * ScalarMultiplication do: its running time depends on the keys.  CURDLE_TRACKER_OWN_CONSTANT_TIME on the _ex forms below
 * puts a constant-time kernel in the chain's place. */
int curdle_whisk_find_own_trackers(const uint8_t* trackers, size_t n, const uint64_t* ks, size_t m, uint8_t* owned);
/* The same over arrays resident in device memory: HIP device pointers to n x 96 bytes, m x 32 bytes and m x n bytes.
 * d_trackers and d_ks must be multiples of 16 (CURDLE_EINVAL otherwise); d_owned may have any alignment.  `stream` is
 * a hipStream_t or NULL for the library's own stream, as in curdle_msm_g1_device: the arrays are read and d_owned is
 * written in that stream's order, and d_owned is complete when the call returns.  The caller's d_ks is read where it
 * is and not touched: the library makes no copy of the keys in this form. */
int curdle_whisk_find_own_trackers_device(const void* d_trackers, size_t n, const void* d_ks, size_t m,
                                          void* d_owned, void* stream);
/* Diagnostics since the library was loaded: out[0] (key, tracker) pairs answered on the device, out[1] launches of
 * the ownership kernel, out[2] those of the pairs that were answered CURDLE_TRACKER_BAD without a chain.  The counters
 * move when a tracker pass has completed: a pass that fails midway leaves its pairs and launches uncounted. */
int curdle_stat_tracker_own(unsigned long long out[3]);
/* The two searches above with a flags word.  flags = 0 IS the call above: same kernel, same counters, same bytes (the
 * calls above pass 0).  A bit that is not defined here: CURDLE_EINVAL before anything else is looked at, copied or
 * launched, also with n = 0 or m = 0; the host form then fills `owned` with CURDLE_TRACKER_UNKNOWN like every negative
 * return.  Everything else -- the limits, n = 0 or m = 0, null pointers, the pointer rule, CURDLE_ENODEV, the one decode
 * per pass of 131,072 trackers, the slot, the staging and the wipes of the keys' copies, the stream semantics, the
 * verdict bytes byte for byte -- is as described above.
 *
 * CURDLE_TRACKER_OWN_CONSTANT_TIME changes the ownership kernel and nothing else: a second kernel
 * (csrc/tracker_own_ct_kernels.hip, k_tracker_own_ct), one LANE per (key, tracker) pair: the 255 bits of the key MSB
 * first, every step one doubling and ALWAYS one mixed addition of the lane's rG, the new accumulator taken by mask
 * selection (the walk of CURDLE_G1_MUL_CONSTANT_TIME's kernel, below), and at the end a projective equality test
 * against krG -- x ZZ = X and y ZZZ = Y mod p, decided by mask arithmetic -- in the place of an inversion.  The GLV chain
 * does not run.  Launches hold at most CURDLE_TRACKER_OWN_PAIRS lanes (the same knob; 262,144; rounded down to a
 * multiple of 256, at least 256): tc = min(trackers of the pass, that) trackers of max(1, that / tc) keys each, back to
 * back on the one stream.  A flagged pass moves curdle_stat_tracker_own_ct and never curdle_stat_tracker_own,
 * curdle_stat_g1_mul_ct or curdle_stat_normalize.
 * WHAT THE FLAG PROMISES: the instruction stream (every branch, every exec mask, every loop count) and the address
 * stream (every load and store address) of the ownership kernel are independent of the values of ks.  The host only
 * copies ks (into the pinned staging and the device buffer that are wiped on the way out; the _device form reads them
 * where they are) and never looks at them.
 * WHAT IS PUBLIC, and does shape both streams: n, m, the pointers, the trackers, their decode statuses (a record that
 * does not decode is answered CURDLE_TRACKER_BAD without a chain), which of rG and krG are infinity -- and the verdicts,
 * which are the call's output: the byte stored for a pair depends on the key, its address does not.
 * WHAT IT DOES NOT PROMISE: anything about data-dependent power draw and clock behaviour of the chip, which is not
 * addressed; and nothing about the default path, whose warning above stays true.
 * OUTSIDE THE PROMISE: the host single call curdle_whisk_is_own_tracker, whose multiplication is the host's and branches
 * on key bits.
 * The flag is NOT a default and nothing is routed through it automatically.  Cost: one lane walks about 4,850
 * dependent field products, about 5 ms however few pairs a launch has. */
#define CURDLE_TRACKER_OWN_CONSTANT_TIME 1u
int curdle_whisk_find_own_trackers_ex(const uint8_t* trackers, size_t n, const uint64_t* ks, size_t m, uint8_t* owned,
                                      unsigned flags);
int curdle_whisk_find_own_trackers_device_ex(const void* d_trackers, size_t n, const void* d_ks, size_t m,
                                             void* d_owned, void* stream, unsigned flags);
/* curdle_stat_tracker_own's three counters for the passes under CURDLE_TRACKER_OWN_CONSTANT_TIME: out[0] pairs, out[1]
 * launches of k_tracker_own_ct, out[2] the pairs answered CURDLE_TRACKER_BAD; completed passes only. */
int curdle_stat_tracker_own_ct(unsigned long long out[3]);
/* ------------------------------------------------------------------------- *
 * Fixed-base scalar multiplication in G1 ON THE GPU; Whisk trackers in bulk
 *   The first step of the tracker life cycle: tracker = (r G, k r G), commitment = k G (computeTracker and getKComm,
 *   whisk/whisk_test.go:98-109), for every validator at once.  Every one of those points is a multiple of ONE point,
 *   so k P is at most 32 mixed additions from a table d 2^(8 w) P of 32 windows x 255 digits and no doubling
 *   (csrc/fbase_kernels.hip; the table is the host layer's curdle_host_fixed_base_table, converted once).
 * ------------------------------------------------------------------------- */
typedef struct curdle_fbase curdle_fbase; /* one point's table of 8,160 multiples on the device */
/* point_affine: a gnark G1Affine.  It must be on the curve, in the prime-order subgroup and not infinity (checked on
 * the host; the kernel's exactness argument needs the subgroup): CURDLE_EINVAL otherwise, the reason in
 * curdle_last_error, *out null.  The table is built on the host and made resident on the calling thread's context
 * (CURDLE_ENODEV without a device).  A handle follows curdle_dbases' rules: it keeps its multiples, makes its copy on
 * another context when a call there first names it, and re-makes it after curdle_shutdown, so it stays usable until it
 * is freed; curdle_fbase_free while a call reads the table is deferred to that call's end.  Null is a no-op. */
int curdle_fbase_create(const uint64_t point_affine[12], curdle_fbase** out);
void curdle_fbase_free(curdle_fbase* b);
#define CURDLE_G1_OUT_AFFINE 0     /* n x 12 limbs, gnark G1Affine, as curdle_g1_normalize_batch writes them */
#define CURDLE_G1_OUT_COMPRESSED 1 /* n x 48 bytes, gnark's compressed encoding */
/* out[i] = (scalars[i] * multipliers[i] mod r) * P, or scalars[i] * P when multipliers is null; P is base's point, the
 * G1 generator when base is null (its table is built at first use on a context, once however many threads race for
 * it, and counts in curdle_stat_fbase).  scalars, multipliers: n Montgomery fr.Elements, below r.  Affine output is
 * bit for bit what curdle_g1_normalize_batch gives for the same point (infinity: all zero), compressed output byte for
 * byte what curdle_g1_compress gives (G1Affine.Bytes; infinity: 0xc0 and zeros).  The results are normalised with one
 * shared inversion per wave; the compressed form encodes the records without a further inversion.
 * The call takes one MSM slot and works in passes of at most CURDLE_FBASE_PASS scalars (knob; 1,048,576; rounded down
 * to a multiple of 256, at least 256), one kernel launch each.  n = 0: CURDLE_OK, nothing read or written, no device
 * needed.  A null scalars or out, or an unknown out_form: CURDLE_EINVAL.  Limit: n <= 2^24.  Every refusal comes
 * before anything is copied or launched.  No host fallback: without a device the call fails with CURDLE_ENODEV.
 * SECRETS.  scalars and multipliers are secrets.  The device buffers and the pinned staging that held them, and the
 * unnormalised results, are overwritten (on the stream that used them) before the call returns on every path.  THE
 * KERNEL READS TABLE ENTRIES AT ADDRESSES CHOSEN BY SCALAR DIGITS and skips zero digits: its memory access pattern
 * and its running time depend on the scalars. */
int curdle_g1_fixed_base_mul_batch(const curdle_fbase* base, const uint64_t* scalars, const uint64_t* multipliers,
                                   size_t n, int out_form, void* out);
/* The same over arrays resident in device memory: HIP device pointers, multiples of 16 (CURDLE_EINVAL otherwise)
 * except a compressed d_out, which may have any alignment.  `stream` is a hipStream_t or NULL for the library's own,
 * as in curdle_msm_g1_device; d_out is complete when the call returns.  The caller's arrays are read where they are:
 * the library makes no copy of the scalars in this form.  d_out must not overlap d_scalars or d_multipliers: affine
 * output in place over the scalars is NOT supported. */
int curdle_g1_fixed_base_mul_batch_device(const curdle_fbase* base, const void* d_scalars, const void* d_multipliers,
                                          size_t n, int out_form, void* d_out, void* stream);
/* Diagnostics since the library was loaded: out[0] scalars multiplied on the device, out[1] launches of the
 * fixed-base kernel, out[2] tables built (uploaded and converted, the generator's included).  The first two move when
 * a pass has completed: a pass that fails midway leaves its scalars and its launch uncounted. */
int curdle_stat_fbase(unsigned long long out[3]);
/* computeTracker (whisk/whisk_test.go:98-104): tracker_out = r G | k r G, both in gnark's compressed encoding.  Host
 * only, no device needed.  k, r: Montgomery fr.Elements.  k r = 0 gives the encoding of infinity, as Bytes() does. */
int curdle_whisk_compute_tracker(const uint64_t k[4], const uint64_t r[4], uint8_t tracker_out[CURDLE_WHISK_TRACKER_SIZE]);
/* getKComm (whisk/whisk_test.go:106-109): out = k G, compressed.  Host only. */
int curdle_whisk_k_commitment(const uint64_t k[4], uint8_t out[48]);
/* n of each at once ON THE GPU: trackers_out + 96 i = r_i G | k_i r_i G and k_commitments_out + 48 i = k_i G, byte for
 * byte what the two single calls write for (ks + 4 i, rs + 4 i).  rs null: r = 1 for every member, the fork's initial
 * trackers (G, k G).  k_commitments_out null: the commitments are not computed.  Per pass ONE launch of the
 * fixed-base kernel over the generator's table for the 3 m (2 m) products of m members, one normalisation and one
 * encoding; a pass is at most CURDLE_FBASE_PASS products.
 * n = 0: CURDLE_OK, no device needed.  Null ks or trackers_out with n > 0: CURDLE_EINVAL.  Limit: n <= 2^22.  On a
 * negative return both outputs are zero (a count beyond the limit is refused without touching them).  No host
 * fallback: CURDLE_ENODEV without a device.  SECRETS: as curdle_g1_fixed_base_mul_batch. */
int curdle_whisk_compute_trackers_batch(const uint64_t* ks, const uint64_t* rs, size_t n, uint8_t* trackers_out,
                                        uint8_t* k_commitments_out);
/* The three batch calls above with a flags word.  flags = 0 IS the call above: same kernel, same counters (the calls
 * above pass 0).  A bit that is not defined here: CURDLE_EINVAL before anything else is looked at, copied or launched
 * (for the tracker batch: without touching the outputs), also with n = 0.  Everything else -- limits, passes,
 * alignment, n = 0, CURDLE_ENODEV, the MSM slot, the wipes, the output bit for bit -- is as described above.
 *
 * CURDLE_FBASE_CONSTANT_TIME: the multiplication runs in a second kernel (csrc/fbase_ct_kernels.hip) over the SAME
 * table.  It walks 64 unsigned 4-bit windows, reads ALL 15 multiples of every window (960 records, a subset of the
 * table) at addresses made of the window number alone, chooses one by mask arithmetic, ALWAYS performs one mixed
 * addition per window and takes the new accumulator by selection; infinity results are stored through a mask.
 * WHAT THE FLAG PROMISES: the device code's instruction stream (every branch, every exec mask beyond the end-of-array
 * guard, every loop count) and its address stream (every load and store address) are independent of the values of
 * scalars and multipliers; they depend on n, on whether multipliers is null and on the pointers.  The host only copies
 * scalars and multipliers (into the pinned staging and the device buffer that are wiped on the way out) and never
 * looks at them.  The normalisation and the encoding that follow work on the RESULTS -- whether a result is infinity,
 * the sign bit of its y -- which are the call's public output; they are the kernels of the default path.
 * WHAT IT DOES NOT PROMISE: anything about data-dependent power draw and clock behaviour of the chip (a multiplier fed
 * zeros draws less), which is not addressed; and nothing about the default path, whose warning above stays true.
 * About twice the default kernel's work by operation count (64 additions and 64 x 15 selected records against 31.9
 * additions on average). */
#define CURDLE_FBASE_CONSTANT_TIME 1u
int curdle_g1_fixed_base_mul_batch_ex(const curdle_fbase* base, const uint64_t* scalars, const uint64_t* multipliers,
                                      size_t n, int out_form, unsigned flags, void* out);
int curdle_g1_fixed_base_mul_batch_device_ex(const curdle_fbase* base, const void* d_scalars, const void* d_multipliers,
                                             size_t n, int out_form, unsigned flags, void* d_out, void* stream);
int curdle_whisk_compute_trackers_batch_ex(const uint64_t* ks, const uint64_t* rs, size_t n, unsigned flags,
                                           uint8_t* trackers_out, uint8_t* k_commitments_out);
/* out[0] scalars multiplied by the constant-time kernel, out[1] its launches; completed passes only.  A pass under
 * CURDLE_FBASE_CONSTANT_TIME counts here and NOT in curdle_stat_fbase[0..1]; tables built stay in curdle_stat_fbase[2]
 * (the table is shared). */
int curdle_stat_fbase_ct(unsigned long long out[2]);
/* ------------------------------------------------------------------------- *
 * Accumulator on the device
 *   msmaccumulator.AccumulateCheck / Verify (msmaccumulator/msmaccumulator.go:23-64) with
 *   the base -> scalar map kept on the GPU as an array of scalar slots indexed by base, for
 *   callers whose bases come from sets that stay resident: the CRS (crs.go:10-18: Gs | Hs |
 *   H | Gt | Gu never change) and the per-verification instance points.  Instead of hashing
 *   96-byte keys on the host (msmaccumulator.go:38-43) and re-uploading and re-converting every
 *   base for the final MultiExp (:59), a check names slot ranges of the resident sets and
 *   describes its scalar vector; an Fr kernel evaluates the vectors -- including the
 *   verifier's O(n) products s_i, s'_i (innerproductargument.go:223-234,
 *   samemultiscalarargument.go:267-277) -- weights them with the check's random alpha and
 *   adds them into the slots; the result feeds the MSM's digit kernel directly.
 * ------------------------------------------------------------------------- */
typedef struct curdle_dbases curdle_dbases; /* a base set on the device, in the kernels' internal form */
int curdle_dbases_create(const uint64_t* points /* n x 12, gnark G1Affine */, size_t n, curdle_dbases** out);
void curdle_dbases_free(curdle_dbases* b);
size_t curdle_dbases_size(const curdle_dbases* b);
/* 1 for a live handle: a set keeps its points and re-creates its device copy as needed (another
 * context, a context re-initialised after curdle_shutdown), so it stays usable until it is freed. */
int curdle_dbases_valid(const curdle_dbases* b);

/* The plain MSM over a resident base set: out = sum_{i < n} scalars[i] * bases[i] over the FIRST n
 * points of the set (n <= curdle_dbases_size).  Replaces (*G1Jac).MultiExp where the bases do not
 * change between calls -- msmaccumulator.Verify's (/root/reference/msmaccumulator/msmaccumulator.go:59)
 * are mostly the CRS (crs.go:10-18): SURVEY.md section 8(b)'s "explicit, caller-managed device
 * handle".  Nothing is uploaded or converted per call (the conversion is 0.10 ms and 360 MB of every
 * 2^20-pair call with gnark-layout inputs); the set's copy on the calling thread's context is made on
 * first use.  Same preconditions as curdle_msm_g1 (bases in G1).
 *   _dbases          scalars in DEVICE memory (n x 32 B Montgomery fr.Elements), synchronous
 *   _dbases_host     scalars in host memory: 32 bytes per pair cross PCIe instead of 128
 *   _dbases_windows  the partial over windows [win_begin, win_end) (win_end = -1: all), already
 *                    scaled -- one device's share of a multi-GPU window split whose every device
 *                    holds the set (curdle_msm_g1_device_windows' counterpart)
 *   _dbases_submit   the asynchronous form; curdle_msm_wait(ticket) finishes it.  The set stays
 *                    referenced until then (curdle_dbases_free in between is deferred). */
int curdle_msm_g1_dbases(const curdle_dbases* bases, const void* d_scalars, size_t n, uint64_t out_jac[18]);
int curdle_msm_g1_dbases_host(const curdle_dbases* bases, const uint64_t* scalars, size_t n, uint64_t out_jac[18]);
int curdle_msm_g1_dbases_windows(const curdle_dbases* bases, const void* d_scalars, size_t n, int window_bits,
                                 int win_begin, int win_end, uint64_t out_jac[18]);
int curdle_msm_g1_dbases_submit(const curdle_dbases* bases, const void* d_scalars, size_t n, int window_bits,
                                int win_begin, int win_end, int* ticket);

#define CURDLE_VEC_EXPLICIT 0 /* x_i = tail[i]: no structured part, n_struct must be 0                */
#define CURDLE_VEC_CONST 1    /* x_i = scale                                                          */
#define CURDLE_VEC_FOLD 2     /* x_i = scale * prod_{j : bit j of i set} gammas[m-1-j]                */
#define CURDLE_VEC_FOLD_POW 3 /* ... * q^(min(i, q_cap) + 1)                                          */
#define CURDLE_DACC_MAX_SEGS 6
#define CURDLE_DACC_MAX_EXTRA 16384
#define CURDLE_SET_CRS 0
#define CURDLE_SET_INST 1
/* One AccumulateCheck: sum_i x_i v_i (== C, which the caller moves to the other side as extra
 * terms).  Offsets index `pool`, an array of Montgomery fr.Elements; the first n_struct
 * elements of x follow the rule of `kind` with weight = alpha * scale folded in by the caller,
 * the n_tail elements after them are explicit and are multiplied by alpha on the device.
 * Segment s says: slots [first, first + len) of resident set `set` take x[vec_first + j];
 * segments may overlap, within a check and between checks: a slot takes the sum.
 * Refused with CURDLE_EINVAL before anything is launched: an unknown kind, nseg > 6, m > 31
 * (any kind), n_struct > 0 for EXPLICIT, n_struct > 2^m for the folded kinds, n_struct > 2^31 or
 * n_struct + n_tail >= 2^32 (element indices and exponents are 32-bit), weight_off or alpha_off
 * outside the pool (any kind, also where the rule does not read them), [tail_off, tail_off +
 * n_tail) outside it, [gammas_off, gammas_off + m) outside it for the folded kinds, q_off
 * outside it for FOLD_POW, a segment past its set or past n_struct + n_tail.  Fields a kind
 * does not use are ignored, not checked, and have no effect on the result: m (up to 31) and
 * gammas_off of EXPLICIT / CONST, q_off and q_cap of every kind but FOLD_POW.  m may exceed
 * log2(n_struct): the leading gammas are then inside the pool and never used. */
typedef struct {
  uint32_t kind, n_struct, m, q_cap;
  uint32_t weight_off, alpha_off, gammas_off, q_off, tail_off, n_tail;
  uint32_t nseg;
  struct {
    uint32_t set, first, len, vec_first;
  } seg[CURDLE_DACC_MAX_SEGS];
} curdle_dacc_check;

typedef struct curdle_dacc curdle_dacc;
/* Starts an accumulation over `crs` and n_inst instance points (host memory, gnark affine):
 * takes a workspace slot and begins copying / converting the bases, then returns; the caller
 * computes its challenges meanwhile. */
int curdle_dacc_begin(const curdle_dbases* crs, const uint64_t* inst_points, size_t n_inst, curdle_dacc** out);
/* Applies the checks, appends the n_extra loose (point, scalar) pairs and runs the MSM over
 * all slots: out_jac = sum over CRS, instance and extra bases (canonical Jacobian), i.e. what
 * msmaccumulator.Verify compares with A_c.  export_scalars (optional, (n_crs + n_inst) x 4)
 * receives the slot scalars the device built, for parity tests.  Ends the accumulation. */
int curdle_dacc_run(curdle_dacc* acc, const curdle_dacc_check* checks, size_t n_checks, const uint64_t* pool,
                    size_t pool_len, const uint64_t* extra_points, const uint64_t* extra_scalars, size_t n_extra,
                    uint64_t out_jac[CURDLE_G1_JAC_U64], uint64_t* export_scalars);
/* The member form: one sum per member of a group from ONE pass over the accumulation's bases.  check_member[c] and
 * extra_member[e] name the member (below n_members) a check or a loose pair belongs to; out_jac[j] is what
 * curdle_dacc_run would return given only member j's checks and loose pairs, over the same pool and the same resident
 * CRS and instance points.  Segments of different members may name the same slots: every member has a row of slot
 * scalars of its own, and the sums come from one batched MSM whose members share the converted bases.  A member
 * without checks and loose pairs gives infinity; n_members = 1 gives curdle_dacc_run's result bit for bit.
 * export_scalars (optional, n_members x (n_crs + n_inst) x 4) receives the rows.  Ends the accumulation, whatever it
 * returns.  Refused like curdle_dacc_run, and with CURDLE_EINVAL before anything is launched: a member index
 * >= n_members; n_members == 0 with checks or loose pairs; n_members > CURDLE_DACC_MAX_MEMBERS; n_members x
 * (n_crs + n_inst) > CURDLE_DACC_MAX_MEMBER_SLOTS; a batched MSM of more than 4,194,304 bucket slots (n_members x the
 * slots of one member's windows: 64 members reach it beyond about 2^15 bases each, fewer members later). */
#define CURDLE_DACC_MAX_MEMBERS 64
#define CURDLE_DACC_MAX_MEMBER_SLOTS ((size_t)1 << 22)
int curdle_dacc_run_members(curdle_dacc* acc, const curdle_dacc_check* checks, const uint32_t* check_member, size_t n_checks,
                            size_t n_members, const uint64_t* pool, size_t pool_len, const uint64_t* extra_points,
                            const uint64_t* extra_scalars, const uint32_t* extra_member, size_t n_extra,
                            uint64_t* out_jac /* n_members x 18, canonical Jacobian */,
                            uint64_t* export_scalars /* optional: n_members x (n_crs + n_inst) x 4 */);
/* The same in two steps, for a caller with work to do while the MSM runs (batch verification:
 * a worker submits its group of proofs and goes on verifying the next ones): submit copies
 * every argument and queues the kernels, poll says without blocking whether they are done
 * (the accumulation holds one of the eight workspace slots until it is waited for: collect it
 * soon after), wait hands out the result and ends the accumulation.  A failed submit ends it
 * too.  export_scalars, if given to submit, must stay valid until wait. */
int curdle_dacc_submit(curdle_dacc* acc, const curdle_dacc_check* checks, size_t n_checks, const uint64_t* pool,
                       size_t pool_len, const uint64_t* extra_points, const uint64_t* extra_scalars, size_t n_extra,
                       uint64_t* export_scalars);
int curdle_dacc_poll(curdle_dacc* acc, int* done);
int curdle_dacc_wait(curdle_dacc* acc, uint64_t out_jac[CURDLE_G1_JAC_U64]);
void curdle_dacc_abort(curdle_dacc* acc); /* ends an accumulation without its result (submitted or not) */
/* Diagnostics: launches of each build of the slot-scalar evaluation since the library was loaded --
 * out[0] the fused front with pool and checks staged in LDS, out[1] the fused front reading global
 * memory, out[2] / out[3] the separate kernel staged / not (accumulations beyond 16,384 bases).
 * The builds compute the same scalars; which one ran is visible here only. */
int curdle_stat_dacc_builds(unsigned long long out[4]);
/* Diagnostics of the member form since the library was loaded: out[0] member-form accumulations run, out[1] members
 * summed by them, out[2] members of failed batch groups that were still verified one by one (the batch verifiers'
 * fall-back when the member form refuses a group's shape). */
int curdle_stat_dacc_members(unsigned long long out[3]);

/* curdleproof.Verify keeps its accumulator on the device by default (the section above);
 * 0 moves it back to the host mirror of msmaccumulator (same accept bit).  Returns the
 * previous setting.  Environment: CURDLE_DEVICE_ACC=0. */
int curdle_verify_set_device_acc(int on);
/* Test hook: the accumulated (base, scalar) list of one verification of a decoded proof,
 * taken before the final MSM from the host mirror (device = 0) or the device accumulator
 * (device = 1), plus the accept bit.  points: cap x 12, scalars: cap x 4 (Montgomery);
 * *n_out entries are written.  Bases may repeat (the device keeps loose points apart). */
int curdle_verify_export_accumulator(const curdle_crs* crs, const curdle_proof* proof, const uint64_t* Rs,
                                     const uint64_t* Ss, const uint64_t* Ts, const uint64_t* Us, size_t ell,
                                     const uint64_t M[CURDLE_G1_JAC_U64], curdle_rand* rand, int device,
                                     uint64_t* points, uint64_t* scalars, size_t cap, size_t* n_out, int* ok);
/* common.IPA (reference common/util.go:26-35): out = sum_i a[i] * b[i] over Fr, Montgomery limbs
 * in and out; CURDLE_EINVAL if the lengths differ (the reference returns an error). */
int curdle_fr_inner_product(const uint64_t* a, size_t a_len, const uint64_t* b, size_t b_len, uint64_t out_fr[4]);
/* pieces exposed for known-answer tests */
int curdle_merlin_test_vector(const char* protocol, const char* label, const uint8_t* msg, size_t msg_len,
                              const char* challenge_label, uint8_t* out, size_t out_len);
int curdle_g1_compress(const uint64_t jac[18], uint8_t out[48]);
int curdle_g1_decompress(const uint8_t in[48], int subgroup_check, uint64_t out_jac[18]);
/* Batched independent scalar multiplications ON THE GPU:
 *   out[i] = addends[i] + scalars[i] * points[i],   i < n
 * points / addends / out gnark affine (addends may be NULL; (0,0) = infinity), scalars Montgomery
 * fr.Elements; n_scalars = n, or 1 for one scalar shared by all points.  Replaces the loops of
 * single ScalarMultiplication calls that dominate the reference's prover: the fold steps
 * G_L[i] += gamma * G_R[i] (innerproductargument.go:155-166, samemultiscalarargument.go:129-135),
 * grandproductargument.go:94-103 and common/util.go:55-63. */
int curdle_g1_scalar_mul_batch(const uint64_t* points, const uint64_t* scalars, size_t n_scalars,
                               const uint64_t* addends, size_t n, uint64_t* out_affine);
/* Batched decoding of gnark's compressed G1 encoding ON THE GPU (square root, curve check,
 * sign selection, and with subgroup_check != 0 the endomorphism subgroup test gnark's Decoder /
 * SetBytes apply -- run BESIDE the square roots, from the records' x alone, on a twisted model
 * of the curve, for batches of up to 32,768 points; behind them in one kernel for larger
 * ones): n x 48 bytes in, n x 12 limbs of gnark affine points out (directly usable as MSM
 * bases), one status byte per point.  Invalid points do not fail the call: they get a
 * non-zero status and (0, 0).  Replaces the per-point
 * G1Affine.SetBytes loops of whisk/types.go:85-95 (4 * ell tracker points per shuffle) and
 * of Proof.FromReader (curdleproof.go:320-356). */
#define CURDLE_DECODE_OK 0
#define CURDLE_DECODE_INFINITY 1        /* valid encoding of the point at infinity; out = (0, 0) */
#define CURDLE_DECODE_BAD_ENCODING 2    /* not the compressed form, x >= p, or stray bits with the infinity flag */
#define CURDLE_DECODE_NOT_ON_CURVE 3
#define CURDLE_DECODE_NOT_IN_SUBGROUP 4
int curdle_g1_decompress_batch(const uint8_t* in, size_t n, int subgroup_check, uint64_t* out_affine, uint8_t* status);
/* The same in two steps, so the caller can work with the points while the subgroup test (the
 * longer of the two chains, on its own stream) is still running: begin decodes -- square root,
 * curve check, sign -- and returns the points with a preliminary status (0, 1, 2 or 3; here
 * points outside the subgroup are still handed out); finish waits for the subgroup test and
 * writes the final status bytes (now possibly 4).  Every begin must be matched by a finish.
 * At most four may be in flight: a fifth begin returns CURDLE_EBUSY (use the one-shot form
 * then). */
int curdle_g1_decompress_begin(const uint8_t* in, size_t n, uint64_t* out_affine, uint8_t* status, int* ticket);
/* begin, split once more: start only launches the two kernels and returns (the caller hashes its
 * transcript from the raw bytes meanwhile); points waits for the square roots and hands back the
 * points; finish as above.  begin = start + points. */
int curdle_g1_decompress_start(const uint8_t* in, size_t n, int* ticket);
int curdle_g1_decompress_points(int ticket, uint64_t* out_affine, uint8_t* status);
int curdle_g1_decompress_finish(int ticket, uint8_t* status);
/* Membership check ON THE GPU for G1 points that arrive IN MEMORY (gnark G1Affine, n x 12 limbs) and so went through
 * no decoder: the instance vectors of curdleproof.Verify (curdleproof.go:199-207 takes []G1Affine from its caller and
 * checks nothing) and any base array handed to the MSM entry points, whose precondition (see curdle_msm_g1) is that
 * every base lies in G1.  One CURDLE_DECODE_* status byte per point, decided in this order: all 24 words zero ->
 * INFINITY (gnark's IsInfinity); X or Y, as a 384-bit integer, >= p -> BAD_ENCODING (not a field element); y^2 != x^3 + 4
 * -> NOT_ON_CURVE (the group law never uses b: a point of another curve y^2 = x^3 + b' would run through every kernel
 * unnoticed, and the subgroup test cannot see it either); with subgroup_check != 0, [z^2] phi(P) + P != inf ->
 * NOT_IN_SUBGROUP; else OK.  Invalid points do not fail the call.  n = 0: CURDLE_OK, no device needed; n > 2^27 or a
 * null pointer with n > 0: CURDLE_EINVAL.  No host fallback: without a device the call fails with CURDLE_ENODEV.
 *   curdle_g1_check_batch          points in host memory
 *   curdle_g1_check_batch_device   points resident in device memory (check a base array once, before a run of
 *                                  CURDLE_MSM_BASES_UNCHANGED calls or before curdle_dbases_create); `stream` as in
 *                                  curdle_msm_g1_device; the status bytes are in HOST memory when it returns. */
int curdle_g1_check_batch(const uint64_t* points, size_t n, int subgroup_check, uint8_t* status);
int curdle_g1_check_batch_device(const void* d_points, size_t n, int subgroup_check, uint8_t* status, void* stream);
/* curdle_verify / curdle_verify_proof with that check on the 4 ell instance points (on the GPU, beside the
 * verification) and on M (on the host).  An instance point at infinity is acceptable, as it is to gnark and the MSM.
 * Any other failed point: CURDLE_EINVAL, *ok = 0, and curdle_last_error names vector, index and reason --
 * "Ss[17]: not in the prime-order subgroup" -- for the first failure in the order Rs, Ss, Ts, Us, M; the verifier's
 * own result is never reported for such an instance.  If every point passes, return code, *ok and error text are
 * those of the unchecked call.  A batch has a checked form of its own: curdle_verify_batch_checked below. */
int curdle_verify_checked(const curdle_crs* crs, const uint8_t* proof, size_t proof_len, const uint64_t* Rs,
                          const uint64_t* Ss, const uint64_t* Ts, const uint64_t* Us, size_t ell,
                          const uint64_t M[CURDLE_G1_JAC_U64], curdle_rand* rand, int* ok);
int curdle_verify_proof_checked(const curdle_crs* crs, const curdle_proof* proof, const uint64_t* Rs,
                                const uint64_t* Ss, const uint64_t* Ts, const uint64_t* Us, size_t ell,
                                const uint64_t M[CURDLE_G1_JAC_U64], curdle_rand* rand, int* ok);
/* The same membership check for gnark G1Jac values (n x 18 limbs: X, Y, Z in Montgomery form), the layout of the
 * verifier's M, of crs.H / Gt / Gu and of every []G1Jac a Go caller holds.  Nothing is normalised on the host and
 * nothing is inverted: the subgroup test runs from the projective coordinates.  Decided in this order: Z all zero words
 * -> INFINITY (gnark's rule for G1Jac: X and Y are not looked at); X, Y or Z >= p -> BAD_ENCODING; Y^2 != X^3 + 4 Z^6
 * -> NOT_ON_CURVE; with subgroup_check != 0, [z^2] phi(P) + P != inf -> NOT_IN_SUBGROUP; else OK.  Arguments, return
 * codes and the rule that picks the kernel build are those of curdle_g1_check_batch / _device. */
int curdle_g1_check_jac_batch(const uint64_t* jac_points, size_t n, int subgroup_check, uint8_t* status);
int curdle_g1_check_jac_batch_device(const void* d_jac_points, size_t n, int subgroup_check, uint8_t* status, void* stream);
/* Batched normalisation and compression ON THE GPU: n gnark G1Jac values (n x 18 limbs: X, Y, Z in Montgomery form) ->
 * n x 48 bytes of gnark's compressed encoding (G1Affine.Bytes), byte for byte what curdle_g1_compress writes for each
 * point; the counterpart of curdle_g1_decompress_batch.  Z all zero words is infinity (0xC0 and 47 zero bytes, whatever
 * X and Y hold); otherwise x = X / Z^2 is written big-endian with the flag 0xA0 if y = Y / Z^3 > (p - 1) / 2 and 0x80
 * otherwise.  One inversion per point (Fermat, a fixed chain), one lane per point.  Nothing is checked: the points are
 * taken as curdle_g1_compress takes them (coordinates below p; curdle_g1_check_jac_batch is the check).
 * n = 0: CURDLE_OK, nothing touched, no device needed; a null pointer with n > 0, or n > 2^27: CURDLE_EINVAL before
 * anything is copied or launched.  No host fallback: without a device the call fails with CURDLE_ENODEV.
 *   curdle_g1_compress_batch          points and bytes in host memory
 *   curdle_g1_compress_batch_device   both resident in device memory (HIP device pointers, ANY alignment); `stream` is
 *                                     a hipStream_t or NULL for the library's own stream, as in curdle_msm_g1_device:
 *                                     the points are read and the bytes written in that stream's order, so the points
 *                                     may have been written on it immediately before.  The bytes stay in device
 *                                     memory; they are complete when the call returns. */
int curdle_g1_compress_batch(const uint64_t* jac_points, size_t n, uint8_t* out);
int curdle_g1_compress_batch_device(const void* d_jac_points, size_t n, void* d_out, void* stream);
/* Batched normalisation ON THE GPU with a SHARED inversion: gnark's BatchJacobianToAffineG1, which the reference calls
 * in 25 places (transcript/transcript.go:26, innerproductargument.go:238-280, ...).  n points in one of two forms ->
 * n gnark G1Affine records (12 limbs: x then y, canonical Montgomery limbs), the layout of every base array of this
 * library (curdle_msm_g1_device, curdle_dbases_create): a device result can be the next call's device input, where
 * the reference copies down, normalises on one core and copies back up (common/util.go:55-82, the fold steps and
 * MultiExps of the inner-product and same-multiscalar arguments).
 *   CURDLE_G1_FORM_JAC   gnark G1Jac, 18 limbs (X, Y, Z): x = X / Z^2, y = Y / Z^3; the denominator is Z
 *   CURDLE_G1_FORM_XYZZ  24 limbs (X, Y, ZZ, ZZZ), what the point kernels of this library write: x = X / ZZ,
 *                        y = Y / ZZZ for any non-zero ZZ and ZZZ; the denominator is ZZ ZZZ
 * A point whose denominator is 0 mod p (decided on the reduced value: limbs that spell p count, and so does ZZ != 0
 * with ZZZ = 0) is infinity whatever X and Y hold, and comes out as 12 zero limbs; it takes no part in the inversion
 * its neighbours share.  One Fermat inversion serves a wave of 64 lanes with one point each (up to 65,536 points) or
 * eight (beyond).  Nothing is checked: coordinates are taken as below 2^384 and the points as they are.
 * n = 0: CURDLE_OK, nothing touched, no device needed.  Refused with CURDLE_EINVAL before anything is copied or
 * launched: a null pointer with n > 0, an unknown form, n > 2^24, a device pointer that is not a multiple of 16 (any
 * element offset into a hipMalloc'd array is one: 144, 192 and 96 are multiples of 16).  No host fallback: without a
 * device the call fails with CURDLE_ENODEV.
 *   curdle_g1_normalize_batch          points and records in host memory, in passes of 2^20 points
 *   curdle_g1_normalize_batch_device   both resident in device memory and not overlapping; `stream` is a hipStream_t
 *                                      or NULL for the library's own stream, as in curdle_g1_compress_batch_device:
 *                                      the points are read and the records written in that stream's order, and the
 *                                      records are complete when the call returns. */
#define CURDLE_G1_FORM_JAC 0
#define CURDLE_G1_FORM_XYZZ 1
int curdle_g1_normalize_batch(const uint64_t* points, int form, size_t n, uint64_t* out_affine);
int curdle_g1_normalize_batch_device(const void* d_points, int form, size_t n, void* d_out_affine, void* stream);
/* curdle_g1_scalar_mul_batch with everything resident: d_out_affine[i] = d_addends[i] + d_scalars[i] * d_points[i],
 * i < n, gnark affine records in and out ((0, 0) = infinity), Montgomery fr.Elements; n_scalars = n, or 1 for one
 * shared scalar; d_addends may be NULL.  The multiplications run into the library's workspace and are normalised from
 * there with the shared inversion above, so d_out_affine may be d_points or d_addends (in place) and may go straight
 * to curdle_msm_g1_device as bases.  `stream`, completion and the pointer rule (every device pointer a multiple of
 * 16) are those of curdle_g1_normalize_batch_device; n > 2^24 or n_scalars neither n nor 1: CURDLE_EINVAL before any
 * device work.  Like curdle_g1_scalar_mul_batch it is NOT constant time in the scalars (the chain branches on their
 * bits), and the workspace that held the unnormalised results is not wiped: for secret scalars there is
 * CURDLE_G1_MUL_CONSTANT_TIME on the _ex forms below. */
int curdle_g1_scalar_mul_batch_device(const void* d_points, const void* d_scalars, size_t n_scalars,
                                      const void* d_addends, size_t n, void* d_out_affine, void* stream);
/* curdle_g1_scalar_mul_batch and curdle_g1_scalar_mul_batch_device with a flags word.  flags = 0 IS the call without
 * flags: same kernel, same counters, same bytes.  A bit that is not defined here: CURDLE_EINVAL before anything else
 * is looked at, copied or launched, also with n = 0.
 *
 * CURDLE_G1_MUL_CONSTANT_TIME: out[i] = scalars[i or 0] * points[i] by a second kernel (csrc/g1_mul_ct_kernels.hip), one
 * lane per pair: the 255 bits of the scalar MSB first, every step one doubling and ALWAYS one mixed addition of the
 * lane's own point, the new accumulator taken by mask selection; the lane then normalises its own result (one
 * fixed-exponent inversion) and writes the canonical affine record through a mask, so k = 0 or an infinity point
 * stores twelve zero words and NOTHING unnormalised leaves the kernel: no normalisation kernel runs.  The records are
 * bit for bit those of the call without flags.
 * addends must be NULL: CURDLE_EINVAL before any device work otherwise (a final addition addend + k P can be
 * exceptional depending on the secret).  n_scalars is n or 1.  d_out_affine may be d_points: a lane reads its record
 * before it writes it.  Limits (n <= 2^24), the pointer rule, n = 0, CURDLE_ENODEV and the stream semantics are those
 * of the calls without flags.  The call works in passes of at most CURDLE_G1_MUL_CT_PASS pairs (knob; 1,048,576;
 * rounded down to a multiple of 256, at least 256), one launch each.  The host form stages the scalars through pinned
 * memory and a device buffer and overwrites both, on the stream that used them, before it returns on every path; the
 * device form reads the caller's scalars where they are and copies nothing.  points must be in the prime-order
 * subgroup for the result to be right and are NOT checked (the kernel's exactness argument needs the subgroup); any
 * other input gives an unspecified record and no fault.
 * WHAT THE FLAG PROMISES: the kernel's instruction stream (every branch, every exec mask beyond the end-of-array guard,
 * every loop count) and its address stream (every load and store address) are independent of the values of scalars;
 * they depend on n, n_scalars, the pointers and on which points are infinity, which is public.  The host only copies
 * scalars and never looks at them.
 * WHAT IT DOES NOT PROMISE: anything about data-dependent power draw and clock behaviour of the chip (a multiplier fed
 * zeros draws less), which is not addressed; and nothing about the default path, whose warning above stays true.
 * Cost: 255 doublings, 255 additions and an inversion in ONE lane per pair, a chain of about 5,300 dependent field
 * products: measured 5.3 ms for any n up to 65,536 and 1.3 times the default call from there (profiles/r24_g1_mul_ct.json). */
#define CURDLE_G1_MUL_CONSTANT_TIME 1u
int curdle_g1_scalar_mul_batch_ex(const uint64_t* points, const uint64_t* scalars, size_t n_scalars,
                                  const uint64_t* addends, size_t n, unsigned flags, uint64_t* out_affine);
int curdle_g1_scalar_mul_batch_device_ex(const void* d_points, const void* d_scalars, size_t n_scalars,
                                         const void* d_addends, size_t n, unsigned flags, void* d_out_affine, void* stream);
/* out[0] scalars multiplied by k_g1_mul_ct, out[1] its launches; completed passes only.  A pass under
 * CURDLE_G1_MUL_CONSTANT_TIME (or the rG column of a pass under CURDLE_TRACKER_PROVE_CONSTANT_TIME) counts here and
 * NOT in curdle_stat_normalize: it runs no normalisation kernel. */
int curdle_stat_g1_mul_ct(unsigned long long out[2]);
/* -------------------------------------------------------------------------
 * Batched inversion in Fp, CONSTANT TIME in the elements: out[i] = in[i]^-1 for i < n, and 0 gives 0 (gnark's
 * fp.Element.Inverse; for a whole vector, what fp.BatchInvert returns).  Items are gnark fp.Elements: 48 bytes,
 * Montgomery, canonical, in and out.  One lane per element (k_fp_invert, csrc/fp_invert_kernels.hip), one launch per
 * 2^20 elements, and the inversion is Bernstein-Yang's division steps (csrc/invert_ds.h): from (delta, f, g) = (1, p, x)
 * a FIXED 1,110 steps -- the paper's bound for 381 bits is 1,101 -- of shifts, additions and masks on the low bits, in 37
 * batches of 30, each followed by one 2 x 2 matrix on the full-width values; the step's two cases are taken by masks.
 * out may be in (a lane reads its item before it writes it and touches no other).
 * flags: CURDLE_FP_INVERT_FERMAT takes the exponent chain x^(p-2) of the point kernels (csrc/invert28.h) instead: the
 * control, bit-identical results.  CURDLE_FP_INVERT_RAW28 is a diagnostic form: items are the 14 uint32 limbs of the
 * library's internal field layer (csrc/fp28.h: 28 bits a limb, Montgomery radix 2^392), 56 bytes, normalised and below
 * 2p going in, canonical coming out -- the form in which the exit of the constant-time MSM calls the inversion.  A bit
 * that is not defined here: CURDLE_EINVAL.
 * An element at or above p (raw form: a value at or above 2p, or a limb at or above 2^28) makes the call fail with
 * CURDLE_EINVAL and, in the host form, out untouched (the _device form has written d_out by then: its contents are
 * unspecified): the lanes OR a violation word into one status word, without a branch, and the host reads that word.
 * THIS VERDICT IS THE ONLY THING ABOUT THE ELEMENTS THE CALL REVEALS.
 * Refusals happen before any device work, in this order: an unknown flag bit, a null pointer with n > 0, n > 2^24, and
 * (the _device form) device pointers that are not multiples of 16.  n = 0 then returns CURDLE_OK without a device.  No
 * host fallback: without a device the call fails with CURDLE_ENODEV.  `stream` is as in curdle_msm_g1_device (the
 * caller's stream, or NULL for the library's); the call returns when its work is done.  One MSM slot is held for the call.
 * The host form stages the elements through pinned memory into a device buffer, inverts them there and brings them back
 * only behind a clean verdict; the buffer and both stagings are overwritten on the stream that used them before it
 * returns on every path.  The device form copies nothing but the status word.
 * WHAT THE FLAG PROMISES (with or without a flag: both inversions are constant-time forms): the kernel's instruction
 * stream (every branch, every exec mask beyond the end-of-array guard, every loop count) and its address stream (every
 * load, store and atomic address) are independent of the values of the elements; they depend on n, flags and the
 * pointers.  The host only copies the elements and never looks at them; of what the device computed it reads the
 * violation word and the result.
 * WHAT IT DOES NOT PROMISE: anything about data-dependent power draw and clock behaviour of the chip (a multiplier fed
 * zeros draws less), which is not addressed.
 * OUTSIDE THE PROMISE: the result itself and the verdict on the range; whatever the caller does with the elements
 * before and after.
 * curdle_stat_fp_invert: out[0] completed calls that ran on a device, out[1] elements in them; out[2] and out[3] count
 * the finish launches of the constant-time MSM (k_msm_ct_finish / _seg, every caller of curdle_msm_g1_ct and its
 * batched and resident-base forms) whose exit inverted by division steps (k_msm_ct_finish_ds / _seg_ds) and on the
 * Fermat chain.  The knob CT_FINISH_DIVSTEPS (curdle_plan_override) chooses: 1 always division steps, 0 never; unset,
 * the library's rule, which is division steps since round 37 measured them.  The result is bit for bit the same either
 * way.
 * Cost: an instruction count, NOT a measurement, of about 25 to 30 thousand 32/64-bit integer instructions per element
 * against about 265 thousand for the Fermat chain; measured (profiles/r37_invert_ds.json) 0.11 / 0.16 / 0.86 / 12.0 ms at
 * n = 64 / 4,096 / 65,536 / 2^20 against 0.50 / 0.54 / 1.27 / 13.6 ms under CURDLE_FP_INVERT_FERMAT; the finish kernel
 * 0.34 against 0.80 ms over one segment of 256 terms and 3.93 against 11.03 ms over 4,096 segments of 16.
 * ------------------------------------------------------------------------- */
#define CURDLE_FP_INVERT_FERMAT 1u   /* the existing chain of invert28.h: the control, bit-identical results */
#define CURDLE_FP_INVERT_RAW28  2u   /* diagnostic: items are 14 u32 internal limbs (radix 2^392), normalised, < 2p */
int curdle_fp_invert_batch(const uint64_t* in, size_t n, uint64_t* out, unsigned flags);
int curdle_fp_invert_batch_device(const void* d_in, size_t n, void* d_out, unsigned flags, void* stream);
int curdle_stat_fp_invert(unsigned long long out[4]);
/* -------------------------------------------------------------------------
 * Constant-time MSM for SECRET scalars: out = sum_i scalars[i] * points[i], the result bit for bit the 18 words
 * curdle_msm_g1 returns on the same input (canonical (x, y, 1), or its encoding of infinity).  curdle_msm_g1 is NOT
 * constant time in the scalars: its sort, its bucket addresses and its large-bucket queue are functions of them.  Here
 * (csrc/msm_ct_kernels.hip) one lane per pair walks the low scalar_bits bits of its scalar MSB first (k_msm_ct_walk:
 * every step one doubling and ALWAYS one mixed addition, the accumulator taken by mask selection, the walk of
 * CURDLE_G1_MUL_CONSTANT_TIME's kernel) and leaves its term k_i P_i unnormalised in a device workspace; the terms are
 * folded in a FIXED order (k_g1_sum_ct: h = ceil(m / 2), term[i] += term[i + h] for i < m - h, m <- h until m = 1) by ONE
 * complete addition that computes the sum, the double and four masks every time and takes b, a, the double, infinity or
 * the sum by mask arithmetic (csrc/g1_add_ct.h); one lane normalises the last term (k_msm_ct_finish, a fixed-exponent
 * inversion) and writes the result through a masked canonical step.
 * Layouts are curdle_msm_g1's: gnark G1Affine records with (0, 0) = infinity, Montgomery fr.Elements.
 * scalar_bits is the caller's PUBLIC bound on the scalars, 1...255 (0 or more: CURDLE_EINVAL); the walk takes that many
 * steps.  PRECONDITIONS, as for CURDLE_G1_MUL_CONSTANT_TIME: the bases lie in the prime-order subgroup and are NOT
 * checked (bases outside it give an unspecified result and no fault); the scalars are canonical, below r.
 * n <= 65,536 (one pass); more is CURDLE_EINVAL: larger sizes are not what secrets come in.  n = 0 returns the
 * infinity encoding without a device.  A scalar at or above 2^scalar_bits makes the call fail with CURDLE_EINVAL and
 * out_jac untouched: the lanes OR a violation word into one status word, without a branch, and the host reads that word
 * beside the result.  THIS VERDICT IS THE ONLY THING ABOUT THE SCALARS THE CALL REVEALS.
 * Refusals happen before any device work, in this order: a null argument, scalar_bits, n, and (the _device form) device
 * pointers that are not multiples of 16.  `stream` is as in curdle_msm_g1_device.  One MSM slot is held for the call.
 * The host form stages the scalars through pinned memory and a device buffer and overwrites both, and both forms
 * overwrite the term workspace (it holds k_i P_i), on the stream that used them, before they return on every path.
 * The call's only device-to-host copy is one block of 160 bytes: the 18 words and the violation word.
 * WHAT THE FLAG PROMISES (there is no flag: these entry points ARE the constant-time form): the instruction stream of
 * the kernels (every branch, every exec mask beyond the end-of-array guard, every loop count) and their address stream
 * (every load, store and atomic address) are independent of the values of scalars and of the terms made from them;
 * they depend on n, scalar_bits, the pointers and on which points are infinity, which is public.  The host only copies
 * scalars and never looks at them; of what the device computed it reads the violation word and the result.
 * WHAT IT DOES NOT PROMISE: anything about data-dependent power draw and clock behaviour of the chip (a multiplier fed
 * zeros draws less), which is not addressed; and nothing about curdle_msm_g1, whose warning above stays true.
 * OUTSIDE THE PROMISE: the result itself and the verdict on scalar_bits; whatever the caller does with the scalars
 * before and after.  It is NOT A DEFAULT: nothing in the library routes to it but curdle_shuffle_permute_commit_ex and
 * curdle_prove_ex, each under its flag.  (Since then also curdle_prove_ct and curdle_whisk_generate_shuffle_proof_ct,
 * below: entry points that ARE constant-time forms, not defaults either.)
 * Cost: one lane's chain of scalar_bits doublings and additions, then ceil(log2 n) levels of additions and one inversion:
 * measured 5.5 ... 6.8 ms at 255 bits and 0.9 ... 2.0 ms at 9 bits for n = 4 ... 65,536, 12 to 27 times curdle_msm_g1_device
 * (profiles/r27_msm_ct.json); the flagged shuffle step below 11.2 ... 12.0 ms at ell = 124 ... 508 against 1.4 ... 1.6 ms.
 * ------------------------------------------------------------------------- */
int curdle_msm_g1_ct(const uint64_t* points, const uint64_t* scalars, size_t n, unsigned scalar_bits, uint64_t out_jac[18]);
int curdle_msm_g1_ct_device(const void* d_points, const void* d_scalars, size_t n, unsigned scalar_bits, uint64_t out_jac[18], void* stream);
/* out[0] pairs walked by k_msm_ct_walk, out[1] its launches, out[2] sums finished; completed calls only. */
int curdle_stat_msm_ct(unsigned long long out[3]);
/* The constant-time MSM, BATCHED: k independent MSMs in ONE walk.  curdle_msm_g1_ct_batch is curdle_msm_g1_batch's shape:
 * `offsets` has k + 1 non-decreasing entries and MSM j covers the pairs [offsets[j], offsets[j+1]) of the concatenated
 * arrays; curdle_msm_g1_ct_multi is curdle_msm_g1_multi's: k base sets of n points against ONE scalar vector.  Layouts,
 * preconditions and scalar_bits (ONE public bound for the whole call) are curdle_msm_g1_ct's; out_jac receives k results
 * of 18 words, result j bit for bit what curdle_msm_g1_ct returns on MSM j alone (an empty MSM: the infinity encoding).
 * A walk costs one lane's chain whether it has 4 pairs or 65,536, so k_msm_ct_walk is launched ONCE over all the pairs
 * of the call; the terms are then folded per MSM, each segment in exactly the order of the single call, by a segmented
 * form of the sum (k_g1_sum_ct_seg: one launch per level for all segments still above 512 terms, from a PUBLIC table of
 * (begin, count) made of `offsets`; k_msm_ct_finish_seg: one block per MSM for the rest, the inversion and the masked
 * canonical step).
 * Limits: at most 65,536 pairs in all (one pass), k <= 4,096, for _multi k n <= 65,536.  k = 0 returns CURDLE_OK and
 * writes nothing; a call whose MSMs are all empty needs no device.  Refusals happen before any device work, in this
 * order: a null argument (offsets always; out_jac, the points and the scalars when k > 0), scalar_bits, k, offsets that
 * decrease, the total, and (the _device form) device pointers that are not multiples of 16; _multi: a null argument,
 * scalar_bits, k, k n, then a null base set.  A scalar at or above 2^scalar_bits ANYWHERE in the call fails the whole
 * call with CURDLE_EINVAL and EVERY word of out_jac stays untouched: there is one status word for the call, and this
 * verdict is the only thing about the scalars the call reveals.
 * One MSM slot is held for the call.  The terms, and for the host forms the scalar staging and its device copy (for
 * _multi: the k replicas of the scalar vector, a host copy of public length), are overwritten on the stream that used
 * them on every way out.  The call's only device-to-host copy is one block of 144 k bytes and the status word.
 * WHAT THE FLAG PROMISES, WHAT IT DOES NOT PROMISE and what is OUTSIDE THE PROMISE are curdle_msm_g1_ct's, word for word,
 * with "n" read as "k and the offsets": the instruction stream and the address stream of the three kernels depend on k,
 * the offsets, scalar_bits, the pointers and on which points are infinity, and on nothing made of the scalars.  It is
 * not a default: nothing routes to it but curdle_prove_ex under its flag.
 * A completed call that ran on the device moves curdle_stat_msm_ct by (pairs walked, 1, MSMs that are not empty). */
int curdle_msm_g1_ct_batch(const uint64_t* points, const uint64_t* scalars, const size_t* offsets, size_t k,
                           unsigned scalar_bits, uint64_t* out_jac);
int curdle_msm_g1_ct_batch_device(const void* d_points, const void* d_scalars, const size_t* offsets, size_t k,
                                  unsigned scalar_bits, uint64_t* out_jac, void* stream);
int curdle_msm_g1_ct_multi(const uint64_t* const* points_sets, size_t k, const uint64_t* scalars, size_t n,
                           unsigned scalar_bits, uint64_t* out_jac);
int curdle_stat_msm_ct_batch(unsigned long long out[3]);   /* batched calls | MSMs in them | level launches (k_g1_sum_ct_seg) */
/* -------------------------------------------------------------------------
 * The constant-time MSM over a RESIDENT, PUBLIC base set, the walk SPLIT INTO CHUNKS.  curdle_msm_g1_ct costs one lane's
 * chain of scalar_bits doublings and additions however few pairs it has.  Where the bases are public and stay -- a CRS,
 * the instance vectors of a proof -- the chain can be cut: k = sum_j 2^(c j) d_j with c-bit digits d_j, so
 * k P = sum_j d_j (2^(c j) P), and the points 2^(c j) P are public arithmetic on public bases, made once and kept.
 * curdle_ct_bases is the handle of that table; in the MSM over it (csrc/msm_ct_bases_kernels.hip) lane (pair, j) walks
 * only the c bits of d_j over its own table point, by the walk of curdle_msm_g1_ct, and the terms go through the same
 * fold (the complete addition: the terms of one pair are multiples of one another and can be equal or opposite) and
 * the same finish.  The chain is c steps instead of scalar_bits.
 *
 * THE HANDLE.  points: n gnark G1Affine records, (0, 0) = infinity.  PRECONDITIONS are curdle_msm_g1_ct's: the bases lie in
 * the prime-order subgroup and are NOT checked (curdle_g1_check_batch checks points for a caller who needs it).
 * chunk_bits is 8, 16, 32 or 64; 0 is the library's choice, 16.  The table is C = ceil(255 / chunk_bits) rows of n gnark
 * G1Affine records: row j holds 2^(chunk_bits j) P_i at table[j n + i], row 0 is the input, infinity stays the all-zero
 * record in every row.  It is built on the device (k_ct_bases_shift: one lane per base, chunk_bits doublings between
 * stores; k_g1_normalize writes the rows) and the handle keeps a host copy of the rows.  Limit: n C <= 65,536.  n = 0
 * gives an empty handle without a device.  Refusals happen before any device work, in this order: a null argument,
 * chunk_bits, n C, and (the _device form) a device pointer that is not a multiple of 16; each is CURDLE_EINVAL with
 * *out null; without a device the call returns CURDLE_ENODEV.  The _device form reads d_points behind what the caller
 * queued on `stream` (as in curdle_msm_g1_device) and keeps nothing of the caller's array.
 * Lifetime is curdle_fbase's and curdle_dbases': the handle stays usable until it is freed; its device copy is made on
 * another context at first use there and re-made after curdle_shutdown, both from the host copy; a free during a call
 * is deferred to that call's end.  THE TABLE IS PUBLIC: nothing of it is wiped, on the device or on the host.
 * curdle_ct_bases_export copies row `chunk` (n records) to the host, for callers who audit the table; chunk >= C is
 * CURDLE_EINVAL.
 *
 * THE MSM.  out = sum_p scalars[p] * P_rows[p]: the 18 words of curdle_msm_g1_ct and of curdle_msm_g1 on the same pairs,
 * bit for bit; the batch gives result j per MSM j over the pairs [offsets[j], offsets[j+1]), an empty MSM the infinity
 * encoding.  rows is always a HOST array of n PUBLIC indices into the base set (for the batch n is offsets[k]); null
 * means 0, 1, ..., n - 1, which requires n <= the set's size; indices may repeat; an entry at or above the size is
 * refused on the host before any device work.  The library stages rows itself: it is public and is not wiped.
 * scalar_bits is ONE public bound for the call, 1...255: Cb = ceil(scalar_bits / chunk_bits) chunks are walked and the
 * top chunk takes scalar_bits - chunk_bits (Cb - 1) steps.  A scalar at or above 2^scalar_bits ANYWHERE in the call
 * fails the whole call with CURDLE_EINVAL and EVERY word of out_jac stays untouched: one status word, as in
 * curdle_msm_g1_ct, and this verdict is the only thing about the scalars the call reveals.
 * Limits: n Cb <= 65,536 terms per call (one pass), k <= 4,096.  n = 0 returns the infinity encoding and k = 0 writes
 * nothing, both without a device, as does a batch whose MSMs are all empty.  Refusals happen before any device work, in
 * this order: a null argument (rows may be null; the scalars when n > 0; for the batch offsets always, out_jac and the
 * scalars when k > 0), scalar_bits, k, offsets that decrease, the term total, a row index out of range, and (the
 * _device forms) a device pointer that is not a multiple of 16.  `stream` is as in curdle_msm_g1_device.
 * One MSM slot is held for the call.  The host forms' scalar staging and its device copy, and in every form the term
 * workspace, are overwritten on the stream that used them on every way out, as in curdle_msm_g1_ct.  The call's only
 * device-to-host copy is the results and the status word: one block of 144 k + 4 bytes.
 * WHAT THE FLAG PROMISES, WHAT IT DOES NOT PROMISE and what is OUTSIDE THE PROMISE are curdle_msm_g1_ct's, word for word.
 * The instruction stream and the address stream also depend on rows, on chunk_bits and on which table points are
 * infinity, all of which are public.  It is not a default: nothing in the library routes to these calls yet unless the
 * caller asks for it by making a curdle_prover_ct (below), whose Proves send their MSMs to the sets form.
 * curdle_stat_msm_ct_bases: out[0] tables built on a device, out[1] calls, out[2] (pair, chunk) lanes walked by
 * k_msm_ct_walk_rows, out[3] MSMs finished that are not empty; completed calls that ran on a device only.  These calls
 * do not move curdle_stat_msm_ct (k_msm_ct_walk does not run); a batched one moves curdle_stat_msm_ct_batch by
 * (1, k, the level launches over count Cb terms per MSM).
 * Cost: profiles/r33_msm_ct_bases.json and DESIGN.md section 0, round 33.
 * ------------------------------------------------------------------------- */
typedef struct curdle_ct_bases curdle_ct_bases;
int curdle_ct_bases_create(const uint64_t* points, size_t n, unsigned chunk_bits, curdle_ct_bases** out);
int curdle_ct_bases_create_device(const void* d_points, size_t n, unsigned chunk_bits, curdle_ct_bases** out, void* stream);
void curdle_ct_bases_free(curdle_ct_bases* b);
size_t curdle_ct_bases_size(const curdle_ct_bases* b);          /* n */
unsigned curdle_ct_bases_chunk_bits(const curdle_ct_bases* b);  /* c */
int curdle_ct_bases_export(const curdle_ct_bases* b, unsigned chunk, uint64_t* rows_out /* n x 12 */);
int curdle_msm_g1_ct_bases(const curdle_ct_bases* b, const uint32_t* rows, const uint64_t* scalars, size_t n,
                           unsigned scalar_bits, uint64_t out_jac[18]);
int curdle_msm_g1_ct_bases_device(const curdle_ct_bases* b, const uint32_t* rows, const void* d_scalars, size_t n,
                                  unsigned scalar_bits, uint64_t out_jac[18], void* stream);
int curdle_msm_g1_ct_bases_batch(const curdle_ct_bases* b, const uint32_t* rows, const uint64_t* scalars,
                                 const size_t* offsets, size_t k, unsigned scalar_bits, uint64_t* out_jac);
int curdle_msm_g1_ct_bases_batch_device(const curdle_ct_bases* b, const uint32_t* rows, const void* d_scalars,
                                        const size_t* offsets, size_t k, unsigned scalar_bits, uint64_t* out_jac, void* stream);
int curdle_stat_msm_ct_bases(unsigned long long out[4]);  /* tables built | calls | (pair, chunk) lanes walked | MSMs finished */
/* The batch over UP TO FOUR resident sets in one call: a prover's MSM mixes bases of several public sets -- a CRS, made
 * once and kept, and the instance vectors of one proof -- and re-building the first inside a combined table per proof
 * would throw away what the handle is for.
 * sets: n_sets handles, 1 ... CURDLE_CT_BASES_MAX_SETS, all of one chunk_bits.  rows is a HOST array of PUBLIC indices
 * into the concatenation of the sets: set s covers [B_s, B_s + n_s) with B_0 = 0 and B_(s+1) = B_s + n_s; an empty set
 * covers nothing; rows may not be null when the call has pairs.
 * Result j is, bit for bit, what curdle_msm_g1_ct_bases_batch returns for the same rows, scalars and offsets over ONE
 * handle created from the concatenated points at the same chunk_bits -- and therefore what curdle_msm_g1_ct_batch and
 * curdle_msm_g1_batch return on those pairs.  Everything else is curdle_msm_g1_ct_bases_batch's: the limits (n Cb <= 65,536
 * terms, k <= 4,096), the one status word, out_jac untouched on a violation, the slot hold, the staging and the wiping,
 * the counters (curdle_stat_msm_ct_bases and curdle_stat_msm_ct_batch move exactly as for the single-handle batch on the
 * same pairs) and the promise: WHAT THE FLAG PROMISES, WHAT IT DOES NOT PROMISE and what is OUTSIDE THE PROMISE are
 * curdle_msm_g1_ct's, word for word.  The ONE walk kernel, k_msm_ct_walk_rows, takes the sets as an argument by value (table,
 * size and first index of each) and a call over one handle is its one-set case: a lane finds its set by at most three
 * compares of rows[p] against the B_s.  Addresses, branch conditions and loop counts stay functions of public values
 * only: rows, the sets' sizes, the chunk index, chunk_bits and scalar_bits.
 * Refusals happen before any device work, in this order: a null argument (sets, any sets[s] of the first four, offsets;
 * out_jac and the scalars when k > 0; rows when the offsets span a pair), n_sets = 0 or above 4, sets whose chunk_bits
 * differ, then the single-handle batch's order: scalar_bits, k, offsets that decrease, the term total, a row index at
 * or above B_(n_sets), and (the _device form) a device pointer that is not a multiple of 16.
 * Every handle of a call is held from before its device work to behind it: a free during the call is deferred, for
 * each of them, as for one handle.
 * Cost: the single-handle batch's on the same pairs: 1.383 against 1.385 ms at 256 pairs, 1.815 against 1.823 ms at 2,048
 * (profiles/r35_prove_ct_resident.json). */
#define CURDLE_CT_BASES_MAX_SETS 4
int curdle_msm_g1_ct_bases_sets_batch(const curdle_ct_bases* const* sets, size_t n_sets, const uint32_t* rows,
                                      const uint64_t* scalars, const size_t* offsets, size_t k,
                                      unsigned scalar_bits, uint64_t* out_jac);
int curdle_msm_g1_ct_bases_sets_batch_device(const curdle_ct_bases* const* sets, size_t n_sets, const uint32_t* rows,
                                             const void* d_scalars, const size_t* offsets, size_t k,
                                             unsigned scalar_bits, uint64_t* out_jac, void* stream);
/* curdle_prove with a flags word.  flags = 0 IS curdle_prove.  A bit that is not defined here: CURDLE_EINVAL before
 * anything else is looked at, with proof_out and *proof_len untouched.
 * CURDLE_PROVE_MSM_CONSTANT_TIME: every MSM of the proof -- the prover funnels them through three functions,
 * alg::MultiExp, MultiExpBatch and MultiExpShared (host/algebra.cpp) -- goes to curdle_msm_g1_ct, _ct_batch and
 * _ct_multi at scalar_bits = 255 instead of the bucket MSM, by a scoped switch on the calling thread.  The proof bytes
 * and rand's state afterwards are bit for bit those of the call without flags.
 * WHAT THE FLAG PROMISES: the DEVICE WORK OF PROVE'S MSMs, and only that, is curdle_msm_g1_ct's: the witness, the
 * blinders and the permuted challenges reach the device as MSM scalars of kernels whose instruction stream and address
 * stream do not depend on them, through staging that is overwritten on every way out; the host's concatenated copy of
 * a batch's scalars is overwritten too.
 * WHAT IT DOES NOT PROMISE: power draw and clock behaviour, as above; and NOTHING ABOUT THE HOST.
 * OUTSIDE THE PROMISE: the host-side operations of Prove on the same secrets are outside and run as they do without the
 * flag: the host Point::Mul calls on r_k, k, r_t and r_u and GroupCommitment::New, the Fr vector arithmetic (the
 * permutation of the challenges is an indexed gather by perm), the generation of the blinders, the ordinary heap
 * copies of the witness, and the alg::ScalarMulBatch calls (their scalars are public challenges).  DESIGN.md section 0
 * lists every one with its line.  They are the next follow-up.  (Built since as curdle_prove_ct, below: this flag's
 * promise is unchanged.)  Under CURDLE_PROVER_FOLD_BASES=1 the recursive provers
 * multiply H by a secret inner product on the host, so there the flagged call is refused with CURDLE_EINVAL.  Linked over
 * a backend without the constant-time MSM, and without a device, the flagged call fails with CURDLE_ENODEV: no fallback.
 * ell is bounded by the primitive: the largest batch of a round must fit 65,536 pairs.  It is not a default. */
#define CURDLE_PROVE_MSM_CONSTANT_TIME 1u
int curdle_prove_ex(const curdle_crs* crs, const uint64_t* Rs, const uint64_t* Ss, const uint64_t* Ts, const uint64_t* Us,
                    size_t ell, const uint64_t M[18], const uint32_t* perm, const uint64_t k[4], const uint64_t rs_m[16],
                    curdle_rand* rand, unsigned flags, uint8_t* proof_out, size_t cap, size_t* proof_len);
int curdle_stat_alg_msm(unsigned long long out[4]);   /* bucket-MSM calls | their pairs | constant-time calls | their pairs,
                                                         counted in alg::MultiExp / MultiExpBatch / MultiExpShared */
/* curdle_shuffle_permute_commit with a flags word.  flags = 0 IS that call.  A bit that is not defined here:
 * CURDLE_EINVAL before anything else is looked at, with the outputs untouched.
 * CURDLE_SHUFFLE_CONSTANT_TIME: the outputs and rand's state afterwards are bit for bit those of the call without
 * flags (the same draw of the blinders at the same point); only the device work differs.  Ts | Us: ONE launch of
 * CURDLE_G1_MUL_CONSTANT_TIME's kernel with the shared scalar k over the 2 ell records Rs | Ss, then an oblivious gather
 * (k_g1_permute_ct: every output lane reads all ell records and keeps the one whose index equals its perm[i] by a mask:
 * ell^2 record reads, no address made of perm).  M: k_msm_ct_walk over the CRS's Gs with the permutation as plain
 * uint32 scalars at bit_length(ell - 1) steps, a second walk over its Hs with the blinders at 255 steps into the same
 * workspace, ONE k_g1_sum_ct over the ell + 4 terms and the finish: M1 = sum perm[i] Gs[i], the UNBLINDED commitment to
 * the permutation, which the call without flags brings to the host, never exists outside the device workspace.
 * ell <= 4,096 under the flag (the gather is quadratic); more is CURDLE_EINVAL.  The range check of perm is the host's
 * existing one: a failing check reveals only that the input was invalid.  k, perm and the blinders' staging, the
 * unpermuted k R_i | k S_i and the term workspace are overwritten on every way out; the only device-to-host copies are
 * Ts | Us and the 160-byte block of M and the violation word.  A flagged call moves curdle_stat_g1_mul_ct by
 * (2 ell, 1), curdle_stat_msm_ct by (ell + 4, 2, 1) and curdle_stat_normalize not at all.
 * The promise, what it does not cover (power draw and clock behaviour) and what is outside it are those of
 * curdle_msm_g1_ct above, for k, perm and the blinders; the host's part outside the promise is the range check of perm,
 * the draw of the blinders from rand and the copies.  NOT covered: curdle_prove and curdle_whisk_generate_shuffle_proof,
 * whose MSMs see the same permutation and blinders on the default path.  It is not a default.  (Their constant-time
 * forms, built since: curdle_prove_ct and curdle_whisk_generate_shuffle_proof_ct, below.) */
/* The gather of the flagged step on its own, everything resident: d_out[i] = d_in[d_perm[i]] for i < n, 96-byte records,
 * d_perm n uint32 below n (an entry at or above n gives a zero record).  Every lane reads all n records; no address is
 * made of d_perm.  n <= 4,096; d_in and d_out multiples of 16 and not overlapping, d_perm a multiple of 4; `stream` as in
 * curdle_msm_g1_device; d_out is complete when the call returns.  Nothing is copied or wiped: the arrays are the caller's. */
int curdle_g1_permute_ct_device(const void* d_in, const void* d_perm, size_t n, void* d_out, void* stream);
#define CURDLE_SHUFFLE_CONSTANT_TIME 1u
int curdle_shuffle_permute_commit_ex(const curdle_crs* crs, const uint64_t* Rs, const uint64_t* Ss, size_t ell,
                                     const uint32_t* perm, const uint64_t k[4], curdle_rand* rand, unsigned flags,
                                     uint64_t* Ts_out, uint64_t* Us_out, uint64_t M_out[18], uint64_t rs_m_out[16]);
/* The oblivious gather over 32-byte records: out[i] = in[perm[i]] for i < n with perm SECRET; an entry at or above n gives
 * a zero record.  The records are bytes to it (Prove hands it fr.Elements, it knows nothing of the field).  The kernel,
 * k_fr_permute_ct (csrc/msm_ct_kernels.hip), is k_g1_permute_ct's body at another record size: lane i loads its own
 * perm[i], walks j = 0 ... n - 1, reads record j and keeps it under a mask made of perm[i] ^ j: n^2 record reads.
 * n <= 4,096 (the gather is quadratic; the shuffle step's cap): more is CURDLE_EINVAL.  n = 0 returns CURDLE_OK without a
 * device, looks at no pointer and writes nothing.  Refusals happen before any device work, in this order: a null
 * argument, n, and (the _device form) d_in / d_out that are not multiples of 16 or that overlap and a d_perm that is
 * not a multiple of 4.  `stream` is as in curdle_msm_g1_device; d_out is complete when the call returns.  One MSM slot is
 * held for the call.  The host form stages perm and the output through the slot's pinned memory and device buffers and
 * overwrites all four, on the stream that used them, on every way out; the input's staging is not overwritten (a caller
 * whose records are secret too uses the _device form on arrays it wipes itself).  The _device form copies and wipes
 * nothing: the arrays are the caller's.
 * WHAT THE FLAG PROMISES (there is no flag: these entry points ARE the constant-time form): no address, branch, loop
 * count or exec mask of the kernel is made of perm or of the records; they depend on n and the pointers.  The host only
 * copies perm and never looks at it.
 * WHAT IT DOES NOT PROMISE: power draw and clock behaviour, as for curdle_msm_g1_ct.
 * OUTSIDE THE PROMISE: the output itself; whatever the caller does with perm before and after.  It is not a default:
 * nothing routes to it but curdle_prove_ct. */
int curdle_fr_permute_ct(const uint64_t* in, const uint32_t* perm, size_t n, uint64_t* out);
int curdle_fr_permute_ct_device(const void* d_in, const void* d_perm, size_t n, void* d_out, void* stream);
int curdle_stat_fr_permute_ct(unsigned long long out[2]);   /* records gathered | launches; completed calls only */
/* curdle_prove in constant-time form: the same arguments, the same proof bytes, rand in the same state afterwards (r_a,
 * r_b, r_k, r_t, r_u and every other draw at the same point); only where the computations on secrets run differs.  There
 * is no flags word.  The body is curdle_prove's under two scoped switches on the calling thread (Prove starts no
 * threads): CURDLE_PROVE_MSM_CONSTANT_TIME's, and a second one (alg::SecretOpsScope) under which
 *   - the twelve host Point::Mul calls on r_k, k, r_a, r_b, r_t, r_u are gone: each pair of GroupCommitment::New is one
 *     batch of four MSMs over six pairs, {Gt}, {R, H}, {Gu}, {S, H}, hence one walk; k R and r_k R never exist unblinded;
 *   - the two gathers by the secret permutation go to curdle_fr_permute_ct: two launches of ell records a Prove;
 *   - proof.A is ONE MSM over the ell + 4 pairs (Gs | Hs; permuted challenges | blinders) and the grand-product
 *     argument's C one MSM over (Gs | Hs; partial products | blinders): the commitments to the first halves alone,
 *     which curdle_prove brings to the host and blinds there, never leave the device workspace;
 *   - the scalar vectors this route creates are overwritten on every way out.
 * Refusals, in this order, with proof_out and *proof_len untouched and nothing drawn from rand: a null argument
 * (proof_out may be null, as for curdle_prove), ell against the CRS, ell > 4,096, CURDLE_PROVER_FOLD_BASES=1 (CURDLE_EINVAL,
 * curdle_prove_ex's message), and a backend without the primitives or no device: CURDLE_ENODEV, no fallback.
 * curdle_whisk_generate_shuffle_proof_ct is curdle_whisk_generate_shuffle_proof in that form: the same arguments and
 * rule for n, the same post-trackers and proof bytes, rand in the same state: GeneratePermutation and GetFr(k) in that
 * order, the batched decode (public), the shuffle step under CURDLE_SHUFFLE_CONSTANT_TIME, curdle_prove_ct, the
 * serialisation.  Its own copies of k, the permutation and the blinders are overwritten on every way out; without a
 * device: CURDLE_ENODEV.
 * WHAT THE FLAG PROMISES (there is no flag: these entry points ARE the constant-time form): on the device, what
 * curdle_msm_g1_ct, CURDLE_SHUFFLE_CONSTANT_TIME and curdle_fr_permute_ct promise; on the host, no branch, loop count or
 * memory address in Prove is made of the witness, the blinders or the permutation, except those listed as outside: what
 * the host still does with them is straight-line field arithmetic in mask form (f_add, f_sub, f_cond_sub, f_neg, fr_mul of
 * csrc/bls12_381.h), copies, and the draws.
 * WHAT IT DOES NOT PROMISE: power draw and clock behaviour, as above; and what the host compiler made of the mask
 * arithmetic (DESIGN.md section 0 records what the shipped x86 code of those five functions shows; read, not tested).
 * OUTSIDE THE PROMISE: rand's own code (GeneratePermutation is a Fisher-Yates that indexes by what it draws); the range
 * check of perm in the shuffle step (curdle_prove_ct, like curdle_prove, makes none: an entry at or above ell gathers a
 * zero record); `if (den.IsZero()) throw` and the constraint self-check in the inner-product argument's GenerateBlinders,
 * branches on a secret-derived value that are taken with negligible probability and reveal only that generation failed;
 * likewise the grand-product prover's self-check `IPA(C, D) != z`, never taken for a well-formed witness;
 * the prover's ordinary std::vector copies of the witness, which are not wiped; the proof itself.  Neither call is a
 * default: nothing routes to them.
 * curdle_stat_host_point_mul: calls of alg::Point::Mul on the CALLING THREAD since it started (a thread-local counter:
 * the batch verifiers multiply on many threads).  A curdle_prove makes 14, a curdle_prove_ct 2 -- Hcrs.Mul(beta) and
 * M.Mul(alpha), both by public challenges.
 * Cost: profiles/r29_prove_ct.json. */
int curdle_prove_ct(const curdle_crs* crs, const uint64_t* Rs, const uint64_t* Ss, const uint64_t* Ts, const uint64_t* Us,
                    size_t ell, const uint64_t M[18], const uint32_t* perm, const uint64_t k[4], const uint64_t rs_m[16],
                    curdle_rand* rand, uint8_t* proof_out, size_t cap, size_t* proof_len);
int curdle_whisk_generate_shuffle_proof_ct(const curdle_crs* crs, const uint8_t* pre_trackers, size_t n, curdle_rand* rand,
                                           uint8_t* post_trackers_out, uint8_t* proof_out);
int curdle_stat_host_point_mul(unsigned long long* out);   /* calls of alg::Point::Mul on the CALLING THREAD */
/* -------------------------------------------------------------------------
 * A CONSTANT-TIME PROVER HANDLE: curdle_prove_ct over resident base tables.  Every base of the prover's MSMs is public
 * and known before its scalars exist -- a CRS point, a record of Rs | Ss | Ts | Us, the point at infinity, the
 * aggregates R and S, and H_beta = beta H, a public multiple of a CRS point -- so each of the proof's MSMs can be the
 * chunked walk of curdle_msm_g1_ct_bases_sets_batch (chunk_bits steps a lane) instead of a lone 255-step chain.
 * These are new entry points, not new flag bits; curdle_prove_ct, curdle_prove_ex, curdle_prove_batch and every other
 * entry point keep their behaviour and their counters, and nothing becomes a default.
 *
 * curdle_prover_ct_create builds ONE table over Gs | Hs | H | Gt | Gu | one all-zero record of the CRS, by
 * curdle_ct_bases_create: ell + 8 records.  chunk_bits: 0 is the library's 16; 8, 16, 32 and 64 are accepted as there.
 * Lifetime, the copy on another context and the re-creation after curdle_shutdown are curdle_ct_bases's own.  THE CRS MUST
 * OUTLIVE THE HANDLE.  Refusals, in this order, with *out null: a null argument, chunk_bits, a CRS too large for one
 * table ((ell + 8) C > 65,536, C = ceil(255 / chunk_bits)), and no device or a backend without the primitives:
 * CURDLE_ENODEV, no fallback.  curdle_prover_ct_free(NULL) does nothing.
 *
 * curdle_prover_ct_prove: the contract is curdle_prove_ct's, word for word, with the handle in the CRS's place: the same
 * refusals in the same order (proof_out and *proof_len untouched, nothing drawn from rand), the same promise and what is
 * outside it, the same proof bytes, rand in the same state afterwards.  The body is curdle_prove_ct's under one more
 * scoped switch on the calling thread (alg::ResidentBasesScope): a registry of resident sets that starts as {the
 * handle's CRS set, this call's Rs | Ss | Ts | Us} -- the second made before the first MSM and before anything is drawn
 * from rand -- and receives {R, S} as a late set right after they exist.  Under it
 *   - MultiExp, MultiExpBatch and MultiExpShared resolve every base of a call to a row by the record's value (a hash
 *     map over PUBLIC points; nothing about a scalar reaches it) and make one curdle_msm_g1_ct_bases_sets_batch at 255
 *     bits; a call with a base that does not resolve, or too large for one pass, takes curdle_prove_ct's path;
 *   - the inner-product argument pushes H with the scalar s beta where it pushed H_beta = beta H with s: the same group
 *     element, the same canonical result.
 * The route depends on shapes and public points only.  If 4 ell C > 65,536 (ell > 1,024 at chunk_bits 16) the instance
 * vectors do not fit a table and the call runs exactly as curdle_prove_ct, with nothing resident: a public decision on
 * ell.  The per-call sets are freed on every way out.  The handle may be used by several threads at once: each call has
 * its own registry, and the CRS set is shared and read-only.
 * curdle_prover_ct_whisk_shuffle_proof is curdle_whisk_generate_shuffle_proof_ct with its Prove in that form; the
 * shuffle step is unchanged.
 * The instruction stream and the address stream also depend on the row lists, on chunk_bits and on which table points
 * are infinity, all of which are public.
 * curdle_stat_alg_msm_resident: out[0] funnel calls that went to the resident tables, out[1] their pairs, out[2] calls
 * under an active scope that took the old path, out[3] their pairs; curdle_stat_alg_msm's constant-time half counts both
 * routes.  Per proof through a handle: out[2] moves by 0, out[0] by curdle_stat_alg_msm's constant-time calls,
 * curdle_stat_msm_ct does not move, curdle_stat_msm_ct_bases' tables move by 2 (the instance set and the late set) and
 * curdle_stat_host_point_mul by 2.  The knob PROVE_RESIDENT_TERMS (curdle_plan_override) lowers the per-call term cap
 * for tests; 0 or a value above 65,536 means "not set".
 * Cost: 40.7 / 46.9 ms a Prove at ell = 124 / 252 against curdle_prove_ct's 143.0 / 154.8 ms in the same process, 3.0 / 3.6 ms
 * for the creation, the Whisk form 52.5 against 154.9 ms; about half of a Prove is the 24 / 26 calls' one-lane finish
 * (profiles/r35_prove_ct_resident.json and DESIGN.md section 0, round 35).
 * ------------------------------------------------------------------------- */
typedef struct curdle_prover_ct curdle_prover_ct;
int  curdle_prover_ct_create(const curdle_crs* crs, unsigned chunk_bits, curdle_prover_ct** out);
void curdle_prover_ct_free(curdle_prover_ct* p);
int  curdle_prover_ct_prove(curdle_prover_ct* p, const uint64_t* Rs, const uint64_t* Ss, const uint64_t* Ts,
                            const uint64_t* Us, size_t ell, const uint64_t M[18], const uint32_t* perm,
                            const uint64_t k[4], const uint64_t rs_m[16], curdle_rand* rand,
                            uint8_t* proof_out, size_t cap, size_t* proof_len);
int  curdle_prover_ct_whisk_shuffle_proof(curdle_prover_ct* p, const uint8_t* pre_trackers, size_t n, curdle_rand* rand,
                                          uint8_t* post_trackers_out, uint8_t* proof_out);
int  curdle_stat_alg_msm_resident(unsigned long long out[4]);  /* resident calls | their pairs | old-path calls under a scope | their pairs */
/* The oblivious gather for k members of one n in ONE launch (k_permute_ct_seg, csrc/msm_ct_kernels.hip: the single
 * gathers' body, block (x, j) serving member j): out[j n + i] = in[j n + perm[j n + i]] for i < n, j < k, over 32-byte
 * records (curdle_fr_permute_ct_batch, _batch_device) or 96-byte records (curdle_g1_permute_ct_batch_device).  An entry
 * at or above n gives a ZERO record, never another member's: the comparison is against t < n inside the member's own
 * segment.  Reads are k n^2 records.  Limits: n <= 4,096, k <= 4,096, k n <= 2^20.  k = 0 or n = 0 returns CURDLE_OK
 * without a device, looks at no pointer and writes nothing.  Refusals, alignment rules, slot hold, staging and wiping
 * are curdle_fr_permute_ct's over k n records, with k and then k n checked after n, and the host form also overwrites
 * the INPUT's pinned and device staging (a group's records may be secret); the promise is
 * curdle_fr_permute_ct's.  curdle_stat_fr_permute_ct moves by (k n, 1) for the 32-byte forms.  It is not a default:
 * nothing routes to it but curdle_prove_batch and curdle_whisk_generate_shuffle_proof_batch under their flag. */
int curdle_fr_permute_ct_batch(const uint64_t* in, const uint32_t* perm, size_t n, size_t k, uint64_t* out);
int curdle_fr_permute_ct_batch_device(const void* d_in, const void* d_perm, size_t n, size_t k, void* d_out, void* stream);
int curdle_g1_permute_ct_batch_device(const void* d_in, const void* d_perm, size_t n, size_t k, void* d_out, void* stream);
/* k proofs over one CRS at one ell, generated in lockstep.  Member i's arguments are Rs[i], Ss[i], Ts[i], Us[i] (ell
 * gnark G1Affine records each), Ms + 18 i, perms[i] (ell entries), ks + 4 i, rs_ms + 16 i and rands[i] (k distinct
 * generators); its proof goes to proofs_out + stride i (at most stride bytes), its length to proof_lens[i], its code to
 * status[i].  THE CONTRACT: member i's bytes, its length and the state of rands[i] afterwards are, bit for bit, those
 * of the single call on member i's arguments -- curdle_prove when flags = 0, curdle_prove_ct under
 * CURDLE_PROVE_BATCH_CONSTANT_TIME.
 * How: members run in groups of at most PROVE_BATCH_GROUP (a knob: default and maximum 64, lowered through
 * curdle_plan_override), one thread per member of a group, each running Prove's body; the device operations of the
 * members of a group meet at each step and go to the device as ONE coalesced call (alg::Lockstep, host/algebra.h: one
 * curdle_msm_g1_batch, or under the flag one curdle_msm_g1_ct_batch and one curdle_fr_permute_ct_batch), split by
 * whole members only where the primitive's limits require it (the knob PROVE_BATCH_PAIRS lowers that cap for tests).
 * So k constant-time proofs of a group cost about the walks of one.
 * Refusals happen before any thread starts, with nothing written and nothing drawn, in this order: an undefined flag
 * bit, a null argument (two members sharing one rand counts as one), ell against the CRS, and under the flag
 * curdle_prove_ct's own: ell > 4,096, CURDLE_PROVER_FOLD_BASES=1, a backend without the primitives or no device
 * (CURDLE_ENODEV, no fallback).  k = 0 is CURDLE_OK without a device.
 * A member that fails on its own gets its code in status[i] and proof_lens[i] = 0, and the others finish; the call
 * returns CURDLE_OK unless the failure was the device's, which fails every member of that step alike.
 * WHAT THE FLAG PROMISES: per member what curdle_prove_ct promises, with what it does not promise and what lies outside;
 * in addition the coalesced staging -- the concatenated host copies of the members' scalars, permutations and gathered
 * records that the group makes for a call -- is wiped like the single calls' staging, on every way out; the member
 * threads are the library's own, started and joined inside the call, and the scoped switches live on them alone.
 * Like curdle_prove_ct it is not a default: nothing routes to it.
 * curdle_whisk_generate_shuffle_proof_batch is curdle_whisk_generate_shuffle_proof for k pre-tracker arrays of one n
 * (pre_trackers[i]: n trackers; post_trackers_out + 96 n i and proofs_out + 4,576 i receive member i's results), under
 * CURDLE_PROVE_BATCH_CONSTANT_TIME curdle_whisk_generate_shuffle_proof_ct: per member the draws and their order are the
 * single call's (GeneratePermutation, then GetFr), all 2 n k tracker points go through ONE batched decode, the shuffle
 * steps and the Proves run in lockstep.  Under the flag each member's shuffle step is expressed through the same
 * funnels: the members share one constant-time multiplication launch over the k 2 n records, one batched gather and
 * one curdle_msm_g1_ct_batch; the normalised outputs are the flagged single step's bits.  ONE DIFFERENCE from the flagged
 * single step, which keeps the unpermuted k R_i | k S_i on the device: here they come back to the host between the
 * multiplication and the gather (beside the public Ts | Us they would give the permutation).  Every copy this call
 * makes of them -- the members' vectors, the group's concatenations, the gather's pinned and device input staging -- is
 * overwritten on every way out; the staging of curdle_g1_scalar_mul_batch_ex's output is wiped as that call promises.
 * A tracker that does not decode, or an n the single call refuses, gives that member the single call's error in
 * status[i] and leaves the others untouched; under the flag with CURDLE_PROVER_FOLD_BASES=1 every member gets
 * curdle_prove_ct's refusal (CURDLE_EINVAL, its text) where the single call meets it: behind the shuffle step and its
 * draws, before any prover work.  The call is then still CURDLE_OK, and curdle_last_error gives the text of the first
 * failed member's error.  What fails either batch call as a whole says which it was: a member thread that could not
 * be started (CURDLE_ENOMEM), a step at which the members' requests disagreed, or a failed device call.
 * curdle_stat_prove_batch: calls | members | groups | coalesced device calls, of both batch calls, completed or not. */
#define CURDLE_PROVE_BATCH_CONSTANT_TIME 1u
int curdle_prove_batch(const curdle_crs* crs, size_t k, size_t ell, const uint64_t* const* Rs, const uint64_t* const* Ss,
                       const uint64_t* const* Ts, const uint64_t* const* Us, const uint64_t* Ms /* k x 18 */,
                       const uint32_t* const* perms, const uint64_t* ks /* k x 4 */, const uint64_t* rs_ms /* k x 16 */,
                       curdle_rand* const* rands, unsigned flags, uint8_t* proofs_out, size_t stride, size_t* proof_lens,
                       int* status);
int curdle_whisk_generate_shuffle_proof_batch(const curdle_crs* crs, size_t k, const uint8_t* const* pre_trackers, size_t n,
                                              curdle_rand* const* rands, unsigned flags, uint8_t* post_trackers_out,
                                              uint8_t* proofs_out, int* status);
int curdle_stat_prove_batch(unsigned long long out[4]);   /* calls | members | groups | coalesced device calls */
/* Diagnostics: out[0] points normalised on the device since the library was loaded, out[1] inversion groups run
 * (one Fermat inversion each; at most one per 64 points of a launch). */
int curdle_stat_normalize(unsigned long long out[2]);
/* curdle_verify_batch with that check on every member's 4 ell instance points and on its M (range, curve equation,
 * subgroup), ON THE GPU and BESIDE the verification: producer threads gather the points of a chunk of members (at most
 * 32,768 points, so that the check runs on four lanes per point; only a single member beyond ell = 8,192 is more) into
 * pinned staging and run ONE affine and ONE Jacobian kernel per chunk, on a decode context when one is free and through
 * an MSM slot otherwise, ahead of the workers that verify.  The producers (4 from nthreads = 16, 2 from 8, else 1) are
 * threads of the `nthreads` budget, as the decoding's two are: from 8 threads the call runs nthreads threads in all,
 * below that at least two workers beside the producers.  Every instance point crosses the link once more; nothing is normalised or tested on the host.
 *   - A member with a failed point gets oks[i] = 0 and faults[i] = its first failure in the order Rs, Ss, Ts, Us, M
 *     (then the lowest index).  It is never verified: no transcript, no recording, no place in a group.
 *   - A point at infinity is acceptable, as in curdle_verify_checked.
 *   - Every other member has faults[i].code = 0 and the oks[i] curdle_verify_batch gives it on the same batch from the
 *     same `rand` state (the k seeds are drawn the same way, before anything else).
 *   - Return codes are curdle_verify_batch's.  On a negative return nothing reads as a verdict: oks[i] = 0 and
 *     faults[i].code = 0xff for every i.  k = 0: CURDLE_OK, no device needed.  faults may be NULL.
 *   - With several contexts the batch is sharded as the unchecked call shards it; each shard's check runs on its
 *     shard's context. */
typedef struct {
  uint8_t code;    /* CURDLE_DECODE_*; 0 or 1 = nothing wrong */
  uint8_t vector;  /* 0 Rs, 1 Ss, 2 Ts, 3 Us, 4 M */
  uint16_t pad;
  uint32_t index;  /* within the vector; 0 for M */
} curdle_point_fault;
int curdle_verify_batch_checked(const curdle_crs* crs, size_t k, const uint8_t* const* proofs, const size_t* proof_lens,
                                const uint64_t* const* Rs, const uint64_t* const* Ss, const uint64_t* const* Ts,
                                const uint64_t* const* Us, size_t ell, const uint64_t* Ms, curdle_rand* rand,
                                int nthreads, int* oks, curdle_point_fault* faults);
/* Diagnostics: out[0] checked batches since the library was loaded, out[1] members their point check rejected,
 * out[2] chunks checked. */
int curdle_stat_batch_checked(unsigned long long out[3]);
/* Diagnostics: checked verifications since the library was loaded whose point check out[0] ran on a decode
 * context beside the verification, out[1] found every decode context taken and ran to its end first.  out[1] also
 * counts every curdle_g1_check_batch / _jac_batch call (host or _device form) that reached the device: such a check
 * always runs to its end before the call returns.  A validated curdle_crs_from_points moves it by two, a TRUSTED one
 * moves nothing. */
int curdle_stat_check_paths(unsigned long long out[2]);

/* ------------------------------------------------------------------------------------------------
 * Batched Merlin transcripts.  ONE program of transcript operations runs over k members, each with
 * its own data: the part of a batch's Fiat-Shamir hashing that depends on input bytes only (the
 * verifier's prelude, curdleproof.go:217-224: 4 ell + 1 encodings appended, ell challenges drawn) is
 * the same program for every proof.  On the device (csrc/transcript_kernels.hip) every member's
 * STROBE-128 state lives in one lane's registers; the positions of the sponge depend on the program
 * alone, so the host compiles the program once per call into constants per rate word.
 *
 * A program is a list of steps:
 *   CURDLE_TR_APPEND      `count` messages of `len` bytes each under `label`, taken in order from the
 *                         member's data: Merlin's AppendMessage, which is what the reference's
 *                         AppendPoints (48-byte encodings) and AppendScalars (32 big-endian bytes)
 *                         do (transcript.go:32-46).
 *   CURDLE_TR_CHALLENGES  `count` times GetAndAppendChallenge(label) (transcript.go:48-58): 32
 *                         challenge bytes read as a big-endian integer, drawn again until it is
 *                         canonical (< r; equal to r is a rejection), then re-appended under the same
 *                         label.  Each writes its 32 big-endian bytes to the member's output.
 * Member i reads its messages back to back from data + i * data_stride and writes challenge j of the
 * program to challenges + (i * n_challenges + j) * 32.
 *
 * Exactly one of transcript_label (a fresh transcript.New(label) for every member, transcript.go:15)
 * and init_states (k exported states, CURDLE_TRANSCRIPT_STATE_SIZE bytes each) is given.  `states`,
 * if not NULL, receives every member's state after the program: the 200 STROBE state bytes, pos,
 * pos_begin, cur_flags and five zero bytes.  A state exported by either entry point continues in
 * either, so a program run whole equals the same program run as two calls.  The states of one call
 * must agree in pos, pos_begin and cur_flags (they do when they come from one earlier call).
 *
 * status[i] != 0: member i drew CURDLE_TRANSCRIPT_MAX_TRIES non-canonical values for one challenge
 * (probability 0.547^256); its challenges and state are then unspecified.  Every wait is bounded.
 * Knob TRANSCRIPT_MAX_TRIES (curdle_plan_override; a test hook) lowers this bound to min(256, value) in
 * both kernels and the host twin so that tests reach the status byte, and the single calls that settle
 * a handed-back member ignore it: they keep 256.
 *
 * CURDLE_EINVAL, before anything is copied or launched: an unknown op, label_len > 32, data_stride
 * below the bytes the program reads, both or neither of transcript_label and init_states, a limit
 * below exceeded, a null pointer that the call would use, states that are not exported states or
 * disagree in position.  k = 0 is CURDLE_OK.
 *
 * curdle_transcript_batch runs on the calling thread's device, on a stream and buffers of its own
 * (made at curdle_init; it takes neither an MSM workspace slot nor a decode context, so a caller may
 * hold those meanwhile), concurrent calls one behind the other.  Without a device it fails with
 * CURDLE_ENODEV: there is no fallback.  curdle_transcript_batch_host runs the same program through
 * the host's Transcript on nthreads threads and needs no device: the twin that tests and
 * measurements compare against.
 *
 * Two kernels run a tape, with the same bits out.  The lane kernel (csrc/transcript_kernels.hip) keeps a
 * whole state in one lane, up to 64 members per wave: the most members per second on a full chip, but a
 * call waits for a chain of about 7,000 dependent instructions per permutation however few members it
 * has.  The sheet kernel (csrc/transcript_sheet_kernels.hip, csrc/keccak_sheet.h) spreads a state's 25
 * words over 25 lanes, two members per wave, and exchanges words between lanes: a shorter chain, more
 * work per member.  Knob TRANSCRIPT_SHEET (CURDLE_TRANSCRIPT_SHEET, curdle_plan_override): 1 always the
 * sheet kernel, 0 never, unset the library's rule by batch size (choose_transcript_kernel in
 * csrc/transcript_api.hip, with the measurements it rests on); TRANSCRIPT_LANES set with
 * TRANSCRIPT_SHEET unset means the lane kernel.  Every caller of the launch follows the same rule: this
 * entry point, the tracker batches that hash on the device, the tracker prover. */
#define CURDLE_TRANSCRIPT_STATE_SIZE 208
#define CURDLE_TR_APPEND 1
#define CURDLE_TR_CHALLENGES 2
#define CURDLE_TRANSCRIPT_MAX_TRIES 256
#define CURDLE_TRANSCRIPT_MAX_MEMBERS 65536     /* k */
#define CURDLE_TRANSCRIPT_MAX_BYTES 1048576     /* bytes one member's program reads */
#define CURDLE_TRANSCRIPT_MAX_CHALLENGES 4096   /* challenges per member */
#define CURDLE_TRANSCRIPT_MAX_MESSAGES 65536    /* steps, and messages + challenges per member */
#define CURDLE_TRANSCRIPT_MAX_TOTAL 1073741824  /* device entry point: k x (bytes per member + 16) */
typedef struct {
  uint32_t op, count, len, label_len; /* len: CURDLE_TR_APPEND only */
  char label[32];
} curdle_transcript_step;
int curdle_transcript_batch(const char* transcript_label, const uint8_t* init_states, const curdle_transcript_step* steps,
                            size_t n_steps, const uint8_t* data, size_t data_stride, size_t k, uint8_t* challenges,
                            uint8_t* states, uint8_t* status);
int curdle_transcript_batch_host(const char* transcript_label, const uint8_t* init_states,
                                 const curdle_transcript_step* steps, size_t n_steps, const uint8_t* data,
                                 size_t data_stride, size_t k, uint8_t* challenges, uint8_t* states, uint8_t* status,
                                 int nthreads);
/* Diagnostics: out[0] members hashed on the device since the library was loaded, out[1] members handed back
 * with a non-zero status. */
int curdle_stat_transcript(unsigned long long out[2]);
/* Diagnostics: the kernel of the calling thread's device's last curdle_transcript_batch alone, by HIP events, in ms
 * (0 before the first call). */
int curdle_transcript_last_kernel_ms(double* out);
/* Diagnostics: members since the library was loaded whose transcripts out[0] the lane kernel hashed, out[1] the sheet
 * kernel -- counted at the launch, so every caller is in it, the tracker batches included. */
int curdle_stat_transcript_paths(unsigned long long out[2]);
/* The device's Keccak-f[1600] alone: `reps` dependent permutations of each of n states (25 little-endian u64 each,
 * host memory; states_out may be states_in).  form 0: a state per lane (what the lane kernel runs), one state per wave;
 * form 1: a state spread over lanes (what the sheet kernel runs), two states per wave.  *kernel_ms, if not NULL, receives
 * the kernel's time alone by HIP events.  Runs like a transcript call (its stream, its buffers, one call at a time).
 * CURDLE_EINVAL before any device work: a null array, form > 1, reps outside 1..CURDLE_KECCAK_PERMUTE_MAX_REPS,
 * n > CURDLE_KECCAK_PERMUTE_MAX_STATES; n = 0 is CURDLE_OK; CURDLE_ENODEV without a device.  For tests and for
 * measuring the chain of dependent permutations. */
#define CURDLE_KECCAK_PERMUTE_MAX_REPS 4096
#define CURDLE_KECCAK_PERMUTE_MAX_STATES 65536
int curdle_keccak_permute_batch(const uint64_t* states_in, size_t n, unsigned form, unsigned reps, uint64_t* states_out,
                                double* kernel_ms);
int curdle_set_last_error(int code, const char* msg);  /* internal: shared by the library's translation units */

/* ------------------------------------------------------------------------- *
 * Profiling and diagnostics (used by bench.py and tests; not part of the
 * reference's surface).
 * ------------------------------------------------------------------------- */
#define CURDLE_PROF_MAX_KERNELS 16 /* phases incl. the "(queue)" pseudo-phase */
typedef struct {
  int n_kernels;
  const char* name[CURDLE_PROF_MAX_KERNELS];
  float ms[CURDLE_PROF_MAX_KERNELS]; /* HIP-event time of each kernel, last MSM call */
  int window_bits;
  int num_windows;
  /* mode 1 only: sorted (pair, window) entries of the last call (zero digits dropped) and the
   * fragments the accumulate kernel emitted -- every fragment's first addition is a copy, so
   * the launch did entries - fragments real mixed additions */
  unsigned long long entries;
  unsigned long long fragments;
  /* mode 1 only: buckets of the last call with more fragments than its merge limit -- what the
   * scan counted for the large-bucket queue, beyond its capacity too (the call then fails) */
  unsigned long long large_buckets;
} curdle_profile;
/* on = 1: every MSM call brackets each kernel with hipEvents on the stream it launches on
 * and keeps the durations of the last call.  on = 2: only the dominant kernel (the bucket
 * accumulation) is bracketed -- two events instead of ten, which a pipelined caller does
 * not notice.  on = 0: off. */
int curdle_profile_enable(int on);
int curdle_profile_last(curdle_profile* out);
/* Diagnostics: what the library's plan decides about the bucket reduction of ONE device-resident MSM of n pairs over
 * windows [win_begin, win_end) (win_end = -1: up to the last; window_bits = 0: the library's choice), called
 * synchronously (pipelined = 0) or through submit / wait (1), under the knobs as they stand:
 *   out[0] 1 if the window leaves the GPU as bit-positioned points (no scalar multiple)
 *   out[1] 1 if the scatter runs in two passes   out[2] buckets per segment   out[3] segments per group
 *   out[4] segments of the call   out[5] the window width   out[6] the merge limit (fragments per bucket)
 *   out[7] sorted positions per accumulate lane
 * Nothing is launched and no device is needed.  CURDLE_EINVAL for arguments an MSM call would refuse. */
int curdle_msm_reduce_plan(size_t n, int window_bits, int win_begin, int win_end, int pipelined, uint32_t out[8]);
/* Diagnostics: the streams that pipelined calls (submit / wait) keep busy on a context created in a process with
 * `hw_queues` hardware queues (GPU_MAX_HW_QUEUES as the HIP runtime reads it; 4 when unset), for whole MSMs
 * (whole_or_range = 0) or window ranges (1), under the knobs as they stand (STREAM_PLAN, MAIN_STREAMS):
 *   out[0] the plan: 1 wide (every slot's tail on a stream of its own), 2 compact (one tail stream for all slots)
 *   out[1] accumulate streams   out[2] sort streams   out[3] tail streams
 * The plan of a context is chosen once, when it is created.  Nothing is launched and no device is needed.
 * CURDLE_EINVAL for hw_queues < 1 and for whole_or_range outside {0, 1}. */
int curdle_msm_stream_plan(int hw_queues, int whole_or_range, uint32_t out[4]);

/* Synthetic MSM bases of SURVEY.md section 8(d), generated on the GPU into
 * device memory: P_i = (k + i*q) * G for i < n, gnark G1Affine layout.  k and
 * q are canonical (non-Montgomery) 256-bit integers, little-endian limbs.
 * Because every P_i has a known discrete log, the exact MSM result at any n is
 * (k*sum(s_i) + q*sum(i*s_i)) * G, which is how full-size runs are checked. */
int curdle_synth_points_walk_device(const uint64_t k[4], const uint64_t q[4], size_t n, void* d_out);

/* Element-wise device self-test of the field / curve primitives, so tests can
 * compare the gfx950 arithmetic with the oracle operation by operation.
 *   op 0: fp_mul(a,b)      in: n x (12+12) u32-limbed Fp pairs, out: n x Fp
 *   op 1: fp_add  2: fp_sub  3: fp_sqr(a)
 *   op 4: fr_from_mont(a)  in: n x Fr pairs (b ignored), out: n x Fr
 *   op 5: xyzz madd: in: n x (XYZZ acc | XYZZ whose X,Y hold the affine addend), out: n x XYZZ
 *   op 6: xyzz add : in: n x (XYZZ | XYZZ),            out: n x XYZZ
 *   op 7: xyzz dbl : in: n x (XYZZ | XYZZ ignored),    out: n x XYZZ
 *   op 8 / 9: the same add / dbl through the lane-distributed ("quad") point operations the
 *             latency-bound kernels use (csrc/quad28.h); op 10: k * (second point) with a
 *             20-bit k derived from the element index, by the quads' double-and-add
 *   op 11: the GLV split every scalar goes through (csrc/bls12_381.h glv_split, run by k_digits and by
 *          the host's scalar multiplication): in: n x 8 words of a CANONICAL scalar k < r,
 *          out: n x (|k1| 4 words | k2 4 words | sign of the k1 term | sign of the k2 term,
 *          0x80000000 = negative), with k = +-|k1| +- k2 * lambda (mod r), both halves < 2^127
 *   op 12: the two ends of the curve change the MSM kernels make (csrc/fp28.h from_gnark_iso_x / _y:
 *          a base enters as (x / 16, y / 64) by shifts of its gnark words; to_gnark_msm: a result
 *          leaves through 2^388 / 2^390) on plain field elements: in: n x (Fp | Fp), out: n x
 *          (Fp | Fp | 1 if the x image is normalised and below 2p | the same for y); the round trip
 *          is the identity (the host build copies)
 *   op 13..16: the device-internal arithmetic (csrc/fp28.h, csrc/quad28.h, the constant-time G1 layer) on RAW internal limbs
 *          (14 x 28-bit limbs per field element, Montgomery radix 2^392, not reduced; no conversion
 *          on either side), so tests can drive every bound those functions state.  Word 0 of an item
 *          is a selector; an item with an unknown selector makes the call fail with CURDLE_EINVAL
 *          before anything is copied or launched.  Device only: on_device = 0 is CURDLE_EINVAL.
 *   op 13: in: sel | 3 pad | a | b | c | d (14 words each), out: r (14 words) | flag | pad.
 *          sel 0 mul_inl(a,b)  1 sqr_inl(a)  2 mul(a,b)  3 sqr(a) (the out-of-line calls)
 *          4 mul2_inl(a,b,c,d)  5 add(a,b)  6/7/8 sub<4/8/16>(a,b)  9/10/11 sub_raw<4/8/16>(a,b)
 *          12 dbl_raw(a)  13 triple_raw(a)  14 x3_fused(a,b,c)  15 norm(a)  16 canonical_lt2p(a)
 *          17 is_zero_lt2p(a) -> flag  18/19/20 cond_sub_pshl<1/2/3>(a)  21 to_gnark(a) and
 *          22..25 to_gnark_msm(a, role 0..3) -> 12 gnark words in r
 *   op 14: one-lane points: in: sel | k | top | pad | A (X28: X, Y, ZZ, ZZZ, 56 words) | B (X28),
 *          out: X28.  sel 0 madd<false>(A, B.x, B.y)  1 madd<true>(A, B.x, B.y)  2 add(A, B)
 *          3 dbl(A)  4 dbl_affine(A.x, A.y)  5 mul_small(B, k)
 *   op 15: the same layout through the quads: sel 0 q28::add(A, B)  1 q28::dbl(A)
 *          2 q28::dbl_outofline(A)  3 q28::mul_small(B, k, top) (top <= 31, k < 2^(top+1))
 *   op 16: the constant-time G1 layer (csrc/g1_walk_ct.h, g1_add_ct.h, g1_exit_ct.h, invert28.h and the fixed-base step
 *          of fbase_walk_ct.h) on raw limbs, each selector the production function of its header, by the rules of
 *          13..15 (device only; a bad selector fails before anything is copied or launched).  ALL items of one call
 *          share the selector (each selector is a kernel of its own): anything else is CURDLE_EINVAL, and so are a
 *          mask word of sel 8 / 9 that is neither 0 nor 0xffffffff and a step count of sel 11 outside 1..255.
 *          in: sel | arg0 | arg1 | pad | A (X28) | B (X28), out: 56 words | 4 flag words, unused words zero.
 *          sel 0 zero_mask(A.x) -> flag 0   1 finite_mask(A's first 24 words) -> flag 0
 *          2 equal_mod_p(A.x, A.y) -> flag 0 (A.x < 2p, A.y < 10p)
 *          3 / 4 / 5 to_gnark_ct<kToExt / kToExtX16 / kToExtY64>(A.x) -> 12 gnark words
 *          6 invert(A.x) -> 14 limbs   7 affine_words_ct(A) -> 24 gnark words
 *          8 madd_bit(A, B.x, B.y, bit = arg0, started = arg1)   9 madd_select(A, B.x, B.y, nz = arg0, started = arg1)
 *          10 add_ct(A, B) -> X28
 *          11 walk_ct: (x2, y2) = (A.x, A.y), the scalar is B's first 8 words (canonical), steps = arg0; the scalar is
 *          shifted left by 256 - steps as k_msm_ct_walk does it -> X28 | started (flag 0) | over (flag 1)
 * (limbs are passed as uint32 little-endian; 24/16/96/8/24/60/116 in and 12/8/48/10/26/16/56/60 out per item)
 * on_device = 0 runs the same header code on the host CPU (ops 0..12). */
int curdle_selftest_op(int op, const uint64_t* in, size_t n, uint64_t* out, int on_device);
/* Words per item operation `op` reads and writes: the ONE table the entry point above, its launcher
 * and its kernel index (a binding sizes its arrays from this instead of keeping a copy).
 * CURDLE_EINVAL for an op the library does not have. */
int curdle_selftest_shape(int op, uint32_t* in_words, uint32_t* out_words);

#ifdef __cplusplus
}
#endif
#endif /* CURDLE_MSM_H */
