// The batched Merlin transcripts with every STROBE state spread over lanes (keccak_sheet.h): k_transcript_sheet reads
// the same TranscriptArgs and tape as k_transcript_batch (transcript_kernels.hip) and writes the same challenges,
// states and status bytes, bit for bit.  The chain of dependent permutations a call waits for is about five times
// shorter in instructions here; per member the kernel does far more work than 64 states per wave do, so which of the
// two a call takes is a rule (choose_transcript_kernel, transcript_api.hip).
//
// A wave holds two members, one per 32-lane half; lane w of a half holds state word w (w < 25).  Absorbing is by lane:
// lane w < 21 reads rate word w of a tape block, one load per block.  A challenge's 32 bytes are the words on lanes
// 0..3; whether they are canonical is made uniform per half by two ballots.  The halves' retry counts differ: the wave
// runs the retry blocks while either half needs a draw, on a copy of the word, and only a half that needs the draw
// takes the copy -- no state runs a block that its own transcript would not.  All 64 lanes stay active throughout
// (the exchanges and the ballots count on it): a half without a member computes on zeros and loads and stores nothing.
//
// Also here: the two kernels of curdle_keccak_permute_batch, `reps` dependent permutations of n states by
// keccak_f1600_dev (one state per lane, one state per wave) and by sheet_keccak_f1600 -- the tests' direct look at
// the permutation and the chain probe of tools/bench_transcript_sheet.py.
#include <hip/hip_runtime.h>

#include "../host/transcript_batch.h"
#include "keccak_dev.h"
#include "keccak_sheet.h"
#include "msm_kernels.h"

namespace curdle {

using transcript::kRateWords;
using transcript::TapeBlock;
using transcript::TapeCtl;
using transcript::TapeWord;

namespace {
// Blocks [first, first + n) of the pool into the lane's word.  `rate`: this lane holds a rate word of a member.
__device__ __forceinline__ uint64_t sheet_run_blocks(uint64_t a, const SheetLane& L, const TapeBlock* pool, uint32_t first, uint32_t n,
                                                     const uint64_t* row, bool rate) {
  for (uint32_t b = 0; b < n; b++) {
    const TapeBlock* blk = pool + first + b;
    if (rate) {
      const TapeWord tw = blk->w[L.w];
      uint64_t x = tw.cmask;
      if (tw.dmask) {
        uint64_t v = row[tw.idx] >> tw.sh;
        if (tw.sh) v |= row[tw.idx + 1] << (64 - tw.sh);
        x ^= v & tw.dmask;
      }
      a ^= x;
    }
    if (blk->run_f) a = sheet_keccak_f1600(a, L);  // wave-uniform
  }
  return a;
}

// The 32 bytes on lanes 0..3 of the half as a big-endian integer against r (fr.Element.SetBytesCanonical; equal to r
// is a rejection), the same answer on every lane of the half.  `rw`: the lane's word of r, most significant on lane 0.
__device__ __forceinline__ bool sheet_canonical(uint64_t ch, const SheetLane& L, uint64_t rw) {
  const uint64_t v = __builtin_bswap64(ch);
  const uint64_t lt = __builtin_amdgcn_ballot_w64(L.w < 4 && v < rw), eq = __builtin_amdgcn_ballot_w64(L.w < 4 && v == rw);
  const uint32_t l = (uint32_t)(lt >> (32 * L.half)), e = (uint32_t)(eq >> (32 * L.half));
  return (l & 1) || ((e & 1) && ((l & 2) || ((e & 2) && ((l & 4) || ((e & 4) && (l & 8))))));
}

// kKnobBound: as in k_transcript_batch -- the retry bound is p.max_tries under test hook TRANSCRIPT_MAX_TRIES, the
// constant transcript::kMaxTries otherwise.
template <bool kKnobBound>
__global__ __launch_bounds__(64) void k_transcript_sheet(TranscriptArgs p) {
  const uint32_t max_tries = kKnobBound ? p.max_tries : (uint32_t)transcript::kMaxTries;  // wave-uniform
  const SheetLane L = sheet_lane_setup();
  const uint32_t m = blockIdx.x * kSheetStatesPerWave + L.half;
  const bool live = m < p.k;  // per half
  const size_t mi = live ? m : 0;
  const bool rate = live && L.w < (uint32_t)kRateWords;
  const uint64_t* row = p.data + mi * p.row_words;
  const uint64_t rw = L.w == 0 ? 0x73eda753299d7d48ull : L.w == 1 ? 0x3339d80809a1d805ull : L.w == 2 ? 0x53bda402fffe5bfeull : 0xffffffff00000001ull;
  uint64_t a = 0;
  if (live && L.w < 25) a = p.init[mi * p.init_stride + L.w];
  uint32_t status = 0;
  for (uint32_t ci = 0; ci < p.n_ctl; ci++) {
    const TapeCtl c = p.ctl[ci];
    if (c.kind == transcript::kBlocks) {
      a = sheet_run_blocks(a, L, p.pool, c.a, c.b, row, rate);
      continue;
    }
    // GetAndAppendChallenge: squeeze32 is the words of lanes 0..3 out, and zeroed
    uint64_t ch = a;
    if (L.w < 4) a = 0;
    bool need = live && !sheet_canonical(ch, L, rw);
    for (uint32_t tries = 1; __builtin_amdgcn_ballot_w64(need) != 0; tries++) {
      if (tries == max_tries) {
        if (need) status = 1;
        break;
      }
      uint64_t t = sheet_run_blocks(a, L, p.pool, c.a, c.b, row, rate);
      const uint64_t drawn = t;
      if (L.w < 4) t = 0;
      if (need) {
        a = t;
        ch = drawn;
      }
      need = need && !sheet_canonical(ch, L, rw);
    }
    // the re-append: its framing from (32, 0), then the 32 bytes at state byte c.d = 40 + label_len, in words 5..13:
    // word w0 + j takes (ch[j] << sh) | (ch[j - 1] >> (64 - sh)) from lanes j and j - 1 of the half
    if (rate) a ^= p.pool[c.c].w[L.w].cmask;
    const uint32_t w0 = c.d >> 3, sh = (c.d & 7) * 8;
    const bool in = w0 >= 5 && w0 <= 9 && L.w >= w0 && L.w < w0 + 5;
    const uint32_t j = in ? L.w - w0 : 0;
    const uint32_t base = 4 * (32 * L.half);
    const uint64_t lo = sheet_fetch(ch, base + 4 * (j < 4 ? j : 0)), hi = sheet_fetch(ch, base + 4 * (j ? j - 1 : 0));
    if (in) {
      uint64_t e = 0;
      if (j < 4) e = lo << sh;
      if (j && sh) e |= hi >> ((64 - sh) & 63);
      a ^= e;
    }
    if (live && L.w < 4) p.challenges[((size_t)m * p.n_challenges + c.e) * 4 + L.w] = ch;
  }
  if (!live) return;
  if (p.states) {
    uint64_t* so = p.states + (size_t)m * 26;
    if (L.w < 25)
      so[L.w] = a;
    else if (L.w == 25)
      so[25] = p.tail;
  }
  if (L.w == 0) p.status[m] = (uint8_t)status;
}

// `reps` dependent Keccak-f on each of n states of 25 words: state m on lane 0 of wave m.  The other lanes permute
// zeros beside it (a wave's instructions cost the same), which keeps the state in vector registers as in
// k_transcript_batch: on one lane alone the compiler moves the whole permutation to the scalar unit.
__global__ __launch_bounds__(64) void k_keccak_permute_lane(const uint64_t* in, uint64_t* out, uint32_t n, uint32_t reps) {
  const uint32_t m = blockIdx.x;
  const bool holds = threadIdx.x == 0 && m < n;
  uint64_t st[25];
#pragma unroll
  for (int i = 0; i < 25; i++) st[i] = holds ? in[(size_t)m * 25 + i] : 0;
  for (uint32_t r = 0; r < reps; r++) keccak_f1600_dev(st);
  if (!holds) return;
#pragma unroll
  for (int i = 0; i < 25; i++) out[(size_t)m * 25 + i] = st[i];
}

// ... and two states per wave on the sheet
__global__ __launch_bounds__(64) void k_keccak_permute_sheet(const uint64_t* in, uint64_t* out, uint32_t n, uint32_t reps) {
  const SheetLane L = sheet_lane_setup();
  const uint32_t m = blockIdx.x * kSheetStatesPerWave + L.half;
  const bool word = m < n && L.w < 25;
  uint64_t a = 0;
  if (word) a = in[(size_t)m * 25 + L.w];
  for (uint32_t r = 0; r < reps; r++) a = sheet_keccak_f1600(a, L);
  if (word) out[(size_t)m * 25 + L.w] = a;
}
}  // namespace

// Called by launch_transcript_batch alone (transcript_kernels.hip), which has filled args.max_tries.
hipError_t launch_transcript_sheet(const TranscriptArgs& args, hipStream_t stream) {
  if (args.k == 0) return hipSuccess;
  const uint32_t blocks = (args.k + kSheetStatesPerWave - 1) / kSheetStatesPerWave;
  if (args.max_tries == (uint32_t)transcript::kMaxTries)
    hipLaunchKernelGGL(k_transcript_sheet<false>, dim3(blocks), dim3(64), 0, stream, args);
  else
    hipLaunchKernelGGL(k_transcript_sheet<true>, dim3(blocks), dim3(64), 0, stream, args);
  return hipGetLastError();
}

hipError_t launch_keccak_permute(const uint64_t* in, uint64_t* out, uint32_t n, uint32_t reps, int sheet, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  if (sheet)
    hipLaunchKernelGGL(k_keccak_permute_sheet, dim3((n + kSheetStatesPerWave - 1) / kSheetStatesPerWave), dim3(64), 0, stream, in, out, n, reps);
  else
    hipLaunchKernelGGL(k_keccak_permute_lane, dim3(n), dim3(64), 0, stream, in, out, n, reps);
  return hipGetLastError();
}

}  // namespace curdle
