// Batched Merlin transcripts on the device (curdle_transcript_batch): Keccak-f[1600] (keccak_dev.h) and the STROBE-128 subset
// Merlin uses (meta-AD, AD, PRF) as a plain sponge, one member's state per lane.
//
// What keeps it a plain sponge: every position is the same for all members (host/transcript_batch.h), so the host
// has compiled the program into a tape.  A block of the tape gives, per rate word, the constant framing bytes (op
// headers, labels, le32 lengths, RunF's marks) and where the member's own bytes enter (a u64 index and a bit shift
// into the member's row, a byte mask).  Lanes read the tape at wave-uniform addresses; absorbing is a statically
// unrolled loop over the 21 rate words, the 25 state lanes are never indexed dynamically, and members diverge in
// one place only: the number of times the retry loop of a challenge runs.
//
// The launch puts `mpw` members on the first lanes of each wave (the rule and its measurements: members_per_wave,
// transcript_api.hip).  The chain of ~500 dependent permutations is what a call waits for, and a wave repeats a try
// until ALL its members have an accepted draw.
#include <hip/hip_runtime.h>

#include <atomic>

#include "../host/knobs.h"
#include "../host/transcript_batch.h"
#include "keccak_dev.h"
#include "msm_kernels.h"

namespace curdle {

using transcript::kRateWords;
using transcript::TapeBlock;
using transcript::TapeCtl;
using transcript::TapeWord;

namespace {
// Blocks [first, first + n) of the pool into the state: per rate word the constants and, where the block says so,
// the member's bytes; Keccak-f where the block ends in one.  `first` and `n` are the same for every lane.
__device__ __forceinline__ void run_blocks(uint64_t st[25], const TapeBlock* pool, uint32_t first, uint32_t n, const uint64_t* row) {
  for (uint32_t b = 0; b < n; b++) {
    const TapeBlock* blk = pool + first + b;
#pragma unroll
    for (int w = 0; w < kRateWords; w++) {
      const TapeWord tw = blk->w[w];
      uint64_t x = tw.cmask;
      if (tw.dmask) {  // wave-uniform
        uint64_t v = row[tw.idx] >> tw.sh;
        if (tw.sh) v |= row[tw.idx + 1] << (64 - tw.sh);
        x ^= v & tw.dmask;
      }
      st[w] ^= x;
    }
    if (blk->run_f) keccak_f1600_dev(st);
  }
}

// PRF output: state bytes 0..31 out, and zeroed (Strobe128::Squeeze from position 0)
__device__ __forceinline__ void squeeze32(uint64_t st[25], uint64_t ch[4]) {
#pragma unroll
  for (int i = 0; i < 4; i++) {
    ch[i] = st[i];
    st[i] = 0;
  }
}

// The 32 bytes as a big-endian integer against r (fr.Element.SetBytesCanonical): equal to r is a rejection.
__device__ __forceinline__ bool canonical(const uint64_t ch[4]) {
  const uint64_t v3 = __builtin_bswap64(ch[0]), v2 = __builtin_bswap64(ch[1]), v1 = __builtin_bswap64(ch[2]), v0 = __builtin_bswap64(ch[3]);
  if (v3 != 0x73eda753299d7d48ull) return v3 < 0x73eda753299d7d48ull;
  if (v2 != 0x3339d80809a1d805ull) return v2 < 0x3339d80809a1d805ull;
  if (v1 != 0x53bda402fffe5bfeull) return v1 < 0x53bda402fffe5bfeull;
  return v0 < 0xffffffff00000001ull;
}

// kKnobBound: the retry bound is the kernel argument p.max_tries (test hook TRANSCRIPT_MAX_TRIES); otherwise the
// constant transcript::kMaxTries, the build every call takes while the knob is unset (launch_transcript_batch).
template <bool kKnobBound>
__global__ __launch_bounds__(64) void k_transcript_batch(TranscriptArgs p) {
  const uint32_t max_tries = kKnobBound ? p.max_tries : (uint32_t)transcript::kMaxTries;  // wave-uniform
  const uint32_t lane = threadIdx.x;
  if (lane >= p.mpw) return;
  const uint32_t m = blockIdx.x * p.mpw + lane;
  if (m >= p.k) return;
  uint64_t st[25];
  const uint64_t* init = p.init + (size_t)m * p.init_stride;
#pragma unroll
  for (int i = 0; i < 25; i++) st[i] = init[i];
  const uint64_t* row = p.data + (size_t)m * p.row_words;
  uint32_t status = 0;
  for (uint32_t ci = 0; ci < p.n_ctl; ci++) {
    const TapeCtl c = p.ctl[ci];
    if (c.kind == transcript::kBlocks) {
      run_blocks(st, p.pool, c.a, c.b, row);
      continue;
    }
    // GetAndAppendChallenge.  The first try's framing ended the blocks before; every later try starts at (32, 0).
    uint64_t ch[4];
    squeeze32(st, ch);
    for (uint32_t tries = 1; !canonical(ch); tries++) {
      if (tries == max_tries) {
        status = 1;
        break;
      }
      run_blocks(st, p.pool, c.a, c.b, row);
      squeeze32(st, ch);
    }
    // the re-append: its framing from (32, 0), then the 32 bytes at state byte c.d = 40 + label_len, in words 5..13
    const TapeBlock* app = p.pool + c.c;
#pragma unroll
    for (int w = 0; w < kRateWords; w++) st[w] ^= app->w[w].cmask;
    const uint32_t w0 = c.d >> 3, sh = (c.d & 7) * 8;
    uint64_t e[5] = {ch[0], ch[1], ch[2], ch[3], 0};
    if (sh) {
      e[0] = ch[0] << sh;
      e[1] = (ch[0] >> (64 - sh)) | (ch[1] << sh);
      e[2] = (ch[1] >> (64 - sh)) | (ch[2] << sh);
      e[3] = (ch[2] >> (64 - sh)) | (ch[3] << sh);
      e[4] = ch[3] >> (64 - sh);
    }
#pragma unroll
    for (int w = 5; w <= 9; w++)
      if (w0 == (uint32_t)w) {
#pragma unroll
        for (int j = 0; j < 5; j++) st[w + j] ^= e[j];
      }
    uint64_t* out = p.challenges + ((size_t)m * p.n_challenges + c.e) * 4;
#pragma unroll
    for (int i = 0; i < 4; i++) out[i] = ch[i];
  }
  if (p.states) {
    uint64_t* so = p.states + (size_t)m * 26;
#pragma unroll
    for (int i = 0; i < 25; i++) so[i] = st[i];
    so[25] = p.tail;
  }
  p.status[m] = (uint8_t)status;
}
std::atomic<unsigned long long> g_paths[2];  // members launched on k_transcript_batch | on k_transcript_sheet
}  // namespace

hipError_t launch_transcript_batch(const TranscriptArgs& caller, hipStream_t stream) {
  if (caller.k == 0) return hipSuccess;
  TranscriptArgs args = caller;
  args.max_tries = (uint32_t)knobs::transcript_max_tries();  // the one place: every launch of either kernel passes here
  hipError_t e;
  if (args.sheet) {
    e = launch_transcript_sheet(args, stream);
  } else {
    const uint32_t blocks = (args.k + args.mpw - 1) / args.mpw;
    if (args.max_tries == (uint32_t)transcript::kMaxTries)
      hipLaunchKernelGGL(k_transcript_batch<false>, dim3(blocks), dim3(64), 0, stream, args);
    else
      hipLaunchKernelGGL(k_transcript_batch<true>, dim3(blocks), dim3(64), 0, stream, args);
    e = hipGetLastError();
  }
  if (e == hipSuccess) g_paths[args.sheet ? 1 : 0].fetch_add(args.k, std::memory_order_relaxed);
  return e;
}

void transcript_path_counts(unsigned long long out[2]) {
  out[0] = g_paths[0].load(std::memory_order_relaxed);
  out[1] = g_paths[1].load(std::memory_order_relaxed);
}

}  // namespace curdle
