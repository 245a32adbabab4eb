// Batched Merlin transcripts (curdle_transcript_batch / _host, include/curdle_msm.h): ONE program of
// transcript operations run over k members' data.  This header is what the host twin (transcript.cpp)
// and the device entry point (csrc/transcript_api.hip) share: the validation of a call and the
// compilation of a program into a tape of STROBE rate blocks.
//
// Why a tape: every position of the sponge is the same for all members.  pos and pos_begin depend on
// the program only, never on data; after a challenge try they are (32, 0) however many tries went
// before (the PRF's forced F resets them, then 32 bytes are squeezed); after the re-append of an
// accepted challenge under a label of L bytes they are (72 + L, 39 + L).  So the framing bytes (op
// headers, labels, le32 lengths, RunF's marks at pos, pos + 1 and byte 167) are constants per rate
// word, and the places where member bytes enter are a source offset and a byte shift per rate word.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/curdle_msm.h"

namespace curdle {
namespace transcript {

constexpr int kRateWords = 21;  // 166 rate bytes + RunF's mark at byte 167: the words a block touches

// One rate word of one block: st[w] ^= cmask ^ (member_bytes & dmask), where member_bytes is the
// unaligned 8-byte read at u64 index `idx`, bit shift `sh` of the member's row (see TapeRowWords).
struct TapeWord {
  uint64_t cmask, dmask;
  uint32_t idx, sh;
};
struct TapeBlock {
  TapeWord w[kRateWords];
  uint32_t run_f, pad[3];  // 1: Keccak-f after the words
};
// The control list.  kBlocks: blocks [a, a + b) of the pool, one behind the other.  kChallenge: squeeze 32 bytes;
// while they are not canonical run blocks [a, a + b) (the retry: label framing and PRF header from (32, 0)) and
// squeeze again; then st ^= block c's constants (the re-append's framing) and the challenge's 32 bytes enter at
// state byte d; it is output number e of the member.
enum : uint32_t { kBlocks = 1, kChallenge = 2 };
struct TapeCtl {
  uint32_t kind, a, b, c, d, e, pad[2];
};
struct Tape {
  std::vector<TapeCtl> ctl;
  std::vector<TapeBlock> pool;
  size_t consumed = 0;      // member bytes the program reads
  size_t n_challenges = 0;  // per member
  uint8_t pos = 0, pos_begin = 0, cur_flags = 0;  // after the program
  size_t permutations = 0;  // Keccak-f runs of a member whose every challenge is accepted at its first try
};
// A member's row on the device: 8 zero bytes, the consumed bytes, zero padding to a multiple of 8, 8 zero bytes.
inline size_t TapeRowWords(size_t consumed) { return 2 + (consumed + 7) / 8; }

constexpr int kMaxTries = 256;  // draws of one challenge before the member is handed back with a status

// Checks a call's shape (CURDLE_EINVAL with *why set, before anything is copied or launched) and, for the entry
// points that continue exported states, that those agree in (pos, pos_begin, cur_flags): one tape serves all members.
int CheckBatchCall(const char* transcript_label, const uint8_t* init_states, const curdle_transcript_step* steps,
                   size_t n_steps, const uint8_t* data, size_t data_stride, size_t k, const uint8_t* challenges,
                   const uint8_t* status, uint8_t start[3], std::string* why);
// The program from (pos, pos_begin, cur_flags) = start.
void CompileTape(const curdle_transcript_step* steps, size_t n_steps, const uint8_t start[3], Tape* out);

}  // namespace transcript
}  // namespace curdle
