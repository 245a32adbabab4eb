// Keccak-f[1600] on a state spread over lanes: the 25 words of a state live on 25 lanes, one u64 each, so a round is
// a handful of instructions per lane where keccak_dev.h's (a whole state per lane) is about 320.  What a call waits
// for in the batched Merlin transcripts is a chain of dependent permutations (transcript_api.hip), and this is the
// shorter chain.
//
// Layout: a wave holds TWO states, one per 32-lane half.  Word (x, y) of a half's state is on lane 5 y + x of the half
// (so word w is on lane w, the order of keccak_dev.h's a[25] and of an exported state); lanes 25..31 of a half idle:
// they run every instruction, fetch from themselves and nobody fetches from them.  The halves never exchange.
//
// Every exchange is a ds_bpermute_b32 pair (a u64) from a per-lane source address that SheetLane holds, set up once:
// no LDS is allocated, no register is indexed dynamically.  A round is three dependent exchange steps:
//   theta 1   the four other words of the lane's column        -> the column parity C[x], known to all five lanes
//   theta 2   C[x - 1] and C[x + 1] from the two neighbours in the lane's plane -> D[x]; then rho by the lane's offset
//   pi + chi  lane (X, Y) fetches the rotated words that pi sends to (X, Y), (X + 1, Y), (X + 2, Y) straight from
//             where they are, which saves the exchange step a separate pi would cost
// and iota on lane 0 from the round constant, which lane `round` holds and v_readlane hands to the wave.
//
// ds_bpermute reads 0 from a lane that is switched off: call sheet_keccak_f1600 with all 64 lanes active.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace curdle {
namespace {
__constant__ uint64_t kSheetRC[24] = {
    0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull,
    0x000000000000808bull, 0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull,
    0x000000000000008aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000aull,
    0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull, 0x8000000000008003ull,
    0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800aull, 0x800000008000000aull,
    0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
// rho's offset of word w = x + 5 y (keccak_dev.h's rotl64 amounts, read by word)
__constant__ uint8_t kSheetRho[32] = {0,  1,  62, 28, 27, 36, 44, 6,  55, 20, 3,  10, 43, 25, 39, 41,
                                      45, 15, 21, 8,  18, 2,  61, 56, 14, 0,  0,  0,  0,  0,  0,  0};

constexpr uint32_t kSheetStatesPerWave = 2;

// A lane's constants.  Source addresses are ds_bpermute's: 4 x the lane of the WAVE to read from.
struct SheetLane {
  uint32_t w;        // the word this lane holds (lane & 31); >= 25: idle
  uint32_t half;     // lane >> 5: which of the wave's two states
  uint32_t col[4];   // (x, y + 1..4): the rest of the column
  uint32_t dm, dp;   // (x - 1, y), (x + 1, y)
  uint32_t chi[3];   // where pi takes (X, Y), (X + 1, Y), (X + 2, Y) from
  uint32_t rho;      // rotation of this lane's word, 0..63
  uint32_t rc_lo, rc_hi;  // lane j < 24 of the wave: round constant j
  uint32_t iota;     // all ones on word 0, else 0
};

__device__ __forceinline__ SheetLane sheet_lane_setup() {
  SheetLane L;
  const uint32_t lane = threadIdx.x & 63;
  L.w = lane & 31;
  L.half = lane >> 5;
  const uint32_t base = lane & 32;
  const bool idle = L.w >= 25;
  const uint32_t x = L.w % 5, y = L.w / 5;
  const uint32_t self = 4 * lane;
#pragma unroll
  for (uint32_t i = 0; i < 4; i++) L.col[i] = idle ? self : 4 * (base + x + 5 * ((y + 1 + i) % 5));
  L.dm = idle ? self : 4 * (base + (x + 4) % 5 + 5 * y);
  L.dp = idle ? self : 4 * (base + (x + 1) % 5 + 5 * y);
#pragma unroll
  for (uint32_t i = 0; i < 3; i++) {
    // b[X'][Y] = rotl(a[sx][sy]) with X' = sy, Y = 2 sx + 3 sy (mod 5): sy = X', sx = 3 Y + X' (mod 5)
    const uint32_t xs = (x + i) % 5;
    L.chi[i] = idle ? self : 4 * (base + (3 * y + xs) % 5 + 5 * xs);
  }
  L.rho = kSheetRho[L.w];
  const uint64_t rc = kSheetRC[lane < 24 ? lane : 0];
  L.rc_lo = (uint32_t)rc;
  L.rc_hi = (uint32_t)(rc >> 32);
  L.iota = L.w == 0 ? 0xffffffffu : 0u;
  return L;
}

// v of the lane at bpermute address `addr`
__device__ __forceinline__ uint64_t sheet_fetch(uint64_t v, uint32_t addr) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute((int)addr, (int)(uint32_t)v);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute((int)addr, (int)(uint32_t)(v >> 32));
  return ((uint64_t)hi << 32) | lo;
}

// The lane's word of Keccak-f[1600] of the state its half holds.  All 64 lanes active.
__device__ __forceinline__ uint64_t sheet_keccak_f1600(uint64_t a, const SheetLane& L) {
#pragma unroll 1
  for (int round = 0; round < 24; round++) {
    // theta
    const uint64_t c = a ^ sheet_fetch(a, L.col[0]) ^ sheet_fetch(a, L.col[1]) ^ sheet_fetch(a, L.col[2]) ^ sheet_fetch(a, L.col[3]);
    const uint64_t cm = sheet_fetch(c, L.dm), cp = sheet_fetch(c, L.dp);
    a ^= cm ^ ((cp << 1) | (cp >> 63));
    // rho (an offset of 0 leaves the word: both shifts are by 0)
    a = (a << L.rho) | (a >> ((64 - L.rho) & 63));
    // pi and chi
    const uint64_t b0 = sheet_fetch(a, L.chi[0]), b1 = sheet_fetch(a, L.chi[1]), b2 = sheet_fetch(a, L.chi[2]);
    a = b0 ^ (~b1 & b2);
    // iota
    const uint32_t rc_lo = (uint32_t)__builtin_amdgcn_readlane((int)L.rc_lo, round);
    const uint32_t rc_hi = (uint32_t)__builtin_amdgcn_readlane((int)L.rc_hi, round);
    a ^= ((uint64_t)(rc_hi & L.iota) << 32) | (rc_lo & L.iota);
  }
  return a;
}
}  // namespace
}  // namespace curdle
