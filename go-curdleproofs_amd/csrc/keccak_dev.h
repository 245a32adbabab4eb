// Keccak-f[1600] on the device, one state per lane: shared by the batched Merlin transcripts (transcript_kernels.hip)
// and the coefficients of the combined tracker check (tracker_combine_kernels.hip).  Device code only; every unit
// that includes this gets its own copy of the round constants.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace curdle {
namespace {
__constant__ uint64_t kKeccakRC[24] = {
    0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull,
    0x000000000000808bull, 0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull,
    0x000000000000008aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000aull,
    0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull, 0x8000000000008003ull,
    0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800aull, 0x800000008000000aull,
    0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};

__device__ __forceinline__ uint64_t rotl64(uint64_t x, int n) { return (x << n) | (x >> (64 - n)); }

// Keccak-f[1600], lane (x, y) at a[x + 5 y]: host/keccak.h's round over named lanes (theta, rho + pi, chi, iota with
// every index a compile-time constant), the 24 rounds a loop.
__device__ __forceinline__ void keccak_f1600_dev(uint64_t a[25]) {
#pragma unroll 1
  for (int round = 0; round < 24; round++) {
    const uint64_t c0 = a[0] ^ a[5] ^ a[10] ^ a[15] ^ a[20];
    const uint64_t c1 = a[1] ^ a[6] ^ a[11] ^ a[16] ^ a[21];
    const uint64_t c2 = a[2] ^ a[7] ^ a[12] ^ a[17] ^ a[22];
    const uint64_t c3 = a[3] ^ a[8] ^ a[13] ^ a[18] ^ a[23];
    const uint64_t c4 = a[4] ^ a[9] ^ a[14] ^ a[19] ^ a[24];
    const uint64_t d0 = c4 ^ rotl64(c1, 1);
    const uint64_t d1 = c0 ^ rotl64(c2, 1);
    const uint64_t d2 = c1 ^ rotl64(c3, 1);
    const uint64_t d3 = c2 ^ rotl64(c4, 1);
    const uint64_t d4 = c3 ^ rotl64(c0, 1);
    // rho + pi: b[y][2x+3y] = rotl(a[x][y] ^ d[x], r[x][y]); bXY is lane (X, Y) of b
    const uint64_t b00 = a[0] ^ d0;
    const uint64_t b13 = rotl64(a[5] ^ d0, 36);
    const uint64_t b21 = rotl64(a[10] ^ d0, 3);
    const uint64_t b34 = rotl64(a[15] ^ d0, 41);
    const uint64_t b42 = rotl64(a[20] ^ d0, 18);
    const uint64_t b02 = rotl64(a[1] ^ d1, 1);
    const uint64_t b10 = rotl64(a[6] ^ d1, 44);
    const uint64_t b23 = rotl64(a[11] ^ d1, 10);
    const uint64_t b31 = rotl64(a[16] ^ d1, 45);
    const uint64_t b44 = rotl64(a[21] ^ d1, 2);
    const uint64_t b04 = rotl64(a[2] ^ d2, 62);
    const uint64_t b12 = rotl64(a[7] ^ d2, 6);
    const uint64_t b20 = rotl64(a[12] ^ d2, 43);
    const uint64_t b33 = rotl64(a[17] ^ d2, 15);
    const uint64_t b41 = rotl64(a[22] ^ d2, 61);
    const uint64_t b01 = rotl64(a[3] ^ d3, 28);
    const uint64_t b14 = rotl64(a[8] ^ d3, 55);
    const uint64_t b22 = rotl64(a[13] ^ d3, 25);
    const uint64_t b30 = rotl64(a[18] ^ d3, 21);
    const uint64_t b43 = rotl64(a[23] ^ d3, 56);
    const uint64_t b03 = rotl64(a[4] ^ d4, 27);
    const uint64_t b11 = rotl64(a[9] ^ d4, 20);
    const uint64_t b24 = rotl64(a[14] ^ d4, 39);
    const uint64_t b32 = rotl64(a[19] ^ d4, 8);
    const uint64_t b40 = rotl64(a[24] ^ d4, 14);
    // chi, and iota on lane (0, 0)
    a[0] = b00 ^ (~b10 & b20) ^ kKeccakRC[round];
    a[1] = b10 ^ (~b20 & b30);
    a[2] = b20 ^ (~b30 & b40);
    a[3] = b30 ^ (~b40 & b00);
    a[4] = b40 ^ (~b00 & b10);
    a[5] = b01 ^ (~b11 & b21);
    a[6] = b11 ^ (~b21 & b31);
    a[7] = b21 ^ (~b31 & b41);
    a[8] = b31 ^ (~b41 & b01);
    a[9] = b41 ^ (~b01 & b11);
    a[10] = b02 ^ (~b12 & b22);
    a[11] = b12 ^ (~b22 & b32);
    a[12] = b22 ^ (~b32 & b42);
    a[13] = b32 ^ (~b42 & b02);
    a[14] = b42 ^ (~b02 & b12);
    a[15] = b03 ^ (~b13 & b23);
    a[16] = b13 ^ (~b23 & b33);
    a[17] = b23 ^ (~b33 & b43);
    a[18] = b33 ^ (~b43 & b03);
    a[19] = b43 ^ (~b03 & b13);
    a[20] = b04 ^ (~b14 & b24);
    a[21] = b14 ^ (~b24 & b34);
    a[22] = b24 ^ (~b34 & b44);
    a[23] = b34 ^ (~b44 & b04);
    a[24] = b44 ^ (~b04 & b14);
  }
}
}  // namespace
}  // namespace curdle
