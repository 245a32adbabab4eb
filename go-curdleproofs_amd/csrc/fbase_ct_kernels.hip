// Constant-time twin of k_fbase_mul (fbase_kernels.hip): out_i = (s_i * m_i mod r) * P from the SAME resident table,
// same inputs, same output, with an instruction stream and an address stream that do not depend on the scalars.
//
// The walk.  64 unsigned 4-bit digits from window 0 upward.  The multiples a 4-bit window v needs, d 2^(4 v) P for
// d = 1..15, are entries of the 8-bit table (table[w * 255 + e - 1] = e 2^(8 w) P, e = 1..255):
//     d 2^(4 v) P = table[(v >> 1) * 255 + (d << (4 * (v & 1))) - 1]                      (16 * 15 = 240 <= 255)
// For every window the lane reads ALL 15 of them -- the addresses are made of the table pointer and the loop counter
// and of nothing else, so they are the same for every lane of every wave -- and keeps the one its digit names by mask
// arithmetic over the 28 limbs (entry & (0 - (d == e)), OR-ed together); digit 0 keeps entry 1, a real point.  960
// records of one 128-byte line each are read per scalar, 122,880 bytes of the 1,044,480-byte table, L2-resident and
// shared by every lane: no LDS copy, no second table.
//
// One mixed addition per window, always, and the new accumulator by selection:
//     d == 0                      keep acc                (the sum is discarded)
//     d != 0, nothing added yet   the chosen affine entry (zz = zzz = 1, y normalised as madd's is_inf arm does)
//     otherwise                   the sum
// "Nothing added yet" is a mask word (started |= d != 0), never a test of zz: the accumulator's zz and zzz are ONE
// until the first addition, and the selection of zz and zzz is a product -- zz * (sum ? PP : 1), zzz * (sum ? PPP : 1)
// -- so neither the old zz and zzz nor a second copy of them is kept, and infinity (k = 0) is `started == 0` at the end.
//
// The addition is the main path of d28::madd (fp28.h) without its three exceptional arms.  Exactness (the argument of
// fbase_kernels.hip, which holds for any window width): the scalar is canonical (k < r), the digits are unsigned and P
// is in the prime-order subgroup, so before window v the accumulator is m P with m = k mod 2^(4 v) < 2^(4 v) <=
// d 2^(4 v), never + the addend, and m + d 2^(4 v) <= k < r, never - the addend.  A sum that is discarded (digit 0, or
// nothing added yet, where the accumulator is not a point at all) may be nonsense: it is integer arithmetic inside the
// limb bounds of fp28.h (x, y < 10p, zz, zzz < 2p, an affine operand below 2p) and traps nothing.  Signed digits would
// halve the reads and break the argument.  tests/fbase_ct_model.py asserts it on every case the tests use.
//
// What may depend on a scalar: data operands of arithmetic and of selects.  What may not: a branch condition, an exec
// mask (beyond i >= n), a load, store or LDS address, a readfirstlane, a loop trip count.  Selects are written as
// mask arithmetic, m = 0 - (cond), (a & m) | (b & ~m); the store masks the twelve words of every coordinate with
// `started`, because is_inf is (s m = 0 mod r), a fact about the secrets -- that such a lane stores zeros is the
// result itself.  DESIGN.md section 0 (round 21) lists every branch and every memory instruction of the build.
//
// The multiply-accumulate trap: no product may see a limb the compiler knows.  The
// initial accumulator is constants, so the window loop stays rolled (#pragma unroll 1, as in k_fbase_mul): inside the
// loop the accumulator is a loop-carried value.  The constant `one` reaches products only through a select with a
// lane mask.
//
// Plain loads and stores, no LDS, no scratch, no inline assembly beyond the field layer's.
#include <hip/hip_runtime.h>

#include "msm_kernels_common.h"
#include "g1_walk_ct.h"  // load_fr_lane, select3, store_words_masked
#include "g1_exit_ct.h"  // to_gnark_ct
#include "fbase_walk_ct.h"  // next_digit4, madd_select

namespace curdle {

__global__ void __launch_bounds__(kBlock, 2)
    k_fbase_mul_ct(const A28* __restrict__ table, const uint4* __restrict__ scalars, const uint4* __restrict__ multipliers,
                   u32 n, G1XYZZ* __restrict__ out) {
  const u32 i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  Fr k;
  {
    Fr s;
    load_fr_lane(s, scalars + 2 * (size_t)i);
    if (multipliers) {  // a kernel argument: uniform over the launch
      Fr m;
      load_fr_lane(m, multipliers + 2 * (size_t)i);
      f_mul_inl<FrParams>(s, s, m);
    }
    f_from_mont<FrParams>(k, s);
  }
  X28 acc;  // not a point until `started`: zz = zzz = one, x and y anything below 2p
  d28::set_one(acc.x);
  d28::set_one(acc.y);
  d28::set_one(acc.zz);
  d28::set_one(acc.zzz);
  u32 started = 0;
#pragma unroll 1
  for (u32 v = 0; v < 64; v++) {
    const u32 d = next_digit4(k);
    const u32 first_entry = (v >> 1) * 255u - 1u, shift = 4u * (v & 1u);
    A28 pt;
    {  // entry 1 for the digits 0 and 1
      A28 e;
      d28::load(e, a28_at(table, first_entry + (1u << shift)));
      const u32 m = 0u - (u32)(d <= 1u);
#pragma unroll
      for (int j = 0; j < d28::N; j++) {
        pt.x.l[j] = e.x.l[j] & m;
        pt.y.l[j] = e.y.l[j] & m;
      }
    }
#pragma unroll
    for (u32 c = 2; c < 16; c++) {
      A28 e;
      d28::load(e, a28_at(table, first_entry + (c << shift)));
      const u32 m = 0u - (u32)(d == c);
#pragma unroll
      for (int j = 0; j < d28::N; j++) {
        pt.x.l[j] |= e.x.l[j] & m;
        pt.y.l[j] |= e.y.l[j] & m;
      }
    }
    const u32 nz = 0u - (u32)(d != 0u);
    madd_select(acc, pt.x, pt.y, nz, started);
    started |= nz;
  }
  // X and Y leave the curve of from_gnark_iso by their own constants (d28::to_gnark_msm's roles), under `started`
  uint4* dst = reinterpret_cast<uint4*>(out + i);
  u32 w[12];
  to_gnark_ct<d28::kToExtX16>(w, acc.x);
  store_words_masked<3>(dst, w, started);
  to_gnark_ct<d28::kToExtY64>(w, acc.y);
  store_words_masked<3>(dst + 3, w, started);
  to_gnark_ct<d28::kToExt>(w, acc.zz);
  store_words_masked<3>(dst + 6, w, started);
  to_gnark_ct<d28::kToExt>(w, acc.zzz);
  store_words_masked<3>(dst + 9, w, started);
}

hipError_t launch_fbase_mul_ct(const void* table28, const void* scalars, const void* multipliers, uint32_t n, void* out_xyzz,
                               hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_fbase_mul_ct, dim3(cdiv(n, kBlock)), dim3(kBlock), 0, stream, reinterpret_cast<const A28*>(table28),
                     (const uint4*)scalars, (const uint4*)multipliers, (u32)n, (G1XYZZ*)out_xyzz);
  return hipGetLastError();
}

}  // namespace curdle
