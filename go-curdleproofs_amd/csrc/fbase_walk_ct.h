// The per-window step of the constant-time fixed-base walk, k_fbase_mul_ct (fbase_ct_kernels.hip): the digit, the
// select-or-one and the ONE mixed addition whose zz and zzz are multiplied by a selected PP or one.  Moved out of that
// unit's anonymous namespace, text unchanged, so that the raw-limb self-test (selftest_ct_kernels.hip) calls the same
// functions.  Device-only; every function is forced inline into its kernel.  The rules of what may depend on a scalar
// and the multiply-accumulate trap are those at the top of fbase_ct_kernels.hip and g1_walk_ct.h.
#pragma once
#include <hip/hip_runtime.h>

#include "msm_kernels_common.h"
#include "g1_walk_ct.h"  // select3

namespace curdle {

namespace {
// the low 4-bit digit of k, and k >> 4: every window is read from word 0, so no register is indexed by the window
__device__ __forceinline__ u32 next_digit4(Fr& k) {
  const u32 d = k.l[0] & 0xfu;
#pragma unroll
  for (int j = 0; j < 7; j++) k.l[j] = (k.l[j] >> 4) | (k.l[j + 1] << 28);
  k.l[7] >>= 4;
  return d;
}
// r = m ? a : one limb by limb, m all ones or zero
__device__ __forceinline__ void select_or_one(F28& r, u32 m, const F28& a) {
#pragma unroll
  for (int i = 0; i < d28::N; i++) r.l[i] = (a.l[i] & m) | (d28::kOne(i) & ~m);
}

// One window's step.  acc: x < 10p, y < 6p, zz, zzz < 2p, limbs normalised; (x2, y2) affine below 2p, normalised.
// nz = 0 - (d != 0), started = all ones once something was added.  d28::madd's main path (EFD madd-2008-s), then the
// selection described at the top of the file; the bounds are madd's (X3 < 10p, Y3 < 2p, products < 2p).
// madd_bit (g1_walk_ct.h) is the same addition and stays a second function: there zz and zzz are SELECTED, here they are
// multiplied by a selected PP or one.  This kernel sits at 249 of the 256 VGPRs its launch bounds allow, and a shared
// core would keep pp live across the rest of the addition.
__device__ __forceinline__ void madd_select(X28& acc, const F28& x2, const F28& y2, u32 nz, u32 started) {
  using namespace d28;
  const u32 sum = nz & started, first = nz & ~started;
  F28 pp, r, t, q, ppp, p;
  mul_inl(p, x2, acc.zz);
  sub_raw<16>(p, p, acc.x);  // P = U2 - X1 < 18p
  mul_inl(r, y2, acc.zzz);
  sub_raw<16>(r, r, acc.y);  // R = S2 - Y1 < 18p
  sqr_inl(pp, p);            // PP < 2p
  mul_inl(ppp, p, pp);       // PPP
  mul_inl(q, acc.x, pp);     // Q
  select_or_one(p, sum, pp);
  mul_inl(acc.zz, acc.zz, p);    // ZZ * PP, or ZZ * 1: the same value (one until the first addition), below 2p again
  select_or_one(p, sum, ppp);
  mul_inl(acc.zzz, acc.zzz, p);
  sqr_inl(t, r);
  x3_fused(t, t, ppp, q);    // X3 = R^2 - PPP - 2Q < 10p
  sub_raw<16>(q, q, t);      // Q - X3 < 18p
  F28 ny, z;
  set_zero(z);
  sub_raw<16>(ny, z, acc.y); // 16p - Y1 (Y1 < 6p)
  mul2_inl(p, r, q, ny, ppp);  // Y3 = R (Q - X3) - Y1 PPP  (mod p), < 2p
  F28 yn = y2;
  norm(yn);
  select3(acc.x, sum, t, first, x2, acc.x);
  select3(acc.y, sum, p, first, yn, acc.y);
}

}  // namespace

}  // namespace curdle
