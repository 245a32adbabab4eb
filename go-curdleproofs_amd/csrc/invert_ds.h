// Constant-time inversion in Fp by division steps (Bernstein, Yang: "Fast constant-time gcd computation and modular
// inversion", 2019), on one lane: the alternative to the Fermat chain of invert28.h, whose 381 squarings and 120
// products each wait for the one before.  Plain C++, host and device, no inline assembly: tests/hostbuild/invert_ds_flow.cpp
// compiles this header under the sanitizers, and tests/fp_divsteps_model.py is its big-integer model, batch for batch.
//
// The algorithm.  The paper's ORIGINAL division step (not the half-delta variant), from (delta, f, g) = (1, p, x) with x
// canonical:
//     delta > 0 and g odd:   (delta, f, g) <- (1 - delta, g, (g - f) / 2)
//     otherwise:             (delta, f, g) <- (1 + delta, f, (g + (g mod 2) f) / 2)
// and the choice taken by masks.  For 0 <= g < f < 2^d, d >= 46, floor((49 d + 57) / 17) steps bring g to 0 (the paper's
// Theorem 11.2): 1,101 for d = 381.  Here: 37 batches of 30 steps, 1,110, every trip count a compile-time constant.  A batch
// walks the low 30 bits of f and g alone (divsteps30) and yields a matrix (u, v; q, r) with
//     (u, v; q, r) (f, g)^T = 2^30 (f', g')^T,   |u| + |v| <= 2^30,  |q| + |r| <= 2^30,
// which is then applied to the full-width f, g (update_fg: an exact shift by 30) and to d, e (update_de), the pair with
// f = d x and g = e x mod p throughout, starting at (0, 1).  At the end g = 0, f = +-1 (f = p for x = 0, where d stays 0)
// and the inverse is sign(f) d.  "g != 0" after the last batch is returned as a violation word: no x below p sets it.
//
// Representation.  f, g, d, e: 13 SIGNED limbs of 30 bits (i32 each; limbs 0..11 in [0, 2^30), limb 12 carries the sign):
// 390 bits for values whose magnitudes stay below 2^381 (f, g: never above their starting ones) and 2^382 (d, e: kept in
// (-2p, p) after every batch).  No instruction branches on a value and no address is made of one; every loop over limbs is
// fully unrolled (a limb array under a run-time index goes to scratch).
//
// Signed arithmetic.  Right shifts of negative i32 / i64 values are ARITHMETIC (floor division by the power of two): what
// gcc, clang and hipcc do, and what C++20 requires.  Every other operation on a value that may wrap is done on unsigned
// words.  The bounds that keep the i64 column sums and the i32 limbs from overflowing are stated at each function.
#pragma once
#include "bls12_381.h"

namespace curdle {
namespace ds {

typedef int32_t i32;
typedef int64_t i64;

static constexpr int L = 13;             // limbs of 30 bits
static constexpr u32 M30 = 0x3fffffffu;
static constexpr u32 M28 = 0x0fffffffu;
static constexpr u32 kPinv30 = 0x30003u;  // p^-1 mod 2^30
static constexpr int kBatches = 37;       // x 30 steps = 1,110 >= 1,101

#define CURDLE_DS_TABLE(name, len, ...)    \
  CURDLE_HD u32 name(int i) {              \
    constexpr u32 t[len] = {__VA_ARGS__};  \
    return t[i];                           \
  }
// p on 13 limbs of 30 bits, and on fp28.h's 14 limbs of 28
CURDLE_DS_TABLE(kP30, 13, 0x3fffaaabu, 0x27fbffffu, 0x153ffffbu, 0x2affffacu, 0x30f6241eu, 0x034a83dau, 0x112bf673u,
                0x12e13ce1u, 0x2cd76477u, 0x1ed90d2eu, 0x29a4b1bau, 0x3a8e5ff9u, 0x001a0111u)
CURDLE_DS_TABLE(kP28, 14, 0xfffaaabu, 0xfefffffu, 0x3ffffb9u, 0xfffeb15u, 0x6241eabu, 0xa0f6b0fu, 0xf6730d2u, 0xf38512bu,
                0x4774b84u, 0x4bacd76u, 0xba7b643u, 0xe69a4b1u, 0x1ea397fu, 0x001a011u)
// 2^(3 * 392) mod p: d28::mul by it takes the body's result on a 2^392, which is a^-1 2^-392, to a^-1 2^392
CURDLE_DS_TABLE(kToMont28, 14, 0x1f7b890u, 0x294cc4du, 0x9f3af22u, 0xb5ba56cu, 0xcb5c0ccu, 0xc0d975cu, 0xc89a8c5u,
                0x6c968b4u, 0x22672eau, 0x91de8c9u, 0x35652a6u, 0x84977c8u, 0x424bbb9u, 0x00141abu)
// 2^(2 * 384 + 392) mod p: the same for a gnark element a 2^384, whose body result a^-1 2^-384 becomes a^-1 2^384
CURDLE_DS_TABLE(kToMontGnark, 14, 0xcc48a88u, 0x146bd94u, 0xdf909b9u, 0x1e8b9d8u, 0xe84e9a3u, 0xfd2645du, 0x8675f98u,
                0x3007c3du, 0xfd7b08fu, 0x88f0b3eu, 0x8135a1bu, 0x9e768f9u, 0x96a1967u, 0x0015c51u)
#undef CURDLE_DS_TABLE

struct Mat {
  i32 u, v, q, r;
};

// all ones iff a < 0, without a signed shift
CURDLE_HD u32 neg_mask(i32 a) { return 0u - ((u32)a >> 31); }

// 30 division steps on the low words f0, g0 of f and g (f odd).  eta = -delta, |eta| <= 1,111 throughout.
// Everything is computed on u32 words that may wrap: after i steps only the low 30 - i bits of f and g are meaningful
// and only bit 0 is looked at; |u| + |v| <= 2^i and |q| + |r| <= 2^i (each step doubles one row or adds the rows), so
// the final entries lie in [-2^30, 2^30] and their u32 words are their two's-complement i32 values.
// Instead of halving g's row the step doubles f's: the matrix stays integral and maps (f, g) to 2^30 (f', g').
CURDLE_HD i32 divsteps30(i32 eta, u32 f0, u32 g0, Mat& t) {
  u32 u = 1, v = 0, q = 0, r = 1, f = f0, g = g0, e = (u32)eta;
#pragma unroll
  for (int i = 0; i < 30; i++) {
    const u32 c1 = 0u - (e >> 31);  // eta < 0: delta > 0
    const u32 c2 = 0u - (g & 1u);   // g odd
    // g <- g + (delta > 0 ? -f : f) under "g odd", and the same on the rows
    g += ((f ^ c1) - c1) & c2;
    q += ((u ^ c1) - c1) & c2;
    r += ((v ^ c1) - c1) & c2;
    const u32 c = c1 & c2;    // the swap: f <- the old g = f + (g - f)
    e = (e ^ c) - (c + 1u);   // swap: -eta - 1 (delta <- 1 - delta); otherwise eta - 1 (delta <- 1 + delta)
    f += g & c;
    u += q & c;
    v += r & c;
    g >>= 1;
    u <<= 1;
    v <<= 1;
  }
  t.u = (i32)u;
  t.v = (i32)v;
  t.q = (i32)q;
  t.r = (i32)r;
  return (i32)e;
}

// (f, g) <- (u f + v g, q f + r g) / 2^30, exactly.  Requires |u| + |v|, |q| + |r| <= 2^30, limbs 0..11 in [0, 2^30),
// |f|, |g| < 2^381 before and after (so |limb 12| < 2^21).  A column sum is at most 2^30 * 2^30 in magnitude plus a
// carry below 2^31: it fits an i64.  The low 30 bits of column 0 are zero by the matrix's construction.
CURDLE_HD void update_fg(i32* f, i32* g, const Mat& t) {
  const i64 u = t.u, v = t.v, q = t.q, r = t.r;
  i64 cf = u * f[0] + v * g[0], cg = q * f[0] + r * g[0];
  cf >>= 30;
  cg >>= 30;
  static_for<1, L>([&](auto ic) {
    constexpr int i = decltype(ic)::value;
    cf += u * f[i] + v * g[i];
    cg += q * f[i] + r * g[i];
    f[i - 1] = (i32)(cf & M30);
    g[i - 1] = (i32)(cg & M30);
    cf >>= 30;
    cg >>= 30;
  });
  f[L - 1] = (i32)cf;
  g[L - 1] = (i32)cg;
}

// (d, e) <- (u d + v e + md p, q d + r e + me p) / 2^30 with md, me the multiples that make the shift exact.
// Requires d, e in (-2p, p), limbs 0..11 in [0, 2^30); ensures the same.  Why the range holds: with sd = [d < 0] and
// se = [e < 0], d + sd p and e + se p lie in (-p, p), so u (d + sd p) + v (e + se p) lies in (-2^30 p, 2^30 p); the
// correction then takes k p away with 0 <= k < 2^30, chosen so that the low 30 bits vanish: the sum lies in
// (-2^31 p, 2^30 p) and its 2^30-th part in (-2p, p).  md = u sd + v se - k lies in (-2^31, 2^30], so a column sum is
// below 2^60 + 2^61 in magnitude plus a carry: it fits an i64; |limb 12| of the result is below 2^22.
CURDLE_HD void update_de(i32* d, i32* e, const Mat& t) {
  const i64 u = t.u, v = t.v, q = t.q, r = t.r;
  const u32 sd = neg_mask(d[L - 1]), se = neg_mask(e[L - 1]);
  i32 md = (i32)((u32)t.u & sd) + (i32)((u32)t.v & se);  // |md| <= |u| + |v| <= 2^30
  i32 me = (i32)((u32)t.q & sd) + (i32)((u32)t.r & se);
  i64 cd = u * d[0] + v * e[0], ce = q * d[0] + r * e[0];
  md -= (i32)((kPinv30 * (u32)cd + (u32)md) & M30);  // cd + p md = 0 mod 2^30
  me -= (i32)((kPinv30 * (u32)ce + (u32)me) & M30);
  cd += (i64)kP30(0) * md;
  ce += (i64)kP30(0) * me;
  cd >>= 30;
  ce >>= 30;
  static_for<1, L>([&](auto ic) {
    constexpr int i = decltype(ic)::value;
    cd += u * d[i] + v * e[i] + (i64)kP30(i) * md;
    ce += q * d[i] + r * e[i] + (i64)kP30(i) * me;
    d[i - 1] = (i32)(cd & M30);
    e[i - 1] = (i32)(ce & M30);
    cd >>= 30;
    ce >>= 30;
  });
  d[L - 1] = (i32)cd;
  e[L - 1] = (i32)ce;
}

// One carry pass over signed limbs below 2^31 in magnitude: limbs 0..11 into [0, 2^30), the sign into limb 12.  The sum is
// taken on unsigned words: in range it cannot wrap, and on the garbage an x at or above p leaves it must not be undefined.
CURDLE_HD void carry30(i32* r) {
  static_for<0, L - 1>([&](auto ic) {
    constexpr int i = decltype(ic)::value;
    r[i + 1] = (i32)((u32)r[i + 1] + (u32)(r[i] >> 30));  // arithmetic shift
    r[i] = (i32)((u32)r[i] & M30);
  });
}

// r <- sign r into [0, p), `negate` all ones or zero.  Requires r in (-2p, p), limbs 0..11 in [0, 2^30).  r + [r < 0] p
// lies in (-p, p); negating it limb by limb keeps every limb within (-2^30, 2^30 + 2^30): no i32 wraps; one more masked
// p after the carry pass gives [0, p).
CURDLE_HD void normalize30(i32* r, u32 negate) {
  const u32 add = neg_mask(r[L - 1]);
  static_for<0, L>([&](auto ic) {
    constexpr int i = decltype(ic)::value;
    const u32 w = (u32)r[i] + (kP30(i) & add);
    r[i] = (i32)((w ^ negate) - negate);
  });
  carry30(r);
  const u32 add2 = neg_mask(r[L - 1]);
  static_for<0, L>([&](auto ic) {
    constexpr int i = decltype(ic)::value;
    r[i] = (i32)((u32)r[i] + (kP30(i) & add2));
  });
  carry30(r);
}

// x <- x^-1 mod p in [0, p), 0 for 0: x on 13 limbs of 30 bits, limbs in [0, 2^30), 0 <= x < p.  Returns the violation
// word: 1 iff g != 0 after the 1,110 steps, which no x below p causes (an x at or above p may: the caller that admits
// one reads the word; nothing else goes wrong with it, every value stays in registers).
CURDLE_HD u32 invert_body(i32* x) {
  i32 f[L], g[L], d[L], e[L];
  static_for<0, L>([&](auto ic) {
    constexpr int i = decltype(ic)::value;
    f[i] = (i32)kP30(i);
    g[i] = x[i];
    d[i] = 0;
    e[i] = i == 0 ? 1 : 0;
  });
  i32 eta = -1;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int b = 0; b < kBatches; b++) {
    Mat t;
    eta = divsteps30(eta, (u32)f[0], (u32)g[0], t);
    update_de(d, e, t);
    update_fg(f, g, t);
  }
  u32 nz = 0;
  static_for<0, L>([&](auto ic) { nz |= (u32)g[decltype(ic)::value]; });
  normalize30(d, neg_mask(f[L - 1]));
  static_for<0, L>([&](auto ic) { x[decltype(ic)::value] = d[decltype(ic)::value]; });
  return (nz | (0u - nz)) >> 31;
}

// ---------------------------------------------------------------------------------------------------------------------
// Repacking: out[j] = bits [WT j, WT (j + 1)) of the integer whose limbs of WF bits are in[0 .. NF).  Every in[i] is
// below 2^WF (the last one may be wider when WF NF exceeds the value's width: its excess lands where the integer has
// it, as long as it stays below bit 32 of that limb); bits at or above WT NT are dropped.  Shifts are compile-time.
// ---------------------------------------------------------------------------------------------------------------------
template <int WF, int NF, int WT, int NT>
CURDLE_HD void repack(u32* out, const u32* in) {
  static_for<0, NT>([&](auto jc) {
    constexpr int j = decltype(jc)::value;
    constexpr int bit = WT * j, i0 = bit / WF, sh = bit % WF;
    u32 v = 0;
    if constexpr (i0 < NF) v = in[i0] >> sh;
    if constexpr (WF - sh < WT && i0 + 1 < NF) v |= in[i0 + 1] << (WF - sh);
    if constexpr (2 * WF - sh < WT && i0 + 2 < NF) v |= in[i0 + 2] << (2 * WF - sh);
    out[j] = WT < 32 ? v & (u32)((1ull << WT) - 1) : v;
  });
}

// The canonical representative of a normalised a < 2p on fp28.h's limbs, by the masked step of to_gnark_ct
// (g1_exit_ct.h): the choice between a and a - p is a select on the borrow.  Limbs 0..12 below 2^28, limb 13 below 2^31.
CURDLE_HD void canonical28_ct(u32* c, const u32* a) {
  u32 d[14], borrow = 0;
  static_for<0, 14>([&](auto ic) {
    constexpr int i = decltype(ic)::value;
    const u32 s = a[i] - kP28(i) - borrow;
    borrow = s >> 31;
    d[i] = i < 13 ? s & M28 : s;
  });
  const u32 lt = 0u - borrow;  // a < p: keep a
  static_for<0, 14>([&](auto ic) {
    constexpr int i = decltype(ic)::value;
    c[i] = (a[i] & lt) | (d[i] & ~lt);
  });
}

// The two entry forms over invert_body.  Mul is fp28.h's Montgomery product on raw limbs, mul(r, a, b): r = a b / 2^392
// mod p, below 2p and normalised for normalised a, b below 2p -- d28::mul on the device (below), a restatement in the
// stand-alone host program.

// y = the Montgomery form (radix 2^392) of the inverse of a: a normalised, below 2p; y normalised, below 2p (the output
// bounds of invert28.h's `invert`); 0 and p give 0.  Returns the violation word (never set: the canonical step comes first).
template <class Mul>
CURDLE_HD u32 invert_limbs28(u32* y, const u32* a, Mul&& mul) {
  u32 c[14], w[L], k[14];
  i32 x[L];
  canonical28_ct(c, a);
  repack<28, 14, 30, L>(w, c);
  static_for<0, L>([&](auto ic) { x[decltype(ic)::value] = (i32)w[decltype(ic)::value]; });
  const u32 viol = invert_body(x);
  static_for<0, L>([&](auto ic) { w[decltype(ic)::value] = (u32)x[decltype(ic)::value]; });
  repack<30, L, 28, 14>(c, w);
  static_for<0, 14>([&](auto ic) { k[decltype(ic)::value] = kToMont28(decltype(ic)::value); });
  mul(y, c, k);
  return viol;
}

// The gnark form: a and y are fp.Elements (12 x u32, Montgomery radix 2^384), a canonical; y canonical.  An a at or above
// p (which the caller's range check reports) may set the violation word and gives an unspecified y.
template <class Mul>
CURDLE_HD u32 invert_gnark_words(u32* y, const u32* a, Mul&& mul) {
  u32 c[14], t[14], w[L], k[14];
  i32 x[L];
  repack<32, 12, 30, L>(w, a);
  static_for<0, L>([&](auto ic) { x[decltype(ic)::value] = (i32)w[decltype(ic)::value]; });
  const u32 viol = invert_body(x);
  static_for<0, L>([&](auto ic) { w[decltype(ic)::value] = (u32)x[decltype(ic)::value]; });
  repack<30, L, 28, 14>(c, w);
  static_for<0, 14>([&](auto ic) { k[decltype(ic)::value] = kToMontGnark(decltype(ic)::value); });
  mul(t, c, k);
  canonical28_ct(c, t);
  repack<28, 14, 32, 12>(y, c);
  return viol;
}

}  // namespace ds
}  // namespace curdle

#if defined(__HIPCC__)
#include "fp28.h"

namespace curdle {
namespace {
struct DsMul28 {
  __device__ __forceinline__ void operator()(u32* r, const u32* a, const u32* b) const {
    d28::F28 x, y, z;
#pragma unroll
    for (int i = 0; i < d28::N; i++) {
      x.l[i] = a[i];
      y.l[i] = b[i];
    }
    d28::mul(z, x, y);
#pragma unroll
    for (int i = 0; i < d28::N; i++) r[i] = z.l[i];
  }
};
// Stands where `invert` (invert28.h) stands: the same input and output bounds.  Returns the violation word.
__device__ __forceinline__ u32 invert_ds(d28::F28& y, const d28::F28& a) { return ds::invert_limbs28(y.l, a.l, DsMul28{}); }
__device__ __forceinline__ u32 invert_ds_gnark(u32* y, const u32* a) { return ds::invert_gnark_words(y, a, DsMul28{}); }
}  // namespace
}  // namespace curdle
#endif
