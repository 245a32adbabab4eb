"""An executable model of the device field and XYZZ point layer (go-curdleproofs_amd/csrc/fp28.h, quad28.h).

Elements are numpy arrays of shape (n, 14), dtype uint64, holding the u32 limbs the kernels hold (14 limbs of
28 bits, Montgomery radix R' = 2^392, lazily reduced).  Every function returns the exact words the kernel
stores, and ASSERTS the bounds the kernel relies on instead of assuming them:

- the contract each function states in its comment (`ContractError`), and
- what the hardware would silently get wrong (`OverflowError_`): a 64-bit column accumulator of a Montgomery
  product that reaches 2^64 (mac28_gfx950.inc drops every carry-out), the doubled cross sum of a square that
  reaches 2^63, a top limb stored as (u32)acc from an accumulator >= 2^32, and a linear limb operation that
  wraps a u32.

A column only ever gains non-negative products before its shift, so the accumulator's largest value in a
column is its value at the column's end whatever the order of the multiply-adds inside it; the model checks
that value, column by column in the kernel's order, and records the largest one it saw (`STATS`).
The point formulas are transliterated from the headers; every bound comment there is an assertion here.
"""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "go-curdleproofs_amd", "csrc", "fp28.h")

P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
N = 14
MASK = (1 << 28) - 1
RP = 1 << 392
RP_INV = pow(RP, -1, P)
N0 = (-pow(P, -1, 1 << 28)) % (1 << 28)
M32 = np.uint64(0xFFFFFFFF)


class ContractError(AssertionError):
    """An input outside what the function's comment allows."""


class OverflowError_(AssertionError):
    """A value the hardware would silently truncate."""


# the largest accumulator value seen per kind of product, for the margin reports of the CPU tests
STATS = {}


def _note(key, value):
    STATS[key] = max(STATS.get(key, 0), value)


def _require(ok, msg, cls=ContractError):
    ok = np.asarray(ok)
    if not ok.all():
        bad = int(np.flatnonzero(~ok.reshape(-1))[0])
        raise cls(f"{msg} (element {bad})")


# ----------------------------------------------------------------------------------------- limbs and ints ---
def limbs_of(v: int):
    """Normalised limbs of v (limbs 0..12 < 2^28, limb 13 the rest; v < 2^396)."""
    assert 0 <= v < 1 << (28 * 13 + 32)
    return [(v >> (28 * i)) & MASK for i in range(13)] + [v >> (28 * 13)]


def arr(vals):
    """list of ints -> normalised (n, 14) array."""
    return np.array([limbs_of(v) for v in vals], dtype=np.uint64).reshape(-1, N)


def rows(limb_lists):
    return np.array(limb_lists, dtype=np.uint64).reshape(-1, N)


def value(a) -> list:
    """The integers an (n, 14) array of (possibly unnormalised) limbs stands for."""
    return [sum(int(x) << (28 * i) for i, x in enumerate(r)) for r in np.asarray(a)]


def value1(limbs) -> int:
    return sum(int(x) << (28 * i) for i, x in enumerate(limbs))


def lt(a, bound: int):
    """Exactly value(a) < bound, vectorised, for limbs < 2^32 and 0 <= bound < 2^396."""
    b = limbs_of(bound)
    c = np.zeros(a.shape[0], dtype=np.int64)
    for i in range(N - 1):
        t = a[:, i].astype(np.int64) - b[i] + c
        c = t >> 28
    return a[:, N - 1].astype(np.int64) - b[N - 1] + c < 0


def normalised(a):
    return (a[:, : N - 1] <= MASK).all(axis=1) & (a[:, N - 1] <= M32)


def limbs_below(a, bits: float):
    return (a.astype(np.float64) < 2.0 ** bits).all(axis=1) if bits != int(bits) else (a < np.uint64(1 << int(bits))).all(axis=1)


def from_mont(v: int) -> int:
    return v * RP_INV % P


def to_mont(v: int) -> int:
    return v * RP % P


# ---------------------------------------------------------------------------------------------- constants ---
def header_tables(path=HEADER):
    """Every CURDLE_D28_TABLE(name, ...) of fp28.h: name -> list of 14 limbs."""
    text = open(path).read()
    out = {}
    for name, body in re.findall(r"CURDLE_D28_TABLE\((\w+),([^)]*)\)", text):
        if name == "name":
            continue
        out[name] = [int(x, 16) for x in re.findall(r"0x([0-9a-fA-F]+)u", body)]
    return out


_T = header_tables()
KP = _T["kP"]
KONE = _T["kOne"]
KK = {4: _T["kK4"], 8: _T["kK8"], 16: _T["kK16"]}
KK8B = _T["kK8B"]
PV = np.array(KP, dtype=np.uint64)


def const(name, n):
    return np.tile(np.array(_T[name], dtype=np.uint64), (n, 1))


def zeros(n):
    return np.zeros((n, N), dtype=np.uint64)


def one(n):
    return const("kOne", n)


# --------------------------------------------------------------------------------------------- products ---
def _columns(pairs):
    """Column sums of sum_pairs a*b: (hi, lo) arrays of shape (n, 27)."""
    n = pairs[0][0].shape[0]
    hi = np.zeros((n, 2 * N - 1), dtype=np.uint64)
    lo = np.zeros((n, 2 * N - 1), dtype=np.uint64)
    for a, b in pairs:
        for i in range(N):
            prod = a[:, i : i + 1] * b          # (n, 14): a_i * b_j, < 2^64
            lo[:, i : i + N] += prod & M32
            hi[:, i : i + N] += prod >> np.uint64(32)
    return hi, lo


def mont(pairs, kind="mul", cols=None, cross_cols=None):
    """sum over `pairs` of a*b (or the column sums `cols`, plus twice `cross_cols`), times 2^-392, the kernel's way: the words
    of (sum + m p) / 2^392 with m = -sum p^-1 mod 2^392, each column's accumulator checked below 2^64."""
    hi, lo = _columns(pairs) if cols is None else cols
    n = hi.shape[0]
    if cross_cols is not None:               # sqr_inl: a column's cross products, summed, then doubled
        chi, clo = cross_cols
        chi += clo >> np.uint64(32)
        clo &= M32
        _note(kind + ":cross", int(chi.max()) << 32)
        _require(chi < np.uint64(1 << 31), f"{kind}: doubled cross sum of a column >= 2^64", OverflowError_)
        hi += chi << np.uint64(1)
        lo += clo << np.uint64(1)
    m = np.zeros((n, N), dtype=np.uint64)
    out = np.zeros((n, N), dtype=np.uint64)
    c_hi = np.zeros(n, dtype=np.uint64)
    c_lo = np.zeros(n, dtype=np.uint64)
    peak = 0
    for k in range(2 * N - 1):
        h = hi[:, k] + c_hi
        l = lo[:, k] + c_lo
        if k < N:
            h += l >> np.uint64(32)
            l &= M32
            mk = ((l * np.uint64(N0)) & np.uint64(MASK))
            m[:, k] = mk
            prod = mk[:, None] * PV[None, :]    # m_k * p_j lands in column k + j
            lo[:, k : k + N] += prod & M32
            hi[:, k : k + N] += prod >> np.uint64(32)
            h = hi[:, k] + c_hi
            l = lo[:, k] + c_lo
        h += l >> np.uint64(32)
        l &= M32
        peak = max(peak, int(h.max()))
        _require(h < np.uint64(1 << 32), f"{kind}: column {k} accumulator >= 2^64", OverflowError_)
        if k < N:
            _require((l & np.uint64(MASK)) == 0, f"{kind}: column {k} not cleared")
        else:
            out[:, k - N] = l & np.uint64(MASK)
        # acc >>= 28
        c_lo = (h << np.uint64(4)) | (l >> np.uint64(28))
        c_hi = np.zeros(n, dtype=np.uint64)
    _note(kind, peak << 32)
    _require(c_lo < np.uint64(1 << 32), f"{kind}: top limb stored from an accumulator >= 2^32", OverflowError_)
    out[:, N - 1] = c_lo
    return out


_W = 2.0 ** (28 * np.arange(N))


def _prod_below(pairs, vmax: int):
    """sum of a*b < vmax for every element: a float estimate, exact big ints where it is close."""
    est = sum((a * _W).sum(axis=1) * (b * _W).sum(axis=1) for a, b in pairs)
    ok = est < float(vmax) * (1 - 2.0 ** -40)
    close = np.flatnonzero(~ok & (est < float(vmax) * (1 + 2.0 ** -40)))
    for i in close:
        ok[i] = sum(value1(a[i]) * value1(b[i]) for a, b in pairs) < vmax
    return ok


def _mul_contract(kind, a, b, vmax):
    _require(limbs_below(a, 30) & limbs_below(b, 30), f"{kind}: limbs >= 2^30")
    _require(_prod_below([(a, b)], vmax), f"{kind}: a*b >= 2^392 p")


def _ensure_lt2p(kind, r):
    _require(normalised(r) & lt(r, 2 * P), f"{kind}: result not normalised below 2p", OverflowError_)
    return r


def mul(a, b, kind="mul_inl"):
    """mul_inl / mul_call: limbs < 2^30, a*b < 2^392 p  =>  r < 2p, normalised."""
    _mul_contract(kind, a, b, RP * P)
    return _ensure_lt2p(kind, mont([(a, b)], kind=kind))


def sqr(a, kind="sqr_inl", contract=True):
    """sqr_inl / sqr_call: a column's cross products a_i a_j (i < j) summed, then doubled by a shift, plus
    the diagonal a_i^2."""
    if contract:
        _mul_contract(kind, a, a, RP * P)
    n = a.shape[0]
    hi = np.zeros((n, 2 * N - 1), dtype=np.uint64)
    lo = np.zeros((n, 2 * N - 1), dtype=np.uint64)
    chi, clo = np.zeros_like(hi), np.zeros_like(lo)
    for i in range(N):
        prod = a[:, i] * a[:, i]
        lo[:, 2 * i] += prod & M32
        hi[:, 2 * i] += prod >> np.uint64(32)
        if i + 1 < N:
            prod = a[:, i : i + 1] * a[:, i + 1 :]      # a_i a_j, j > i: column i + j
            clo[:, 2 * i + 1 : i + N] += prod & M32
            chi[:, 2 * i + 1 : i + N] += prod >> np.uint64(32)
    return _ensure_lt2p(kind, mont(None, kind=kind, cols=(hi, lo), cross_cols=(chi, clo)))


def mul2(a, b, c, d, kind="mul2_inl"):
    """mul2_inl: (a b + c d) / 2^392.  Limbs < 2^30 with (a, b) not both above 2^29.6, c limbs < 2^29.2,
    d normalised, a b + c d < 2^392 p."""
    _require(limbs_below(a, 30) & limbs_below(b, 30), f"{kind}: a, b limbs >= 2^30")
    _require(limbs_below(a, 29.6) | limbs_below(b, 29.6), f"{kind}: a and b both with limbs above 2^29.6")
    _require(limbs_below(c, 29.2), f"{kind}: c limbs >= 2^29.2")
    _require(normalised(d), f"{kind}: d not normalised")
    _require(_prod_below([(a, b), (c, d)], RP * P), f"{kind}: ab + cd >= 2^392 p")
    return _ensure_lt2p(kind, mont([(a, b), (c, d)], kind=kind))


# ------------------------------------------------------------------------------------- linear operations ---
def _u32(x, what):
    _require((x >= 0) & (x < (1 << 32)), f"{what}: a u32 limb wraps", OverflowError_)
    return x.astype(np.uint64)


def norm(a):
    a = a.astype(np.int64)
    out = np.zeros_like(a)
    c = np.zeros(a.shape[0], dtype=np.int64)
    for i in range(N - 1):
        t = _u32(a[:, i] + c, "norm").astype(np.int64)
        out[:, i] = t & MASK
        c = t >> 28
    out[:, N - 1] = _u32(a[:, N - 1] + c, "norm")
    return out.astype(np.uint64)


def add(a, b):
    return norm(_u32(a.astype(np.int64) + b.astype(np.int64), "add"))


def _kk(K, n):
    return np.tile(np.array(KK[K], dtype=np.int64), (n, 1))


def sub_raw(K, a, b):
    """a - b + K p without the carry pass.  Requires b normalised and b < (K-1)p."""
    _require(normalised(b) & lt(b, (K - 1) * P), f"sub_raw<{K}>: b not normalised below {K - 1}p")
    r = a.astype(np.int64) + _kk(K, a.shape[0]) - b.astype(np.int64)
    return _u32(r, f"sub_raw<{K}>")


def sub(K, a, b):
    return norm(sub_raw(K, a, b))


def dbl_raw(a):
    return _u32(a.astype(np.int64) * 2, "dbl_raw")


def triple_raw(a):
    return _u32(a.astype(np.int64) * 3, "triple_raw")


def x3_fused(rr, c, q):
    """rr - (c + 2q) + 8p: rr, c, q normalised and < 2p each => r < 10p."""
    for v, nm in ((rr, "rr"), (c, "c"), (q, "q")):
        _require(normalised(v) & lt(v, 2 * P), f"x3_fused: {nm} not normalised below 2p")
    kb = np.tile(np.array(KK8B, dtype=np.int64), (rr.shape[0], 1))
    r = norm(_u32(rr.astype(np.int64) + kb - c.astype(np.int64) - 2 * q.astype(np.int64), "x3_fused"))
    _require(lt(r, 10 * P), "x3_fused: X3 >= 10p", OverflowError_)
    return r


def canonical_lt2p(a):
    """The kernel's borrow chain: subtract p if no borrow comes out of the top."""
    ai = a.astype(np.int64)
    d = np.zeros_like(ai)
    borrow = np.zeros(a.shape[0], dtype=np.int64)
    for i in range(N):
        t = ai[:, i] - KP[i] - borrow
        borrow = (t < 0).astype(np.int64)
        d[:, i] = t & (MASK if i < N - 1 else 0xFFFFFFFF)
    return np.where((borrow == 0)[:, None], d, ai).astype(np.uint64)


def kpshl(S):
    v = P << S
    return limbs_of(v)


def cond_sub_pshl(S, a):
    ai = a.astype(np.int64)
    k = kpshl(S)
    d = np.zeros_like(ai)
    borrow = np.zeros(a.shape[0], dtype=np.int64)
    for i in range(N):
        t = ai[:, i] - k[i] - borrow
        borrow = (t < 0).astype(np.int64)
        d[:, i] = t & (MASK if i < N - 1 else 0xFFFFFFFF)
    return np.where((borrow == 0)[:, None], d, ai).astype(np.uint64)


def is_zero_lt2p(a):
    return (a == 0).all(axis=1) | (a == PV[None, :]).all(axis=1)


def all_zero(a):
    return (a == 0).all(axis=1)


def to_gnark(a, table="kToExt"):
    """internal (< 32p) -> 12 gnark words (canonical), as 14 words with the top two zero."""
    _require(lt(a, 32 * P), "to_gnark: input >= 32p")
    t = canonical_lt2p(mul(a, const(table, a.shape[0])))
    vals = value(t)
    _require(np.array([v < P for v in vals]), "to_gnark: not canonical", OverflowError_)
    return np.array([[(v >> (32 * k)) & 0xFFFFFFFF for k in range(12)] + [0, 0] for v in vals],
                    dtype=np.uint64).reshape(-1, N)


def to_gnark_msm(a, role):
    return to_gnark(a, ("kToExtX16", "kToExtY64", "kToExt", "kToExt")[role])


# ------------------------------------------------------------------------------------------------ points ---
# A point is a tuple (X, Y, ZZ, ZZZ) of (n, 14) arrays.  Stored-point invariant: X < 10p, Y < 6p,
# ZZ, ZZZ < 2p, limbs normalised (quad28.h; fp28.h's struct comment allows Y < 10p).
Y_BOUND = 6


def check_stored(pt, what, y_bound=None):
    x, y, zz, zzz = pt
    yb = Y_BOUND if y_bound is None else y_bound
    for v, nm, k in ((x, "X", 10), (y, "Y", yb), (zz, "ZZ", 2), (zzz, "ZZZ", 2)):
        _require(normalised(v) & lt(v, k * P), f"{what}: stored {nm} not normalised below {k}p", OverflowError_)


def _take(pt, idx):
    return tuple(c[idx] for c in pt)


def _put(dst, idx, src):
    for d, s in zip(dst, src):
        d[idx] = s


def set_inf(n):
    return (one(n), one(n), zeros(n), zeros(n))


def dbl_affine(x1, y1):
    """mdbl-2008-s-1: x1 < 2p, y1 < 4p normalised, not infinity."""
    _require(normalised(x1) & lt(x1, 2 * P), "dbl_affine: x1 not normalised below 2p")
    _require(normalised(y1) & lt(y1, 4 * P), "dbl_affine: y1 not normalised below 4p")
    u = dbl_raw(y1)
    v = sqr(u, "sqr")
    w = mul(u, v, "mul")
    s = mul(x1, v, "mul")
    t = sqr(x1, "sqr")
    m = triple_raw(t)
    t = sqr(m, "sqr")
    x3 = x3_fused(t, zeros(x1.shape[0]), s)
    t = sub_raw(16, s, x3)
    _require(lt(t, 18 * P), "dbl_affine: S - X3 >= 18p", OverflowError_)
    t = mul(m, t, "mul")
    u = mul(w, y1, "mul")
    y3 = sub(4, t, u)
    _require(lt(y3, 6 * P), "dbl_affine: Y3 >= 6p", OverflowError_)
    return (x3, y3, v, w)


def dbl(pt):
    """dbl-2008-s-1 (fp28.h dbl)."""
    x, y, zz, zzz = pt
    u = dbl_raw(y)
    v = sqr(u, "sqr")
    w = mul(u, v, "mul")
    s = mul(x, v, "mul")
    t = sqr(x, "sqr")
    m = triple_raw(t)
    t = sqr(m, "sqr")
    x3 = x3_fused(t, zeros(x.shape[0]), s)
    t = sub_raw(16, s, x3)
    _require(lt(t, 18 * P), "dbl: S - X3 >= 18p", OverflowError_)
    t = mul(m, t, "mul")
    u = mul(w, y, "mul")
    y3 = sub(4, t, u)
    _require(lt(y3, 6 * P), "dbl: Y3 >= 6p", OverflowError_)
    return (x3, y3, mul(v, zz, "mul"), mul(w, zzz, "mul"))


def madd(pt, x2, y2, inline=True):
    """madd-2008-s with the exceptional cases: x2 < 2p normalised, y2 < 4p with limbs < 2^30."""
    pm = (lambda a, b: mul(a, b, "mul_inl")) if inline else (lambda a, b: mul(a, b, "mul"))
    ps = (lambda a: sqr(a, "sqr_inl")) if inline else (lambda a: sqr(a, "sqr"))
    _require(normalised(x2) & lt(x2, 2 * P), "madd: x2 not normalised below 2p")
    _require(limbs_below(y2, 30) & lt(y2, 4 * P), "madd: y2 not below 4p with limbs < 2^30")
    n = x2.shape[0]
    out = tuple(c.copy() for c in pt)
    inf = all_zero(pt[2])
    i_inf = np.flatnonzero(inf)
    if len(i_inf):
        _put(out, i_inf, (x2[i_inf], norm(y2[i_inf]), one(len(i_inf)), one(len(i_inf))))
    i = np.flatnonzero(~inf)
    if not len(i):
        return out
    X, Y, ZZ, ZZZ = _take(pt, i)
    X2, Y2 = x2[i], y2[i]
    p = sub_raw(16, pm(X2, ZZ), X)
    _require(lt(p, 18 * P), "madd: P >= 18p", OverflowError_)
    r = sub_raw(16, pm(Y2, ZZZ), Y)
    _require(lt(r, 18 * P), "madd: R >= 18p", OverflowError_)
    pp = ps(p)
    same = is_zero_lt2p(pp)
    j = np.flatnonzero(same)
    if len(j):
        t = sqr(r[j], "sqr")
        dbl_case = is_zero_lt2p(t)
        res = set_inf(len(j))
        jd = np.flatnonzero(dbl_case)
        if len(jd):
            _put(res, jd, dbl_affine(X2[j][jd], norm(Y2[j][jd])))
        _put(out, i[j], res)
    k = np.flatnonzero(~same)
    if len(k):
        p, r, pp, X, Y, ZZ, ZZZ = p[k], r[k], pp[k], X[k], Y[k], ZZ[k], ZZZ[k]
        ppp = pm(p, pp)
        q = pm(X, pp)
        zz3 = pm(ZZ, pp)
        zzz3 = pm(ZZZ, ppp)
        t = ps(r)
        x3 = x3_fused(t, ppp, q)
        q = sub_raw(16, q, x3)
        _require(lt(q, 18 * P), "madd: Q - X3 >= 18p", OverflowError_)
        ny = sub_raw(16, zeros(len(k)), Y)
        y3 = mul2(r, q, ny, ppp)
        _put(out, i[k], (x3, y3, zz3, zzz3))
    return out


def add_pts(a, b):
    """add-2008-s with the exceptional cases (fp28.h add)."""
    out = tuple(c.copy() for c in a)
    binf, ainf = all_zero(b[2]), all_zero(a[2])
    i = np.flatnonzero(ainf & ~binf)
    if len(i):
        _put(out, i, _take(b, i))
    i = np.flatnonzero(~ainf & ~binf)
    if not len(i):
        return out
    A, B = _take(a, i), _take(b, i)
    u1 = mul(A[0], B[2], "mul")
    u2 = mul(B[0], A[2], "mul")
    s1 = mul(A[1], B[3], "mul")
    s2 = mul(B[1], A[3], "mul")
    p = sub_raw(4, u2, u1)
    r = sub_raw(4, s2, s1)
    pp = sqr(p, "sqr")
    same = is_zero_lt2p(pp)
    j = np.flatnonzero(same)
    if len(j):
        t = sqr(r[j], "sqr")
        dcase = is_zero_lt2p(t)
        res = set_inf(len(j))
        jd = np.flatnonzero(dcase)
        if len(jd):
            _put(res, jd, dbl(_take(A, j[jd])))
        _put(out, i[j], res)
    k = np.flatnonzero(~same)
    if len(k):
        A, B = _take(A, k), _take(B, k)
        p, r, pp, u1, s1 = p[k], r[k], pp[k], u1[k], s1[k]
        ppp = mul(p, pp, "mul")
        q = mul(u1, pp, "mul")
        zz3 = mul(mul(A[2], B[2], "mul"), pp, "mul")
        zzz3 = mul(mul(A[3], B[3], "mul"), ppp, "mul")
        t = sqr(r, "sqr")
        x3 = x3_fused(t, ppp, q)
        q = sub_raw(16, q, x3)
        q = mul(r, q, "mul")
        s1 = mul(s1, ppp, "mul")
        y3 = sub(4, q, s1)
        _require(lt(y3, 6 * P), "add: Y3 >= 6p", OverflowError_)
        _put(out, i[k], (x3, y3, zz3, zzz3))
    return out


def quad_dbl(pt):
    """quad28.h dbl: the same products as fp28.h dbl (a Montgomery product's words depend only on the
    integer product), and NO infinity test: ZZ3 = V * 0 keeps infinity at infinity."""
    return dbl(pt)


def quad_add(a, b):
    """quad28.h add: the same products as fp28.h add outside the exceptional branches; the doubling
    branch runs q28::dbl."""
    return add_pts(a, b)


def mul_small(b, k: list):
    """fp28.h mul_small: left-to-right double-and-add from k's top bit (infinity for k = 0)."""
    n = b[0].shape[0]
    r = set_inf(n)
    ks = np.array(k, dtype=np.uint64)
    for bit in range(31, -1, -1):
        active = np.flatnonzero((ks >> np.uint64(bit)) != 0)   # the loop starts at each k's top bit
        if not len(active):
            continue
        sub_r = dbl(_take(r, active))
        _put(r, active, sub_r)
        ad = active[((ks[active] >> np.uint64(bit)) & np.uint64(1)) == 1]
        if len(ad):
            _put(r, ad, add_pts(_take(r, ad), _take(b, ad)))
    return r


def quad_mul_small(b, k: list, top: int):
    """quad28.h mul_small: double-and-add from bit `top` (doublings of infinity above k's top bit)."""
    n = b[0].shape[0]
    r = set_inf(n)
    ks = np.array(k, dtype=np.uint64)
    for bit in range(top, -1, -1):
        r = quad_dbl(r)
        ad = np.flatnonzero(((ks >> np.uint64(bit)) & np.uint64(1)) == 1)
        if len(ad):
            _put(r, ad, quad_add(_take(r, ad), _take(b, ad)))
    return r


def affine(pt):
    """(X, Y, ZZ, ZZZ) internal -> list of plain affine points (x, y) or None for infinity."""
    out = []
    for x, y, zz, zzz in zip(*(value(c) for c in pt)):
        zz, zzz = from_mont(zz), from_mont(zzz)
        if zz == 0:
            out.append(None)
            continue
        out.append((from_mont(x) * pow(zz, -1, P) % P, from_mont(y) * pow(zzz, -1, P) % P))
    return out


# ------------------------------------------------------------------------------------------- generators ---
def top_below(v: int, K: int) -> int:
    """The largest value below K p congruent to v."""
    return v % P + (K - 1) * P


def push_limbs(v: int, cap_bits: int = 30):
    """A representation of v whose limbs 0..12 are pushed towards 2^cap_bits by borrowing from the next
    limb."""
    L = limbs_of(v)
    F = list(L)
    cap = 1 << cap_bits
    for i in range(N - 1):
        most = (cap - 1 - F[i]) >> 28
        b = min(most, F[i + 1])
        F[i] += b << 28
        F[i + 1] -= b
    assert value1(F) == v and all(0 <= f < cap for f in F[: N - 1])
    return F


def push_limbs_cap(v: int, cap: int):
    """push_limbs towards a cap that need not be a power of two (each low limb the most below `cap`)."""
    L = limbs_of(v)
    for i in range(N - 1):
        b = min(max((cap - 1 - L[i]) >> 28, 0), L[i + 1])
        L[i] += b << 28
        L[i + 1] -= b
    assert value1(L) == v
    return L


def push_limbs_cap_rows(vals, cap: int):
    return rows([push_limbs_cap(v, cap) for v in vals])


def isqrt_below(bound: int) -> int:
    """The largest a with a * a < bound."""
    from math import isqrt
    return isqrt(bound - 1)


def low_limbs_at(top: int, limb: int = (1 << 30) - 1):
    """Limbs 0..12 all `limb`, limb 13 `top`."""
    return [limb] * (N - 1) + [top]


def neg_words(y):
    """The words of sub_raw<4>(0, y): a negated affine y as k_accumulate makes it."""
    return sub_raw(4, zeros(y.shape[0]), y)


def rand_reps(vals, cap, rng):
    """Representations of the ints `vals` with limbs 0..12 pushed by random amounts towards `cap` (an int,
    need not be a power of two), vectorised."""
    F = arr(vals).astype(np.int64)
    for i in range(N - 1):
        most = np.maximum((cap - 1 - F[:, i]) >> 28, 0)
        b = np.minimum((rng.random(len(F)) * (most + 1)).astype(np.int64), F[:, i + 1])
        F[:, i] += b << 28
        F[:, i + 1] -= b
    return F.astype(np.uint64)
