"""An executable, limb-exact model of the constant-time G1 layer: go-curdleproofs_amd/csrc/g1_walk_ct.h, g1_add_ct.h,
g1_exit_ct.h, invert28.h and madd_select of fbase_walk_ct.h, built on the field model of tests/fp28_model.py.

Every function is a transliteration of the header's and returns the exact words the kernel stores (selftest operation
16 hands them out as they are).  Every bound comment of the headers is an assertion here: the input contracts
(`ContractError`), and what the arithmetic relies on without checking (`OverflowError_`) -- P, R, Q - X3 < 18p, the
differences of add_ct < 6p, X3 < 10p, Y3 < 6p / < 2p, "the output is a legal input of add_ct and d28::dbl", that the
product of equal_mod_p is 0 or p exactly when the operands are congruent, and that bit 31 of every limb difference of
the masked canonical step is the borrow.  Sums that the kernels compute and discard (P + P, P + (-P), the double of
four ones) go through the same assertions: they must stay inside the limb bounds too.

Masks are numpy uint64 arrays holding 0 or 0xffffffff.  COUNTS says how often each arm and boundary was taken since it
was last cleared; WRONG holds the names of the deliberately wrong variants that are switched on (tests only: each must
change a word of the case set, tests/test_g1_ct_model.py).
"""
import numpy as np

import fp28_model as m
from fp28_model import ContractError, OverflowError_, STATS, P, N, MASK, M32, const, mul, mul2, sqr, sub, sub_raw, x3_fused, dbl

ONES = np.uint64(0xFFFFFFFF)
COUNTS = {}
WRONG = set()
# the largest product of the masked canonical step seen per constant, as a fraction t / p (a float: a report, not a check)
T_OVER_P = {}

INV_EXP = [0xFFFFAAA9, 0xB9FEFFFF, 0xB153FFFF, 0x1EABFFFE, 0xF6B0F624, 0x6730D2A0,
           0xF38512BF, 0x64774B84, 0x434BACD7, 0x4B1BA7B6, 0x397FE69A, 0x1A0111EA]   # p - 2 (invert28.h kInvExp)
assert sum(w << (32 * i) for i, w in enumerate(INV_EXP)) == P - 2


def _count(key, by=1):
    COUNTS[key] = COUNTS.get(key, 0) + int(by)


def _mask(cond):
    return np.where(np.asarray(cond), ONES, np.uint64(0))


def _is_mask(w):
    w = np.asarray(w, dtype=np.uint64)
    return (w == 0) | (w == ONES)


def _below(v, K, what, cls=ContractError):
    m._require(m.normalised(v) & m.lt(v, K * P), f"{what} not normalised below {K}p", cls)


# ------------------------------------------------------------------------------------------ g1_add_ct.h ---
def zero_mask(a):
    """all ones iff every limb of a is zero"""
    return _mask((np.asarray(a) == 0).all(axis=1))


def finite_mask(w):
    """all ones iff the 24 words are not all zero"""
    return _mask((np.asarray(w) != 0).any(axis=1))


def equal_mod_p(a, b):
    """all ones iff a == b mod p; a < 2p, b < 10p, both normalised."""
    _below(a, 2, "equal_mod_p: a")
    _below(b, 10, "equal_mod_p: b")
    n = a.shape[0]
    d = sub_raw(16, a, b)
    m._require(m.lt(d, 18 * P), "equal_mod_p: a - b + 16p >= 18p", OverflowError_)
    # a - b + 16p > 6p: the difference is never the integer 0, so the product below is never the integer 0 either
    # (d one + m p = 0 needs d = 0) and congruent operands always give exactly p.  The `== 0` leg is unreachable.
    m._require(~m.lt(m.norm(d), 6 * P), "equal_mod_p: difference below 6p", OverflowError_)
    e = mul(d, m.one(n), "mul")
    is0, isp = (e == 0).all(axis=1), (e == m.PV[None, :]).all(axis=1)
    va, vb = m.value(a), m.value(b)
    congruent = np.array([(x - y) % P == 0 for x, y in zip(va, vb)], dtype=bool)
    m._require((is0 | isp) == congruent, "equal_mod_p: e is 0 or p but the operands are not congruent, or the reverse", OverflowError_)
    m._require(~is0, "equal_mod_p: e == 0 reached", OverflowError_)
    _count("equal:e==p", isp.sum())
    _count("equal:e==0", is0.sum())
    _count("equal:neither", (~(is0 | isp)).sum())
    keep = [j for j in range(N) if f"equal_drops_limb_{j}" not in WRONG]
    o0 = np.zeros(n, dtype=np.uint64)
    op = np.zeros(n, dtype=np.uint64)
    for j in keep:
        o0 |= e[:, j]
        op |= e[:, j] ^ m.PV[j]
    neither = (o0 != 0) & (op != 0)
    return _mask(~neither)


def _select(pairs, n):
    """OR of (mask & value) limb by limb: what select4 / select3 compute."""
    r = np.zeros((n, N), dtype=np.uint64)
    for mk, v in pairs:
        r |= v & np.asarray(mk, dtype=np.uint64)[:, None]
    return r


def check_add_operand(pt, what, cls=ContractError):
    x, y, zz, zzz = pt
    for v, nm, K in ((x, "x", 10), (y, "y", 10), (zz, "zz", 2), (zzz, "zzz", 2)):
        _below(v, K, f"{what}: {nm}", cls)


def add_ct(a, b):
    """acc += b, complete, by selection.  Returns (point, arm) with arm in 1..5 per element."""
    check_add_operand(a, "add_ct acc")
    check_add_operand(b, "add_ct b")
    n = a[0].shape[0]
    a_inf, b_inf = zero_mask(a[2]), zero_mask(b[2])
    twice = dbl(a)
    u1 = mul(a[0], b[2], "mul")
    u2 = mul(b[0], a[2], "mul")
    s1 = mul(a[1], b[3], "mul")
    s2 = mul(b[1], a[3], "mul")
    eq_x, eq_y = equal_mod_p(u2, u1), equal_mod_p(s2, s1)
    p = sub_raw(4, u2, u1)
    m._require(m.lt(p, 6 * P), "add_ct: P >= 6p", OverflowError_)
    r = sub_raw(4, s2, s1)
    m._require(m.lt(r, 6 * P), "add_ct: R >= 6p", OverflowError_)
    pp = sqr(p, "sqr")
    ppp = mul(p, pp, "mul")
    q = mul(u1, pp, "mul")
    t = mul(a[2], b[2], "mul")
    zz3 = mul(t, pp, "mul")
    t = mul(a[3], b[3], "mul")
    zzz3 = mul(t, ppp, "mul")
    t = sqr(r, "sqr")
    x3 = x3_fused(t, ppp, q)
    q = sub_raw(16, q, x3)
    m._require(m.lt(q, 18 * P), "add_ct: Q - X3 >= 18p", OverflowError_)
    q = mul(r, q, "mul")
    s1 = mul(s1, ppp, "mul")
    y3 = sub(4, q, s1)
    m._require(m.lt(y3, 6 * P), "add_ct: Y3 >= 6p", OverflowError_)
    both = (a_inf ^ ONES) & (b_inf ^ ONES)
    take_b = a_inf
    take_a = (a_inf ^ ONES) & b_inf
    take_dbl = both & eq_x & eq_y
    take_sum = both & (eq_x ^ ONES)
    if "add_doubles_on_eq_x_alone" in WRONG:
        take_dbl = both & eq_x
    first = a if "add_takes_acc_when_a_inf" in WRONG else b
    out = tuple(_select(((take_b, first[c]), (take_a, a[c]), (take_dbl, twice[c]), (take_sum, (x3, y3, zz3, zzz3)[c])), n)
                for c in range(4))
    arm = np.where(take_b != 0, 1, np.where(take_a != 0, 2, np.where(take_dbl != 0, 3, np.where(take_sum != 0, 5, 4))))
    if not WRONG:
        for k in range(1, 6):
            _count(f"add_ct:arm{k}", (arm == k).sum())
        m._require(((take_b != 0).astype(int) + (take_a != 0) + (take_dbl != 0) + (take_sum != 0)) <= 1, "add_ct: masks overlap",
                   OverflowError_)
        check_add_operand(out, "add_ct result", OverflowError_)        # a legal input of add_ct and of d28::dbl again
        z4 = arm == 4
        m._require(~z4 | np.all([(c == 0).all(axis=1) for c in out], axis=0), "add_ct: arm 4 is not 56 zero words", OverflowError_)
    return out, arm


# ----------------------------------------------------------------------------------------- g1_walk_ct.h ---
def next_bit_msb(k):
    """(bit 255 of k, k << 1) for k an (n, 8) array of u32 words."""
    b = k[:, 7] >> np.uint64(31)
    out = np.zeros_like(k)
    for j in range(7, 0, -1):
        out[:, j] = ((k[:, j] << np.uint64(1)) | (k[:, j - 1] >> np.uint64(31))) & M32
    out[:, 0] = (k[:, 0] << np.uint64(1)) & M32
    return b, out


def check_walk_acc(acc, what, cls=ContractError):
    x, y, zz, zzz = acc
    for v, nm, K in ((x, "x", 10), (y, "y", 6), (zz, "zz", 2), (zzz, "zzz", 2)):
        _below(v, K, f"{what}: {nm}", cls)


def _madd_core(acc, x2, y2, what):
    """The main path of madd-2008-s as madd_bit and madd_select both run it, up to PP, PPP, X3 and Y3."""
    check_walk_acc(acc, f"{what} acc")
    _below(x2, 2, f"{what}: x2")
    _below(y2, 2, f"{what}: y2")
    X, Y, ZZ, ZZZ = acc
    n = X.shape[0]
    p = sub_raw(16, mul(x2, ZZ), X)
    m._require(m.lt(p, 18 * P), f"{what}: P >= 18p", OverflowError_)
    r = sub_raw(16, mul(y2, ZZZ), Y)
    m._require(m.lt(r, 18 * P), f"{what}: R >= 18p", OverflowError_)
    pp = sqr(p)
    ppp = mul(p, pp)
    q = mul(X, pp)
    t = sqr(r)
    x3 = x3_fused(t, ppp, q)
    q = sub_raw(16, q, x3)
    m._require(m.lt(q, 18 * P), f"{what}: Q - X3 >= 18p", OverflowError_)
    ny = sub_raw(16, m.zeros(n), Y)
    y3 = mul2(r, q, ny, ppp)                                           # asserted below 2p by the field model
    return pp, ppp, x3, y3


def _masks(bit, started, what):
    bit, started = np.asarray(bit, dtype=np.uint64), np.asarray(started, dtype=np.uint64)
    m._require(_is_mask(bit) & _is_mask(started), f"{what}: a mask word that is neither 0 nor all ones")
    for b in (0, 1):
        for s in (0, 1):
            _count(f"{what}:bit={b},started={s}", (((bit != 0) == b) & ((started != 0) == s)).sum())
    return bit & started, bit & (started ^ ONES)


def madd_bit(acc, x2, y2, bit, started):
    """One step's addition of g1_walk_ct.h: sum = bit & started, first = bit & ~started, otherwise acc stays."""
    sm, first = _masks(bit, started, "madd_bit")
    n = x2.shape[0]
    pp, ppp, x3, y3 = _madd_core(acc, x2, y2, "madd_bit")
    keep = (sm | first) ^ ONES
    one = m.one(n)
    zz3 = mul(acc[2], pp)
    zzz3 = mul(acc[3], ppp)
    zz_first = acc[2] if "madd_bit_first_keeps_zz" in WRONG else one
    out = (_select(((sm, x3), (first, x2), (keep, acc[0])), n), _select(((sm, y3), (first, y2), (keep, acc[1])), n),
           _select(((sm, zz3), (first, zz_first), (keep, acc[2])), n), _select(((sm, zzz3), (first, one), (keep, acc[3])), n))
    check_walk_acc(out, "madd_bit result", OverflowError_)
    return out


def madd_select(acc, x2, y2, nz, started):
    """One window's step of the fixed-base walk: zz and zzz are MULTIPLIED by a selected PP / PPP or one (digit 0 and the
    first addition still multiply by one, which may change the representative), the first arm stores the normalised y."""
    sm, first = _masks(nz, started, "madd_select")
    n = x2.shape[0]
    pp, ppp, x3, y3 = _madd_core(acc, x2, y2, "madd_select")
    keep = (sm | first) ^ ONES
    one = m.one(n)
    zz3 = mul(acc[2], _select(((sm, pp), (sm ^ ONES, one)), n))
    zzz3 = mul(acc[3], _select(((sm, ppp), (sm ^ ONES, one)), n))
    yn = m.norm(y2)
    out = (_select(((sm, x3), (first, x2), (keep, acc[0])), n), _select(((sm, y3), (first, yn), (keep, acc[1])), n), zz3, zzz3)
    check_walk_acc(out, "madd_select result", OverflowError_)
    return out


def scalar_words(ks):
    return np.array([[(k >> (32 * j)) & 0xFFFFFFFF for j in range(8)] for k in ks], dtype=np.uint64).reshape(-1, 8)


def walk_ct(k, x2, y2, steps):
    """k: (n, 8) canonical scalar words; steps: one public count per element, 1..255.  The shift by 256 - steps with its
    `over` word as k_msm_ct_walk does it, then walk_ct.  Elements with fewer steps than the longest wait as four ones
    (their own first step comes later): per element the sequence of operations is exactly the kernel's.
    Returns (acc, started, over)."""
    steps = np.asarray(steps, dtype=np.int64)
    n = len(steps)
    m._require((steps >= 1) & (steps <= 255), "walk_ct: steps outside 1..255")
    k = k.copy()
    over = np.zeros(n, dtype=np.uint64)
    for s in range(int(steps.min()), 256):
        b, shifted = next_bit_msb(k)
        act = steps <= s
        over |= np.where(act, b, np.uint64(0))
        k = np.where(act[:, None], shifted, k)
    acc = tuple(m.one(n) for _ in range(4))
    started = np.zeros(n, dtype=np.uint64)
    top = int(steps.max())
    for it in range(top):
        act = steps >= top - it
        b, shifted = next_bit_msb(k)
        bit = _mask(b != 0)
        d = dbl(acc)
        new = madd_bit(d, x2, y2, bit, (started | bit) if "walk_updates_started_first" in WRONG else started)
        acc = tuple(np.where(act[:, None], nw, old) for nw, old in zip(new, acc))
        started = np.where(act, started | bit, started)
        k = np.where(act[:, None], shifted, k)
    return acc, started, over


# ----------------------------------------------------------------------------------------- g1_exit_ct.h ---
def pack(a):
    """14 limbs -> 12 saturated words, the kernel's shifts (limbs outside 28 bits land where the kernel puts them)."""
    n = a.shape[0]
    w = np.zeros((n, 12), dtype=np.uint64)
    for k in range(12):
        bit = 32 * k
        j, sh = bit // 28, bit % 28
        v = a[:, j] >> np.uint64(sh)
        if j + 1 < N:
            v = v | (a[:, j + 1] << np.uint64(28 - sh))
        if 28 - sh + 28 < 32 and j + 2 < N:
            v = v | (a[:, j + 2] << np.uint64(56 - sh))
        w[:, k] = v & M32
    return w


def to_gnark_ct(a, table="kToExt"):
    """d28::to_gnark with the masked canonical step: 12 words.  Contract: that of the product (limbs < 2^30,
    a Const < 2^392 p)."""
    n = a.shape[0]
    use = "kToExt" if (table == "kToExtX16" and "x16_exit_uses_kToExt" in WRONG) else table
    t = mul(a, const(use, n), "mul")
    ti = t.astype(np.int64)
    d = np.zeros_like(ti)
    borrow = np.zeros(n, dtype=np.int64)
    for i in range(N):
        diff = ti[:, i] - m.KP[i] - borrow
        s = diff & 0xFFFFFFFF                                         # the u32 the kernel holds
        m._require(((s >> 31) == 1) == (diff < 0), "to_gnark_ct: bit 31 of a limb difference is not the borrow", OverflowError_)
        borrow = s >> 31
        d[:, i] = s & MASK if (i < N - 1 or "canonical_masks_top_limb" in WRONG) else s
    lt_p = borrow == 1
    keep_t = lt_p
    if "canonical_never_subtracts" in WRONG:
        keep_t = np.ones(n, dtype=bool)
    if "canonical_subtracts_only_above_p" in WRONG:
        keep_t = lt_p | (t == m.PV[None, :]).all(axis=1)
    out = np.where(keep_t[:, None], ti, d).astype(np.uint64)
    if not WRONG:
        _count(f"exit:{table}:t<p", lt_p.sum())
        _count(f"exit:{table}:t>=p", (~lt_p).sum())
        if n:
            big = t[np.argmax((t * m._W).sum(axis=1))]
            T_OVER_P[table] = max(T_OVER_P.get(table, 0.0), m.value1(big) / P)
        m._require(m.normalised(out) & m.lt(out, P), "to_gnark_ct: result not canonical", OverflowError_)
    return pack(out)


def exit_t(a, table="kToExt"):
    """The product the canonical step of to_gnark_ct sees (for building cases): integers."""
    return m.value(mul(a, const(table, a.shape[0]), "mul"))


def invert(d):
    """d^(p-2) on the fixed 3-bit windows of invert28.h: the same windows, the same order of sqr / sqr_inl / mul."""
    _below(d, 2, "invert: d")
    t2 = sqr(d, "sqr")
    t3 = mul(t2, d, "mul")
    t4 = sqr(t2, "sqr")
    t5 = mul(t4, d, "mul")
    t6 = sqr(t3, "sqr")
    t7 = mul(t6, d, "mul")
    tab = {1: d, 2: t2, 3: t3, 4: t4, 5: t5, 6: t5 if "invert_uses_t5_for_window_6" in WRONG else t6, 7: t7}
    y = t6
    for w in range(125, -1, -1):
        y = sqr(sqr(sqr(y)))
        bit = 3 * w
        e = INV_EXP[bit >> 5] >> (bit & 31)
        if (bit & 31) > 29:
            e |= (INV_EXP[(bit >> 5) + 1] << (32 - (bit & 31))) & 0xFFFFFFFF
        if e & 7:
            y = mul(y, tab[e & 7], "mul")
    return y


def affine_exit_operands(acc):
    """(ix, iy): the two values affine_words_ct hands to the masked canonical step, x = X zzz / (zz zzz), y = Y zz / (zz zzz)."""
    check_add_operand(acc, "affine_words_ct acc")
    x, y, zz, zzz = acc
    d = mul(zz, zzz, "mul")
    inv = invert(d)
    ix = mul(inv, zzz, "mul")
    iy = mul(inv, zz, "mul")
    return mul(x, ix, "mul"), mul(y, iy, "mul")


def exit_subtracts(a, table="kToExt"):
    """Per element: does the canonical step of to_gnark_ct<table> take t - p (t >= p)?"""
    return ~m.lt(mul(a, const(table, a.shape[0]), "mul"), P)


def affine_words_ct(acc):
    """The canonical gnark record (x | y), 24 words, of acc with one inversion."""
    ix, iy = affine_exit_operands(acc)
    if not WRONG:
        gx, gy = exit_subtracts(ix), exit_subtracts(iy)
        _count("affine:x>=p", (gx & ~gy).sum())
        _count("affine:y>=p", (gy & ~gx).sum())
        _count("affine:both>=p", (gx & gy).sum())
    return np.concatenate([to_gnark_ct(ix), to_gnark_ct(iy)], axis=1)


def from_gnark(w):
    """d28::from_gnark on canonical gnark values (integers x 2^384 mod p): the product by kToInt, below 2p."""
    return mul(m.arr(list(w)), const("kToInt", len(w)), "mul")


def mul_ct_exit(k, pts):
    """k_g1_mul_ct (and the walk and finish of the constant-time MSM on one term) for a small scalar 0 < k < 4 on the affine
    points `pts` (plain integers): the steps above k's top bit only double four ones, which the first addition
    overwrites whole, so two steps are the 255.  Returns (x subtracts, y subtracts, acc): whether the canonical step of
    each coordinate takes t - p, and the accumulator entering the exit."""
    assert 0 < k < 4
    x2 = from_gnark([x * (1 << 384) % P for x, _ in pts])
    y2 = from_gnark([y * (1 << 384) % P for _, y in pts])
    acc, started, _ = walk_ct(scalar_words([k] * len(pts)), x2, y2, [2] * len(pts))
    assert (started != 0).all()
    ix, iy = affine_exit_operands(acc)
    return exit_subtracts(ix), exit_subtracts(iy), acc


# ------------------------------------------------------------------------------------- k_fbase_mul_ct ---
def from_gnark_iso(pts):
    """d28::from_gnark_iso_x / _y on affine points (plain integers): the A28 words k_convert_points stores for a base, which
    are the records of the resident fixed-base table.  No product: the gnark words shifted left by 4 and by 2 bits, then
    the conditional subtractions of 8p, 4p, 2p (x) and 2p (y)."""
    x = m.arr([(px * (1 << 384) % P) << 4 for px, _ in pts])
    for S in (3, 2, 1):
        x = m.cond_sub_pshl(S, x)
    y = m.cond_sub_pshl(1, m.arr([(py * (1 << 384) % P) << 2 for _, py in pts]))
    _below(x, 2, "from_gnark_iso: x", OverflowError_)
    _below(y, 2, "from_gnark_iso: y", OverflowError_)
    return x, y


def fbase_window_table(add, base):
    """The 64 x 15 records k_fbase_mul_ct reads: tab[v][d - 1] = d 2^(4 v) base for d = 1..15, as (x, y) arrays of shape
    (64, 15, 14).  `add` is the affine group addition (oracle/py)."""
    pts, b = [], base
    for _ in range(64):
        cur = b
        for _d in range(15):
            pts.append(cur)
            cur = add(cur, b)
        b = cur                                            # 16 b
    x, y = from_gnark_iso(pts)
    return x.reshape(64, 15, N), y.reshape(64, 15, N), pts


def fbase_walk_ct(k, tab):
    """k_fbase_mul_ct's walk: 64 unsigned 4-bit digits from window 0 upward, digit 0 keeps entry 1, one madd_select a
    window.  k: (n, 8) canonical scalar words.  Returns (acc, started)."""
    tx, ty, _ = tab
    n = k.shape[0]
    acc = tuple(m.one(n) for _ in range(4))
    started = np.zeros(n, dtype=np.uint64)
    for v in range(64):
        d = ((k[:, v // 8] >> np.uint64(4 * (v % 8))) & np.uint64(15)).astype(np.int64)
        idx = np.maximum(d, 1) - 1
        nz = _mask(d != 0)
        acc = madd_select(acc, tx[v][idx], ty[v][idx], nz, started)
        started = started | nz
    return acc, started


def fbase_exit_words(acc, started):
    """The 48 gnark words k_fbase_mul_ct stores: X and Y through their own constants, ZZ and ZZZ through kToExt, masked."""
    w = np.concatenate([to_gnark_ct(acc[0], "kToExtX16"), to_gnark_ct(acc[1], "kToExtY64"), to_gnark_ct(acc[2]), to_gnark_ct(acc[3])],
                       axis=1)
    return w & np.asarray(started, dtype=np.uint64)[:, None]


# ----------------------------------------------------------------------------------------------- helpers ---
def gnark_value(w):
    """The residues a block of 12-word gnark elements (Montgomery R = 2^384, canonical) stands for."""
    rinv = pow(1 << 384, -1, P)
    out = []
    for row in np.asarray(w):
        v = sum(int(x) << (32 * j) for j, x in enumerate(row))
        assert v < P, "gnark words not canonical"
        out.append(v * rinv % P)
    return out


class wrong:
    """with wrong("name"): the model runs the deliberately wrong variant `name`."""

    def __init__(self, *names):
        self.names = names

    def __enter__(self):
        WRONG.update(self.names)

    def __exit__(self, *a):
        WRONG.difference_update(self.names)


WRONG_VARIANTS = (["canonical_never_subtracts", "canonical_subtracts_only_above_p", "canonical_masks_top_limb",
                   "x16_exit_uses_kToExt"] + [f"equal_drops_limb_{j}" for j in range(N)] +
                  ["add_doubles_on_eq_x_alone", "add_takes_acc_when_a_inf", "madd_bit_first_keeps_zz",
                   "walk_updates_started_first", "invert_uses_t5_for_window_6"])
