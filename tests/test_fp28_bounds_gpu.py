"""The device field and XYZZ point layer (csrc/fp28.h, csrc/quad28.h) on raw limbs, word for word against the
executable model of tests/fp28_model.py, at the bounds each function states: values up to 32p, limbs pushed
to 2^30, stored points with X in [9p, 10p), Y up to 10p, ZZ / ZZZ in [p, 2p), negated affine y in the form
k_accumulate makes it, and the exceptional branches on non-canonical coordinates.  Selftest operations 13..15
feed the words a test writes to the primitive as they are (include/curdle_msm.h)."""
import random

import numpy as np
import pytest

import fp28_model as m

pytestmark = pytest.mark.gpu
P = m.P
N_RANDOM = 1 << 16

SEL = {n: i for i, n in enumerate((
    "mul_inl", "sqr_inl", "mul", "sqr", "mul2_inl", "add", "sub4", "sub8", "sub16", "sub_raw4", "sub_raw8",
    "sub_raw16", "dbl_raw", "triple_raw", "x3_fused", "norm", "canonical_lt2p", "is_zero_lt2p", "cond_sub_pshl1",
    "cond_sub_pshl2", "cond_sub_pshl3", "to_gnark", "to_gnark_msm0", "to_gnark_msm1", "to_gnark_msm2",
    "to_gnark_msm3"))}
PT_SEL = {"madd": 0, "madd_inl": 1, "add": 2, "dbl": 3, "dbl_affine": 4, "mul_small": 5}
Q_SEL = {"add": 0, "dbl": 1, "dbl_outofline": 2, "mul_small": 3}


# -------------------------------------------------------------------------------------------- plumbing ---
def field_call(gpu, sel, a, b=None, c=None, d=None):
    n = a.shape[0]
    inp = np.zeros((n, 60), dtype=np.uint32)
    inp[:, 0] = sel
    for off, v in ((4, a), (18, b), (32, c), (46, d)):
        if v is not None:
            inp[:, off:off + 14] = v
    out = gpu.selftest_op(13, inp, True)
    return out[:, :14].astype(np.uint64), out[:, 14]


def point_call(gpu, op, sel, A, B=None, k=None, top=0):
    n = A[0].shape[0]
    inp = np.zeros((n, 116), dtype=np.uint32)
    inp[:, 0] = sel
    if k is not None:
        inp[:, 1] = k
    inp[:, 2] = top
    inp[:, 4:60] = np.concatenate(A, axis=1)
    if B is not None:
        inp[:, 60:116] = np.concatenate(B, axis=1)
    out = gpu.selftest_op(op, inp, True).astype(np.uint64)
    return tuple(out[:, 14 * j:14 * (j + 1)] for j in range(4))


def same_words(dev, model, what):
    dev, model = np.asarray(dev), np.asarray(model)
    bad = np.flatnonzero((dev != model).reshape(len(dev), -1).any(axis=1))
    assert not len(bad), f"{what}: {len(bad)} elements differ, first {bad[0]}: {dev[bad[0]]} != {model[bad[0]]}"


def same_point(dev, model, what):
    for j, nm in enumerate("X Y ZZ ZZZ".split()):
        same_words(dev[j], model[j], f"{what} {nm}")


# ----------------------------------------------------------------------------------- field operations ---
EDGE = [0, 1, P - 1, P, P + 1, 2 * P - 1]


def _below(vals, K):
    return [v for v in vals if 0 <= v < K * P]


def _field_cases(name, rng):
    """(a, b, c, d) for one selector: the boundary families, then N_RANDOM random representations over the
    selector's whole permitted range."""
    rnd = random.Random(SEL[name])
    n = N_RANDOM
    cap30 = 1 << 30

    def rand_vals(K):
        return [rnd.randrange(K * P) for _ in range(n)]

    def edge_vals(K):
        return _below(EDGE + [m.top_below(v, K) for v in (0, 1, P - 1)] + [K * P - 1], K)

    if name in ("mul_inl", "mul", "sqr_inl", "sqr") or name.startswith("to_gnark"):
        unary = name.startswith("sqr") or name.startswith("to_gnark")
        ev = edge_vals(32)
        A = [m.limbs_of(v) for v in ev] + [m.push_limbs(v) for v in ev]
        A.append(m.low_limbs_at(0))                                   # all low limbs at 2^30 - 1
        A.append(m.low_limbs_at(m.limbs_of(32 * P - 1)[13] - 4))      # the same just below 32p
        if name.startswith("sqr"):
            s = m.isqrt_below(m.RP * P)                               # the largest a with a^2 < 2^392 p
            A += [m.limbs_of(s), m.push_limbs(s)]
        a = m.rows(A)
        b = None
        if not unary:
            # every pair of the edge representations, and the largest a*b below 2^392 p
            ia, ib = np.meshgrid(np.arange(len(a)), np.arange(len(a)))
            a, b = a[ia.ravel()], a[ib.ravel()]
            ea, eb = [], []
            for y in (P + 1, 2 * P - 1, 7 * P + 3, 32 * P - 1):
                x = (m.RP * P - 1) // y
                ea += [m.limbs_of(x), m.push_limbs(x)]
                eb += [m.limbs_of(y), m.push_limbs(y)]
            a = np.concatenate([a, m.rows(ea)])
            b = np.concatenate([b, m.rows(eb)])
            b = np.concatenate([b, m.rand_reps(rand_vals(32), cap30, rng)])
        a = np.concatenate([a, m.rand_reps(rand_vals(32), cap30, rng)])
        return a, b, None, None
    if name == "mul2_inl":
        c296, c292 = int(2 ** 29.6), int(2 ** 29.2)
        A, B = [], []
        for K in (2, 18):                     # each leg of the contract at its limit
            for v in edge_vals(K):
                for ca, cb in ((30, c296), (c296, 30), (c296, c296)):
                    A.append(m.push_limbs(v, ca) if ca == 30 else m.rand_reps([v], ca, rng)[0].tolist())
                    w = m.top_below(v + 1, K)
                    B.append(m.push_limbs(w, cb) if cb == 30 else m.push_limbs_cap(w, cb))
        a = np.concatenate([m.rows(A), m.rand_reps(rand_vals(18), cap30, rng)])
        b = np.concatenate([m.rows(B), m.rand_reps(rand_vals(18), c296, rng)])
        sw = np.arange(len(a)) % 2 == 1       # the random pairs with the wide operand on either side
        sw[: len(A)] = False
        a[sw], b[sw] = b[sw].copy(), a[sw].copy()
        # c: a negated Y (16p - Y, Y normalised below 15p) or random limbs up to 2^29.2; d normalised < 2p
        yv = [m.top_below(rnd.randrange(P), 15) if i % 4 == 0 else rnd.randrange(15 * P) for i in range(len(a))]
        c = m.sub_raw(16, m.zeros(len(a)), m.arr(yv))
        half = np.arange(len(a)) % 2 == 0
        c[half] = m.push_limbs_cap_rows([rnd.randrange(18 * P) for _ in range(int(half.sum()))], c292)
        d = m.arr([m.top_below(rnd.randrange(P), 2) if i % 3 == 0 else rnd.randrange(2 * P) for i in range(len(a))])
        return a, b, c, d
    if name == "add":
        return m.arr(edge_vals(16) + rand_vals(16)), m.arr(edge_vals(16)[::-1] + rand_vals(16)), None, None
    if name.startswith("sub"):
        K = int(name[7:] if name.startswith("sub_raw") else name[3:])
        ev = edge_vals(2)
        bv = _below(EDGE + [(K - 1) * P - 1, (K - 1) * P - 2, m.top_below(1, K - 1)], K - 1)
        ia, ib = np.meshgrid(np.arange(len(ev)), np.arange(len(bv)))
        a = m.rows([m.push_limbs(ev[i]) if j % 2 else m.limbs_of(ev[i]) for j, i in enumerate(ia.ravel())])
        a = np.concatenate([a, m.rand_reps(rand_vals(2), cap30, rng)])
        b = np.concatenate([m.arr([bv[i] for i in ib.ravel()]), m.arr(rand_vals(K - 1))])
        return a, b, None, None
    if name in ("dbl_raw", "triple_raw"):
        K = 16 if name == "dbl_raw" else 10
        return m.arr(edge_vals(K) + rand_vals(K)), None, None, None
    if name == "x3_fused":
        ev = edge_vals(2)
        g = np.array(np.meshgrid(*(np.arange(len(ev)),) * 3)).reshape(3, -1)
        return tuple(np.concatenate([m.arr([ev[i] for i in g[j]]), m.arr(rand_vals(2))]) for j in range(3)) + (None,)
    if name == "norm":
        a = rng.integers(0, 1 << 31, size=(n, 14), dtype=np.uint64)
        a[:, 13] >>= np.uint64(8)
        a[0, :13], a[0, 13] = (1 << 31) - 1, 0
        return a, None, None, None
    if name in ("canonical_lt2p", "is_zero_lt2p"):
        return m.arr(EDGE + [2, P - 2, P + 2] + rand_vals(2)), None, None, None
    if name.startswith("cond_sub_pshl"):
        S = int(name[-1])
        ev = [(P << S) + d for d in (-2, -1, 0, 1, 2)] + [0, (P << (S + 1)) - 1]
        return m.arr(ev + rand_vals(1 << (S + 1))), None, None, None
    raise AssertionError(name)


def _field_model(name, a, b, c, d):
    flag = np.zeros(len(a), dtype=np.uint64)
    if name in ("mul_inl", "mul"):
        r = m.mul(a, b, name)
    elif name in ("sqr_inl", "sqr"):
        r = m.sqr(a, name)
    elif name == "mul2_inl":
        r = m.mul2(a, b, c, d)
    elif name == "add":
        r = m.add(a, b)
    elif name.startswith("sub_raw"):
        r = m.sub_raw(int(name[7:]), a, b)
    elif name.startswith("sub"):
        r = m.sub(int(name[3:]), a, b)
    elif name == "dbl_raw":
        r = m.dbl_raw(a)
    elif name == "triple_raw":
        r = m.triple_raw(a)
    elif name == "x3_fused":
        r = m.x3_fused(a, b, c)
    elif name == "norm":
        r = m.norm(a)
    elif name == "canonical_lt2p":
        r = m.canonical_lt2p(a)
    elif name == "is_zero_lt2p":
        r, flag = m.zeros(len(a)), m.is_zero_lt2p(a).astype(np.uint64)
    elif name.startswith("cond_sub_pshl"):
        r = m.cond_sub_pshl(int(name[-1]), a)
    elif name == "to_gnark":
        r = m.to_gnark(a)
    else:
        r = m.to_gnark_msm(a, int(name[-1]))
    return r, flag


@pytest.mark.parametrize("name", list(SEL))
def test_field_op_words_at_the_bounds(gpu, name):
    """Every field primitive on its boundary families and 2^16 random representations over its whole
    permitted range: the device words are the model's words (and the model asserts the bounds)."""
    rng = np.random.default_rng(SEL[name] + 100)
    a, b, c, d = _field_cases(name, rng)
    r, flag = _field_model(name, a, b, c, d)
    dr, dflag = field_call(gpu, SEL[name], a, b, c, d)
    same_words(dr, r, name)
    same_words(dflag[:, None], flag[:, None], name + " flag")
    if name in ("mul_inl", "mul", "sqr_inl", "sqr", "mul2_inl"):   # and the model against plain big ints
        for i in range(0, len(a), 97):
            ab = m.value1(a[i]) * m.value1(a[i] if b is None else b[i])
            cd = 0 if c is None else m.value1(c[i]) * m.value1(d[i])
            assert m.value1(dr[i]) % P == (ab + cd) * m.RP_INV % P
    if name == "is_zero_lt2p":
        assert list(dflag[:4]) == [1, 0, 0, 1]                         # a value of exactly p is zero
    if name.startswith("to_gnark"):
        assert (dr[:, 12:] == 0).all()


# ------------------------------------------------------------------------------------- point operations ---
@pytest.fixture(scope="module")
def multiples(oracle):
    """j G for j = 1..64, affine."""
    out, g = [], (oracle.GX, oracle.GY)
    acc = g
    for _ in range(64):
        out.append(acc)
        acc = oracle.add(acc, g)
    return out


def stored(points, rng, xk=10, yk=6, zk=2):
    """Internal XYZZ of the affine points (None: infinity) at the top of the stored-point bounds:
    X in [(xk-1)p, xk p), Y in [(yk-1)p, yk p), ZZ, ZZZ in [(zk-1)p, zk p)."""
    X, Y, ZZ, ZZZ = [], [], [], []
    one = m.value1(m.KONE)
    for pt in points:
        if pt is None:
            X.append(one), Y.append(one), ZZ.append(0), ZZZ.append(0)
            continue
        z = int(rng.integers(1, 1 << 62))
        x, y = pt
        X.append(m.to_mont(x * z ** 2) + (xk - 1) * P)
        Y.append(m.to_mont(y * z ** 3) + (yk - 1) * P)
        ZZ.append(m.to_mont(z ** 2) + (zk - 1) * P)
        ZZZ.append(m.to_mont(z ** 3) + (zk - 1) * P)
    return tuple(m.arr(v) for v in (X, Y, ZZ, ZZZ))


def affine_in(points, xk=2, neg=False, y_top=False):
    """(x2, y2) for madd: x2 in [(xk-1)p, xk p); y2 canonical or lifted to [3p, 4p), or the words
    k_accumulate's negation sub_raw<4>(0, y) gives (the point is then -pt)."""
    x = m.arr([m.to_mont(px) + (xk - 1) * P for px, _ in points])
    if neg:
        return x, m.neg_words(m.arr([m.to_mont(py) for _, py in points]))
    return x, m.arr([m.to_mont(py) + (3 * P if y_top else 0) for _, py in points])


def check_affine(pt, expect, what):
    for i, (g, e) in enumerate(zip(m.affine(pt), expect)):
        assert g == e, f"{what}: element {i}"


def test_point_ops_at_the_stored_point_extremes(gpu, oracle, multiples):
    """madd<false> / madd<true> / add / dbl / dbl_affine / mul_small on one lane and add / dbl / mul_small
    through the quads, at the extremes of the stored-point invariant, including the exceptional branches
    on non-canonical coordinates: device words = model words, the affine result = the oracle's, the output
    is a stored point again, madd<true> = madd<false> and quad = one lane, word for word."""
    rng = np.random.default_rng(7)
    G = multiples
    n = 512
    ia = rng.integers(0, 64, size=n)
    ib = rng.integers(0, 64, size=n)
    ib[:32] = ia[:32]                         # the same point: PP is exactly p, madd doubles
    A_aff = [G[i] for i in ia]
    B_aff = [G[i] for i in ib]
    A_aff[32:40] = [None] * 8                 # accumulator at infinity
    for xk, yk, yt in ((10, 6, False), (10, 10, True), (2, 2, False)):
        A = stored(A_aff, rng, xk=xk, yk=yk)
        for neg in (False, True):
            x2, y2 = affine_in(B_aff, xk=2, neg=neg, y_top=yt)
            b_pts = [oracle.neg(b) for b in B_aff] if neg else B_aff
            mdl = m.madd(A, x2, y2)
            m.check_stored(mdl, "madd")
            B = (x2, y2, m.one(n), m.one(n))
            for sel in ("madd", "madd_inl"):
                same_point(point_call(gpu, 14, PT_SEL[sel], A, B), mdl, f"{sel} X<{xk}p Y<{yk}p neg={neg}")
            check_affine(mdl, [oracle.add(a, b) for a, b in zip(A_aff, b_pts)], "madd")
        # general additions: B a stored point at the same extremes; opposite / equal / infinite cases inside
        b_pts = list(B_aff)
        b_pts[40:48] = [oracle.neg(a) for a in A_aff[40:48]]
        b_pts[48:52] = [None] * 4
        B = stored(b_pts, rng, xk=xk, yk=yk)
        mdl = m.add_pts(A, B)
        m.check_stored(mdl, "add", y_bound=max(yk, 6))          # infinity + B is B as it came
        same_point(point_call(gpu, 14, PT_SEL["add"], A, B), mdl, f"add X<{xk}p Y<{yk}p")
        same_point(point_call(gpu, 15, Q_SEL["add"], A, B), mdl, f"quad add X<{xk}p Y<{yk}p")
        check_affine(mdl, [oracle.add(a, b) for a, b in zip(A_aff, b_pts)], "add")
        mdl = m.dbl(A)
        m.check_stored(mdl, "dbl", y_bound=max(yk, 6))          # infinity doubles to itself
        for op, sel in ((14, PT_SEL["dbl"]), (15, Q_SEL["dbl"]), (15, Q_SEL["dbl_outofline"])):
            same_point(point_call(gpu, op, sel, A), mdl, f"dbl op {op}.{sel} X<{xk}p Y<{yk}p")
        check_affine(mdl, [oracle.add(a, a) for a in A_aff], "dbl")   # infinity doubles to infinity
    # dbl_affine: x1 in [p, 2p), y1 canonical and in [3p, 4p)
    for yt in (False, True):
        x1, y1 = affine_in(A_aff[40:], xk=2, y_top=yt)
        A = (x1, y1, m.one(len(x1)), m.one(len(x1)))
        mdl = m.dbl_affine(x1, y1)
        m.check_stored(mdl, "dbl_affine")
        same_point(point_call(gpu, 14, PT_SEL["dbl_affine"], A), mdl, "dbl_affine")
        check_affine(mdl, [oracle.add(a, a) for a in A_aff[40:]], "dbl_affine")
    # small multiples: one lane from k's top bit, quads from bit 11 (doublings of infinity first)
    B = stored(B_aff[:128], rng, xk=10, yk=10)
    k = rng.integers(0, 1 << 12, size=128).astype(np.uint32)
    k[:3] = (0, 1, (1 << 12) - 1)
    mdl = m.mul_small(B, [int(v) for v in k])
    same_point(point_call(gpu, 14, PT_SEL["mul_small"], B, B, k=k), mdl, "mul_small")
    expect = [oracle.scalar_mul(int(kk), b) for kk, b in zip(k, B_aff[:128])]
    check_affine(mdl, expect, "mul_small")
    qmdl = m.quad_mul_small(B, [int(v) for v in k], 11)
    same_point(point_call(gpu, 15, Q_SEL["mul_small"], B, B, k=k, top=11), qmdl, "quad mul_small")
    check_affine(qmdl, expect, "quad mul_small")
    nz = np.flatnonzero(k != 0)           # k = 0: the quads double infinity, which keeps ZZ = 0 only
    same_point(m._take(qmdl, nz), m._take(mdl, nz), "quad mul_small = one lane")


def test_chained_walks_stay_inside_the_bounds(gpu, oracle, multiples):
    """4096 walks of 256 steps, a random mix of madd<true> with a random sign, add and dbl, each step's device
    output the next step's input, seeded from extreme representations of points with known discrete logs:
    every step equals the model word for word and keeps the stored-point invariant, and the end points are
    the discrete logs the steps imply."""
    rng = np.random.default_rng(11)
    G = multiples
    n, steps = 4096, 256
    logs = rng.integers(1, 65, size=n).astype(object)
    A = stored([G[k - 1] for k in logs], rng, xk=10, yk=10)
    aff_x, aff_y = affine_in(G, xk=2)                       # addends j G: affine with x in [p, 2p) ...
    aff_yn = m.neg_words(m.arr([m.to_mont(y) for _, y in G]))
    st = stored(G, rng, xk=10, yk=6)                         # ... and stored at the extremes
    ones = m.one(n)
    for step in range(steps):
        kind = rng.integers(0, 3, size=n)                    # 0 madd, 1 add, 2 dbl
        j = rng.integers(0, 64, size=n)
        neg = rng.integers(0, 2, size=n) == 1
        sel = np.array([PT_SEL["madd_inl"], PT_SEL["add"], PT_SEL["dbl"]], dtype=np.uint32)[kind]
        x2, y2 = aff_x[j], np.where(neg[:, None], aff_yn[j], aff_y[j])
        is_m = (kind == 0)[:, None]
        B = tuple(np.where(is_m, u, v[j]) for u, v in zip((x2, y2, ones, ones), st))
        dev = point_call(gpu, 14, sel, A, B)
        mdl = tuple(c.copy() for c in A)
        s = np.flatnonzero(kind == 0)
        m._put(mdl, s, m.madd(m._take(A, s), x2[s], y2[s]))
        s = np.flatnonzero(kind == 1)
        m._put(mdl, s, m.add_pts(m._take(A, s), m._take(B, s)))
        s = np.flatnonzero(kind == 2)
        m._put(mdl, s, m.dbl(m._take(A, s)))
        same_point(dev, mdl, f"walk step {step}")
        m.check_stored(dev, f"walk step {step}")
        delta = np.where(neg & (kind == 0), -(j + 1), j + 1).astype(object)
        logs = np.where(kind == 2, logs * 2, logs + delta) % oracle.R
        A = dev
    got = m.affine(m._take(A, np.arange(256)))
    g = (oracle.GX, oracle.GY)
    for i in range(256):
        assert got[i] == oracle.scalar_mul(int(logs[i]), g), i
