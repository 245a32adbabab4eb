"""The case sets of selftest operation 16 (the constant-time G1 layer on raw limbs), shared by the CPU tests of the
model (test_g1_ct_model.py) and the GPU tests (test_g1_ct_bounds_gpu.py).

A case set is one input block of operation 16, uint64[n, 116] holding u32 words (sel | arg0 | arg1 | pad | A | B), plus
what the CPU tests need to check the model against arithmetic it does not share (`info`).  model_out(inp) is the
expected output block, uint64[n, 60], from tests/g1_ct_model.py: the GPU tests compare it with the device word for word.

Sizes of the random blocks, with the model's time for the selector's whole case set on one CPU core: 2^14 elements for
the field-level selectors (zero_mask, finite_mask 0.1 s; equal_mod_p 0.9 s; to_gnark_ct 0.6 - 0.9 s per constant), 2^10
for invert (501 products a lane, 2.8 s) and for affine_words_ct (507 products, 3.7 s), 2^10 for madd_bit / madd_select
(2.0 - 2.4 s with the 254 doublings of four ones) and add_ct (0.8 s), and 256 lanes of walks with all step counts in ONE
run of 255 model steps: 8.0 s for the model (7.3 s at 86 lanes: a run costs 255 doublings and additions almost whatever the
lane count), above the few seconds aimed at and kept, because fewer lanes save next to nothing.  The field tests of
test_fp28_bounds_gpu.py use 2^16 per selector; the composite models are 500 times as many products a lane.
"""
import functools
import random

import numpy as np

import bls12381_ref as oracle
import fp28_model as m
import g1_ct_model as g

P, R = m.P, oracle.R
SEL = {n: i for i, n in enumerate(("zero_mask", "finite_mask", "equal_mod_p", "to_gnark_ct", "to_gnark_ct_x16", "to_gnark_ct_y64",
                                   "invert", "affine_words_ct", "madd_bit", "madd_select", "add_ct", "walk_ct"))}
EXIT_TABLE = {"to_gnark_ct": "kToExt", "to_gnark_ct_x16": "kToExtX16", "to_gnark_ct_y64": "kToExtY64"}
N_FIELD, N_POINT = 1 << 14, 1 << 10
ONES = 0xFFFFFFFF
EDGE = [0, 1, P - 1, P, P + 1, 2 * P - 1]          # the edge list of test_fp28_bounds_gpu.py
G1 = (oracle.GX, oracle.GY)


# ------------------------------------------------------------------------------------------------ blocks ---
def block(sel, n, A=None, B=None, arg0=0, arg1=0):
    inp = np.zeros((n, 116), dtype=np.uint64)
    inp[:, 0] = SEL[sel]
    inp[:, 1] = arg0
    inp[:, 2] = arg1
    for off, pt in ((4, A), (60, B)):
        if pt is None:
            continue
        for c, v in enumerate(pt):
            if v is not None:
                inp[:, off + 14 * c: off + 14 * c + v.shape[1]] = v
    assert (inp <= ONES).all()
    return inp


def _pt(inp, off):
    return tuple(inp[:, off + 14 * c: off + 14 * (c + 1)].copy() for c in range(4))


def model_out(inp):
    """The words operation 16 must return for `inp` (one selector per block)."""
    n = inp.shape[0]
    sel = int(inp[0, 0])
    assert (inp[:, 0] == sel).all()
    name = list(SEL)[sel]
    A, B = _pt(inp, 4), _pt(inp, 60)
    out = np.zeros((n, 60), dtype=np.uint64)
    if name == "zero_mask":
        out[:, 56] = g.zero_mask(A[0])
    elif name == "finite_mask":
        out[:, 56] = g.finite_mask(inp[:, 4:28])
    elif name == "equal_mod_p":
        out[:, 56] = g.equal_mod_p(A[0], A[1])
    elif name in EXIT_TABLE:
        out[:, :12] = g.to_gnark_ct(A[0], EXIT_TABLE[name])
    elif name == "invert":
        out[:, :14] = g.invert(A[0])
    elif name == "affine_words_ct":
        out[:, :24] = g.affine_words_ct(A)
    elif name in ("madd_bit", "madd_select"):
        fn = g.madd_bit if name == "madd_bit" else g.madd_select
        out[:, :56] = np.concatenate(fn(A, B[0], B[1], inp[:, 1], inp[:, 2]), axis=1)
    elif name == "add_ct":
        out[:, :56] = np.concatenate(g.add_ct(A, B)[0], axis=1)
    else:
        acc, started, over = g.walk_ct(inp[:, 60:68], A[0], A[1], inp[:, 1])
        out[:, :56] = np.concatenate(acc, axis=1)
        out[:, 56], out[:, 57] = started, over
    return out


# ------------------------------------------------------------------------------------------------ points ---
@functools.lru_cache(maxsize=None)
def multiples(count=64):
    """j G for j = 1..count, affine."""
    out, acc = [], G1
    for _ in range(count):
        out.append(acc)
        acc = oracle.add(acc, G1)
    return out


def stored(points, rnd, xk=10, yk=6, zk=2):
    """Internal XYZZ of the affine points (None: infinity, ZZ = ZZZ = 0) under a random scaling z each, at the top of
    the bounds: X in [(xk-1)p, xk p), Y in [(yk-1)p, yk p), ZZ, ZZZ in [(zk-1)p, zk p)."""
    X, Y, ZZ, ZZZ = [], [], [], []
    one = m.value1(m.KONE)
    for pt in points:
        if pt is None:
            X.append(one), Y.append(one), ZZ.append(0), ZZZ.append(0)
            continue
        z = rnd.randrange(2, 1 << 62)
        x, y = pt
        X.append(m.to_mont(x * z ** 2) + (xk - 1) * P)
        Y.append(m.to_mont(y * z ** 3) + (yk - 1) * P)
        ZZ.append(m.to_mont(z ** 2) + (zk - 1) * P)
        ZZZ.append(m.to_mont(z ** 3) + (zk - 1) * P)
    return tuple(m.arr(v) for v in (X, Y, ZZ, ZZZ))


def affine_in(points, lift=0):
    """(x2, y2) internal, in [lift p, (lift + 1) p)."""
    return (m.arr([m.to_mont(x) + lift * P for x, _ in points]), m.arr([m.to_mont(y) + lift * P for _, y in points]))


# ---------------------------------------------------------------------------------------------- families ---
def mask_families(name):
    """zero_mask on the 14 limbs of A.x, finite_mask on the first 24 words of A."""
    width = 14 if name == "zero_mask" else 24
    fams = {}

    def blk(words):
        inp = block(name, len(words))
        inp[:, 4:4 + words.shape[1]] = words
        return inp

    fams["all_zero"] = blk(np.zeros((1, width), dtype=np.uint64))
    hot = np.zeros((width * 32, width), dtype=np.uint64)
    for w in range(width):
        for b in range(32):
            hot[w * 32 + b, w] = 1 << b
    fams["one_hot"] = blk(hot)
    fams["all_ones"] = blk(np.full((1, width), ONES, dtype=np.uint64))
    # words the mask must NOT read: set bits behind the operand only
    behind = np.zeros((32, 56), dtype=np.uint64)
    for b in range(32):
        behind[b, width + (b % (56 - width))] = 1 << b
    fams["behind_the_operand"] = blk(behind)
    rng = np.random.default_rng(SEL[name])
    rnd = rng.integers(0, 1 << 32, size=(N_FIELD, width), dtype=np.uint64)
    rnd[::2] = 0
    rnd[::4, rng.integers(0, width)] = 5
    fams["random"] = blk(rnd)
    return fams


def _eq_block(pairs):
    a, b = m.arr([x for x, _ in pairs]), m.arr([y for _, y in pairs])
    return block("equal_mod_p", len(pairs), A=(a, b, None, None))


def equal_families():
    rnd = random.Random(2)
    fams = {}
    residues = [0, 1, P - 1] + [rnd.randrange(P) for _ in range(5)]
    fams["representatives"] = _eq_block([(v + i * P, v + j * P) for v in residues for i in (0, 1) for j in range(10)])
    off = []
    for v in residues:
        for i in (0, 1):
            for j in range(10):
                for d in (-1, 1):
                    if 0 <= v + j * P + d < 10 * P:
                        off.append((v + i * P, v + j * P + d))
    fams["off_by_one"] = _eq_block(off)
    # The reduced difference e = (a - b + 16p) one / 2^392 off 0, or off p, in exactly ONE limb j: what an OR that drops limb j
    # would call equal.  e is rho or rho + p for the canonical residue rho = a - b mod p, and it is rho only when
    # rho 2^392 >= (a - b + 16p) one, that is rho above about 2^370: "e = d 2^(28 j), one limb nonzero" exists for limb 13
    # alone, and for every limb below it the one-limb case is e = p + d 2^(28 j) (no carry: d is small).  Both kinds are
    # searched through the model's product, and every limb must get at least one.
    one_limb = []
    for j in range(m.N):
        found = 0
        for delta in (1, 3, 100, 1000):
            rho = delta << (28 * j)
            if rho >= P:
                continue
            cand = []
            for _ in range(64):
                w = rnd.randrange(P)
                cand.append(((w + rho) % P + rnd.randrange(2) * P, w + rnd.randrange(10) * P))
            a, b = m.arr([x for x, _ in cand]), m.arr([y for _, y in cand])
            e = m.mul(m.sub_raw(16, a, b), m.one(len(cand)), "mul")
            pv = m.PV[None, :]
            lone = np.flatnonzero(((e != 0).sum(axis=1) == 1) & (e[:, j] != 0))
            near = np.flatnonzero(((e != pv).sum(axis=1) == 1) & (e[:, j] != pv[0, j]))
            one_limb += [cand[i] for i in lone[:2]] + [cand[i] for i in near[:2]]
            found += len(lone) + len(near)
        assert found, j
    fams["one_limb"] = _eq_block(one_limb)
    fams["corners"] = _eq_block([(0, 0), (2 * P - 1, 10 * P - 1), (0, 10 * P - 1), (2 * P - 1, 0)])
    pairs = []
    for i in range(N_FIELD):
        a = rnd.randrange(2 * P)
        pairs.append((a, a % P + rnd.randrange(10) * P) if i % 2 else (a, rnd.randrange(10 * P)))
    fams["random"] = _eq_block(pairs)
    return fams


def exit_tau_max(table, K=10):
    """The largest tau for which some a < K p gives t = tau + p in to_gnark_ct (see exit_targets)."""
    c = m.value1(m._T[table])
    f = m.RP % P * pow(c, -1, P) % P
    assert f in (4, 16, 256) and (m.RP - f * c) % P == 0 and 0 < f * c < m.RP
    u = (m.RP - f * c) // P
    return ((K - 1) * c - 1) // u


def exit_targets(table, K=10):
    """Inputs a < K p whose product t = a Const / 2^392 lands on chosen values.  t is tau or tau + p with tau the canonical
    residue, and t = tau exactly when tau 2^392 >= a Const.  The three constants are 2^384, 2^388, 2^390 mod p, so
    a = 2^392 / Const mod p is 256, 16 or 4 and gives t = 1; the same a plus p gives t = p + 1; every nonzero multiple
    of p gives t = p.  Returns {name: a}."""
    c = m.value1(m._T[table])
    cinv = pow(c, -1, P)

    def a_of(tau):
        return tau * m.RP % P * cinv % P

    out = {"t=0": 0, "t=1": a_of(1), "t=p-1": a_of(P - 1), "t=p": P, "t=p_from_9p": 9 * P, "t=p+1": a_of(1) + P}
    # The largest t below the caller's bound.  f = 2^392 / Const mod p is 2^8, 2^4 or 2^2, so a(tau) = f tau for every tau below
    # p / f, and with a = f tau + j p the condition tau 2^392 < a Const reads tau u < j Const, u = (2^392 - f Const) / p:
    # the largest tau is (j Const - 1) // u at the top representative j = K - 1.
    out["t=max"] = a_of(exit_tau_max(table, K)) + (K - 1) * P
    assert out["t=max"] < K * P
    return out


def exit_families(name):
    table = EXIT_TABLE[name]
    rnd = random.Random(SEL[name])
    c = m.value1(m._T[table])
    cinv = pow(c, -1, P)
    fams = {}

    def blk(vals):
        return block(name, len(vals), A=(m.arr(vals), None, None, None))

    fams["targets"] = blk(list(exit_targets(table).values()))
    edge = []
    for K in (2, 10):
        edge += [v for v in EDGE + [m.top_below(v, K) for v in (0, 1, P - 1)] + [K * P - 1] if v < K * P]
    fams["edges"] = blk(edge)
    # t >= p on purpose: tau below (K - 1) p Const / 2^392 at the top representative
    sub = []
    for K in (2, 10):
        lim = ((K - 1) * P * c) >> 392
        for _ in range(128):
            sub.append(rnd.randrange(lim) * m.RP % P * cinv % P + (K - 1) * P)
    fams["subtracting"] = blk(sub)
    fams["random"] = blk([rnd.randrange((2 if i % 2 else 10) * P) for i in range(N_FIELD)])
    return fams


def invert_families():
    rnd = random.Random(6)
    one = m.value1(m.KONE)

    def blk(vals):
        return block("invert", len(vals), A=(m.arr(vals), None, None, None))

    return {"edges": blk([0, one, P - 1, P, P + 1, 2 * P - 1]), "random": blk([rnd.randrange(2 * P) for _ in range(N_POINT)])}


def affine_families():
    """info: the affine (x, y) residues each record stands for (None: not a point, the words are whatever 0 inverts to)."""
    rnd = random.Random(7)
    G = multiples()
    pts = [G[rnd.randrange(64)] for _ in range(N_POINT // 4)]
    fams = {}
    for nm, (xk, yk, zk) in {"x<10p,y<6p": (10, 6, 2), "y<10p": (10, 10, 2), "below_p": (1, 1, 1)}.items():
        fams[nm] = (block("affine_words_ct", len(pts), A=stored(pts, rnd, xk, yk, zk)), list(pts))
    z = m.zeros(1)
    fams["all_zero"] = (block("affine_words_ct", 1, A=(z, z, z, z)), [None])
    o = m.one(1)
    fams["four_ones"] = (block("affine_words_ct", 1, A=(o, o, o, o)), [(1, 1)])
    # The canonical step subtracts when the gnark value tau of a coordinate is below (its last product's operand) Const /
    # 2^392, about p / 1400: records whose x, y or both have a SMALL gnark value.  affine_words_ct is field arithmetic,
    # so these need not be curve points.
    rinv = pow(1 << 384, -1, P)
    small = []
    for i in range(24):
        tx = rnd.randrange(1, 1 << 40) if i % 3 != 1 else rnd.randrange(P)
        ty = rnd.randrange(1, 1 << 40) if i % 3 != 0 else rnd.randrange(P)
        small.append((tx * rinv % P, ty * rinv % P))
    fams["subtracting"] = (block("affine_words_ct", len(small), A=stored(small, rnd, 10, 6, 2)), small)
    return fams


def _ones_doubled(t):
    acc = tuple(m.one(1) for _ in range(4))
    for _ in range(t):
        acc = m.dbl(acc)
    return acc


def madd_families(name):
    """Every family with all four (bit, started) combinations.  info: (acc affine or None, P affine) per element."""
    rnd = random.Random(SEL[name])
    G = multiples()
    fams = {}

    def four(acc, x2, y2, info):
        n = x2.shape[0]
        blocks, infos = [], []
        for bit in (0, ONES):
            for started in (0, ONES):
                blocks.append(block(name, n, A=acc, B=(x2, y2, None, None), arg0=bit, arg1=started))
                infos += info
        return np.concatenate(blocks), infos

    n = N_POINT // 8
    ia = [rnd.randrange(64) for _ in range(n)]
    ib = [(i + 1 + rnd.randrange(63)) % 64 for i in ia]
    assert all(i != j for i, j in zip(ia, ib))
    A_aff, B_aff = [G[i] for i in ia], [G[j] for j in ib]
    x2, y2 = affine_in(B_aff)
    fams["generic"] = four(stored(A_aff, rnd, 1, 1, 1), x2, y2, list(zip(A_aff, B_aff)))
    x2, y2 = affine_in(B_aff, lift=1)
    fams["at_the_bounds"] = four(stored(A_aff, rnd, 10, 6, 2), x2, y2, list(zip(A_aff, B_aff)))
    # the nonsense sums: P = acc and P = -acc under a non-trivial scaling of acc
    same = [G[i] for i in ia[:16]]
    x2, y2 = affine_in(same, lift=1)
    fams["P=acc"] = four(stored(same, rnd, 10, 6, 2), x2, y2, list(zip(same, same)))
    opp = [oracle.neg(p) for p in same]
    x2, y2 = affine_in(opp)
    fams["P=-acc"] = four(stored(same, rnd, 10, 6, 2), x2, y2, list(zip(same, opp)))
    # not yet a point: four ones doubled t times
    for t in (0, 1, 2, 254):
        x2, y2 = affine_in(B_aff[:4], lift=t % 2)
        acc = tuple(np.repeat(c, 4, axis=0) for c in _ones_doubled(t))
        fams[f"ones_doubled_{t}"] = four(acc, x2, y2, [(None, b) for b in B_aff[:4]])
    return fams


def add_families():
    """info: (a, b) affine points or None per element.  The fold is separate (fold_terms)."""
    rnd = random.Random(10)
    G = multiples()
    n = N_POINT // 4
    ia = [rnd.randrange(64) for _ in range(n)]
    ib = [(i + 1 + rnd.randrange(63)) % 64 for i in ia]
    A_aff, B_aff = [G[i] for i in ia], [G[j] for j in ib]
    fams = {}

    def fam(a_pts, b_pts, bounds_a=(10, 6, 2), bounds_b=(10, 6, 2)):
        return (block("add_ct", len(a_pts), A=stored(a_pts, rnd, *bounds_a), B=stored(b_pts, rnd, *bounds_b)), list(zip(a_pts, b_pts)))

    fams["generic"] = fam(A_aff, B_aff, (1, 1, 1), (1, 1, 1))
    fams["at_the_bounds"] = fam(A_aff, B_aff, (10, 10, 2), (10, 10, 2))
    fams["mixed_bounds"] = fam(A_aff, B_aff, (10, 6, 2), (1, 1, 1))
    k = 32
    fams["a_infinite"] = fam([None] * k, B_aff[:k], (10, 10, 2), (10, 10, 2))
    fams["b_infinite"] = fam(A_aff[:k], [None] * k, (10, 10, 2), (10, 10, 2))
    fams["both_infinite"] = fam([None] * 4, [None] * 4)
    # the same point and a point and its negative under INDEPENDENT scalings (stored draws a fresh z for each operand)
    fams["same_point"] = fam(A_aff[:k], A_aff[:k], (10, 10, 2), (10, 6, 2))
    fams["same_point_below_p"] = fam(A_aff[:k], A_aff[:k], (1, 1, 1), (2, 2, 2))
    fams["opposite"] = fam(A_aff[:k], [oracle.neg(p) for p in A_aff[:k]], (10, 10, 2), (10, 6, 2))
    fams["opposite_below_p"] = fam(A_aff[:k], [oracle.neg(p) for p in A_aff[:k]], (1, 1, 1), (2, 2, 2))
    # an infinite operand whose x and y are those of a finite point: zz = 0 alone decides
    inp, info = fam(A_aff[:8], B_aff[:8])
    inp[:, 4 + 28:4 + 56] = 0
    fams["a_infinite_by_zz_alone"] = (inp, [(None, b) for _, b in info])
    return fams


def fold_terms():
    """Nine terms j G for k_g1_sum_ct's fold-in-half order (h = ceil(m / 2), term[i] += term[i + h] for i < m - h), placed so
    that the exceptional arms meet, also on operands that are themselves outputs of add_ct:
        level 1 (m = 9, h = 5)   5 + 5 = 10 (the double), 9 + (-9) = infinity, infinity + 12 (arm 1), 2 + 8 = 10
        level 2 (m = 5, h = 3)   10 + 10 = 20: the double again, of a doubled point and a sum under different scalings;
                                 infinity (arm 4's zero words) + 31 (arm 1)
        level 3 (m = 3, h = 2)   20 + 12 = 32          level 4 (m = 2, h = 1)   32 + 31 = 63
    Returns (X28 block, affine list)."""
    rnd = random.Random(11)
    G = multiples()
    pts = [G[4], G[8], None, G[1], G[30], G[4], oracle.neg(G[8]), G[11], G[7]]
    return stored(pts, rnd, 10, 6, 2), pts


def fold_levels(terms, add_fn):
    """Runs the fold with add_fn(a, b) -> point (X28 tuples of arrays); returns the term array after every level."""
    terms = tuple(c.copy() for c in terms)
    mcount, out = terms[0].shape[0], []
    while mcount > 1:
        h = (mcount + 1) // 2
        i = np.arange(mcount - h)
        res = add_fn(m._take(terms, i), m._take(terms, i + h))
        m._put(terms, i, res)
        out.append(tuple(c[:h].copy() for c in terms))
        mcount = h
    return out


def walk_families():
    """info: (k, steps, affine point or None) per element; the expected point is (k mod 2^steps) P.  256 lanes."""
    rnd = random.Random(12)
    G = multiples()
    ks, steps, pts, lifts = [], [], [], []

    def put(k, s, pt, lift=0):
        ks.append(k), steps.append(s), pts.append(pt), lifts.append(lift)

    for s in (1, 2, 9, 64, 255):
        for k in sorted({0, 1, 2, 3, 1 << (s - 1), (1 << s) - 1}):
            if k < (1 << s):
                put(k, s, G[rnd.randrange(64)], lift=k & 1)
    for k in (R - 1, R - 2, (R - 1) // 2, (R + 1) // 2):
        put(k, 255, G[rnd.randrange(64)])
        put(k, 255, G[rnd.randrange(64)], lift=1)            # an affine operand in [p, 2p)
    for _ in range(206):
        put(rnd.randrange(R), 255, G[rnd.randrange(64)], lift=rnd.randrange(2))
    # an affine operand AT the bound: x2, y2 or both exactly 2p - 1.  Not a curve point (pt None: no group law to compare
    # with); the walk is field arithmetic and the model asserts that it stays inside the limb bounds.
    top = []
    for k, s in ((rnd.randrange(R), 255), (R - 1, 255), (3, 2), (1 << 63, 64)):
        for which in ("x", "y", "xy"):
            put(k, s, None)
            top.append((len(ks) - 1, which))
    n_plain = len(ks)
    # a set bit at or above `steps`: the `over` word is 1 and the walk is that of the low bits
    for k, s in (((1 << 9) + 5, 9), ((1 << 200) + 1, 64), ((1 << 255) | 3, 255), (1 << 1, 1), (R - 1, 64), (1 << 255, 2)):
        put(k, s, G[rnd.randrange(64)], lift=1)
    shown = [p if p is not None else G[0] for p in pts]
    xv = [m.to_mont(p[0]) + l * P for p, l in zip(shown, lifts)]
    yv = [m.to_mont(p[1]) + l * P for p, l in zip(shown, lifts)]
    for i, which in top:
        if "x" in which:
            xv[i] = 2 * P - 1
        if "y" in which:
            yv[i] = 2 * P - 1
    x2, y2 = m.arr(xv), m.arr(yv)
    inp = block("walk_ct", len(ks), A=(x2, y2, None, None), arg0=np.array(steps, dtype=np.uint64))
    inp[:, 60:68] = g.scalar_words(ks)
    return inp, list(zip(ks, steps, pts)), n_plain


def twin_role(table):
    """The role of fp28_model.to_gnark_msm (selftest operation 13's to_gnark_msm selectors) whose model uses `table`."""
    probe = m.arr([5, P + 7, 3 * P - 1])
    want = m.to_gnark(probe, table)
    roles = [r for r in range(4) if (m.to_gnark_msm(probe, r) == want).all()]
    assert roles, table
    return roles[0]
