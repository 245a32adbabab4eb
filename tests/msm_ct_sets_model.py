"""Model of the constant-time MSM over up to four resident base sets in one call (curdle_msm_g1_ct_bases_sets_batch;
csrc/msm_ct_bases_kernels.hip: k_msm_ct_walk_rows with its sets by value) on top of tests/msm_ct_bases_model.py, and the
case set of its GPU tests.  Nothing of the library.

The index rule.  Set s covers the global rows [B_s, B_s + n_s) with B_0 = 0 and B_(s+1) = B_s + n_s; an empty set covers
nothing.  A lane finds its set as the kernel does: starting from set 0 it moves to set t = 1, 2, 3 whenever
row >= B_t, where B_t of a set the call does not have is the total -- three compares, no search.  Empty sets share their
first index with the set behind them, which the last matching compare picks.  locate() asserts that the set found holds
the row.

Everything behind the load is the single-set model: the terms of pair p lie at term[p Cb + j] and the segmented fold
runs on them, so the result over sets is the result over ONE set made of the concatenated points -- which
fold_sets checks against msm_ct_bases_model.fold_call on every case.

The arms.  As in the single-set model the two exceptional arms of add_ct need two pairs on one point; here the SAME
point is resident in two DIFFERENT sets (the prover's registry keeps the first occurrence, but the primitive must not
care): equal scalars give "double" at the first level, opposite scalars leave "infinity" for the last addition."""
import numpy as np

import msm_ct_bases_model as cb
import msm_ct_model as mm
from msm_ct_model import R

MAX_SETS = 4
SET_SIZES = ((1,), (3, 5), (64, 1, 65), (0, 7, 0, 2), (17, 17, 17, 17))
ALL_WIDTHS = SET_SIZES[:3]          # the shapes every chunk width runs; the other two at c = 16
MIXED_COUNTS = cb.MIXED_COUNTS
LEVEL_COUNTS = cb.LEVEL_COUNTS
BATCH_SIZES = (100, 1, 199)         # the three sets the long batches cycle over
BITS = (1, 9, 16, 17, 255)


def firsts(sizes):
    """B_0 ... B_(n_sets): the first global row of every set, and the total."""
    assert 1 <= len(sizes) <= MAX_SETS
    out = [0]
    for n in sizes:
        out.append(out[-1] + n)
    return out


def locate(row, sizes):
    """(set, local row) of a global row, by the kernel's three compares."""
    b = firsts(sizes)
    total = b[-1]
    assert 0 <= row < total, (row, sizes)
    first = b[:-1] + [total] * (MAX_SETS - len(sizes))          # sets the call does not have begin at the total
    s = 0
    for t in range(1, MAX_SETS):
        if row >= first[t]:
            s = t
    assert s < len(sizes) and 0 <= row - first[s] < sizes[s], (row, sizes, s)
    return s, row - first[s]


def split(gs, sizes):
    """The concatenated g-list as one list per set."""
    b = firsts(sizes)
    assert len(gs) == b[-1]
    return [list(gs[b[s]:b[s + 1]]) for s in range(len(sizes))]


def pairs_over_sets(gs, sizes, rows, ks):
    """[(k, g)] with g read the way the kernel reads it: set by set."""
    sets = split(gs, sizes)
    out = []
    for k, r in zip(ks, rows):
        s, local = locate(r, sizes)
        out.append((k, sets[s][local]))
    return out


def fold_sets(gs, sizes, rows, ks, counts, c, bits, walk=False):
    """[(total, arms)] per MSM over the sets; asserted equal to the fold over the concatenated single set."""
    over_sets = cb.fold_call(pairs_over_sets(gs, sizes, rows, ks), counts, c, bits, walk)
    single = cb.fold_call([(k, gs[r]) for k, r in zip(ks, rows)], counts, c, bits, False)
    assert over_sets == single
    return over_sets


# ---------------------------------------------------------------------------
# The case set.  A case is (name, sizes, g-list of the concatenation, rows, scalars, counts per MSM, bits).
# ---------------------------------------------------------------------------
def _counts(n):
    """Three MSMs, the middle one empty."""
    return [n // 2, 0, n - n // 2]


def row_cases(oracle, sizes):
    """Rows at the first and last record of every set, reversed, repeated, alternating between the sets lane by lane;
    the concatenation has infinity records at its ends and in its middle."""
    b = firsts(sizes)
    total = b[-1]
    base = cb.Bases(oracle, total, cb.edge_infinities(total), seed=3500 + total)
    _, ks = mm._pool(oracle)
    full = [s for s in range(len(sizes)) if sizes[s]]
    edges = [r for s in full for r in (b[s], b[s + 1] - 1)]
    lists = {"edges": edges,
             "reversed": list(range(total - 1, -1, -1)),
             "repeated": [(7 * i) % max(1, total // 2) for i in range(total)],
             "alternating": [b[full[p % len(full)]] + (p // len(full)) % sizes[full[p % len(full)]] for p in range(2 * total + 1)]}
    out = []
    for name, rows in lists.items():
        sc = [ks[(3 * p + len(rows)) % len(ks)] for p in range(len(rows))]
        out.append(("%s over %s" % (name, "+".join(map(str, sizes))), tuple(sizes), base.g, rows, sc, _counts(len(rows)), 255))
    return out


def arm_cases(oracle, c):
    """The single-set arm families on a point of the SECOND set, and the same point resident in two sets."""
    gs, ks = mm._pool(oracle)
    g, k = gs[0], ks[0]
    h = (cb.chunks(255, c) + 1) // 2
    cat = [g, gs[1], gs[2], g]                                    # sets (2, 2): g is row 0 and row 3
    sizes = (2, 2)
    return [("digits (2^c - 1, 1, 0, ...)", sizes, cat, [3], [(1 << c) - 1 + (1 << c)], [1], 255),
            ("only digit h set", sizes, cat, [3], [1 << (c * h)], [1], 255),
            ("random", sizes, cat, [3], [k], [1], 255),
            ("one point in two sets, equal scalars", sizes, cat, [0, 3], [k, k], [2], 255),
            ("one point in two sets, opposite scalars", sizes, cat, [3, 0], [k, R - k], [2], 255)]


def arms(c):
    """Every arm of add_ct, pinned: arm -> (case, m, i) in msm_ct_model.fold's listing."""
    n = cb.chunks(255, c)
    return {"sum": ("random", n, 0),
            "a": ("digits (2^c - 1, 1, 0, ...)", n, 0),
            "b": ("only digit h set", n, 0),
            "double": ("one point in two sets, equal scalars", 2 * n, 0),
            "infinity": ("one point in two sets, opposite scalars", 2, 0)}


def batch_case(oracle, counts, start=0):
    """A long batch at c = 16 with rows cycling over three sets: pair p reads set p mod 3."""
    sizes = BATCH_SIZES
    b = firsts(sizes)
    base = cb.Bases(oracle, b[-1], (0, 100, b[-1] - 1), seed=3600)
    _, ks = mm._pool(oracle)
    total = sum(counts)
    rows = [b[p % 3] + (start + 13 * p) % sizes[p % 3] for p in range(total)]
    sc = [ks[(start + p) % len(ks)] for p in range(total)]
    return ("cycling %s" % (list(counts),), sizes, base.g, rows, sc, list(counts), 255)


def bits_cases(oracle):
    """scalar_bits 1 / 9 / 16 / 17 / 255 at c = 16 over sets (3, 5), every scalar with its top bit set."""
    sizes = (3, 5)
    base = cb.Bases(oracle, 8, seed=3700)
    _, ks = mm._pool(oracle)
    out = []
    for bits in BITS:
        top = [(1 << (bits - 1)) | (k & ((1 << (bits - 1)) - 1)) for k in ks[20:27]]
        top = [k if k < R else R - 1 for k in top]
        top[0] = min((1 << bits) - 1, R - 1)
        out.append(("bits=%d, top bit set" % bits, sizes, base.g, [7, 0, 3, 2, 4, 7, 1], top, [3, 4], bits))
    return out


def violation_case(case):
    """The case with a scalar of exactly 2^bits at its last index (bits < 255)."""
    name, sizes, gs, rows, ks, counts, bits = case
    assert bits < 255
    return (name + ", 2^bits last", sizes, gs, rows, [k & ((1 << bits) - 1) for k in ks[:-1]] + [1 << bits], counts, bits)


def widths_of(sizes):
    return cb.CHUNK_BITS if tuple(sizes) in ALL_WIDTHS else (16,)


def all_cases(oracle):
    """Every case with a result that the GPU test runs, as (c, case)."""
    out = []
    for sizes in SET_SIZES:
        for case in row_cases(oracle, sizes):
            out += [(c, case) for c in widths_of(sizes)]
    for c in cb.CHUNK_BITS:
        out += [(c, case) for case in arm_cases(oracle, c)]
    out += [(16, batch_case(oracle, MIXED_COUNTS, 40)), (16, batch_case(oracle, LEVEL_COUNTS, 100))]
    out += [(16, case) for case in bits_cases(oracle)]
    return out


# ---------------------------------------------------------------------------
# Arrays and expected words
# ---------------------------------------------------------------------------
def offsets_of(counts):
    return np.cumsum([0] + list(counts)).astype(np.uint64)


def totals(case, c, walk=False):
    """The model's total per MSM, from the fold over the sets' chunk terms."""
    name, sizes, gs, rows, ks, counts, bits = case
    return [t for t, _ in fold_sets(gs, sizes, rows, ks, counts, c, bits, walk)]


def expected(oracle, coracle, case, c):
    return np.array([mm.expected_jac(oracle, coracle, t) for t in totals(case, c)], dtype=np.uint64).reshape(-1, 18)
