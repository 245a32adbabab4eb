"""Big-integer model of the constant-time MSM over a resident base set with the walk split into chunks
(csrc/msm_ct_bases_kernels.hip, csrc/msm_ct_bases_api.hip) on top of tests/msm_ct_model.py, and the case set of its
GPU tests.

Nothing of the library.  A base is a multiple g G of the generator (None: infinity), as in msm_ct_model.

The split.  k = sum_j 2^(c j) d_j with c-bit digits; a call with the public bound `bits` walks Cb = ceil(bits / c)
chunks, chunk j over steps(j) = c bits, the top one over bits - c (Cb - 1).  The table row j holds 2^(c j) P, so lane
(p, j) leaves the multiple d_j 2^(c j) g at term[p Cb + j], and pairs [begin, begin + count) own the run
[begin Cb, (begin + count) Cb): msm_ct_model.fold (msm_ct_batch_model.fold_segments) runs on it as it is.

Exactness.  Q = 2^(c j) P has order r like P.  walk_chunk asserts on EVERY step behind the first set bit -- the sum
2m Q + Q is computed whether the bit keeps it or not -- that 2m Q is neither Q nor -Q: with d < 2^64 < r the prefix
satisfies 1 < 2m + 1 < 2^64, so not even a discarded sum is exceptional.  The model must find none at all; k = r - 1, the
one scalar whose 255-step walk discards (r - 1) P + P, is among the cases.

The arms between the chunk terms.  The terms of ONE pair are d_j 2^(c j) g with k = sum_j d_j 2^(c j) < r.  Two disjoint
partial sums a, b of them satisfy a + b <= k < r, so they are never opposite, and the one that holds the highest
non-zero digit is the larger, so they are never equal: within the run of one pair add_ct takes "sum", "a" or "b" and
NEVER "double" or "infinity" (fold_one_pair asserts that on every case).  The two exceptional arms between chunk terms
need two pairs on one row: equal scalars put equal terms Cb apart ("double" at the first level, chunk by chunk), and
opposite scalars k, r - k leave the two halves of r g for the last addition ("infinity").  ARMS pins all five."""
import numpy as np

import msm_ct_batch_model as bm
import msm_ct_model as mm
from msm_ct_model import R

CHUNK_BITS = (8, 16, 32, 64)
DEFAULT_CHUNK_BITS = 16
MAX_TERMS = 65536
MAX_MSMS = 4096
SIZES = (1, 2, 3, 63, 64, 65, 257, 513)
EXPORT_SIZES = (1, 63, 64, 65, 257)
MIXED_COUNTS = bm.MIXED_COUNTS
LEVEL_COUNTS = bm.LEVEL_COUNTS


def chunks(bits, c):
    return (bits + c - 1) // c


def steps(j, c, bits):
    """The public step count of chunk j."""
    cb = chunks(bits, c)
    assert 0 <= j < cb
    return c if j + 1 < cb else bits - c * (cb - 1)


def skipped(j, c, bits):
    """The bits shifted out between `bits` and the chunk's top: a function of j, c and bits alone."""
    return bits - (c * j + steps(j, c, bits))


def digits(k, c, bits):
    """The Cb digits of k < 2^bits, chunk 0 first; digit j is below 2^steps(j)."""
    assert 1 <= bits <= 255 and 0 <= k < R and k >> bits == 0, (hex(k), bits)
    cb = chunks(bits, c)
    ds = [(k >> (c * j)) & ((1 << c) - 1) for j in range(cb)]
    assert sum(d << (c * j) for j, d in enumerate(ds)) == k
    assert all(d >> steps(j, c, bits) == 0 for j, d in enumerate(ds))
    assert all(skipped(j, c, bits) + steps(j, c, bits) + c * j == bits for j in range(cb))
    return ds


def table_multiples(g, c):
    """The multiples of G the table's C rows hold for the base g G (None: infinity in every row)."""
    return [None if g is None else g * pow(2, c * j, R) % R for j in range(chunks(255, c))]


def walk_chunk(d, nsteps):
    """walk_ct over `nsteps` bits of d, MSB first, on the multiple m of Q the accumulator holds.  Asserts that no sum
    the lane computes, kept or discarded, is exceptional; returns (m, sums computed)."""
    assert 0 <= d < 1 << nsteps and nsteps <= 64
    m, started, sums = 0, False, 0
    for t in range(nsteps - 1, -1, -1):
        bit = (d >> t) & 1
        if not started:
            m, started = (1, True) if bit else (0, False)
            continue
        m *= 2                                                   # the doubling: never infinity, r is odd
        assert m % R != 0
        assert m % R != 1 and (m + 1) % R != 0, (hex(d), t)      # Q + Q and Q + (-Q): kept or not, never
        sums += 1
        m += bit
    assert m == d
    return m, sums


def terms(pairs, c, bits, walk=True):
    """[(k, g)] -> the multiples of G at term[p Cb + j] (0: the all-zero record)."""
    out = []
    for k, g in pairs:
        row = table_multiples(g, c)
        for j, d in enumerate(digits(k, c, bits)):
            if walk:
                assert walk_chunk(d, steps(j, c, bits))[0] == d
            out.append(0 if g is None else d * row[j] % R)
    return out


def fold_one_pair(k, g, c, bits):
    """The fold over the run of ONE pair: (total, arms).  Asserts the claim of the docstring: no double, no infinity."""
    total, taken = mm.fold(terms([(k, g)], c, bits))
    assert all(a in ("sum", "a", "b") for _, _, a in taken), (hex(k), c, bits)
    assert total == (0 if g is None else k * g % R)
    return total, taken


def fold_call(pairs, counts, c, bits, walk=True):
    """[(total mod r, arms)] per MSM of a call over the concatenated pairs; counts: pairs per MSM."""
    cb = chunks(bits, c)
    return bm.fold_segments(terms(pairs, c, bits, walk), [n * cb for n in counts])


def level_launches(counts, c, bits):
    """msm_ct_batch_model's rule on count Cb terms per MSM."""
    return bm.level_launches([n * chunks(bits, c) for n in counts])


# ---------------------------------------------------------------------------
# Base sets.  P_i = (A + i Q) G, what the C oracle's points_walk makes in one call; `inf` positions are infinity.
# ---------------------------------------------------------------------------
class Bases:
    def __init__(self, oracle, n, inf=(), seed=3101):
        self.n, self.inf = n, tuple(sorted(set(i for i in inf if 0 <= i < n)))
        self.a, self.q = [v or 1 for v in mm.gm.fm._rand(oracle, seed, 2)]
        self.g = [None if i in self.inf else (self.a + i * self.q) % R for i in range(n)]
        assert all(g is None or g for g in self.g)

    def limbs(self, coracle, c=0, j=0):
        """Row j of the table for chunk width c as uint64[n, 12] (row 0: the set itself)."""
        s = pow(2, c * j, R)
        pts = coracle.points_walk(self.a * s % R, self.q * s % R, self.n) if self.n else np.zeros((0, 12), dtype=np.uint64)
        for i in self.inf:
            pts[i] = 0
        return pts


def edge_infinities(n):
    """Infinity bases at the start, in the middle and at the end."""
    return (0, n // 2, n - 1) if n >= 4 else ()


# ---------------------------------------------------------------------------
# The case set.  A case is (name, g-set [g | None], rows [index] | None, scalars [k], bits).
# ---------------------------------------------------------------------------
def pairs_of(case):
    _, gs, rows, ks, _ = case
    rows = range(len(ks)) if rows is None else rows
    return [(k, gs[r]) for k, r in zip(ks, rows)]


def arm_cases(oracle, c):
    """n = 1 and n = 2, one row: the families of the chunk boundary."""
    gs, ks = mm._pool(oracle)
    g, k = gs[0], ks[0]
    cb = chunks(255, c)
    h = (cb + 1) // 2
    ones = (1 << 254) - 1
    assert ones < R
    return [("digits (2^c - 1, 1, 0, ...)", [g], [0], [(1 << c) - 1 + (1 << c)], 255),
            ("all-ones digits", [g], [0], [ones], 254),
            ("k = 2^c", [g], [0], [1 << c], 255),
            ("k = 2^c - 1", [g], [0], [(1 << c) - 1], 255),
            ("k = 2^c at c + 1 bits", [g], [0], [1 << c], c + 1),
            ("k = 2^c - 1 at c bits", [g], [0], [(1 << c) - 1], c),
            ("k = r - 1", [g], [0], [R - 1], 255),
            ("only digit h set", [g], [0], [1 << (c * h)], 255),
            ("random", [g], [0], [k], 255),
            ("the same row twice, opposite scalars", [g], [0, 0], [k, R - k], 255),
            ("the same row twice, equal scalars", [g], [0, 0], [k, k], 255),
            ("two rows, P and -P, equal scalars", [g, R - g], [0, 1], [k, k], 255),
            ("an infinity row beside a point", [None, g], [0, 1], [k, ks[1]], 255)]


def arms(c):
    """Every arm of add_ct between chunk terms, pinned: arm -> (case, m, i) in msm_ct_model.fold's listing."""
    cb = chunks(255, c)
    return {"sum": ("random", cb, 0),
            "a": ("digits (2^c - 1, 1, 0, ...)", cb, 0),
            "b": ("only digit h set", cb, 0),
            "double": ("the same row twice, equal scalars", 2 * cb, 0),
            "infinity": ("the same row twice, opposite scalars", 2, 0)}


def size_cases(oracle, n):
    """Random scalars over a walk set of n bases; edges: scalars 0 / 1 / r - 1 and infinity rows at the edges; all
    pairs on one row; rows as a reversal and with repeats (rows None is the random case)."""
    _, ks = mm._pool(oracle)
    ks = list(ks[:n])
    plain, holes = Bases(oracle, n), Bases(oracle, n, edge_infinities(n))
    edge = list(ks)
    for i, k in ((0, 0), (n - 1, 0), (n // 2, 0), (n // 3, 1), (2 * n // 3, R - 1)):   # later entries win at small n
        edge[i] = k
    return [("random n=%d, rows null" % n, plain.g, None, ks, 255),
            ("edges n=%d" % n, holes.g, None, edge, 255),
            ("one row n=%d" % n, plain.g, [n // 2] * n, ks, 255),
            ("reversed rows n=%d" % n, holes.g, list(range(n - 1, -1, -1)), ks, 255),
            ("repeated rows n=%d" % n, plain.g, [(7 * i) % max(1, n // 2) for i in range(n)], ks, 255)]


def bits_list(c):
    return sorted(set(b for b in (1, c - 1, c, c + 1, 2 * c, 254, 255) if 1 <= b <= 255))


def bits_cases(oracle, c, n=5):
    """Every scalar with its top bit set (bit bits - 1) and the bits below random; at 255 bits r - 1 leads."""
    gs, ks = mm._pool(oracle)
    out = []
    for b in bits_list(c):
        top = [(1 << (b - 1)) | (k & ((1 << (b - 1)) - 1)) for k in ks[10:10 + n]]
        top = [k if k < R else R - 1 for k in top]
        top[0] = min((1 << b) - 1, R - 1)
        out.append(("c=%d bits=%d, top bit set" % (c, b), gs[:n], None, top, b))
    return out


def violation_cases(oracle, c, n=5):
    """A scalar of exactly 2^bits at the last index (no case at 255 bits: 2^255 is not a canonical scalar)."""
    out = []
    for name, gs, rows, ks, b in bits_cases(oracle, c, n):
        if b < 255 and 1 << b < R:
            out.append((name + ", 2^bits last", gs, rows, [k & ((1 << b) - 1) for k in ks[:-1]] + [1 << b], b))
    return out


def batch_case(oracle, counts, start=0):
    """(g-set, rows, scalars, offsets) of a batch over one walk set: MSM j covers counts[j] pairs, rows wander."""
    _, ks = mm._pool(oracle)
    total = sum(counts)
    size = 300
    base = Bases(oracle, size, (0, 150, 299))
    rows = [(start + 13 * p) % size for p in range(total)]
    sc = [ks[(start + p) % len(ks)] for p in range(total)]
    offs = np.cumsum([0] + list(counts)).astype(np.uint64)
    return base, rows, sc, offs


def all_cases(oracle):
    """Every case with a result that the GPU tests run, as (c, case)."""
    out = []
    for c in CHUNK_BITS:
        out += [(c, case) for case in arm_cases(oracle, c) + bits_cases(oracle, c)]
        for n in SIZES:
            out += [(c, case) for case in size_cases(oracle, n)]
    return out


# ---------------------------------------------------------------------------
# Arrays and expected words
# ---------------------------------------------------------------------------
def set_limbs(oracle, coracle, gs):
    return np.array([mm.gm.point_limbs(oracle, coracle, g) for g in gs], dtype=np.uint64).reshape(-1, 12)


def total_of(case, c, walk=False):
    """The model's total of a single call: the fold over the chunk terms."""
    pairs = pairs_of(case)
    if not pairs:
        return 0
    total, _ = fold_call(pairs, [len(pairs)], c, case[4], walk)[0]
    assert total == sum(k * g for k, g in pairs if g is not None) % R
    return total


def expected(oracle, coracle, case, c):
    return mm.expected_jac(oracle, coracle, total_of(case, c))
