"""Big-integer model of the BATCHED constant-time MSM (csrc/msm_ct_kernels.hip: k_g1_sum_ct_seg, k_msm_ct_finish_seg)
on top of tests/msm_ct_model.py, and the case set of its GPU tests.

Nothing of the library.  One walk leaves the terms of k MSMs behind each other; MSM j owns term[begin_j, begin_j + n_j).
The segment rule: every segment is folded by msm_ct_model.fold ON ITS OWN -- h = ceil(m / 2), term[b + i] +=
term[b + i + h] for i < m - h, m <- h -- with the levels above TAIL (512) terms run by the level launches, one launch a
level for all segments together, and the rest by the segment's one block, which recomputes where the launches left it
by `while m > 512: m = ceil(m / 2)`, a function of the count alone.  split() is that rule written out and must give
msm_ct_model.fold's additions in msm_ct_model.fold's order; level_launches() is what the host launches for a list of
counts.

one_big_fold() is DELIBERATELY WRONG: it folds the whole array as one segment and reads result j at term[begin_j].  It
is here so that the tests can show that the boundary cases tell the two apart.

A case is (name, segments, bits) with segments a list of lists of (k, g) as in msm_ct_model; a multi case is
(name, gsets, ks, bits): k base sets against one scalar vector."""
import numpy as np

import msm_ct_model as mm
from msm_ct_model import R

TAIL = 512            # kMsmCtSumTail
MAX_PAIRS = 65536     # kMsmCtMax
MAX_MSMS = 4096
LEAD = 7              # pairs in front of a call's first pair in the arrays build() makes: offsets[0] = 7

K1_SIZES = (1, 2, 3, 64, 65, 513)
MIXED_COUNTS = (0, 1, 2, 3, 5, 0, 64, 65, 127, 0)
LEVEL_COUNTS = (513, 3, 1025, 0, 512)
NO_LEVEL_COUNTS = (512, 512)
ROUND_COUNTS = (129, 128, 129, 128)
BITS = (1, 9, 255)
MULTI_SHAPES = tuple((k, n) for k in (1, 3, 6) for n in (1, 129, 300))


def tail_size(count):
    """Where the level launches leave a segment: what the block starts from."""
    m = count
    while m > TAIL:
        m = (m + 1) // 2
    return m


def size_at_level(count, level):
    """The segment's size when launch number `level` (from 0) starts: the kernel's own derivation."""
    m = count
    for _ in range(level):
        if m <= TAIL:
            break
        m = (m + 1) // 2
    return m


def level_launches(counts):
    """Launches of k_g1_sum_ct_seg for these counts: levels while ANY segment is above TAIL."""
    level = 0
    while any(size_at_level(c, level) > TAIL for c in counts):
        level += 1
    return level


def split(ts):
    """One segment's fold in two parts, as the kernels run it: (total, additions of the level launches, additions of
    the block), the additions as msm_ct_model.fold lists them."""
    ts, launched, block = list(ts), [], []
    m = len(ts)
    assert m >= 1
    while m > TAIL:
        h = (m + 1) // 2
        for i in range(m - h):
            launched.append((m, i, mm.arm(ts[i], ts[i + h])))
            ts[i] = (ts[i] + ts[i + h]) % R
        m = h
    assert m == tail_size(len(ts))
    while m > 1:
        h = (m + 1) // 2
        for i in range(m - h):
            block.append((m, i, mm.arm(ts[i], ts[i + h])))
            ts[i] = (ts[i] + ts[i + h]) % R
        m = h
    return ts[0], launched, block


def fold_segments(ts, counts):
    """[(total mod r, additions)] per segment of the concatenated terms; an empty segment is (0, [])."""
    out, b = [], 0
    for n in counts:
        out.append(mm.fold(ts[b:b + n]) if n else (0, []))
        b += n
    assert b == len(ts)
    return out


def one_big_fold(ts, counts):
    """WRONG ON PURPOSE: one fold over all the terms, result j read where segment j begins."""
    ts = list(ts)
    m = len(ts)
    while m > 1:
        h = (m + 1) // 2
        for i in range(m - h):
            ts[i] = (ts[i] + ts[i + h]) % R
        m = h
    out, b = [], 0
    for n in counts:
        out.append(ts[b] if n else 0)
        b += n
    return out


def is_edge(count, m, i):
    """An addition of the first level that touches the segment's first or last term."""
    return m == count and (i == 0 or i + (m + 1) // 2 == m - 1)


# ---------------------------------------------------------------------------
# The case set
# ---------------------------------------------------------------------------
def _take(oracle, n, start=0):
    gs, ks = mm._pool(oracle)
    return [(ks[(start + i) % len(ks)], gs[(start + 3 * i + 1) % len(gs)]) for i in range(n)]


def _segments(oracle, counts, start=0):
    out = []
    for n in counts:
        out.append(_take(oracle, n, start))
        start += n
    return out


def k1_cases(oracle):
    return [("k=1 n=%d" % n, [_take(oracle, n, 11)], 255) for n in K1_SIZES]


def mixed_case(oracle):
    return ("mixed segments", _segments(oracle, MIXED_COUNTS, 40), 255)


def boundary_cases(oracle):
    gs, ks = mm._pool(oracle)
    k, g = ks[0], gs[0]
    P, N = (k, g), (k, R - g)
    a, b, c, d = _take(oracle, 4, 5)
    mid = _take(oracle, 3, 20)
    return [("[P] [-P]", [[P], [N]], 255),
            ("[.., P] [-P, ..]", [[a, b, P], [N, c, d]], 255),
            ("[P, -P] [P, P]", [[P, N], [P, P]], 255),
            ("all terms equal inside a segment", [[P] * 5, [(ks[1], gs[1])] * 4, [N] * 3], 255),
            ("zero scalars and infinity bases at both edges",
             [[(0, g)] + mid + [(0, gs[2])], [(k, None)] + mid + [(ks[1], None)], [(0, g), (k, None)]], 255)]


# every arm of add_ct at a segment edge: arm -> (case, segment, m, i)
ARMS_AT_EDGES = {
    "sum": ("[.., P] [-P, ..]", 0, 3, 0),
    "infinity": ("[P, -P] [P, P]", 0, 2, 0),
    "double": ("[P, -P] [P, P]", 1, 2, 0),
    "b": ("zero scalars and infinity bases at both edges", 0, 5, 0),
    "a": ("zero scalars and infinity bases at both edges", 0, 5, 1),
}


def level_cases(oracle):
    return [("level path [513, 3, 1025, 0, 512]", _segments(oracle, LEVEL_COUNTS, 100), 255),
            ("no level [512, 512]", _segments(oracle, NO_LEVEL_COUNTS, 300), 255)]


def round_case(oracle):
    return ("Prove's round shape", _segments(oracle, ROUND_COUNTS, 500), 255)


def bits_cases(oracle, counts=(3, 65, 2)):
    """Every scalar at 2^bits - 1 (at 255 bits r - 1, the largest canonical scalar)."""
    out = []
    for b in BITS:
        top = min((1 << b) - 1, R - 1)
        out.append(("bits=%d, scalars at the top" % b, [[(top, g) for _, g in seg] for seg in _segments(oracle, counts, 700)], b))
    return out


def violation_cases(oracle, counts=(3, 65, 2)):
    """One scalar of exactly 2^bits, in the LAST MSM only.  No case at 255 bits: 2^255 is not a canonical scalar."""
    out = []
    for b in BITS[:-1]:
        segs = [[(k & ((1 << b) - 1), g) for k, g in seg] for seg in _segments(oracle, counts, 700)]
        segs[-1][-1] = (1 << b, segs[-1][-1][1])
        out.append(("bits=%d, 2^bits in the last MSM" % b, segs, b))
    return out


def all_cases(oracle):
    """Every batch case with a result."""
    return k1_cases(oracle) + [mixed_case(oracle)] + boundary_cases(oracle) + level_cases(oracle) + [round_case(oracle)] + \
        bits_cases(oracle)


def multi_cases(oracle):
    gs, ks = mm._pool(oracle)
    out = []
    for k, n in MULTI_SHAPES:
        gsets = [[gs[(17 * j + 5 * i + 2) % len(gs)] for i in range(n)] for j in range(k)]
        if n > 1:
            gsets[-1][0] = None                        # an infinity base in the last set
        out.append(("multi k=%d n=%d" % (k, n), gsets, [ks[(i + 900) % len(ks)] for i in range(n)], 255))
    return out


def multi_as_batch(gsets, ks):
    """The same MSMs as batch segments: the scalar vector replicated."""
    return [[(k, g) for k, g in zip(ks, gset)] for gset in gsets]


# ---------------------------------------------------------------------------
# Arrays
# ---------------------------------------------------------------------------
_memo = {}


def _limbs(oracle, coracle, g):
    if g not in _memo:
        _memo[g] = mm.gm.point_limbs(oracle, coracle, g)
    return _memo[g]


def arrays(oracle, coracle, segments, lead=LEAD):
    """(points uint64[lead + n, 12], scalars uint64[lead + n, 4], offsets uint64[k + 1]) with offsets[0] = lead: the
    call's pairs start behind `lead` pairs that belong to no MSM."""
    flat = _take(oracle, lead, 77) + [p for seg in segments for p in seg]
    pts = np.array([_limbs(oracle, coracle, g) for _, g in flat], dtype=np.uint64).reshape(-1, 12)
    sc = mm.to_limbs(oracle, [k for k, _ in flat]) if flat else np.zeros((0, 4), dtype=np.uint64)
    offs = np.cumsum([lead] + [len(seg) for seg in segments]).astype(np.uint64)
    return pts, sc, offs


def expected(oracle, coracle, segments, bits):
    """uint64[k, 18]: the model's point per segment, as the 18 words the library returns."""
    counts = [len(seg) for seg in segments]
    ts = mm.terms([p for seg in segments for p in seg], bits)
    return np.array([mm.expected_jac(oracle, coracle, total) for total, _ in fold_segments(ts, counts)],
                    dtype=np.uint64).reshape(-1, 18)
