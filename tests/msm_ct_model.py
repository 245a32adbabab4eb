"""Big-integer model of the constant-time MSM (csrc/msm_ct_kernels.hip, csrc/g1_add_ct.h): the walk at a public step
count `bits`, the fixed fold-in-half sum with the arm every addition takes, and the case set of the GPU tests.

Nothing of the library.  Every base is a multiple g G of the generator (None: infinity), so a term k_i P_i is the
multiple k_i g_i mod r and, the group having prime order r, two terms are the same point iff their multiples are equal
and negatives iff they sum to 0 mod r: the fold below IS the fold over the real points (fold_points does it over the
affine points of oracle/py; tests/test_msm_ct_model.py holds the two against each other).  The expected 18 words come
from the C oracle: (total mod r) G.

The walk.  k_msm_ct_walk shifts the scalar left by 256 - bits and takes `bits` steps: for k < 2^bits these are the last
`bits` steps of g1_mul_ct_model.walk(k), whose first 255 - bits steps are idle, so walk() here calls it -- the exactness
claim (the accumulator 2m P is neither P nor -P) is asserted on every kept sum -- and checks exactly that.

The sum.  h = ceil(m / 2); term[i] = add_ct(term[i], term[i + h]) for i < m - h; m <- h; until m = 1.  add_ct's arms, in
its priority:  "b" (a is infinity), "a" (b is infinity), "double" (the same point), "infinity" (a point and its
negative), "sum"."""
import numpy as np

import g1_mul_ct_model as gm
from g1_mul_ct_model import R, to_limbs  # noqa: F401  (what the tests take from here)

ARMS = ("b", "a", "double", "infinity", "sum")
SIZES = (1, 3, 4, 63, 64, 65, 255, 256, 257, 513, 1025)
BITS = (1, 9, 64, 254, 255)
MAX_PAIRS = 65536


def walk(k, bits):
    """The multiple the lane's term holds after `bits` steps (k itself), with gm.walk's assertions on every kept sum."""
    assert 1 <= bits <= 255 and 0 <= k < R and k < 1 << bits, (hex(k), bits)
    m, steps, exceptional = gm.walk(k)
    assert all(kind == gm.IDLE for _, _, kind in steps[: gm.STEPS - bits])   # the steps the shift drops do nothing
    return m, exceptional


def violates(k, bits):
    return k >> bits != 0


def terms(pairs, bits):
    """[(k, g)] -> the multiples of G the workspace holds (0: the all-zero record)."""
    return [0 if g is None else walk(k, bits)[0] * g % R for k, g in pairs]


def arm(a, b):
    if a == 0:
        return "b"
    if b == 0:
        return "a"
    if a == b:
        return "double"
    if (a + b) % R == 0:
        return "infinity"
    return "sum"


def fold(ts):
    """The fold-in-half sum over multiples of G.  Returns (total mod r, [(m, i, arm)]) in the order of the levels."""
    ts, taken = list(ts), []
    m = len(ts)
    assert m >= 1
    while m > 1:
        h = (m + 1) // 2
        for i in range(m - h):
            taken.append((m, i, arm(ts[i], ts[i + h])))
            ts[i] = (ts[i] + ts[i + h]) % R
        m = h
    return ts[0], taken


def fold_points(oracle, pts):
    """The same fold over affine points (None: infinity): (point, [(m, i, arm)])."""
    pts, taken = list(pts), []
    m = len(pts)
    while m > 1:
        h = (m + 1) // 2
        for i in range(m - h):
            a, b = pts[i], pts[i + h]
            if a is None:
                kind = "b"
            elif b is None:
                kind = "a"
            elif a == b:
                kind = "double"
            elif a[0] == b[0]:
                kind = "infinity"
            else:
                kind = "sum"
            taken.append((m, i, kind))
            pts[i] = oracle.add(a, b)
        m = h
    return pts[0], taken


# ---------------------------------------------------------------------------
# The case set.  A case is (name, pairs [(k, g)], bits); build() gives its arrays.
# ---------------------------------------------------------------------------
_cache = {}


def _pool(oracle):
    """1,025 random multiples and 1,025 random scalars, drawn once."""
    if "pool" not in _cache:
        v = gm.fm._rand(oracle, 2601, 2 * SIZES[-1])
        _cache["pool"] = ([g or 1 for g in v[: SIZES[-1]]], [k or 1 for k in v[SIZES[-1]:]])
    return _cache["pool"]


def arm_cases(oracle):
    """n = 2: the arms in isolation."""
    gs, ks = _pool(oracle)
    g, k = gs[0], ks[0]
    return [("(P, P), equal scalars", [(k, g), (k, g)], 255),
            ("(P, -P)", [(k, g), (k, R - g)], 255),
            ("scalar 0 first", [(0, g), (k, gs[1])], 255),
            ("scalar 0 second", [(k, g), (0, gs[1])], 255),
            ("both scalars 0", [(0, g), (0, gs[1])], 255),
            ("base infinity first", [(k, None), (ks[1], gs[1])], 255),
            ("base infinity second", [(k, g), (ks[1], None)], 255),
            ("two different points", [(k, g), (ks[1], gs[1])], 255)]


def size_cases(oracle, n):
    gs, ks = _pool(oracle)
    rnd = [(ks[i], gs[i]) for i in range(n)]
    edges = list(rnd)
    for i, k in ((0, 0), (n - 1, 0), (n // 2, 0), (n // 3, 1), (2 * n // 3, R - 1)):   # later entries win at small n
        edges[i] = (k, edges[i][1])
    if n >= 4:
        edges[0] = (edges[0][0] or 5, None)            # infinity bases at the edges, beside the zero scalars
        edges[n - 1] = (5, None)
        edges[1] = (0, edges[1][1])
        edges[n - 2] = (0, edges[n - 2][1])
    return [("random n=%d" % n, rnd, 255),
            ("all equal n=%d" % n, [(ks[0], gs[0])] * n, 255),
            ("P / -P alternating n=%d" % n, [(ks[0], gs[0] if i % 2 == 0 else R - gs[0]) for i in range(n)], 255),
            ("edges n=%d" % n, edges, 255)]


def bits_cases(oracle, n=65):
    """Every scalar at 2^bits - 1 (at 255 bits the largest canonical scalar, r - 1: 2^255 - 1 is not below r)."""
    gs, _ = _pool(oracle)
    return [("bits=%d, scalars at the top" % b, [(min((1 << b) - 1, R - 1), gs[i]) for i in range(n)], b) for b in BITS]


def violation_cases(oracle, n=65):
    """A scalar of exactly 2^bits at the first, a middle and the last index.  bits = 255 has no such case: 2^255 is not
    a canonical scalar (r < 2^255), and canonical scalars are the call's precondition."""
    gs, ks = _pool(oracle)
    out = []
    for b in BITS[:-1]:
        assert 1 << b < R
        for where, at in (("first", 0), ("middle", n // 2), ("last", n - 1)):
            pairs = [(ks[i] & ((1 << b) - 1), gs[i]) for i in range(n)]
            pairs[at] = (1 << b, pairs[at][1])
            out.append(("bits=%d, 2^bits at the %s index" % (b, where), pairs, b))
    return out


def all_cases(oracle):
    """Every case the GPU tests compare against the model (the violations apart, which have no result)."""
    out = arm_cases(oracle) + bits_cases(oracle)
    for n in SIZES:
        out += size_cases(oracle, n)
    return out


def build(oracle, coracle, pairs, bits):
    """(points uint64[n, 12], scalars uint64[n, 4] Montgomery, expected uint64[18], arms) of a case without violation."""
    pts = np.array([gm.point_limbs(oracle, coracle, g) for _, g in pairs], dtype=np.uint64).reshape(-1, 12)
    sc = to_limbs(oracle, [k for k, _ in pairs])
    total, taken = fold(terms(pairs, bits))
    return pts, sc, expected_jac(oracle, coracle, total), taken


def arrays(oracle, coracle, pairs):
    """Points and scalars alone (a case with a violation has no model result)."""
    pts = np.array([gm.point_limbs(oracle, coracle, g) for _, g in pairs], dtype=np.uint64).reshape(-1, 12)
    return pts, to_limbs(oracle, [k for k, _ in pairs])


def expected_jac(oracle, coracle, total):
    """The 18 words of (total mod r) G: canonical (x, y, 1), or (1, 1, 0) for infinity."""
    if total % R == 0:
        return np.array(oracle.jac_to_mont_limbs(oracle.INF), dtype=np.uint64)
    aff = [int(v) for v in gm.point_limbs(oracle, coracle, total % R)]
    return np.array(aff + oracle.jac_to_mont_limbs(oracle.INF)[:6], dtype=np.uint64)


def bit_length_bound(ell):
    """The step count of the shuffle's permutation walk: bit_length(ell - 1), at least 1."""
    return max(1, (ell - 1).bit_length())
