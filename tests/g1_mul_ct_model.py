"""Big-integer model of the constant-time variable-base walk (csrc/g1_mul_ct_kernels.hip): k P by the 255 bits of k
MSB first, every step one doubling and ALWAYS one addition of P, the new accumulator by selection

    bit 0                      the doubled accumulator     (the sum is DISCARDED)
    bit 1, nothing added yet   P                           (FIRST)
    bit 1 otherwise            the sum                     (KEPT)

Nothing of the library: the walk is over Python integers (walk: the multiple m of P the accumulator holds) or over the
affine points of oracle/py (walk_points), the expected records come from the C oracle.

The model asserts the kernel's exactness argument on every kept sum -- the accumulator 2m P is neither P nor -P: for a
point of prime order r that is 2m != +-1 mod r, which 2m >= 2 and 2m + 1 <= k < r give -- and REPORTS the discarded
sums that are exceptional (P + P or P + (-P), which the kernel computes as nonsense inside its limb bounds and throws
away).  With 0 <= k < r there is exactly one: k = r - 1, last step, (r - 1) P + P."""
import numpy as np

import fbase_model as fm
from fbase_model import LAMBDA, R, to_limbs  # noqa: F401  (what the tests take from here)

STEPS = 255
IDLE, FIRST, KEPT, DISCARDED = "idle", "first", "kept", "discarded"


def bits_msb(k):
    assert 0 <= k < R < 1 << STEPS
    return [(k >> j) & 1 for j in range(STEPS - 1, -1, -1)]


def walk(k):
    """The walk on the multiple m of P.  Returns (m, steps, exceptional): steps[j] = (prefix m before the step's
    doubling, bit, kind); exceptional = [(step, "P+(-P)" | "P+P")] for the discarded sums that are exceptional."""
    m, started, steps, exceptional = 0, False, [], []
    for j, bit in enumerate(bits_msb(k)):
        before = m
        m *= 2                                             # the doubling: 2m P, never infinity for 0 < m (r is odd)
        assert not started or m % R != 0, hex(k)
        if bit and not started:
            kind, m, started = FIRST, 1, True
        elif bit:
            kind = KEPT
            assert m >= 2 and m % R != 1, hex(k)           # the addend is not the accumulator
            assert m + 1 <= k < R and (m + 1) % R != 0, hex(k)   # ... nor its negative
            m += 1
        elif started:
            kind = DISCARDED
            if (m + 1) % R == 0:
                exceptional.append((j, "P+(-P)"))
            elif m % R == 1:
                exceptional.append((j, "P+P"))
        else:
            kind = IDLE
        steps.append((before, bit, kind))
    assert m == k, hex(k)                                  # the prefix read so far, at the end all of k
    return m, steps, exceptional


def walk_points(oracle, k, pt):
    """The same walk over affine points (any curve point, None = infinity).  Asserts on every kept sum that the
    accumulator's x is not the addend's; returns (k pt, exceptional) with exceptional as in walk()."""
    acc, started, exceptional = None, False, []
    for j, bit in enumerate(bits_msb(k)):
        if started:
            acc = oracle.add(acc, acc)
            assert pt is None or acc is not None, (hex(k), j)
        if bit and not started:
            acc, started = pt, True
        elif bit:
            assert pt is None or acc[0] != pt[0], (hex(k), j)      # neither P nor -P: madd's main path is exact
            acc = oracle.add(acc, pt)
        elif started and pt is not None and acc[0] == pt[0]:
            exceptional.append((j, "P+P" if acc[1] == pt[1] else "P+(-P)"))
    return acc, exceptional


# ---------------------------------------------------------------------------
# The scalar families.  Each is a list of (name, scalar).
# ---------------------------------------------------------------------------
def special():
    return [("0", 0), ("1", 1), ("2", 2), ("3", 3), ("r-1", R - 1), ("r-2", R - 2), ("(r-1)/2", (R - 1) // 2),
            ("(r+1)/2", (R + 1) // 2), ("lambda", LAMBDA), ("r-lambda", R - LAMBDA)]


def single_bits():
    out = [("2^%d" % j, 1 << j) for j in range(STEPS) if 1 << j < R]
    assert len(out) == 255
    return out


def all_ones():
    """2^j - 1 up to 2^254 - 1: every lower bit set, an addition kept at every step behind the first."""
    return [("2^%d-1" % j, (1 << j) - 1) for j in range(1, STEPS)]


def randoms(oracle, n=200, seed=2401):
    return [("random %d" % j, k) for j, k in enumerate(fm._rand(oracle, seed, n))]


def low_zero(oracle, n=32):
    return [("low 128 zero %d" % j, (k >> 128) << 128) for j, k in enumerate(fm._rand(oracle, 2402, n))]


def high_zero(oracle, n=32):
    return [("high 128 zero %d" % j, k & ((1 << 128) - 1)) for j, k in enumerate(fm._rand(oracle, 2403, n))]


def scalar_families(oracle):
    fams = {"special": special(), "single_bits": single_bits(), "all_ones": all_ones(), "randoms": randoms(oracle),
            "low_zero": low_zero(oracle), "high_zero": high_zero(oracle)}
    for cases in fams.values():
        assert len(cases) <= 1000
        for _, k in cases:
            walk(k)
    return fams


# ---------------------------------------------------------------------------
# The points.  Subgroup points are (name, multiple of G) so that expected records come from one C call; None is
# infinity.  A point and its negative lie side by side.
# ---------------------------------------------------------------------------
def subgroup_multiples(oracle):
    """(name, g) with the point g G: the generator, random points, three of them beside their negatives."""
    rnd = fm._rand(oracle, 2404, 6)
    out = [("G", 1)] + [("random point %d" % j, g) for j, g in enumerate(rnd)]
    for j, g in enumerate(rnd[:3]):
        out += [("P %d" % j, g), ("-P %d" % j, R - g)]
    return out


def top_x_points(oracle, n=6):
    """Curve points whose x has the top bits of p (x just below p), the points of the compression and normalisation
    tests: (x, y) and (x, -y).  They are NOT in the prime-order subgroup -- their order is a multiple of r -- so the
    default chain (GLV) does not multiply them; the walk does, and walk_points asserts that on each use."""
    P = oracle.P
    out, x = [], P - 1
    while len(out) < n:
        rhs = (x * x * x + 4) % P
        y = pow(rhs, (P + 1) // 4, P)
        if y * y % P == rhs:
            out += [(x, y), (x, P - y)]
        x -= 1
    assert all(pt[0] >> 376 == P >> 376 and oracle.is_on_curve(pt) for pt in out)
    return out[:n]


_points = {}


def point_limbs(oracle, coracle, g):
    """The gnark G1Affine record of g G (g None: infinity, twelve zeros)."""
    if g is None or g % R == 0:
        return np.zeros(12, dtype=np.uint64)
    if g not in _points:
        _points[g] = np.array(coracle.scalar_mul_gen(g % R), dtype=np.uint64)
    return _points[g]


def expected_limbs(oracle, coracle, k, g):
    """The record of k (g G): the C oracle's (k g mod r) G."""
    walk(k)
    return point_limbs(oracle, coracle, None if g is None else k * g % R)


def pairs_for(oracle, scalars, with_infinity=True):
    """One point per scalar, cycling through the subgroup points (and infinity): [(k, g)]."""
    pool = [g for _, g in subgroup_multiples(oracle)] + ([None] if with_infinity else [])
    return [(k, pool[i % len(pool)]) for i, k in enumerate(scalars)]


def arrays(oracle, coracle, pairs):
    """(points uint64[n, 12], scalars uint64[n, 4] Montgomery, expected uint64[n, 12]) of [(k, g)]."""
    pts = np.array([point_limbs(oracle, coracle, g) for _, g in pairs], dtype=np.uint64).reshape(-1, 12)
    sc = to_limbs(oracle, [k for k, _ in pairs])
    want = np.array([expected_limbs(oracle, coracle, k, g) for k, g in pairs], dtype=np.uint64).reshape(-1, 12)
    return pts, sc, want
