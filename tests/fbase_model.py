"""Big-integer model of the fixed-base scalar multiplication (csrc/fbase_kernels.hip): k P as the sum over the 32
unsigned 8-bit digits d_w of k of the table entries d_w 2^(8 w) P, walked from window 0 upward.  Nothing of the library:
the digits are Python integers, the expected points come from the C oracle (coracle.scalar_mul_gen for the generator,
coracle.msm_naive over one pair for another base) and their bytes from oracle.compress.

The model asserts the kernel's exactness argument on every case it emits (check_exact): before window w the partial
sum is m P with m < 2^(8 w) <= d 2^(8 w) and m + d 2^(8 w) <= k < r, so the accumulator never meets + or - the next
addend and the only exceptional addition is the first one, into infinity.  A change of digit scheme (signed digits, wider
windows) fails here before it fails on the GPU."""
import numpy as np

WINDOWS, BITS = 32, 8
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
LAMBDA = 0xAC45A4010001A40200000000FFFFFFFF      # z^2 - 1: the GLV eigenvalue, lambda^2 + lambda + 1 = 0 mod r
OTHER_BASE = 7                                   # the second base of the GPU tests is 7 G


def digits(k):
    """The 32 unsigned digits of a canonical scalar, window 0 first."""
    assert 0 <= k < R
    return [(k >> (BITS * w)) & 0xFF for w in range(WINDOWS)]


def check_exact(k):
    """The exactness argument on scalar k; returns the number of additions (non-zero digits)."""
    m, adds = 0, 0
    for w, d in enumerate(digits(k)):
        if d == 0:
            continue
        a = d << (BITS * w)
        assert m < (1 << (BITS * w)) <= a, hex(k)              # never + the addend
        assert m + a <= k < R and (m + a) % R != 0, hex(k)     # never - the addend
        m += a
        adds += 1
    assert m == k
    return adds


def first_window(k):
    """The window of the first addition (into infinity), or None for k = 0."""
    return next((w for w, d in enumerate(digits(k)) if d), None)


def product(k, m=None):
    """The scalar the kernel multiplies by: k, or k m mod r."""
    return k % R if m is None else k * m % R


def expected_affine(oracle, coracle, k, base=None):
    """k * base (an integer multiple of G; None: G) as 12 Montgomery limbs, (0, 0) for infinity."""
    k %= R
    check_exact(k)
    if base is None:
        return np.array(coracle.scalar_mul_gen(k), dtype=np.uint64)
    pt = np.array([coracle.scalar_mul_gen(base)], dtype=np.uint64)
    sc = np.array([oracle.fr_to_mont_limbs(k)], dtype=np.uint64)
    jac = coracle.msm_naive(pt, sc)
    if not jac[12:].any():
        return np.zeros(12, dtype=np.uint64)
    return np.array(jac[:12], dtype=np.uint64)


_cache = {}


def expected(oracle, coracle, k, base=None):
    """(affine record uint64[12], compressed bytes) of k * base; computed once per (k, base)."""
    key = (k % R, base)
    if key not in _cache:
        aff = expected_affine(oracle, coracle, k, base)
        _cache[key] = (aff, oracle.compress(oracle.affine_from_mont_limbs([int(v) for v in aff])))
    return _cache[key]


def expected_arrays(oracle, coracle, ks, base=None):
    """(uint64[n, 12], uint8[n, 48]) for a list of scalars."""
    pairs = [expected(oracle, coracle, k, base) for k in ks]
    aff = np.array([a for a, _ in pairs], dtype=np.uint64).reshape(-1, 12)
    comp = np.frombuffer(b"".join(c for _, c in pairs), dtype=np.uint8).reshape(-1, 48)
    return aff, comp


def to_limbs(oracle, ks):
    """Scalars -> (n, 4) Montgomery fr limbs."""
    return np.array([oracle.fr_to_mont_limbs(k % R) for k in ks], dtype=np.uint64).reshape(-1, 4)


def _rand(oracle, seed, n):
    rand = oracle.Rand(seed)
    return [rand.get_fr() for _ in range(n)]


# ---------------------------------------------------------------------------
# The case families of the GPU tests.  Each is a list of (name, scalar).
# ---------------------------------------------------------------------------
def small_and_top():
    return [(str(k), k) for k in (0, 1, 2, 255, 256, 257)] + [("r-1", R - 1), ("r-2", R - 2)]


def single_digits():
    """d 2^(8 w) for d in {1, 128, 255} and every window; in window 31 only up to the top byte of r - 1."""
    top = (R - 1) >> 248
    out = []
    for w in range(WINDOWS):
        for d in (1, 128, 255):
            if w == 31 and d > top:
                continue
            out.append(("%d<<%d" % (d, 8 * w), d << (8 * w)))
    return out


def all_ff():
    """2^(8 w) - 1: every lower digit 0xff."""
    return [("2^%d-1" % (8 * w), (1 << (8 * w)) - 1) for w in range(1, WINDOWS)]


def zero_runs():
    """2^(8 w) plus one low digit: a run of zero digits between two additions."""
    return [("2^%d+%d" % (8 * w, d), (1 << (8 * w)) + d) for w in range(2, WINDOWS) for d in (1, 200)]


def low_zero(oracle):
    """For every w a random scalar with its w low digits zero: the first addition lands in every window."""
    out = []
    for w, k in enumerate(_rand(oracle, 1701, WINDOWS)):
        v = (k >> (8 * w)) << (8 * w)
        if (v >> (8 * w)) & 0xFF == 0:
            v |= 1 << (8 * w)
        out.append(("low %d zero" % w, v % R))
    return out


def randoms(oracle, n=200, seed=1702):
    return [("random %d" % j, k) for j, k in enumerate(_rand(oracle, seed, n))]


def digit_families(oracle):
    fams = {"small_and_top": small_and_top(), "single_digits": single_digits(), "all_ff": all_ff(), "zero_runs": zero_runs(),
            "low_zero": low_zero(oracle), "randoms": randoms(oracle)}
    for cases in fams.values():
        for _, k in cases:
            check_exact(k)
    return fams


def multiplier_cases(oracle):
    """(name, s, m): the product s m mod r is what is multiplied."""
    rnd = _rand(oracle, 1703, 44)
    a, b, c = rnd[:3]
    out = [("m=0", a, 0), ("m=1", a, 1), ("m=r-1", a, R - 1), ("s=0", 0, b), ("s=r-1", R - 1, b),
           ("s*m=0 both", 0, 0), ("s*m=1", c, pow(c, -1, R)), ("s*m=r-1", c, (R - pow(c, -1, R)) % R),
           ("(r-1)^2=1", R - 1, R - 1), ("lambda*lambda", LAMBDA, LAMBDA)]
    out += [("pair %d" % j, rnd[4 + 2 * j], rnd[5 + 2 * j]) for j in range(20)]
    for _, s, m in out:
        check_exact(product(s, m))
    return out


def whisk_scalars(oracle):
    """The k and r values of the Whisk tests, crossed by their users: named ones and a dozen random."""
    named = [("0", 0), ("1", 1), ("2", 2), ("r-1", R - 1), ("r-2", R - 2), ("lambda", LAMBDA), ("2^128", 1 << 128)]
    return named + [("random %d" % j, k) for j, k in enumerate(_rand(oracle, 1704, 12))]


def tracker_bytes(oracle, coracle, k, r):
    """computeTracker (whisk_test.go:98-104) and getKComm (:106-109): (96 bytes r G | k r G, 48 bytes k G)."""
    return (expected(oracle, coracle, r)[1] + expected(oracle, coracle, product(k, r))[1], expected(oracle, coracle, k)[1])
