"""Big-integer model of the constant-time fixed-base walk (csrc/fbase_ct_kernels.hip): k P as the sum over the 64
unsigned 4-bit digits d_v of k of the multiples d_v 2^(4 v) P, walked from window 0 upward, each multiple read from the
8-bit table of csrc/fbase_kernels.hip (entry w 255 + e - 1 = e 2^(8 w) P, e = 1..255) at

    index(v, d) = (v >> 1) 255 + (d << (4 (v & 1))) - 1.

Nothing of the library: digits and indices are Python integers, the expected points are fbase_model's (the C oracle).
The model asserts, on every case it emits, the exactness argument per 4-bit window (the accumulator never meets + or -
the addend) and that the chosen multiples sum to k: signed digits, a wider window or another subset mapping fail here
before they fail on the GPU."""
import fbase_model as fm
from fbase_model import R, expected_arrays, to_limbs  # noqa: F401  (what the GPU tests take from here)

WINDOWS, BITS = 64, 4
TABLE_WINDOWS, TABLE_DIGITS = 32, 255


def digits(k):
    """The 64 unsigned digits of a canonical scalar, window 0 first."""
    assert 0 <= k < R
    return [(k >> (BITS * v)) & 0xF for v in range(WINDOWS)]


def index(v, d):
    """Where d 2^(4 v) P lies in the 8-bit table."""
    assert 0 <= v < WINDOWS and 1 <= d <= 15
    return (v >> 1) * TABLE_DIGITS + (d << (4 * (v & 1))) - 1


def multiple_at(idx):
    """The multiple of P that table entry idx holds: e 2^(8 w) for idx = w 255 + e - 1."""
    assert 0 <= idx < TABLE_WINDOWS * TABLE_DIGITS
    w = idx // TABLE_DIGITS
    return (idx - TABLE_DIGITS * w + 1) << (8 * w)


def check_exact(k):
    """The exactness argument on scalar k, window by window, through the table's indices; returns the number of
    additions that count (non-zero digits)."""
    m, adds = 0, 0
    for v, d in enumerate(digits(k)):
        if d == 0:
            continue
        a = multiple_at(index(v, d))
        assert a == d << (BITS * v), (hex(k), v, d)
        assert m < (1 << (BITS * v)) <= a, hex(k)              # never + the addend
        assert m + a <= k < R and (m + a) % R != 0, hex(k)     # never - the addend
        m += a
        adds += 1
    assert m == k                                              # the chosen multiples sum to k
    return adds


def first_window(k):
    """The window of the first addition that counts, or None for k = 0."""
    return next((v for v, d in enumerate(digits(k)) if d), None)


# ---------------------------------------------------------------------------
# The case families.  Each is a list of (name, scalar).
# ---------------------------------------------------------------------------
def small_and_top():
    return [(str(k), k) for k in (0, 1, 2, 15, 16, 17, 255, 256)] + [("r-1", R - 1), ("r-2", R - 2)]


def single_digits():
    """d 2^(4 v) for d in {1, 8, 15} and every window; in window 63 only up to the top nibble of r - 1."""
    top = (R - 1) >> 252
    out = []
    for v in range(WINDOWS):
        for d in (1, 8, 15):
            if v == WINDOWS - 1 and d > top:
                continue
            out.append(("%d<<%d" % (d, 4 * v), d << (4 * v)))
    return out


def all_f():
    """2^(4 v) - 1: every lower digit 0xf."""
    return [("2^%d-1" % (4 * v), (1 << (4 * v)) - 1) for v in range(WINDOWS)]


def zero_runs():
    """2^(4 v) plus one low digit: a run of zero digits between two additions."""
    return [("2^%d+%d" % (4 * v, d), (1 << (4 * v)) + d) for v in range(1, WINDOWS) for d in (1, 9)]


def low_zero(oracle):
    """For every v a random scalar with its v low digits zero: the first addition lands in every window, odd ones
    included."""
    out = []
    for v, k in enumerate(fm._rand(oracle, 2101, WINDOWS)):
        x = (k >> (4 * v)) << (4 * v)
        if (x >> (4 * v)) & 0xF == 0:
            x |= 1 << (4 * v)
        assert x < R and first_window(x) == v
        out.append(("low %d zero" % v, x))
    return out


EVEN_MASK = sum(0xF << (8 * j) for j in range(32))          # the digits of the even windows


def half_zero(oracle):
    """Every even digit zero, every odd digit zero: each half of the subset mapping (e = d, e = 16 d) alone."""
    out = []
    for j, k in enumerate(fm._rand(oracle, 2102, 8)):
        out.append(("even digits zero %d" % j, (k & ~EVEN_MASK) % R))
        out.append(("odd digits zero %d" % j, k & EVEN_MASK))
    for name, k in out:
        ds = digits(k)
        assert not any(ds[0::2]) if name.startswith("even") else not any(ds[1::2]), name
    return out


def randoms(oracle, n=200, seed=2103):
    return [("random %d" % j, k) for j, k in enumerate(fm._rand(oracle, seed, n))]


def digit_families(oracle):
    fams = {"small_and_top": small_and_top(), "single_digits": single_digits(), "all_f": all_f(), "zero_runs": zero_runs(),
            "low_zero": low_zero(oracle), "half_zero": half_zero(oracle), "randoms": randoms(oracle)}
    for cases in fams.values():
        assert len(cases) < 1000
        for _, k in cases:
            check_exact(k)
    return fams


def multiplier_cases(oracle):
    """fbase_model.multiplier_cases: (name, s, m), the product s m mod r is what is walked; it includes 0, 1 and r - 1."""
    out = fm.multiplier_cases(oracle)
    for _, s, m in out:
        check_exact(fm.product(s, m))
    return out
