"""A big-integer model of the constant-time Fp inversion by division steps (go-curdleproofs_amd/csrc/invert_ds.h).

The model runs the batched algorithm EXACTLY as the header does -- Bernstein-Yang's original division step with delta
starting at 1, f = p, g = x; 37 batches of 30 steps walked on the low 30 bits of f and g; one 2 x 2 matrix (u, v; q, r)
per batch applied to the full-width f, g (an exact shift by 30) and to d, e (multiples of p chosen by p^-1 mod 2^30,
then an exact shift by 30) -- and ASSERTS at every batch what the header's limb code relies on:

- the divisions by 2^30 are exact,
- |u| + |v| <= 2^30 and |q| + |r| <= 2^30,
- |f| and |g| stay below 2^381,
- d and e lie in (-2p, p).

At the end it asserts g = 0 and f = +-1 (f = p for x = 0), and callers compare the result with pow(x, p - 2, p).  It
records the step at which g first became 0.  It also holds the two repackings (28 <-> 30 and 32 <-> 30 bit limbs), the
Montgomery product of fp28.h as an integer formula and the constants of the two entry forms, and gives the exact words
each entry form returns.  The case families below are the inputs of the CPU tests and of the GPU tests.
"""
import random

P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
BATCH = 30
BATCHES = 37
STEPS = BATCH * BATCHES  # 1,110
BOUND = (49 * 381 + 57) // 17  # the paper's bound for d = 381: 1,101
M30 = (1 << 30) - 1
PINV30 = pow(P, -1, 1 << 30)
R392 = 1 << 392
R384 = 1 << 384
NP392 = (-pow(P, -1, R392)) % R392
# y = mul28(t, K28): t = a^-1 2^-392 (the body's result on a 2^392) -> a^-1 2^392
K28 = pow(2, 3 * 392, P)
# y = canonical(mul28(t, KGNARK)): t = a^-1 2^-384 (the body's result on a 2^384) -> a^-1 2^384
KGNARK = pow(2, 2 * 384 + 392, P)


def divsteps30(delta, f0, g0):
    """30 division steps on the low 30 bits.  Returns (delta, (u, v, q, r)) with (u, v; q, r) (f, g)^T = 2^30 (f', g')^T."""
    u, v, q, r = 1, 0, 0, 1
    f, g = f0, g0
    for _ in range(BATCH):
        assert f & 1
        if delta > 0 and g & 1:
            delta, f, g, u, v, q, r = 1 - delta, g, g - f, q, r, q - u, r - v
        else:
            odd = g & 1
            delta, g, q, r = 1 + delta, g + odd * f, q + odd * u, r + odd * v
        # g <- g / 2 by doubling the first row instead of halving the second: the matrix stays integral
        assert g & 1 == 0
        g >>= 1
        u, v = 2 * u, 2 * v
    return delta, (u, v, q, r)


def first_zero_step(x):
    """The number of plain division steps after which g is 0, from (1, p, x)."""
    delta, f, g, n = 1, P, x, 0
    while g:
        if delta > 0 and g & 1:
            delta, f, g = 1 - delta, g, (g - f) // 2
        else:
            delta, g = 1 + delta, (g + (g & 1) * f) // 2
        n += 1
    return n


def update_de(d, e, t):
    u, v, q, r = t
    md = (u if d < 0 else 0) + (v if e < 0 else 0)
    me = (q if d < 0 else 0) + (r if e < 0 else 0)
    cd = u * (d & M30) + v * (e & M30)
    ce = q * (d & M30) + r * (e & M30)
    md -= (PINV30 * (cd & M30) + md) & M30
    me -= (PINV30 * (ce & M30) + me) & M30
    assert -(1 << 31) < md <= 1 << 30 and -(1 << 31) < me <= 1 << 30
    nd = u * d + v * e + P * md
    ne = q * d + r * e + P * me
    assert nd & M30 == 0 and ne & M30 == 0, "d, e: the division by 2^30 is not exact"
    return nd >> 30, ne >> 30


def invert_body(x, stats=None):
    """The header's body on a canonical x: returns (x^-1 mod p or 0, violation)."""
    assert 0 <= x < 1 << 390
    delta, f, g, d, e = 1, P, x, 0, 1
    canonical = x < P
    for b in range(BATCHES):
        delta, t = divsteps30(delta, f & M30, g & M30)
        u, v, q, r = t
        assert abs(u) + abs(v) <= 1 << 30 and abs(q) + abs(r) <= 1 << 30, "matrix bound"
        nf, ng = u * f + v * g, q * f + r * g
        assert nf & M30 == 0 and ng & M30 == 0, "f, g: the division by 2^30 is not exact"
        f, g = nf >> 30, ng >> 30
        d, e = update_de(d, e, t)
        if canonical:
            assert abs(f) < 1 << 381 and abs(g) < 1 << 381, "|f|, |g| < 2^381"
        assert -2 * P < d < P and -2 * P < e < P, "d, e in (-2p, p)"
    violation = int(g != 0)
    if canonical:
        assert g == 0 and (f in (1, -1) or (x == 0 and f == P)), (x, f, g)
    # sign(f) d into [0, p) by masks: add p if negative, negate under f < 0, add p if negative
    if d < 0:
        d += P
    if f < 0:
        d = -d
    if d < 0:
        d += P
    if canonical:
        assert 0 <= d < P
    return d % P if canonical else d, violation


# --------------------------------------------------------------------------------------------- limb forms ---
def limbs(v, width, n):
    assert 0 <= v < 1 << (width * n)
    return [(v >> (width * i)) & ((1 << width) - 1) for i in range(n)]


def value(ls, width):
    return sum(int(l) << (width * i) for i, l in enumerate(ls))


def repack(ls, w_from, w_to, n_to):
    """Limbs of width w_from -> limbs of width w_to holding the same integer (the header's shifts and masks)."""
    return limbs(value(ls, w_from), w_to, n_to)


def limbs28(v):
    """fp28.h's normalised form: limbs 0..12 below 2^28, limb 13 the rest."""
    assert 0 <= v < 1 << (28 * 13 + 32)
    return [(v >> (28 * i)) & 0x0FFFFFFF for i in range(13)] + [v >> (28 * 13)]


def mul28(a, b):
    """d28::mul as an integer formula: (a b + m p) / 2^392 with m = -a b / p mod 2^392; below 2p for a b < 2^392 p."""
    t = a * b
    m = (t * NP392) % R392
    r = (t + m * P) >> 392
    assert (t + m * P) % R392 == 0 and r < 2 * P
    return r


def invert_raw28(a):
    """invert_ds(F28&, const F28&): a normalised, below 2p, Montgomery radix 2^392.  Returns (y, violation), y below 2p
    with y = a^-1 2^784 mod p, i.e. the Montgomery form of the inverse; 0 and p give 0."""
    assert 0 <= a < 2 * P
    c = a - P if a >= P else a  # the masked canonical step
    l30 = repack(limbs28(c), 28, 30, 13)
    t, viol = invert_body(value(l30, 30))
    t28 = repack(limbs(t, 30, 13), 30, 28, 14)
    return mul28(value(t28, 28), K28), viol


def invert_gnark(a):
    """The gnark form: a canonical, 12 x u32, Montgomery radix 2^384.  Returns (y, violation), y canonical."""
    assert 0 <= a < 1 << 384
    l30 = repack(limbs(a, 32, 12), 32, 30, 13)
    t, viol = invert_body(value(l30, 30))
    if a >= P:
        return None, 1
    t28 = repack(limbs(t, 30, 13), 30, 28, 14)
    y = mul28(value(t28, 28), KGNARK)
    return (y - P if y >= P else y), viol


def want_gnark(a):
    """out = in^-1 for gnark elements: a = x 2^384 -> x^-1 2^384; 0 -> 0."""
    x = a * pow(R384, -1, P) % P
    return pow(x, P - 2, P) * R384 % P


def want_raw28(a):
    x = a * pow(R392, -1, P) % P
    return pow(x, P - 2, P) * R392 % P


# ------------------------------------------------------------------------------------------------- cases ---
EDGE_KS = (27, 28, 29, 30, 31, 59, 60, 61, 379, 380)


def fixed_cases():
    c = [0, 1, 2, P - 1, P - 2, (P + 1) // 2, (P - 1) // 2, R384 % P, R392 % P]
    for k in EDGE_KS:
        c += [1 << k, P - (1 << k)]
    return c


_LONGEST = None


def longest_cases():
    """The 64 values with the largest step counts out of 20,000 drawn from a fixed seed, with their counts."""
    global _LONGEST
    if _LONGEST is None:
        rng = random.Random(0xD1755)
        drawn = [rng.randrange(P) for _ in range(20000)]
        scored = sorted(((first_zero_step(x), x) for x in drawn), reverse=True)[:64]
        _LONGEST = [(x, n) for n, x in scored]
    return _LONGEST


def random_cases(n=1000):
    rng = random.Random(0x1EAF)
    return [rng.randrange(P) for _ in range(n)]


def all_cases():
    return fixed_cases() + [x for x, _ in longest_cases()] + random_cases()


RAW_EXTRA = (P, P + 1, 2 * P - 1)
