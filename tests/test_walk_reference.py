"""The vectorised closed form of tests/walk_reference.py against the per-row sum with Python integers: odd sizes,
several seeds and block lengths (carries across blocks), slices that start inside the walk, and the largest words --
scalars near r - 1 and words of 2^255 - 1 and 2^256 - 1, whose pieces are all at their maximum."""
import numpy as np
import pytest

from walk_reference import mont_sums, walk_exponent, walk_expected


def _per_row(oracle, k, q, sc, start):
    s = [oracle.fr_from_mont_limbs([int(v) for v in row]) for row in sc]
    s0 = sum(s) % oracle.R
    s1 = sum((start + i) * v for i, v in enumerate(s)) % oracle.R
    return (k * s0 + q * s1) % oracle.R


def _words(vals):
    return np.array([[(v >> (64 * j)) & ((1 << 64) - 1) for j in range(4)] for v in vals], dtype=np.uint64)


@pytest.mark.parametrize("n,seed,block", [(1, 0, 1 << 20), (7, 1, 1 << 20), (1000, 2, 1 << 20), (4099, 3, 1024),
                                          (65537, 4, 1 << 16), (20001, 5, 3)])
def test_closed_form_matches_the_per_row_sum(oracle, n, seed, block):
    rng = np.random.default_rng(seed)
    k, q = oracle.Rand(seed + 10).get_frs(2)
    sc = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    sc[:, 3] &= np.uint64((1 << 62) - 1)
    for start in (0, 5, (1 << 26) + 3):
        assert walk_exponent(oracle, k, q, sc, start, block) == _per_row(oracle, k, q, sc, start), (start, block)


def test_closed_form_at_the_largest_words(oracle):
    R = oracle.R
    vals = [R - 1, R - 2, (1 << 255) - 1, (1 << 256) - 1, 0, 1] * 700 + [R - 1] * 3
    sc = _words(vals)
    k, q = oracle.Rand(3).get_frs(2)
    for block in (1 << 20, 1000, 1):
        assert walk_exponent(oracle, k, q, sc, 0, block) == _per_row(oracle, k, q, sc, 0), block
        assert walk_exponent(oracle, k, q, sc[5:], 5, block) == _per_row(oracle, k, q, sc[5:], 5), block
    # the two raw sums themselves, against Python integers
    m = [sum(int(w) << (64 * j) for j, w in enumerate(row)) for row in sc]
    assert mont_sums(sc, 999) == (sum(m), sum(i * v for i, v in enumerate(m)))
    # a block of 2^20 rows at the maximum: the largest partials the vectorised sums reach
    big = np.full((1 << 20, 4), np.uint64((1 << 64) - 1))
    n = 1 << 20
    top = (1 << 256) - 1
    assert mont_sums(big) == (n * top, n * (n - 1) // 2 * top)


def test_closed_form_point_matches_the_oracle_msm(oracle, coracle):
    """The whole point, not only the exponent: against the C oracle's Pippenger over the walk's own points."""
    rng = np.random.default_rng(9)
    k, q = oracle.Rand(1).get_frs(2)
    n, start = 300, 17
    pts = coracle.points_walk(k, q, start + n)[start:]
    sc = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    sc[:, 3] &= np.uint64((1 << 62) - 1)
    assert (walk_expected(oracle, coracle, k, q, sc, start) == coracle.msm_pippenger(np.ascontiguousarray(pts), sc, threads=4)).all()
