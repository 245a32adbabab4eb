"""The big-integer model of the fixed-base multiplication (tests/fbase_model.py) against itself and the oracles: the
digits recompose to the scalar, the expected points are the oracle's, the case families hold what they claim, and the
exactness argument of csrc/fbase_kernels.hip holds on every case (and is seen to fail where it must)."""
import pytest

import fbase_model as fm


@pytest.fixture(scope="module")
def families(oracle):
    return fm.digit_families(oracle)


def test_constants_and_digits(oracle, families):
    assert fm.R == oracle.R and (fm.LAMBDA * fm.LAMBDA + fm.LAMBDA + 1) % fm.R == 0
    assert fm.WINDOWS * fm.BITS == 256 and fm.R < 1 << 255
    for cases in families.values():
        for name, k in cases:
            d = fm.digits(k)
            assert len(d) == 32 and all(0 <= x <= 255 for x in d), name
            assert sum(x << (8 * w) for w, x in enumerate(d)) == k, name
            assert fm.check_exact(k) == sum(1 for x in d if x), name
    assert fm.digits(fm.R - 1)[31] == 0x73 and fm.check_exact(fm.R - 1) == 28   # r - 1 ends in four zero digits
    assert fm.digits(0) == [0] * 32 and fm.check_exact(0) == 0 and fm.first_window(0) is None
    with pytest.raises(AssertionError):
        fm.digits(fm.R)                                  # not canonical: the argument does not cover it


def test_the_families_hold_what_they_claim(oracle, families):
    assert [k for _, k in families["small_and_top"]] == [0, 1, 2, 255, 256, 257, fm.R - 1, fm.R - 2]
    sd = dict(families["single_digits"])
    assert len(sd) == 31 * 3 + 1 and max(sd.values()) == 1 << 248 and (128 << 248) >= fm.R
    assert all(fm.check_exact(k) == 1 for k in sd.values())
    assert {fm.first_window(k) for k in sd.values()} == set(range(32))
    ff = families["all_ff"]
    assert len(ff) == 31 and all(fm.digits(k)[:w + 1] == [255] * (w + 1) and not any(fm.digits(k)[w + 1:]) for w, (_, k) in enumerate(ff))
    zr = families["zero_runs"]
    assert len(zr) == 60
    for _, k in zr:
        d = fm.digits(k)
        assert fm.check_exact(k) == 2 and d[0] in (1, 200) and d[1] == 0
    lz = families["low_zero"]
    assert [fm.first_window(k) for _, k in lz] == list(range(32))       # the first addition lands in every window
    rn = families["randoms"]
    assert len(rn) == 200 and len({k for _, k in rn}) == 200
    assert sum(fm.first_window(k) == 0 for _, k in rn) >= 195
    total = sum(len(c) for c in families.values())
    assert 400 <= total <= 500 and all(len(c) < 1000 for c in families.values())


def test_multiplier_and_whisk_cases(oracle):
    mc = fm.multiplier_cases(oracle)
    prod = {name: fm.product(s, m) for name, s, m in mc}
    assert prod["m=0"] == prod["s=0"] == prod["s*m=0 both"] == 0
    assert prod["s*m=1"] == prod["(r-1)^2=1"] == 1 and prod["s*m=r-1"] == fm.R - 1
    assert prod["lambda*lambda"] == fm.R - fm.LAMBDA - 1
    assert {m for _, _, m in mc} >= {0, 1, fm.R - 1} and len(mc) == 30
    ws = fm.whisk_scalars(oracle)
    assert len(ws) == 19 and {k for _, k in ws} >= {0, 1, 2, fm.R - 1, fm.R - 2, fm.LAMBDA, 1 << 128}


def test_expected_points_are_the_oracles(oracle, coracle):
    inf = bytes([0xC0]) + bytes(47)
    aff, comp = fm.expected(oracle, coracle, 0)
    assert not aff.any() and comp == inf
    aff, comp = fm.expected(oracle, coracle, 1)
    assert [int(v) for v in aff] == oracle.affine_to_mont_limbs(oracle.G1) and comp == oracle.compress(oracle.G1)
    for k in (2, 255, 256, fm.R - 1, fm.LAMBDA):
        pt = oracle.scalar_mul(k, oracle.G1)
        for base, want in ((None, pt), (fm.OTHER_BASE, oracle.scalar_mul(fm.OTHER_BASE, pt))):
            aff, comp = fm.expected(oracle, coracle, k, base)
            assert [int(v) for v in aff] == oracle.affine_to_mont_limbs(want), (k, base)
            assert comp == oracle.compress(want), (k, base)
    assert fm.expected(oracle, coracle, fm.R - 1)[1] == oracle.compress(oracle.neg(oracle.G1))
    assert not fm.expected(oracle, coracle, 0, fm.OTHER_BASE)[0].any()
    a, c = fm.expected_arrays(oracle, coracle, [0, 1, 2])
    assert a.shape == (3, 12) and c.shape == (3, 48) and bytes(c[0]) == inf
    t, kc = fm.tracker_bytes(oracle, coracle, 5, 3)
    assert t == oracle.compress(oracle.scalar_mul(3, oracle.G1)) + oracle.compress(oracle.scalar_mul(15, oracle.G1))
    assert kc == oracle.compress(oracle.scalar_mul(5, oracle.G1))


def test_the_exactness_check_fails_for_another_digit_scheme():
    """A signed recoding writes 255 as 256 - 1 and starts with the addend -P, which the bounds of the argument refuse:
    the check is not vacuous."""
    def signed_walk(k):
        m = 0
        for w, d in enumerate(fm.digits(k)):
            a = d << (8 * w)
            if d > 128:
                a -= 1 << (8 * (w + 1))          # borrow: what a signed recoding adds instead
            if a:
                assert 0 <= m < (1 << (8 * w)) <= a and m + a <= k
                m += a
    with pytest.raises(AssertionError):
        signed_walk(255)
    signed_walk(127)
