"""The big-integer model of the constant-time fixed-base walk (tests/fbase_ct_model.py): the subset mapping into the
8-bit table names the right multiple for all 960 (window, digit) pairs, the 64 digits recompose to the scalar, the case
families hold what they claim, and the exactness argument of csrc/fbase_ct_kernels.hip holds per 4-bit window on every
case (and is seen to fail where it must)."""
import pytest

import fbase_ct_model as cm4
import fbase_model as fm


@pytest.fixture(scope="module")
def families(oracle):
    return cm4.digit_families(oracle)


def test_the_subset_mapping_for_all_960_pairs():
    seen = set()
    for v in range(64):
        for d in range(1, 16):
            idx = cm4.index(v, d)
            assert 0 <= idx < 32 * 255
            w = idx // 255
            assert w == v >> 1                                              # the entry lies in the byte window of v
            assert ((idx - 255 * w + 1) << (8 * w)) == d << (4 * v) == cm4.multiple_at(idx), (v, d)
            seen.add(idx)
    assert len(seen) == 960                                                 # 960 different records
    assert cm4.index(0, 1) == 0 and cm4.index(1, 15) == 239 and cm4.index(63, 15) == 31 * 255 + 239
    assert max(seen) < fm.WINDOWS * 255 and 16 * 15 <= 255
    with pytest.raises(AssertionError):
        cm4.index(0, 0)                                                     # digit 0 names no entry


def test_constants_and_digits(oracle, families):
    assert cm4.R == oracle.R == fm.R and cm4.WINDOWS * cm4.BITS == 256 and cm4.R < 1 << 255
    for cases in families.values():
        for name, k in cases:
            d = cm4.digits(k)
            assert len(d) == 64 and all(0 <= x <= 15 for x in d), name
            assert sum(x << (4 * v) for v, x in enumerate(d)) == k, name
            assert cm4.check_exact(k) == sum(1 for x in d if x), name
            assert sum(cm4.multiple_at(cm4.index(v, x)) for v, x in enumerate(d) if x) == k, name
            assert [lo | (hi << 4) for lo, hi in zip(d[0::2], d[1::2])] == fm.digits(k), name    # two nibbles are the byte
    assert cm4.digits(cm4.R - 1)[63] == 7 and cm4.check_exact(cm4.R - 1) == 52       # r - 1: twelve zero nibbles, eight at its low end
    assert cm4.digits(cm4.R - 1)[:9] == [0] * 8 + [15]
    assert cm4.digits(0) == [0] * 64 and cm4.check_exact(0) == 0 and cm4.first_window(0) is None
    with pytest.raises(AssertionError):
        cm4.digits(cm4.R)                                    # not canonical: the argument does not cover it


def test_the_families_hold_what_they_claim(oracle, families):
    assert [k for _, k in families["small_and_top"]] == [0, 1, 2, 15, 16, 17, 255, 256, cm4.R - 1, cm4.R - 2]
    sd = dict(families["single_digits"])
    assert len(sd) == 63 * 3 + 1 and max(sd.values()) == 1 << 252 and (8 << 252) >= cm4.R
    assert all(cm4.check_exact(k) == 1 for k in sd.values())
    assert {cm4.first_window(k) for k in sd.values()} == set(range(64))
    ff = families["all_f"]
    assert len(ff) == 64 and ff[0][1] == 0
    assert all(cm4.digits(k)[:v] == [15] * v and not any(cm4.digits(k)[v:]) for v, (_, k) in enumerate(ff))
    zr = families["zero_runs"]
    assert len(zr) == 126
    for _, k in zr:
        d = cm4.digits(k)
        assert d[0] in (1, 9) and cm4.check_exact(k) == 2 and sum(1 for x in d if x == 0) == 62
    lz = families["low_zero"]
    assert [cm4.first_window(k) for _, k in lz] == list(range(64))      # the first addition lands in every window
    hz = families["half_zero"]
    assert len(hz) == 16
    for name, k in hz:
        d = cm4.digits(k)
        used = {cm4.index(v, x) % 255 + 1 for v, x in enumerate(d) if x}
        if name.startswith("even"):
            assert not any(d[0::2]) and any(d[1::2]) and all(e % 16 == 0 for e in used), name      # entries 16 d only
        else:
            assert not any(d[1::2]) and any(d[0::2]) and all(e < 16 for e in used), name           # entries d only
    rn = families["randoms"]
    assert len(rn) == 200 and len({k for _, k in rn}) == 200
    assert all(len(c) < 1000 for c in families.values())


def test_multiplier_cases(oracle):
    mc = cm4.multiplier_cases(oracle)
    prod = {name: fm.product(s, m) for name, s, m in mc}
    assert {0, 1, cm4.R - 1} <= set(prod.values()) and len(mc) == 30 and len(mc) < 1000
    assert mc == fm.multiplier_cases(oracle)


def test_the_exactness_check_fails_for_another_digit_scheme():
    """A signed recoding writes 15 as 16 - 1 and starts with the addend -P, which the bounds of the argument refuse: the
    check is not vacuous."""
    def signed_walk(k):
        m = 0
        for v, d in enumerate(cm4.digits(k)):
            a = d << (4 * v)
            if d > 8:
                a -= 1 << (4 * (v + 1))          # borrow: what a signed recoding adds instead
            if a:
                assert 0 <= m < (1 << (4 * v)) <= a and m + a <= k
                m += a
    with pytest.raises(AssertionError):
        signed_walk(15)
    signed_walk(7)
