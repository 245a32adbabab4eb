"""The model of the constant-time MSM (tests/msm_ct_model.py) against the oracle, without a GPU: for every case the
GPU tests use, the walk's exactness claim holds on every kept sum (asserted inside the model), the fold-in-half sum of
the terms is the oracle's MSM, the fold over multiples of G is the fold over the real points, and the case set takes
EVERY arm of add_ct -- pinned here with where."""
import pytest

import msm_ct_model as mm


@pytest.fixture(scope="module")
def cases(oracle):
    return mm.all_cases(oracle)


def test_every_case_agrees_with_the_oracles_msm(oracle, coracle, cases):
    assert len(cases) == 8 + len(mm.BITS) + 4 * len(mm.SIZES)
    for name, pairs, bits in cases:
        pts, sc, want, taken = mm.build(oracle, coracle, pairs, bits)
        assert len(pairs) <= mm.MAX_PAIRS and len(taken) == len(pairs) - 1, name   # m terms: m - 1 additions
        assert (coracle.msm_pippenger(pts, sc, threads=4) == want).all(), name


def test_the_fold_over_multiples_is_the_fold_over_the_points(oracle):
    """Small cases over the affine points of oracle/py: the same arms at the same places, the same point."""
    picked = mm.arm_cases(oracle) + mm.size_cases(oracle, 3) + mm.size_cases(oracle, 4) + \
        [(n, p[:9], b) for n, p, b in mm.size_cases(oracle, 63)]
    for name, pairs, bits in picked:
        total, taken = mm.fold(mm.terms(pairs, bits))
        pts = [None if g is None or k == 0 else oracle.scalar_mul(k * g % mm.R, oracle.G1) for k, g in pairs]
        point, taken_points = mm.fold_points(oracle, pts)
        assert taken_points == taken, name
        assert point == (None if total == 0 else oracle.scalar_mul(total, oracle.G1)), name


def test_the_walk_at_a_public_step_count(oracle):
    """k < 2^bits walks to k; the steps the shift drops are idle; r - 1 at 255 bits discards P + (-P) in its last step."""
    for bits in mm.BITS:
        top = min((1 << bits) - 1, mm.R - 1)
        for k in (0, 1, top, top >> 1, 1 << (bits - 1)):
            assert mm.walk(k, bits)[0] == k
        assert mm.violates(1 << bits, bits) and not mm.violates(top, bits)
    assert mm.walk(mm.R - 1, 255)[1] == [(254, "P+(-P)")]
    with pytest.raises(AssertionError):
        mm.walk(1 << 9, 9)
    assert [mm.bit_length_bound(e) for e in (1, 2, 3, 4, 60, 124, 252, 508, 512, 513, 4096)] == [1, 1, 2, 2, 6, 7, 8, 9, 9, 10, 12]


def test_the_case_set_takes_every_arm_and_where(oracle, cases):
    by_name = {name: mm.fold(mm.terms(pairs, bits))[1] for name, pairs, bits in cases}
    # the arms in isolation
    assert by_name["(P, P), equal scalars"] == [(2, 0, "double")]
    assert by_name["(P, -P)"] == [(2, 0, "infinity")]
    assert by_name["scalar 0 first"] == [(2, 0, "b")] and by_name["base infinity first"] == [(2, 0, "b")]
    assert by_name["scalar 0 second"] == [(2, 0, "a")] and by_name["base infinity second"] == [(2, 0, "a")]
    assert by_name["both scalars 0"] == [(2, 0, "b")]                      # a_inf comes first
    assert by_name["two different points"] == [(2, 0, "sum")]
    seen = set()
    for n in mm.SIZES:
        # random terms: general sums only
        assert {a for _, _, a in by_name["random n=%d" % n]} <= {"sum"}
        # all terms equal: term i of a level holds c_i copies, and the addition is the double iff c_i == c_(i + h)
        counts, want, m = [1] * n, [], n
        while m > 1:
            h = (m + 1) // 2
            for i in range(m - h):
                want.append((m, i, "double" if counts[i] == counts[i + h] else "sum"))
                counts[i] += counts[i + h]
            m = h
        assert by_name["all equal n=%d" % n] == want
        if n >= 4:
            assert {"double", "sum"} <= {a for _, _, a in want} or (n & (n - 1)) == 0   # a power of two only doubles
        # P / -P alternating: signed counts; a level adds c_i and c_(i + h)
        signed, want, m = [1 if i % 2 == 0 else -1 for i in range(n)], [], n
        while m > 1:
            h = (m + 1) // 2
            for i in range(m - h):
                a, b = signed[i], signed[i + h]
                want.append((m, i, "b" if a == 0 else "a" if b == 0 else "double" if a == b else "infinity" if a == -b else "sum"))
                signed[i] += signed[i + h]
            m = h
        assert by_name["P / -P alternating n=%d" % n] == want
        for fam in ("random", "all equal", "P / -P alternating", "edges"):
            seen |= {a for _, _, a in by_name["%s n=%d" % (fam, n)]}
    assert seen == set(mm.ARMS)
    # whole subtrees at infinity: at n = 63 and 64 (h = 32 is even: i and i + h have the same sign) the first level
    # doubles, at n = 65 (h = 33) every pair is P + (-P) and the next level adds infinities
    assert {a for m, _, a in by_name["P / -P alternating n=64"] if m == 64} == {"double"}
    assert {a for m, _, a in by_name["P / -P alternating n=65"] if m == 65} == {"infinity"}
    assert {a for m, _, a in by_name["P / -P alternating n=65"] if m == 33} <= {"b", "a"}
    assert {a for m, _, a in by_name["P / -P alternating n=63"] if m == 63} == {"double"}
    # the edges family meets infinity operands on both sides
    assert {"a", "b"} <= {a for n in mm.SIZES if n >= 63 for _, _, a in by_name["edges n=%d" % n]}


def test_the_violation_cases(oracle):
    cases = mm.violation_cases(oracle)
    assert len(cases) == 3 * (len(mm.BITS) - 1)
    for name, pairs, bits in cases:
        bad = [i for i, (k, _) in enumerate(pairs) if mm.violates(k, bits)]
        assert len(bad) == 1 and pairs[bad[0]][0] == 1 << bits and all(k < mm.R for k, _ in pairs), name
    assert {b[0] for b in ([i for i, (k, _) in enumerate(p) if mm.violates(k, bits)] for _, p, bits in cases)} == {0, 32, 64}
