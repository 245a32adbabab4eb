"""tests/g1_mul_ct_model.py against the oracle, without a GPU: the walk's final multiple is k on every case of every
family (so k P is the oracle's scalar multiplication, which the point-level walk confirms on real points), the
exactness argument holds on every kept sum, and the one exceptional discarded sum -- k = r - 1, last step,
(r - 1) P + P -- is where the kernel's header says it is, so the GPU tests provably exercise it."""
import pytest

import g1_mul_ct_model as gm


@pytest.fixture(scope="module")
def families(oracle):
    return gm.scalar_families(oracle)


def test_the_families_are_what_the_issue_lists(families):
    assert {n for n, _ in families["special"]} == {"0", "1", "2", "3", "r-1", "r-2", "(r-1)/2", "(r+1)/2", "lambda", "r-lambda"}
    assert [k for _, k in families["single_bits"]] == [1 << j for j in range(255)]
    assert families["all_ones"][-1][1] == (1 << 254) - 1 and len(families["all_ones"]) == 254
    assert all(k % (1 << 128) == 0 and k for _, k in families["low_zero"])
    assert all(k < 1 << 128 for _, k in families["high_zero"])
    assert len(families["randoms"]) == 200
    assert (gm.LAMBDA * gm.LAMBDA + gm.LAMBDA + 1) % gm.R == 0


def test_every_case_walks_to_k_and_only_r_minus_1_discards_an_exceptional_sum(families):
    for fam, cases in families.items():
        for name, k in cases:
            m, steps, exceptional = gm.walk(k)                      # asserts the argument on every kept sum
            assert m == k and len(steps) == 255, name
            kinds = [kind for _, _, kind in steps]
            assert kinds.count(gm.FIRST) == (1 if k else 0), name
            assert kinds.count(gm.KEPT) == max(0, bin(k).count("1") - 1), name
            assert exceptional == ([(254, "P+(-P)")] if k == gm.R - 1 else []), name


def test_the_walk_on_real_points_is_the_oracles_scalar_multiplication(oracle, coracle, families):
    """The point-level walk: every special scalar on G and on a random point, a sample of every other family, and the
    top-x points (outside the subgroup: their order is a multiple of r, and the walk asserts its own exactness)."""
    g = dict(gm.subgroup_multiples(oracle))["random point 0"]
    pt = oracle.scalar_mul(g, oracle.G1)
    cases = [(k, p, gg) for _, k in families["special"] for p, gg in ((oracle.G1, 1), (pt, g))]
    for fam in ("single_bits", "all_ones", "randoms", "low_zero", "high_zero"):
        cases += [(k, pt, g) for _, k in families[fam][::37]]
    for k, p, gg in cases:
        got, exceptional = gm.walk_points(oracle, k, p)
        assert got == oracle.scalar_mul(k, p), hex(k)
        assert exceptional == gm.walk(k)[2], hex(k)
        want = gm.expected_limbs(oracle, coracle, k, gg)            # what the GPU tests compare with
        assert [int(v) for v in want] == (oracle.affine_to_mont_limbs(got) if got is not None else [0] * 12), hex(k)
    rm1 = gm.walk_points(oracle, gm.R - 1, pt)
    assert rm1 == (oracle.neg(pt), [(254, "P+(-P)")])               # the discarded sum is exactly P + (-P)
    assert gm.walk_points(oracle, 5, None) == (None, [])            # infinity stays infinity
    for p in gm.top_x_points(oracle):
        assert not oracle.scalar_mul(gm.R, p) is None               # not in the subgroup
        for k in (1, 2, gm.R - 1, families["randoms"][0][1]):
            got, _ = gm.walk_points(oracle, k, p)
            assert got == oracle.scalar_mul(k, p)


def test_pairs_and_arrays(oracle, coracle):
    pairs = gm.pairs_for(oracle, [0, 1, 2, 3, gm.R - 1] * 3)
    pts, sc, want = gm.arrays(oracle, coracle, pairs)
    assert pts.shape == (15, 12) and sc.shape == (15, 4) and want.shape == (15, 12)
    assert any(g is None for _, g in pairs)                         # an infinity point is among them
    assert not want[0].any() and (want[1] == pts[1]).all()          # 0 P = infinity, 1 P = P
    names = [n for n, _ in gm.subgroup_multiples(oracle)]
    assert names.index("-P 0") == names.index("P 0") + 1            # P beside -P
