"""The model of the batched constant-time MSM (tests/msm_ct_batch_model.py) against the oracle, without a GPU: the
segment rule is msm_ct_model's fold segment by segment, the split between the level launches and a segment's block
gives that fold's additions in that fold's order, the number of level launches for a list of counts, the model's point
per segment is the oracle's MSM on every case the GPU tests use, the case set takes every arm of add_ct AT A SEGMENT
EDGE -- pinned here with where -- and a fold that ran across a boundary would give a different point on the boundary
cases."""
import numpy as np
import pytest

import msm_ct_batch_model as bm
import msm_ct_model as mm


@pytest.fixture(scope="module")
def cases(oracle):
    return bm.all_cases(oracle)


def test_the_split_between_the_level_launches_and_the_block():
    assert [bm.tail_size(c) for c in (1, 2, 511, 512, 513, 1024, 1025, 2049, 65536)] == [1, 2, 511, 512, 257, 512, 257, 257, 512]
    assert [bm.size_at_level(1025, l) for l in range(4)] == [1025, 513, 257, 257]
    assert [bm.size_at_level(513, l) for l in range(3)] == [513, 257, 257]
    assert [bm.size_at_level(512, l) for l in range(3)] == [512, 512, 512]
    for c in (1, 3, 512, 513, 1024, 1025, 1027, 4097):
        assert bm.size_at_level(c, 20) == bm.tail_size(c)
        ts = [(7 * i + 3) % mm.R for i in range(c)]
        total, launched, block = bm.split(ts)
        want_total, want = mm.fold(ts)
        assert total == want_total and launched + block == want
        assert all(m > bm.TAIL for m, _, _ in launched) and all(m <= bm.TAIL for m, _, _ in block)
        # the launches of a segment alone: one per level above the tail
        assert bm.level_launches([c]) == len({m for m, _, _ in launched})
    assert bm.level_launches(bm.LEVEL_COUNTS) == 2 and bm.level_launches(bm.NO_LEVEL_COUNTS) == 0
    assert bm.level_launches(bm.MIXED_COUNTS) == 0 and bm.level_launches(bm.ROUND_COUNTS) == 0
    assert bm.level_launches([16] * bm.MAX_MSMS) == 0 and bm.level_launches([bm.MAX_PAIRS]) == 7
    assert bm.level_launches([]) == 0 and bm.level_launches([0, 0]) == 0
    assert bm.level_launches([513, 65536 - 513]) == 7                     # the widest segment decides


def test_the_case_set_is_the_one_the_issue_names(oracle, cases):
    by_name = {name: [len(s) for s in segs] for name, segs, _ in cases}
    assert [by_name["k=1 n=%d" % n] for n in bm.K1_SIZES] == [[1], [2], [3], [64], [65], [513]]
    assert by_name["mixed segments"] == [0, 1, 2, 3, 5, 0, 64, 65, 127, 0]
    offs = np.cumsum([bm.LEAD] + by_name["mixed segments"])
    assert all(int(o) % 64 for o in offs)                                  # no offset is a multiple of 64
    assert all(int(o - bm.LEAD) % 64 for o in offs[2:])                    # nor a begin behind the call's first pair
    assert by_name["level path [513, 3, 1025, 0, 512]"] == [513, 3, 1025, 0, 512]
    assert by_name["no level [512, 512]"] == [512, 512] and by_name["Prove's round shape"] == [129, 128, 129, 128]
    assert all(sum(c) <= bm.MAX_PAIRS and len(c) <= bm.MAX_MSMS for c in by_name.values())
    assert [(len(g), len(k)) for _, g, k, _ in bm.multi_cases(oracle)] == list(bm.MULTI_SHAPES)


def test_the_models_point_per_segment_is_the_oracles_msm(oracle, coracle, cases):
    inf = np.array(oracle.jac_to_mont_limbs(oracle.INF), dtype=np.uint64)
    multi = [(name, bm.multi_as_batch(gsets, ks), bits) for name, gsets, ks, bits in bm.multi_cases(oracle)]
    for name, segs, bits in cases + multi:
        pts, sc, offs = bm.arrays(oracle, coracle, segs)
        want = bm.expected(oracle, coracle, segs, bits)
        assert want.shape == (len(segs), 18) and int(offs[0]) == bm.LEAD, name
        for j in range(len(segs)):
            b, e = int(offs[j]), int(offs[j + 1])
            got = coracle.msm_pippenger(pts[b:e], sc[b:e], threads=4) if e > b else inf
            assert (got == want[j]).all(), (name, j)


def test_every_arm_of_add_ct_at_a_segment_edge_and_where(oracle, cases):
    by_name = {name: (segs, bits) for name, segs, bits in cases}
    assert set(bm.ARMS_AT_EDGES) == set(mm.ARMS)
    for arm, (name, j, m, i) in bm.ARMS_AT_EDGES.items():
        segs, bits = by_name[name]
        taken = mm.fold(mm.terms(segs[j], bits))[1]
        assert (m, i, arm) in taken and bm.is_edge(len(segs[j]), m, i), (arm, name)
    # all terms equal inside a segment: the balanced additions double, and each segment does so on its own
    segs, bits = by_name["all terms equal inside a segment"]
    assert [mm.fold(mm.terms(s, bits))[1] for s in segs] == [
        [(5, 0, "double"), (5, 1, "double"), (3, 0, "sum"), (2, 0, "sum")],
        [(4, 0, "double"), (4, 1, "double"), (2, 0, "double")],
        [(3, 0, "double"), (2, 0, "sum")]]
    # zeros and infinity bases at both edges, in a segment of scalars and in one of bases; the last segment is all infinity
    segs, bits = by_name["zero scalars and infinity bases at both edges"]
    folds = [mm.fold(mm.terms(s, bits))[1] for s in segs]
    assert folds[0][:2] == [(5, 0, "b"), (5, 1, "a")] and folds[1][:2] == [(5, 0, "b"), (5, 1, "a")]
    assert folds[2] == [(2, 0, "b")] and mm.fold(mm.terms(segs[2], bits))[0] == 0
    # [P] [-P]: no addition at all; [P, -P]: the segment is infinity
    segs, bits = by_name["[P] [-P]"]
    assert [mm.fold(mm.terms(s, bits))[1] for s in segs] == [[], []]
    segs, bits = by_name["[P, -P] [P, P]"]
    assert mm.fold(mm.terms(segs[0], bits))[0] == 0


def test_a_fold_across_a_boundary_gives_a_different_point(oracle):
    """The deliberately wrong model -- one fold over all the terms, result j read at term[begin_j] -- differs from the
    segment rule on every boundary case (and agrees with it where there is one segment: it is the same fold)."""
    for name, segs, bits in bm.boundary_cases(oracle) + [bm.mixed_case(oracle), bm.round_case(oracle)]:
        counts = [len(s) for s in segs]
        ts = mm.terms([p for s in segs for p in s], bits)
        right = [t for t, _ in bm.fold_segments(ts, counts)]
        wrong = bm.one_big_fold(ts, counts)
        assert wrong != right, name
    name, segs, bits = bm.boundary_cases(oracle)[0]                          # [P] [-P]: P + (-P) lands in result 0
    ts = mm.terms([p for s in segs for p in s], bits)
    assert bm.one_big_fold(ts, [1, 1])[0] == 0 and bm.fold_segments(ts, [1, 1])[0][0] != 0
    for name, segs, bits in bm.k1_cases(oracle):
        ts = mm.terms(segs[0], bits)
        assert bm.one_big_fold(ts, [len(ts)]) == [mm.fold(ts)[0]], name


def test_the_violation_cases(oracle):
    cases = bm.violation_cases(oracle)
    assert [b for _, _, b in cases] == [1, 9]
    for name, segs, bits in cases:
        bad = [(j, i) for j, s in enumerate(segs) for i, (k, _) in enumerate(s) if mm.violates(k, bits)]
        assert bad == [(len(segs) - 1, len(segs[-1]) - 1)] and segs[-1][-1][0] == 1 << bits, name
        assert all(k < mm.R for s in segs for k, _ in s), name
