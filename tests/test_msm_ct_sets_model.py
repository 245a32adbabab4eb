"""The model of the constant-time MSM over several resident sets (tests/msm_ct_sets_model.py) against itself, against
the single-set model and against the C oracle's MSM: the global-row to (set, local row) rule with empty sets anywhere,
the result over sets equal to the result over the concatenated single set on every case the GPU test uses, and every
arm of add_ct with the SAME point resident in two different sets.  No GPU."""
import pytest

import msm_ct_bases_model as cb
import msm_ct_model as mm
import msm_ct_sets_model as sm
from msm_ct_model import R


def test_the_row_rule_with_empty_sets_anywhere():
    shapes = list(sm.SET_SIZES) + [(5,), (0, 5), (5, 0), (0, 0, 5), (5, 0, 0, 0), (0, 0, 0, 5), (2, 0, 0, 3), (0, 1, 0, 0),
                                   (1, 1, 1, 1), (3, 0, 4), sm.BATCH_SIZES]
    for sizes in shapes:
        b = sm.firsts(sizes)
        assert b[0] == 0 and b[-1] == sum(sizes) and len(b) == len(sizes) + 1
        want = [(s, i) for s, n in enumerate(sizes) for i in range(n)]      # the concatenation, record by record
        assert [sm.locate(r, sizes) for r in range(b[-1])] == want
        for r in (-1, b[-1], b[-1] + 1):
            with pytest.raises(AssertionError):
                sm.locate(r, sizes)
        gs = list(range(100, 100 + b[-1]))
        parts = sm.split(gs, sizes)
        assert [len(p) for p in parts] == list(sizes) and sum(parts, []) == gs
        assert [g for _, g in sm.pairs_over_sets(gs, sizes, range(b[-1]), [1] * b[-1])] == gs
    for bad in ((), (1, 1, 1, 1, 1)):
        with pytest.raises(AssertionError):
            sm.firsts(bad)


def test_the_row_lists_touch_every_set_at_both_ends(oracle):
    for sizes in sm.SET_SIZES:
        cases = {c[0].split(" ")[0]: c for c in sm.row_cases(oracle, sizes)}
        assert set(cases) == {"edges", "reversed", "repeated", "alternating"}
        b = sm.firsts(sizes)
        full = [s for s, n in enumerate(sizes) if n]
        assert set(cases["edges"][3]) == {r for s in full for r in (b[s], b[s + 1] - 1)}
        assert cases["reversed"][3] == list(range(b[-1] - 1, -1, -1))
        alt = [sm.locate(r, sizes)[0] for r in cases["alternating"][3]]
        assert alt[:len(full)] == full and all(alt[p] == full[p % len(full)] for p in range(len(alt)))
        if b[-1] >= 4:
            gs = cases["reversed"][2]
            assert gs[0] is None and gs[-1] is None and gs[b[-1] // 2] is None      # infinity records are read
        for case in cases.values():
            assert sum(case[5]) == len(case[3]) == len(case[4]) and case[5][1] == 0


@pytest.mark.parametrize("c", cb.CHUNK_BITS)
def test_every_arm_with_one_point_resident_in_two_sets(oracle, c):
    cases = {case[0]: case for case in sm.arm_cases(oracle, c)}
    took = set()
    for arm, (name, m, i) in sm.arms(c).items():
        _, sizes, gs, rows, ks, counts, bits = cases[name]
        (total, taken), = sm.fold_sets(gs, sizes, rows, ks, counts, c, bits, walk=True)
        assert (m, i, arm) in taken, (arm, name, [t for t in taken if t[:2] == (m, i)])
        took |= {a for _, _, a in taken}
    assert took == set(mm.ARMS)
    # the two pairs of the exceptional cases read DIFFERENT sets and the same point
    for name in ("one point in two sets, equal scalars", "one point in two sets, opposite scalars"):
        _, sizes, gs, rows, ks, counts, bits = cases[name]
        where = [sm.locate(r, sizes) for r in rows]
        assert {s for s, _ in where} == {0, 1}
        pairs = sm.pairs_over_sets(gs, sizes, rows, ks)
        assert pairs[0][1] == pairs[1][1] is not None
    n = cb.chunks(255, c)
    _, sizes, gs, rows, ks, counts, bits = cases["one point in two sets, equal scalars"]
    (total, taken), = sm.fold_sets(gs, sizes, rows, ks, counts, c, bits)
    k = ks[0]
    assert total == 2 * k * gs[0] % R
    # "double" at the first level, chunk by chunk, wherever the digit is not zero
    assert [a for m, _, a in taken if m == 2 * n] == ["double" if (k >> (c * j)) & ((1 << c) - 1) else "b" for j in range(n)]
    _, sizes, gs, rows, ks, counts, bits = cases["one point in two sets, opposite scalars"]
    (total, taken), = sm.fold_sets(gs, sizes, rows, ks, counts, c, bits)
    assert total == 0 and [a for m, _, a in taken if m == 2] == ["infinity"]


def test_the_model_over_sets_agrees_with_the_single_set_and_the_oracles_msm_on_every_gpu_case(oracle, coracle):
    done = {}
    seen = 0
    for c, case in sm.all_cases(oracle):
        name, sizes, gs, rows, ks, counts, bits = case
        want = sm.expected(oracle, coracle, case, c)                 # fold_sets asserts the concatenated single set inside
        key = (name, bits, tuple(ks))
        if key not in done:                                           # the row cases are the same pairs for every chunk width
            pairs = sm.pairs_over_sets(gs, sizes, rows, ks)
            pts = cb.set_limbs(oracle, coracle, [g for _, g in pairs])
            sc = mm.to_limbs(oracle, ks)
            offs = sm.offsets_of(counts).astype(int)
            done[key] = [coracle.msm_pippenger(pts[a:b], sc[a:b], threads=4) for a, b in zip(offs[:-1], offs[1:])]
        for j, got in enumerate(done[key]):
            assert (want[j] == got).all(), (c, name, j)
        seen += 1
    assert len(done) >= 30 and seen >= 60
    for case in sm.bits_cases(oracle):
        if case[6] < 255:
            bad = sm.violation_case(case)
            assert mm.violates(bad[4][-1], bad[6]) and not any(mm.violates(k, bad[6]) for k in bad[4][:-1])
