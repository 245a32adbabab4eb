"""The model of the chunked constant-time MSM (tests/msm_ct_bases_model.py) against itself, against the bit-serial walk
of tests/g1_mul_ct_model.py, against the affine points of oracle/py and against the C oracle's MSM: the digit split for
every chunk width and every scalar_bits, the table rows, the per-lane walk with the exactness claim on every kept AND
every discarded sum, the term order p Cb + j, the fold with the arm every addition takes, and the oracle's MSM on every
case the GPU tests use.  No GPU."""
import numpy as np
import pytest

import g1_mul_ct_model as gm
import msm_ct_bases_model as cb
import msm_ct_model as mm
from msm_ct_model import R


def _register_walk(k, c, bits, j):
    """The kernel's scalar register: eight words shifted left one bit a step, every bit read at the top.  Returns
    (violation, digit read over the chunk's steps)."""
    reg, over = k, 0
    for _ in range(bits, 256):
        over |= (reg >> 255) & 1
        reg = (reg << 1) & ((1 << 256) - 1)
    for _ in range(cb.skipped(j, c, bits)):
        reg = (reg << 1) & ((1 << 256) - 1)
    d = 0
    for _ in range(cb.steps(j, c, bits)):
        d = 2 * d + ((reg >> 255) & 1)
        reg = (reg << 1) & ((1 << 256) - 1)
    return over, d


@pytest.mark.parametrize("c", cb.CHUNK_BITS)
def test_the_digit_split_for_every_scalar_bits(oracle, c):
    rnd = gm.fm._rand(oracle, 3102, 4)
    for bits in range(1, 256):
        n = cb.chunks(bits, c)
        assert c * (n - 1) < bits <= c * n
        assert sum(cb.steps(j, c, bits) for j in range(n)) == bits
        assert all(cb.steps(j, c, bits) == c for j in range(n - 1)) and 1 <= cb.steps(n - 1, c, bits) <= c
        top = min((1 << bits) - 1, R - 1)
        for k in [0, 1, top, 1 << (bits - 1)] + [v & ((1 << bits) - 1) for v in rnd[:2]]:
            if k >= R:
                continue
            ds = cb.digits(k, c, bits)
            assert len(ds) == n
            for j in (0, n // 2, n - 1):
                assert _register_walk(k, c, bits, j) == (0, ds[j]), (bits, j, hex(k))
        # a scalar at or above 2^bits is the violation, in every chunk's lane
        if bits < 255 and 1 << bits < R:
            for j in (0, n - 1):
                assert _register_walk(1 << bits, c, bits, j)[0] == 1
                assert _register_walk((1 << bits) | 5, c, bits, j)[0] == 1
    assert cb.chunks(255, c) == {8: 32, 16: 16, 32: 8, 64: 4}[c]


@pytest.mark.parametrize("c", cb.CHUNK_BITS)
def test_the_table_rows(oracle, coracle, c):
    """Row j is 2^(c j) P: by c doublings of the affine point between rows, by the C oracle's multiple, and with
    infinity staying the zero record."""
    base = cb.Bases(oracle, 5, (0, 2, 4))
    rows = [base.limbs(coracle, c, j) for j in range(cb.chunks(255, c))]
    assert (rows[0] == cb.set_limbs(oracle, coracle, base.g)).all()
    for i, g in enumerate(base.g):
        mult = cb.table_multiples(g, c)
        assert len(mult) == len(rows)
        for j, m in enumerate(mult):
            assert (rows[j][i] == gm.point_limbs(oracle, coracle, m)).all(), (i, j)
            assert m is None or m % R != 0                       # 2 is invertible mod r: never infinity
    # the doublings themselves, over the affine points of oracle/py
    pt = oracle.affine_from_mont_limbs([int(v) for v in rows[0][1]])
    for j in (1, 2):
        for _ in range(c):
            pt = oracle.add(pt, pt)
        assert pt == oracle.affine_from_mont_limbs([int(v) for v in rows[j][1]])


def test_no_sum_of_a_chunk_walk_is_exceptional(oracle):
    """Every digit of every case scalar, and the digits at the bounds, through walk_chunk (which asserts on kept and
    discarded sums alike) and through the 255-step model, which must report no exceptional discarded sum for them --
    while it does for k = r - 1 walked whole."""
    assert gm.walk(R - 1)[2] == [(254, "P+(-P)")]
    seen = set()
    for c in cb.CHUNK_BITS:
        for s in (1, c - 1, c):
            seen |= {(d, s) for d in (0, 1, (1 << s) - 1, 1 << (s - 1), (1 << s) - 2) if 0 <= d < 1 << s}
        for case in cb.arm_cases(oracle, c) + cb.bits_cases(oracle, c) + cb.size_cases(oracle, 65):
            for k in case[3]:
                seen |= {(d, cb.steps(j, c, case[4])) for j, d in enumerate(cb.digits(k, c, case[4]))}
    assert len(seen) > 1000
    for n, (d, s) in enumerate(sorted(seen)):
        m, sums = cb.walk_chunk(d, s)
        assert m == d and sums == max(0, d.bit_length() - 1)
        if n % 7 == 0:                                            # the bit-serial model agrees: nothing exceptional
            m255, st, exceptional = gm.walk(d)
            assert m255 == d and exceptional == []
            assert sum(1 for _, _, kind in st if kind in (gm.KEPT, gm.DISCARDED)) == sums


@pytest.mark.parametrize("c", cb.CHUNK_BITS)
def test_the_term_order_and_the_arms_between_chunk_terms(oracle, c):
    cases = {case[0]: case for case in cb.arm_cases(oracle, c)}
    # term[p Cb + j] = d_j 2^(c j) g_rows[p]
    case = cases["the same row twice, opposite scalars"]
    pairs = cb.pairs_of(case)
    n = cb.chunks(255, c)
    ts = cb.terms(pairs, c, 255)
    assert len(ts) == 2 * n
    for p, (k, g) in enumerate(pairs):
        for j in range(n):
            assert ts[p * n + j] == ((k >> (c * j)) & ((1 << c) - 1)) * pow(2, c * j, R) * g % R
    # one pair alone: sum, a and b only (asserted inside), whatever the digits
    for case in cases.values():
        if len(case[3]) == 1:
            total, taken = cb.fold_one_pair(case[3][0], case[1][0], c, case[4])
            assert len(taken) == cb.chunks(case[4], c) - 1
    # every arm, where the table says
    took = set()
    for arm, (name, m, i) in cb.arms(c).items():
        pairs = cb.pairs_of(cases[name])
        total, taken = cb.fold_call(pairs, [len(pairs)], c, cases[name][4])[0]
        assert (m, i, arm) in taken, (arm, name, [t for t in taken if t[:2] == (m, i)])
        took |= {a for _, _, a in taken}
    assert took == set(mm.ARMS)
    # P and -P on two rows: every chunk's pair of terms is opposite at the first level
    pairs = cb.pairs_of(cases["two rows, P and -P, equal scalars"])
    total, taken = cb.fold_call(pairs, [2], c, 255)[0]
    k = pairs[0][0]
    assert total == 0
    assert [a for m, _, a in taken if m == 2 * n] == ["infinity" if (k >> (c * j)) & ((1 << c) - 1) else "b" for j in range(n)]


def test_the_segments_of_a_batch_and_the_level_rule(oracle):
    """MSM s owns [offsets[s] Cb, offsets[s + 1] Cb); the level launches are msm_ct_batch_model's on count Cb."""
    for counts in (cb.MIXED_COUNTS, cb.LEVEL_COUNTS):
        base, rows, sc, offs = cb.batch_case(oracle, counts)
        pairs = [(k, base.g[r]) for k, r in zip(sc, rows)]
        for c in (16, 64):
            got = cb.fold_call(pairs, counts, c, 255, walk=False)
            at = 0
            for n, (total, taken) in zip(counts, got):
                assert total == sum(k * g for k, g in pairs[at:at + n] if g is not None) % R
                assert len(taken) == max(0, n * cb.chunks(255, c) - 1)
                at += n
    assert cb.level_launches(cb.LEVEL_COUNTS, 16, 255) == 6      # 1025 x 16 = 16,400 terms: six halvings to 512 or below
    assert cb.level_launches(cb.LEVEL_COUNTS, 64, 255) == 4      # 1025 x 4
    assert cb.level_launches(cb.MIXED_COUNTS, 16, 255) == 2      # 127 x 16 = 2,032
    assert cb.level_launches((1, 2), 16, 9) == 0


def test_the_model_agrees_with_the_oracles_msm_on_every_gpu_case(oracle, coracle):
    done = {}
    for c, case in cb.all_cases(oracle):
        name, gs, rows, ks, bits = case
        pairs = cb.pairs_of(case)
        walk = len(pairs) <= 65 or name.startswith("random")
        want = mm.expected_jac(oracle, coracle, cb.total_of(case, c, walk))
        key = (name, bits, tuple(ks))                             # the size cases are the same pairs for every c
        if key not in done:
            pts = cb.set_limbs(oracle, coracle, [g for _, g in pairs])
            done[key] = coracle.msm_pippenger(pts, mm.to_limbs(oracle, [k for k, _ in pairs]), threads=4)
        assert (want == done[key]).all(), (c, name)
    for c in cb.CHUNK_BITS:
        for case in cb.violation_cases(oracle, c):
            assert mm.violates(case[3][-1], case[4]) and not any(mm.violates(k, case[4]) for k in case[3][:-1])
    assert len(done) >= 50
