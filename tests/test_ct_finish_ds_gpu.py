"""The finish of the constant-time MSM with the division-step exit (k_msm_ct_finish_ds, k_msm_ct_finish_seg_ds,
csrc/msm_ct_kernels.hip) behind knob CT_FINISH_DIVSTEPS: every caller with the knob at 1 against the knob at 0 in the
same process, bit for bit, and against the C oracle's MSM -- curdle_msm_g1_ct at n = 1, 2, 3 (with two cancelling terms:
the result is infinity and the exit inverts 0) and 513 (one level launch before the finish), the batch over the counts
[0, 1, 2, 3, 5, 0, 64, 65, 127, 0], curdle_msm_g1_ct_bases_sets_batch over sets of 3 and 5 rows at c = 16, and the prover
handle at ell = 4 and 12 (the proof bytes, the next draws of rand, curdle_verify accepting).  curdle_stat_fp_invert's
out[2] and out[3] say which finish ran, and the existing curdle_stat_msm_ct* counters move exactly as with the knob at 0."""
import numpy as np
import pytest

from test_prove_ct_gpu import instance

pytestmark = pytest.mark.gpu

COUNTS = [0, 1, 2, 3, 5, 0, 64, 65, 127, 0]


def stats(cm):
    return cm.stat_msm_ct(), cm.stat_msm_ct_batch(), cm.stat_msm_ct_bases(), cm.stat_alg_msm(), cm.stat_alg_msm_resident()


def moved(a, b):
    return tuple({n: y[n] - x[n] for n in x} for x, y in zip(a, b))


def both(cm, call):
    """call() with the knob at 0 and at 1: (the two results, the finish launches of each run); the other counters of
    the two runs are compared here."""
    out, launches, others = [], [], []
    for knob in (0, 1):
        with cm.knobs(CT_FINISH_DIVSTEPS=knob):
            f0, s0 = cm.stat_fp_invert(), stats(cm)
            out.append(call())
            f1, s1 = cm.stat_fp_invert(), stats(cm)
        assert (f1["calls"], f1["elements"]) == (f0["calls"], f0["elements"])
        launches.append((f1["finish_divsteps"] - f0["finish_divsteps"], f1["finish_fermat"] - f0["finish_fermat"]))
        others.append(moved(s0, s1))
    assert others[0] == others[1], "the existing counters move as with the knob at 0"
    assert launches[0][0] == 0 and launches[1][1] == 0 and launches[0][1] == launches[1][0] > 0, launches
    return out, launches[1][0]


@pytest.fixture(scope="module")
def pairs(coracle, oracle):
    """600 points and Montgomery scalars below r, and the encoding of infinity."""
    k, q = oracle.Rand(35).get_frs(2)
    pts = coracle.points_walk(k, q, 600)
    sc = np.random.default_rng(35).integers(0, 1 << 64, size=(600, 4), dtype=np.uint64)
    sc[:, 3] &= np.uint64((1 << 62) - 1)
    inf = np.array(oracle.jac_to_mont_limbs(oracle.INF), dtype=np.uint64)
    return pts, sc, inf


def negated(oracle, row):
    return np.array(oracle.affine_to_mont_limbs(oracle.neg(oracle.affine_from_mont_limbs([int(v) for v in row]))), dtype=np.uint64)


def want_msm(coracle, inf, pts, sc):
    return coracle.msm_pippenger(pts, sc, threads=4) if len(pts) else inf


@pytest.mark.parametrize("n", [1, 2, 3, 513])
def test_the_single_call(gpu, oracle, coracle, pairs, n):
    pts, sc, inf = pairs
    p, s = pts[:n].copy(), sc[:n].copy()
    (off, on), launches = both(gpu, lambda: gpu.msm_g1_ct(p, s))
    assert launches == 1
    assert (on == off).all() and (on == want_msm(coracle, inf, p, s)).all()
    if n in (2, 3):
        # two cancelling terms, folded together by the fixed order (term[0] += term[h]): at n = 2 the sum is infinity and
        # the exit inverts 0; at n = 3 the third term alone is the result
        h = (n + 1) // 2
        p[h], s[h] = negated(oracle, p[0]), s[0]
        (off, on), _ = both(gpu, lambda: gpu.msm_g1_ct(p, s))
        want = inf if n == 2 else want_msm(coracle, inf, p[1:2], s[1:2])
        assert (on == off).all() and (on == want).all()


def test_the_knob_unset_is_the_library_s_rule(gpu, pairs):
    """Unset takes one of the two builds for every launch, and the same words."""
    pts, sc, _ = pairs
    gpu.plan_override("CT_FINISH_DIVSTEPS", None)
    f0 = gpu.stat_fp_invert()
    got = gpu.msm_g1_ct(pts[:5], sc[:5])
    f1 = gpu.stat_fp_invert()
    assert sorted((f1["finish_divsteps"] - f0["finish_divsteps"], f1["finish_fermat"] - f0["finish_fermat"])) == [0, 1]
    with gpu.knobs(CT_FINISH_DIVSTEPS=1):
        assert (gpu.msm_g1_ct(pts[:5], sc[:5]) == got).all()


def test_the_batch(gpu, coracle, pairs):
    pts, sc, inf = pairs
    offs = np.concatenate([[0], np.cumsum(COUNTS)]).astype(np.uint64)
    n = int(offs[-1])
    (off, on), launches = both(gpu, lambda: gpu.msm_g1_ct_batch(pts[:n], sc[:n], offs))
    assert launches == 1 and on.shape == (len(COUNTS), 18)
    want = np.stack([want_msm(coracle, inf, pts[int(a):int(b)], sc[int(a):int(b)]) for a, b in zip(offs[:-1], offs[1:])])
    assert (on == off).all() and (on == want).all()


def test_the_sets_batch_over_3_and_5_rows(gpu, coracle, pairs):
    pts, sc, inf = pairs
    sets = [gpu.CtBases(np.ascontiguousarray(pts[:3]), 16), gpu.CtBases(np.ascontiguousarray(pts[3:8]), 16)]
    try:
        rows = np.array([0, 7, 2, 3, 4, 1, 5, 6, 7, 0, 3], dtype=np.uint32)
        offs = [0, 3, 3, 8, 11]
        s = sc[:len(rows)]
        (off, on), launches = both(gpu, lambda: gpu.msm_g1_ct_bases_sets_batch(sets, rows, s, offs))
        assert launches == 1
        want = np.stack([want_msm(coracle, inf, np.ascontiguousarray(pts[rows[a:b]]), s[a:b]) for a, b in zip(offs[:-1], offs[1:])])
        assert (on == off).all() and (on == want).all()
    finally:
        for h in sets:
            h.free()


@pytest.mark.parametrize("ell", [4, 12])
def test_the_prover_handle(gpu, ell):
    crs, Rs, Ss, Ts, Us, M, perm, k, rs_m = instance(gpu, ell, "random")
    prover = gpu.ProverCt(crs)
    try:
        def prove():
            rand = gpu.Rand(500 + ell)
            proof = prover.prove(Rs, Ss, Ts, Us, M, perm, k, rs_m, rand)
            return proof, rand.get_frs(3)
        calls = gpu.stat_msm_ct_bases()["calls"]
        ((p0, d0), (p1, d1)), launches = both(gpu, prove)
        assert p1 == p0 and (d1 == d0).all()
        # every MSM call of a proof over the resident tables ends in one finish launch
        assert 2 * launches == gpu.stat_msm_ct_bases()["calls"] - calls
        assert gpu.verify(crs, p1, Rs, Ss, Ts, Us, M, gpu.Rand(43)) is True
    finally:
        prover.free()
