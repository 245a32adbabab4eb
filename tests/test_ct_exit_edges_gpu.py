"""The subtracting arm of the masked canonical step (csrc/g1_exit_ct.h to_gnark_ct: t >= p, the words are t - p) inside the
SHIPPED constant-time kernels.  tests/golden/ct_exit_edges.json lists points j G and scalars k in {1, 2, 3} for which the
limb-exact model says the exit product of x or of y reaches p (tools/find_ct_exit_edges.py found them; a CPU test in
tests/test_g1_ct_model.py re-checks each with the model).  With such a small scalar the accumulator entering the exit is
a function of the point's words alone, and it is the same accumulator in every path below: k_g1_mul_ct; the
constant-time MSM at n = 1 (k_msm_ct_walk, then write_result of k_msm_ct_finish); at n = 3 with two cancelling terms
placed so that the fold hands the term through add_ct's copying arm untouched (Q + (-Q) = zero words, then infinity +
term); and the batched form with one member (k_msm_ct_finish_seg).  Each result is compared with the C oracle.

k_fbase_mul_ct hands the accumulator's X and Y themselves to to_gnark_ct<kToExtX16> and <kToExtY64>.  The file's `fbase`
section lists scalars, found by the model of its 64-window walk over the generator's table among 2^17 uniform ones,
whose X exit or Y exit takes t - p: they go through curdle_g1_fixed_base_mul_batch_ex with the constant-time flag, in
both output forms, against the C oracle."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def edges(oracle, coracle):
    doc = json.load(open(os.path.join(ROOT, "tests", "golden", "ct_exit_edges.json")))
    ent = doc["entries"]
    assert ent and {e["kind"] for e in ent} >= {"x", "y"}
    pts = np.array([coracle.scalar_mul_gen(e["j"]) for e in ent], dtype=np.uint64).reshape(-1, 12)
    sc = np.array([oracle.fr_to_mont_limbs(e["k"]) for e in ent], dtype=np.uint64).reshape(-1, 4)
    want = np.array([coracle.scalar_mul_gen(e["k"] * e["j"]) for e in ent], dtype=np.uint64).reshape(-1, 12)
    return ent, pts, sc, want


def _jac(oracle, aff):
    return np.array([int(v) for v in aff] + oracle.jac_to_mont_limbs(oracle.INF)[:6], dtype=np.uint64)


def test_g1_mul_ct_on_the_exit_edges(gpu, edges):
    ent, pts, sc, want = edges
    before = gpu.stat_g1_mul_ct()
    got = gpu.g1_scalar_mul_batch(pts, sc, flags=gpu.G1_MUL_CONSTANT_TIME)
    assert gpu.stat_g1_mul_ct()["scalars"] - before["scalars"] == len(ent)      # k_g1_mul_ct ran
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), [ent[i] for i in bad]


def test_msm_ct_on_the_exit_edges(gpu, oracle, coracle, edges):
    ent, pts, sc, want = edges
    q = np.array(coracle.scalar_mul_gen(7777), dtype=np.uint64)
    nq = np.array(oracle.affine_to_mont_limbs(oracle.neg(oracle.scalar_mul(7777, (oracle.GX, oracle.GY)))), dtype=np.uint64)
    s5 = np.array(oracle.fr_to_mont_limbs(5), dtype=np.uint64)
    for i, e in enumerate(ent):
        jac = _jac(oracle, want[i])
        assert (gpu.msm_g1_ct(pts[i:i + 1], sc[i:i + 1]) == jac).all(), ("n = 1", e)
        # term 0 + term 2 = 5 Q - 5 Q: zero words; then infinity + term 1: the term's own words reach write_result
        p3, s3 = np.stack([q, pts[i], nq]), np.stack([s5, sc[i], s5])
        assert (gpu.msm_g1_ct(p3, s3) == jac).all(), ("n = 3", e)
        assert (gpu.msm_g1_ct_batch(pts[i:i + 1], sc[i:i + 1], [0, 1]) == jac[None, :]).all(), ("batch of one", e)
    all_jac = np.stack([_jac(oracle, w) for w in want])
    assert (gpu.msm_g1_ct_batch(pts, sc, list(range(len(ent) + 1))) == all_jac).all()      # and every entry as a member of one batch


def test_fbase_mul_ct_on_the_exit_edges(gpu, oracle, coracle):
    doc = json.load(open(os.path.join(ROOT, "tests", "golden", "ct_exit_edges.json")))["fbase"]
    ent = doc["entries"]
    assert ent and {e["kind"] for e in ent} >= {"x", "y"}
    ks = [int(e["k"], 16) for e in ent]
    sc = np.array([oracle.fr_to_mont_limbs(k) for k in ks], dtype=np.uint64).reshape(-1, 4)
    want = np.array([coracle.scalar_mul_gen(k) for k in ks], dtype=np.uint64).reshape(-1, 12)
    before = gpu.stat_fbase_ct()
    got = gpu.g1_fixed_base_mul_batch(sc, flags=gpu.FBASE_CONSTANT_TIME)
    assert gpu.stat_fbase_ct()["scalars"] - before["scalars"] == len(ks)                # k_fbase_mul_ct ran
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), [ent[i] for i in bad]
    comp = gpu.g1_fixed_base_mul_batch(sc, out_form=gpu.G1_OUT_COMPRESSED, flags=gpu.FBASE_CONSTANT_TIME)
    pt = lambda k: oracle.scalar_mul(k, (oracle.GX, oracle.GY))
    assert [bytes(row) for row in comp] == [oracle.compress(pt(k)) for k in ks]
