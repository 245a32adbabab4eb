"""curdle_whisk_generate_shuffle_proof_ct on the GPU against curdle_whisk_generate_shuffle_proof, two seeds: the same
post-trackers, the same 4,576 proof bytes, rand in the same state, curdle_whisk_is_valid_shuffle_proof accepting; the
unflagged call's errors for a tracker that does not decode and for n = 123; and the counters of the route: one pass of
the constant-time scalar multiplication over 248 points, the shuffle step's two walks over 128 pairs and one sum plus
what a curdle_prove_ct at ell = 124 moves, two host Point::Mul calls (both by public challenges)."""
import numpy as np
import pytest

from test_prove_ct_gpu import instance

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup(gpu):
    crs = gpu.CRS(gpu.WHISK_ELL, gpu.Rand(4))
    r = gpu.Rand(31)
    trk, _ = gpu.whisk_compute_trackers_batch(r.get_frs(gpu.WHISK_ELL), r.get_frs(gpu.WHISK_ELL), commitments=False)
    return crs, [trk[i].tobytes() for i in range(gpu.WHISK_ELL)]


def stats(cm):
    return cm.stat_g1_mul_ct(), cm.stat_msm_ct(), cm.stat_fr_permute_ct(), cm.stat_alg_msm()


def diff(a, b):
    return [{n: y[n] - x[n] for n in x} for x, y in zip(a, b)]


@pytest.fixture(scope="module")
def prove_moves(gpu):
    """What one curdle_prove_ct at ell = 124 moves: a function of ell alone (test_prove_secret_ops_gpu.py)."""
    crs, Rs, Ss, Ts, Us, M, perm, k, rs_m = instance(gpu, gpu.WHISK_ELL, "identity")
    s0 = stats(gpu)
    gpu.prove_ct(crs, Rs, Ss, Ts, Us, M, perm, k, rs_m, gpu.Rand(3))
    return diff(s0, stats(gpu))


@pytest.mark.parametrize("seed", (61, 62))
def test_the_ct_call_is_the_unflagged_one(gpu, setup, prove_moves, seed):
    crs, pre = setup
    ell = gpu.WHISK_ELL
    r0, r1 = gpu.Rand(seed), gpu.Rand(seed)
    post0, proof0 = gpu.whisk_generate_shuffle_proof(crs, pre, r0)
    mul0, s0 = gpu.stat_host_point_mul(), stats(gpu)
    post1, proof1 = gpu.whisk_generate_shuffle_proof_ct(crs, pre, r1)
    mul1, s1 = gpu.stat_host_point_mul(), stats(gpu)
    assert post1 == post0 and proof1 == proof0 and len(proof1) == 4576
    assert (r0.get_frs(3) == r1.get_frs(3)).all()
    assert gpu.whisk_is_valid_shuffle_proof(crs, pre, post1, proof1, gpu.Rand(43)) is True
    g1mul, msm, fr, alg = diff(s0, s1)
    p_g1mul, p_msm, p_fr, p_alg = prove_moves
    assert (g1mul["scalars"], g1mul["launches"]) == (2 * ell, 1) and p_g1mul == {n: 0 for n in p_g1mul}
    assert msm == {"pairs": ell + 4 + p_msm["pairs"], "walks": 2 + p_msm["walks"], "sums": 1 + p_msm["sums"]}
    assert fr == {"records": 2 * ell, "launches": 2} == p_fr
    assert alg == p_alg and alg["bucket_calls"] == 0 and alg["bucket_pairs"] == 0      # the step's MSM is not the funnel's
    assert mul1 - mul0 == 2


def test_the_errors_are_the_unflagged_call_s(gpu, setup):
    crs, pre = setup
    bad = list(pre)
    bad[5] = bytes([0xFF]) * 96                                 # x >= p: not an encoding
    for trackers in (bad, pre[:123]):
        got = []
        for call in (gpu.whisk_generate_shuffle_proof, gpu.whisk_generate_shuffle_proof_ct):
            r = gpu.Rand(7)
            with pytest.raises(gpu.CurdleError) as e:
                call(crs, trackers, r)
            got.append((e.value.code, e.value.msg, r.get_frs(2).tolist()))
        assert got[0] == got[1], got
    assert "ELL trackers" in got[0][1]
