"""curdle_prove_ex under CURDLE_PROVE_MSM_CONSTANT_TIME on the GPU: the flagged Prove against the unflagged one at
ell = 4, 12, 60, 124 and once at 252, over the identity, the reversal and a random permutation -- the proof bytes, the
next draws of rand and curdle_verify accepting the flagged proof -- and the counters: under the flag the bucket half of
curdle_stat_alg_msm does not move, the constant-time half moves by exactly the calls and pairs the unflagged run moved
the bucket half, and curdle_stat_msm_ct by the same pairs; without the flag the constant-time half does not move."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PERMS = ("identity", "reversal", "random")


def instance(cm, ell, which):
    rand = cm.Rand(ell)
    crs = cm.CRS(ell, rand)
    perm = {"identity": np.arange(ell, dtype=np.uint32), "reversal": np.arange(ell, dtype=np.uint32)[::-1].copy(),
            "random": np.asarray(cm.Rand(42).generate_permutation(ell), dtype=np.uint32)}[which]
    k = rand.get_fr()
    Rs = rand.get_g1_affines(ell)
    Ss = rand.get_g1_affines(ell)
    Ts, Us, M, rs_m = cm.shuffle_permute_commit(crs, Rs, Ss, perm, k, rand)
    return crs, Rs, Ss, Ts, Us, M, perm, k, rs_m


def prove_both(cm, inst, seed):
    """(unflagged proof, flagged proof, what the unflagged run moved, what the flagged run moved); the draws of rand
    after the two calls are compared here."""
    crs, Rs, Ss, Ts, Us, M, perm, k, rs_m = inst
    r0, r1 = cm.Rand(seed), cm.Rand(seed)
    s0 = cm.stat_alg_msm(), cm.stat_msm_ct()
    plain = cm.prove(crs, Rs, Ss, Ts, Us, M, perm, k, rs_m, r0)
    s1 = cm.stat_alg_msm(), cm.stat_msm_ct()
    flagged = cm.prove(crs, Rs, Ss, Ts, Us, M, perm, k, rs_m, r1, flags=cm.PROVE_MSM_CONSTANT_TIME)
    s2 = cm.stat_alg_msm(), cm.stat_msm_ct()
    assert (r0.get_frs(3) == r1.get_frs(3)).all()
    d = lambda a, b: {n: b[n] - a[n] for n in a}
    return plain, flagged, (d(s0[0], s1[0]), d(s0[1], s1[1])), (d(s1[0], s2[0]), d(s1[1], s2[1]))


def check(cm, ell, which):
    inst = instance(cm, ell, which)
    crs, Rs, Ss, Ts, Us, M = inst[:6]
    plain, flagged, moved_plain, moved_flagged = prove_both(cm, inst, 1000 + ell)
    assert flagged == plain, (ell, which)
    assert cm.verify(crs, flagged, Rs, Ss, Ts, Us, M, cm.Rand(43)) is True
    # flags = 0 IS curdle_prove
    assert cm.prove(crs, *inst[1:], cm.Rand(1000 + ell), flags=0) == plain
    (alg0, ct0), (alg1, ct1) = moved_plain, moved_flagged
    assert alg0["bucket_calls"] > 0 and alg0["bucket_pairs"] > 0 and alg0["ct_calls"] == 0 and alg0["ct_pairs"] == 0
    assert ct0 == {"pairs": 0, "walks": 0, "sums": 0}
    assert alg1 == {"bucket_calls": 0, "bucket_pairs": 0, "ct_calls": alg0["bucket_calls"], "ct_pairs": alg0["bucket_pairs"]}
    assert ct1["pairs"] == alg0["bucket_pairs"] and ct1["walks"] == alg0["bucket_calls"]
    return alg0


@pytest.mark.parametrize("ell", (4, 12, 60, 124))
def test_the_flagged_prove_is_the_unflagged_one(gpu, ell):
    moved = [check(gpu, ell, which) for which in PERMS]
    assert moved[0] == moved[1] == moved[2]                                 # the MSM shapes are public: a function of ell


def test_the_flagged_prove_at_ell_252(gpu):
    check(gpu, 252, "random")


def test_a_flagged_prove_beside_an_msm_and_a_verification(gpu, oracle, coracle):
    """The switch is the calling thread's: the other thread's MSM and verification take the bucket path meanwhile (their
    results are checked; the flagged proof is the unflagged one)."""
    inst = instance(gpu, 60, "random")
    crs, Rs, Ss, Ts, Us, M, perm, k, rs_m = inst
    plain = gpu.prove(crs, Rs, Ss, Ts, Us, M, perm, k, rs_m, gpu.Rand(5))
    a, q = oracle.Rand(1).get_frs(2)
    bases = coracle.points_walk(a, q, 4096)
    t = np.random.default_rng(4096).integers(0, 1 << 62, size=(4096, 4), dtype=np.uint64)
    exp = coracle.msm_pippenger(bases, t, threads=4)
    errors = []

    def worker():
        try:
            for _ in range(3):
                assert (gpu.msm_g1(bases, t) == exp).all()
                assert gpu.verify(crs, plain, Rs, Ss, Ts, Us, M, gpu.Rand(43)) is True
        except BaseException as e:  # noqa: BLE001 - reported by the main thread
            errors.append(e)

    th = threading.Thread(target=worker)
    th.start()
    flagged = gpu.prove(crs, Rs, Ss, Ts, Us, M, perm, k, rs_m, gpu.Rand(5), flags=gpu.PROVE_MSM_CONSTANT_TIME)
    th.join()
    assert not errors, errors
    assert flagged == plain
