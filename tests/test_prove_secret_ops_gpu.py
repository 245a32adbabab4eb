"""curdle_prove_ct on the GPU against curdle_prove at ell = 4, 12, 60, 124 over the identity, the reversal and a random
permutation and once at 252: the proof bytes, the next draws of rand, curdle_verify accepting, and the counters that
prove the route -- the bucket MSM is still; the constant-time half of curdle_stat_alg_msm moves by the unflagged run's
calls + 2 and pairs + 12 (the two batches of four MSMs over six pairs that replace the twelve secret Point::Mul calls),
curdle_stat_msm_ct's pairs and walks likewise; curdle_stat_fr_permute_ct by (2 ell, 2); curdle_stat_host_point_mul by 2
where the unflagged run moved it by 14 -- all equal across the permutations, the shapes being public.  Then k = 0, 1 and
r - 1, an instance whose Rs are all infinity, and a call beside another thread's bucket MSM and verification."""
import threading

import numpy as np
import pytest

from test_prove_ct_gpu import PERMS, instance

pytestmark = pytest.mark.gpu

R_MODULUS = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


def stats(cm):
    return cm.stat_alg_msm(), cm.stat_msm_ct(), cm.stat_fr_permute_ct(), cm.stat_host_point_mul()


def moved(a, b):
    return tuple(b[i] - a[i] if isinstance(a[i], int) else {n: b[i][n] - a[i][n] for n in a[i]} for i in range(len(a)))


def prove_both(cm, inst, seed):
    crs, Rs, Ss, Ts, Us, M, perm, k, rs_m = inst
    r0, r1 = cm.Rand(seed), cm.Rand(seed)
    s0 = stats(cm)
    plain = cm.prove(crs, Rs, Ss, Ts, Us, M, perm, k, rs_m, r0)
    s1 = stats(cm)
    ct = cm.prove_ct(crs, Rs, Ss, Ts, Us, M, perm, k, rs_m, r1)
    s2 = stats(cm)
    assert (r0.get_frs(3) == r1.get_frs(3)).all()
    return plain, ct, moved(s0, s1), moved(s1, s2)


def check(cm, inst, seed, what, verify=True):
    crs, Rs, Ss, Ts, Us, M = inst[:6]
    ell = crs.ell
    plain, ct, m0, m1 = prove_both(cm, inst, seed)
    assert ct == plain, what
    if verify:
        assert cm.verify(crs, ct, Rs, Ss, Ts, Us, M, cm.Rand(43)) is True
    (alg0, ct0, fr0, mul0), (alg1, ct1, fr1, mul1) = m0, m1
    assert alg0["bucket_calls"] > 0 and alg0["ct_calls"] == 0 and ct0 == {"pairs": 0, "walks": 0, "sums": 0}
    assert fr0 == {"records": 0, "launches": 0} and mul0 == 14, what
    assert alg1 == {"bucket_calls": 0, "bucket_pairs": 0, "ct_calls": alg0["bucket_calls"] + 2,
                    "ct_pairs": alg0["bucket_pairs"] + 12}, what
    assert ct1["pairs"] == alg0["bucket_pairs"] + 12 and ct1["walks"] == alg0["bucket_calls"] + 2, what
    assert fr1 == {"records": 2 * ell, "launches": 2} and mul1 == 2, what
    return m0, m1


@pytest.mark.parametrize("ell", (4, 12, 60, 124))
def test_prove_ct_is_prove(gpu, ell):
    seen = [check(gpu, instance(gpu, ell, which), 1000 + ell, (ell, which)) for which in PERMS]
    assert seen[0] == seen[1] == seen[2]                        # the shapes are public: a function of ell


def test_prove_ct_at_ell_252(gpu):
    check(gpu, instance(gpu, 252, "random"), 1252, 252)


def fr_mont(value):
    """The fr.Element of an integer: value 2^256 mod r, four little-endian 64-bit limbs."""
    m = value * pow(2, 256, R_MODULUS) % R_MODULUS
    return np.array([(m >> (64 * i)) & ((1 << 64) - 1) for i in range(4)], dtype=np.uint64)


@pytest.mark.parametrize("kval", (0, 1, R_MODULUS - 1))
def test_edge_scalars(gpu, kval):
    """k = 0: T = k R is infinity and the 2-term MSM must return r_t H; k = 1: one addition at the last step; k = r - 1:
    the walk's one exceptional discarded sum.  The instance is committed with the same k, by the unflagged shuffle step."""
    ell = 12
    rand = gpu.Rand(ell)
    crs = gpu.CRS(ell, rand)
    perm = np.asarray(gpu.Rand(42).generate_permutation(ell), dtype=np.uint32)
    k = fr_mont(kval)
    Rs, Ss = rand.get_g1_affines(ell), rand.get_g1_affines(ell)
    Ts, Us, M, rs_m = gpu.shuffle_permute_commit(crs, Rs, Ss, perm, k, rand)
    if kval == 0:
        assert not Ts.any() and not Us.any()                     # k R_i: infinity, gnark's (0, 0)
    # with k = 0 the instance is degenerate (every T_i, U_i at infinity): the proof bytes are compared, not verified
    check(gpu, (crs, Rs, Ss, Ts, Us, M, perm, k, rs_m), 77, ("k", kval), verify=kval != 0)


def test_all_infinity_Rs(gpu):
    """proof.R = sum a_i R_i is infinity: an infinity base of the commitment MSM (public), a zero term."""
    ell = 12
    rand = gpu.Rand(ell)
    crs = gpu.CRS(ell, rand)
    perm = np.arange(ell, dtype=np.uint32)[::-1].copy()
    k = rand.get_fr()
    Rs, Ss = np.zeros((ell, 12), dtype=np.uint64), rand.get_g1_affines(ell)
    Ts, Us, M, rs_m = gpu.shuffle_permute_commit(crs, Rs, Ss, perm, k, rand)
    assert not Ts.any()
    # a degenerate instance: the proof bytes are compared with the unflagged call's, not verified
    check(gpu, (crs, Rs, Ss, Ts, Us, M, perm, k, rs_m), 78, "Rs at infinity", verify=False)


def test_prove_ct_beside_an_msm_and_a_verification(gpu, oracle, coracle):
    """Both switches are the calling thread's: the other thread's MSM and verification take the bucket path meanwhile
    and its Point::Mul counter does not see this thread's calls."""
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

    before = gpu.stat_host_point_mul(), gpu.stat_fr_permute_ct()
    th = threading.Thread(target=worker)
    th.start()
    ct = gpu.prove_ct(crs, Rs, Ss, Ts, Us, M, perm, k, rs_m, gpu.Rand(5))
    th.join()
    assert not errors, errors
    assert ct == plain
    assert gpu.stat_host_point_mul() - before[0] == 2
    assert gpu.stat_fr_permute_ct()["launches"] - before[1]["launches"] == 2
