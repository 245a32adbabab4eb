"""curdle_prover_ct on the GPU: curdle_prover_ct_prove against curdle_prove_ct and curdle_prove at ell = 4, 12, 60, 124 over
the identity, the reversal and a random permutation and once at 252 -- the proof bytes, the next draws of rand,
curdle_verify accepting -- and the counters that prove the route: every funnel call of the proof resident
(curdle_stat_alg_msm_resident's resident calls move by the constant-time calls of curdle_stat_alg_msm, its fallback calls by
0), the unchunked walk still (curdle_stat_msm_ct), two tables built per proof (the instance set and the late set {R, S})
and none for the CRS after the handle's creation, two host Point::Mul calls.  Then k = 0, 1 and r - 1, an instance whose
Rs are all infinity, the term cap under PROVE_RESIDENT_TERMS, handles at chunk_bits 8 and 32, two threads through one
handle beside a bucket MSM, two handles over two CRSs, the Whisk form, and the boundary on ell where the instance
vectors stop fitting a table.  (The file of curdle_prove_ex's tests is test_prove_ct_gpu.py; this one is named after the
handle.)"""
import threading

import numpy as np
import pytest

from test_prove_ct_gpu import PERMS, instance
from test_prove_secret_ops_gpu import R_MODULUS, fr_mont

pytestmark = pytest.mark.gpu


def stats(cm):
    return (cm.stat_alg_msm(), cm.stat_alg_msm_resident(), cm.stat_msm_ct(), cm.stat_msm_ct_bases(), cm.stat_fr_permute_ct(),
            cm.stat_host_point_mul())


def moved(a, b):
    return tuple(b[i] - a[i] if isinstance(a[i], int) else {n: b[i][n] - a[i][n] for n in a[i]} for i in range(len(a)))


def check(cm, inst, seed, what, verify=True, chunk_bits=0, plain=True):
    """The handle's proof against curdle_prove_ct's (and curdle_prove's); returns what the handle's run moved."""
    crs, Rs, Ss, Ts, Us, M, perm, k, rs_m = inst
    prover = cm.ProverCt(crs, chunk_bits)
    try:
        r0, r1, r2 = cm.Rand(seed), cm.Rand(seed), cm.Rand(seed)
        s0 = stats(cm)
        ct = cm.prove_ct(crs, Rs, Ss, Ts, Us, M, perm, k, rs_m, r1)
        s1 = stats(cm)
        got = prover.prove(Rs, Ss, Ts, Us, M, perm, k, rs_m, r2)
        s2 = stats(cm)
        assert got == ct, what
        assert (r1.get_frs(3) == r2.get_frs(3)).all(), what
        if plain:
            assert cm.prove(crs, Rs, Ss, Ts, Us, M, perm, k, rs_m, r0) == got, what
        if verify:
            assert cm.verify(crs, got, Rs, Ss, Ts, Us, M, cm.Rand(43)) is True
        (alg0, res0, ct0, bases0, fr0, mul0), (alg1, res1, ct1, bases1, fr1, mul1) = moved(s0, s1), moved(s1, s2)
        # curdle_prove_ct itself: nothing resident, nothing counted under a scope
        assert res0 == {n: 0 for n in res0} and bases0 == {n: 0 for n in bases0} and ct0["walks"] == alg0["ct_calls"] > 0
        # the handle: the same funnel calls and pairs, every one of them resident
        assert alg1 == alg0 and alg1["bucket_calls"] == 0, what
        assert res1 == {"resident_calls": alg1["ct_calls"], "resident_pairs": alg1["ct_pairs"], "fallback_calls": 0,
                        "fallback_pairs": 0}, what
        assert ct1 == {"pairs": 0, "walks": 0, "sums": 0}, what          # the unchunked walk does not run
        c = 16 if chunk_bits == 0 else chunk_bits
        assert bases1 == {"tables": 2, "calls": alg1["ct_calls"], "lanes": alg1["ct_pairs"] * ((255 + c - 1) // c),
                          "msms": bases1["msms"]}, what
        assert fr1 == fr0 == {"records": 2 * crs.ell, "launches": 2} and mul1 == mul0 == 2, what
        return alg1, res1, bases1
    finally:
        prover.free()


@pytest.mark.parametrize("ell", (4, 12, 60, 124))
def test_the_handle_s_prove_is_prove_ct(gpu, ell):
    seen = [check(gpu, instance(gpu, ell, which), 1000 + ell, (ell, which)) for which in PERMS]
    assert seen[0] == seen[1] == seen[2]                        # the shapes are public: a function of ell
    rounds = (ell + 4).bit_length() - 1
    assert seen[0][0]["ct_calls"] == 10 + 2 * rounds


def test_the_handle_s_prove_at_ell_252(gpu):
    check(gpu, instance(gpu, 252, "random"), 1252, 252)


@pytest.mark.parametrize("kval", (0, 1, R_MODULUS - 1))
def test_edge_scalars(gpu, kval):
    ell = 12
    rand = gpu.Rand(ell)
    crs = gpu.CRS(ell, rand)
    perm = np.asarray(gpu.Rand(42).generate_permutation(ell), dtype=np.uint32)
    k = fr_mont(kval)
    Rs, Ss = rand.get_g1_affines(ell), rand.get_g1_affines(ell)
    Ts, Us, M, rs_m = gpu.shuffle_permute_commit(crs, Rs, Ss, perm, k, rand)
    inst = (crs, Rs, Ss, Ts, Us, M, perm, k, rs_m)
    check(gpu, inst, 77, ("k", kval), verify=kval != 0)
    if kval == 0:
        # every T_i, U_i at infinity (zero records, resident like any other): the prover proves, byte for byte as
        # curdle_prove_ct does, and the verifier refuses such a statement before it reads any proof
        assert not Ts.any() and not Us.any()
        prover = gpu.ProverCt(crs)
        proof = prover.prove(Rs, Ss, Ts, Us, M, perm, k, rs_m, gpu.Rand(77))
        prover.free()
        with pytest.raises(gpu.CurdleError, match="randomizer is zero"):
            gpu.verify(crs, proof, Rs, Ss, Ts, Us, M, gpu.Rand(43))


def test_all_infinity_Rs(gpu):
    """proof.R is infinity: the late set is {the zero record, S}, and the zero record keeps its row in the CRS set."""
    ell = 12
    rand = gpu.Rand(ell)
    crs = gpu.CRS(ell, rand)
    perm = np.arange(ell, dtype=np.uint32)[::-1].copy()
    k = rand.get_fr()
    Rs, Ss = np.zeros((ell, 12), dtype=np.uint64), rand.get_g1_affines(ell)
    Ts, Us, M, rs_m = gpu.shuffle_permute_commit(crs, Rs, Ss, perm, k, rand)
    assert not Ts.any()
    check(gpu, (crs, Rs, Ss, Ts, Us, M, perm, k, rs_m), 78, "Rs at infinity", verify=False)


def test_three_proofs_through_one_handle_build_the_crs_table_once(gpu):
    inst = instance(gpu, 60, "random")
    crs, Rs, Ss, Ts, Us, M, perm, k, rs_m = inst
    want = [gpu.prove_ct(crs, Rs, Ss, Ts, Us, M, perm, k, rs_m, gpu.Rand(s)) for s in (1, 2, 3)]
    t0 = gpu.stat_msm_ct_bases()["tables"]
    prover = gpu.ProverCt(crs)
    assert gpu.stat_msm_ct_bases()["tables"] == t0 + 1
    for i, s in enumerate((1, 2, 3)):
        assert prover.prove(Rs, Ss, Ts, Us, M, perm, k, rs_m, gpu.Rand(s)) == want[i]
        assert gpu.stat_msm_ct_bases()["tables"] == t0 + 1 + 2 * (i + 1)
    prover.free()
    prover.free()


def test_some_calls_fall_back_under_the_term_cap(gpu):
    """PROVE_RESIDENT_TERMS = 2,048 at ell = 60 and c = 16: calls of up to 128 pairs are resident, the larger ones take
    curdle_prove_ct's path; the bytes do not change."""
    inst = instance(gpu, 60, "reversal")
    crs, Rs, Ss, Ts, Us, M, perm, k, rs_m = inst
    want = gpu.prove_ct(crs, Rs, Ss, Ts, Us, M, perm, k, rs_m, gpu.Rand(9))
    prover = gpu.ProverCt(crs)
    s0 = stats(gpu)
    with gpu.knobs(PROVE_RESIDENT_TERMS=2048):
        got = prover.prove(Rs, Ss, Ts, Us, M, perm, k, rs_m, gpu.Rand(9))
    alg, res, ct, bases, _, _ = moved(s0, stats(gpu))
    assert got == want
    assert res["resident_calls"] > 0 and res["fallback_calls"] > 0
    assert res["resident_calls"] + res["fallback_calls"] == alg["ct_calls"]
    assert res["resident_pairs"] + res["fallback_pairs"] == alg["ct_pairs"]
    assert ct["walks"] == res["fallback_calls"] and bases["calls"] == res["resident_calls"]
    s0 = stats(gpu)
    assert prover.prove(Rs, Ss, Ts, Us, M, perm, k, rs_m, gpu.Rand(9)) == want       # the knob is back: all resident
    assert moved(s0, stats(gpu))[1]["fallback_calls"] == 0
    prover.free()


@pytest.mark.parametrize("chunk_bits", (8, 32))
def test_other_chunk_widths(gpu, chunk_bits):
    check(gpu, instance(gpu, 12, "random"), 50 + chunk_bits, chunk_bits, chunk_bits=chunk_bits)


def test_two_threads_through_one_handle_beside_a_bucket_msm(gpu, oracle, coracle):
    inst = instance(gpu, 60, "random")
    crs, Rs, Ss, Ts, Us, M, perm, k, rs_m = inst
    want = {s: gpu.prove_ct(crs, Rs, Ss, Ts, Us, M, perm, k, rs_m, gpu.Rand(s)) for s in (5, 6)}
    prover = gpu.ProverCt(crs)
    a, q = oracle.Rand(1).get_frs(2)
    bases = coracle.points_walk(a, q, 4096)
    t = np.random.default_rng(4096).integers(0, 1 << 62, size=(4096, 4), dtype=np.uint64)
    exp = coracle.msm_pippenger(bases, t, threads=4)
    errors = []

    def worker(seed):
        try:
            for _ in range(2):
                assert prover.prove(Rs, Ss, Ts, Us, M, perm, k, rs_m, gpu.Rand(seed)) == want[seed]
        except BaseException as e:  # noqa: BLE001 - reported by the main thread
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(s,)) for s in (5, 6)]
    for th in threads:
        th.start()
    msms = [gpu.msm_g1(bases, t) for _ in range(3)]
    for th in threads:
        th.join()
    assert not errors, errors
    for got in msms:
        assert (got == exp).all()
    prover.free()


def test_two_handles_over_two_crss(gpu):
    a, b = instance(gpu, 12, "random"), instance(gpu, 28, "identity")
    pa, pb = gpu.ProverCt(a[0]), gpu.ProverCt(b[0], 32)
    for _ in range(2):
        for inst, p in ((a, pa), (b, pb)):
            crs, rest = inst[0], inst[1:]
            assert p.prove(*rest, gpu.Rand(3)) == gpu.prove_ct(crs, *rest, gpu.Rand(3))
    # a handle refuses another CRS's ell, as curdle_prove_ct refuses it for its own CRS
    with pytest.raises(gpu.CurdleError) as e:
        pb.crs = a[0]
        pb.prove(*a[1:], gpu.Rand(3))
    assert e.value.code == gpu.EINVAL and "does not match the CRS" in e.value.msg
    pa.free()
    pb.free()


@pytest.mark.parametrize("seed", (61, 62))
def test_the_whisk_form(gpu, seed):
    crs = gpu.CRS(gpu.WHISK_ELL, gpu.Rand(4))
    r = gpu.Rand(31)
    trk, _ = gpu.whisk_compute_trackers_batch(r.get_frs(gpu.WHISK_ELL), r.get_frs(gpu.WHISK_ELL), commitments=False)
    pre = [trk[i].tobytes() for i in range(gpu.WHISK_ELL)]
    prover = gpu.ProverCt(crs)
    r0, r1 = gpu.Rand(seed), gpu.Rand(seed)
    post0, proof0 = gpu.whisk_generate_shuffle_proof_ct(crs, pre, r0)
    s0 = stats(gpu)
    post1, proof1 = prover.whisk_shuffle_proof(pre, r1)
    alg, res, ct, bases, fr, mul = moved(s0, stats(gpu))
    assert post1 == post0 and proof1 == proof0 and len(proof1) == 4576
    assert (r0.get_frs(3) == r1.get_frs(3)).all()
    assert gpu.whisk_is_valid_shuffle_proof(crs, pre, post1, proof1, gpu.Rand(43)) is True
    assert res["fallback_calls"] == 0 and res["resident_calls"] == alg["ct_calls"] == 10 + 2 * 7
    assert ct["walks"] == 2 and bases["tables"] == 2 and mul == 2          # the shuffle step's two walks, unchanged
    # the errors are the existing call's
    for trackers in (pre[:123],):
        got = []
        for call in (lambda t, r: gpu.whisk_generate_shuffle_proof_ct(crs, t, r), prover.whisk_shuffle_proof):
            rr = gpu.Rand(7)
            with pytest.raises(gpu.CurdleError) as e:
                call(trackers, rr)
            got.append((e.value.code, e.value.msg, rr.get_frs(2).tolist()))
        assert got[0] == got[1], got
    prover.free()


def _big_instance(cm, ell):
    rand = cm.Rand(ell)
    crs = cm.CRS(ell, rand)
    perm = np.asarray(cm.Rand(42).generate_permutation(ell), dtype=np.uint32)
    k = rand.get_fr()
    Rs, Ss = rand.get_g1_affines(ell), rand.get_g1_affines(ell)
    Ts, Us, M, rs_m = cm.shuffle_permute_commit(crs, Rs, Ss, perm, k, rand)
    return crs, Rs, Ss, Ts, Us, M, perm, k, rs_m


def test_the_boundary_on_ell(gpu):
    """A CRS has ell + 4 a power of two, so the sizes around the boundary 4 ell C <= 65,536 at c = 16 are ell = 1,020
    (65,280 records: the last one whose instance vectors fit; every call resident) and ell = 2,044 (the first that does
    not: the handle's CRS table still exists, the call runs as curdle_prove_ct, every funnel call is counted as a
    fallback and no table is built).  Both decisions are public: they depend on ell and chunk_bits alone."""
    for ell, fits in ((1020, True), (2044, False)):
        inst = _big_instance(gpu, ell)
        crs, rest = inst[0], inst[1:]
        want = gpu.prove_ct(crs, *rest, gpu.Rand(11))
        prover = gpu.ProverCt(crs)
        s0 = stats(gpu)
        got = prover.prove(*rest, gpu.Rand(11))
        alg, res, ct, bases, fr, mul = moved(s0, stats(gpu))
        prover.free()
        assert got == want, ell
        rounds = (ell + 4).bit_length() - 1
        assert alg["ct_calls"] == 10 + 2 * rounds
        if fits:
            assert res["fallback_calls"] == 0 and res["resident_calls"] == alg["ct_calls"] and ct["walks"] == 0
            assert bases["tables"] == 2
        else:
            assert res["resident_calls"] == 0 and res["fallback_calls"] == alg["ct_calls"] and res["fallback_pairs"] == alg["ct_pairs"]
            assert ct["walks"] == alg["ct_calls"] and bases == {n: 0 for n in bases}
