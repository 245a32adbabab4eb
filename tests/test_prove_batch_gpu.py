"""curdle_prove_batch on the GPU against the single calls of the same build: k members over one CRS with different
permutations (identity, reversal, random), different k (0, 1, r - 1, random) and different seeds; per member the proof
bytes and length are the single call's (curdle_prove without the flag, curdle_prove_ct under it), the next two draws of
its rand are equal, and curdle_verify accepts (for k = 0 the prover proves, byte for byte as the single call does, but
Ts[0] is the point at infinity and the verifier refuses such a statement before it reads any proof: that refusal is
what is asserted there).  That coalescing happened is asserted on the counters: under the default
group size curdle_stat_alg_msm moves by the CALLS of one single Prove and k times its pairs.  PROVE_BATCH_GROUP = 2 makes
three groups of five members, PROVE_BATCH_PAIRS splits a step, and neither changes a byte.  Under the flag
curdle_stat_msm_ct's walks are one single constant-time Prove's, curdle_stat_fr_permute_ct moves by (2 ell k, 2) and the
calling thread multiplies no point on the host.  One batch runs beside a thread with a bucket MSM and a verification."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R_MOD = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


def mont(x):
    """The Montgomery fr.Element of the integer x, four little-endian limbs."""
    v = (x << 256) % R_MOD
    return np.array([(v >> (64 * i)) & ((1 << 64) - 1) for i in range(4)], dtype=np.uint64)


_crs, _members, _singles = {}, {}, {}


def the_crs(cm, ell):
    if ell not in _crs:
        _crs[ell] = cm.CRS(ell, cm.Rand(ell))
    return _crs[ell]


def member(cm, ell, i):
    """Member i's statement and witness (computed once): its own points, permutation, k and blinders."""
    if (ell, i) not in _members:
        crs = the_crs(cm, ell)
        rand = cm.Rand(7000 + 100 * ell + i)
        perm = (np.arange(ell, dtype=np.uint32), np.arange(ell, dtype=np.uint32)[::-1].copy(),
                np.asarray(cm.Rand(42 + i).generate_permutation(ell), dtype=np.uint32))[i % 3]
        k = (mont(0), mont(1), mont(R_MOD - 1), rand.get_fr())[i % 4]
        Rs, Ss = rand.get_g1_affines(ell), rand.get_g1_affines(ell)
        Ts, Us, M, rs_m = cm.shuffle_permute_commit(crs, Rs, Ss, perm, k, rand)
        _members[(ell, i)] = (Rs, Ss, Ts, Us, M, perm, k, rs_m)
    return _members[(ell, i)]


def deltas(cm, before=None):
    now = {"alg": cm.stat_alg_msm(), "ct": cm.stat_msm_ct(), "gather": cm.stat_fr_permute_ct(), "batch": cm.stat_prove_batch(),
           "mul": cm.stat_host_point_mul()}
    if before is None:
        return now
    return {n: (now[n] - before[n] if n == "mul" else {f: now[n][f] - before[n][f] for f in now[n]}) for n in now}


def single(cm, ell, i, flags):
    """Member i's single call (once): (proof bytes or the error code, the rand's next two draws, what the call moved)."""
    key = (ell, i, flags)
    if key not in _singles:
        m = member(cm, ell, i)
        rand = cm.Rand(9000 + i)
        s0 = deltas(cm)
        try:
            proof = (cm.prove_ct if flags else cm.prove)(the_crs(cm, ell), *m, rand)
        except cm.CurdleError as e:
            proof = e.code
        _singles[key] = (proof, rand.get_frs(2), deltas(cm, s0))
    return _singles[key]


def run_batch(cm, ell, k, flags):
    rands = [cm.Rand(9000 + i) for i in range(k)]
    s0 = deltas(cm)
    proofs, status = cm.prove_batch(the_crs(cm, ell), [member(cm, ell, i) + (rands[i],) for i in range(k)], flags)
    return proofs, status, [r.get_frs(2) for r in rands], deltas(cm, s0)


def check_members(cm, ell, k, flags, proofs, status, draws):
    crs = the_crs(cm, ell)
    for i in range(k):
        want, want_draws, _ = single(cm, ell, i, flags)
        if isinstance(want, int):
            assert status[i] == want and proofs[i] == b"", (ell, k, i)
        else:
            assert status[i] == 0 and proofs[i] == want, (ell, k, i)
            Rs, Ss, Ts, Us, M = member(cm, ell, i)[:5]
            if i % 4 == 0:                               # k = 0: Ts[0] is infinity, a statement the verifier refuses unread
                with pytest.raises(cm.CurdleError, match="randomizer is zero"):
                    cm.verify(crs, proofs[i], Rs, Ss, Ts, Us, M, cm.Rand(43))
            else:
                assert cm.verify(crs, proofs[i], Rs, Ss, Ts, Us, M, cm.Rand(43)) is True, (ell, k, i)
        assert (draws[i] == want_draws).all(), (ell, k, i)


@pytest.mark.parametrize("flags", (0, 1))
@pytest.mark.parametrize("ell,k", [(ell, k) for ell in (4, 12) for k in (1, 2, 3, 5, 17)] + [(60, 3)])
def test_a_batch_is_its_single_calls_and_coalesces(gpu, ell, k, flags):
    cm = gpu
    singles = [single(cm, ell, i, flags) for i in range(k)]
    proofs, status, draws, moved = run_batch(cm, ell, k, flags)
    check_members(cm, ell, k, flags, proofs, status, draws)
    assert all(not isinstance(s[0], int) for s in singles), "every member of this batch proves on its own"
    one = singles[0][2]
    for s in singles:                                    # the shapes are public: a function of ell
        assert s[2]["alg"] == one["alg"] and s[2]["ct"]["walks"] == one["ct"]["walks"]
    calls, pairs = ("ct_calls", "ct_pairs") if flags else ("bucket_calls", "bucket_pairs")
    assert one["alg"][calls] > 0
    assert moved["alg"][calls] == one["alg"][calls], "the calls of ONE single Prove"
    assert moved["alg"][pairs] == k * one["alg"][pairs], "... with k times its pairs"
    other = ("bucket_calls", "bucket_pairs") if flags else ("ct_calls", "ct_pairs")
    assert moved["alg"][other[0]] == 0 and moved["alg"][other[1]] == 0
    gathers = 2 if flags else 0
    assert moved["batch"] == {"calls": 1, "members": k, "groups": 1, "device_calls": one["alg"][calls] + gathers}
    if flags:
        assert moved["ct"]["walks"] == one["ct"]["walks"] and moved["ct"]["pairs"] == k * one["ct"]["pairs"]
        assert (moved["gather"]["records"], moved["gather"]["launches"]) == (2 * ell * k, 2)
        assert (one["gather"]["records"], one["gather"]["launches"]) == (2 * ell, 2)
        assert moved["mul"] == 0, "the calling thread multiplies no point on the host"
    else:
        assert moved["ct"] == {"pairs": 0, "walks": 0, "sums": 0} and moved["gather"] == {"records": 0, "launches": 0}


@pytest.mark.parametrize("flags", (0, 1))
def test_groups_of_two_make_three_groups_of_five_members(gpu, flags):
    cm, ell, k = gpu, 12, 5
    with cm.knobs(PROVE_BATCH_GROUP=2):
        proofs, status, draws, moved = run_batch(cm, ell, k, flags)
    check_members(cm, ell, k, flags, proofs, status, draws)
    one = single(cm, ell, 0, flags)[2]
    calls = "ct_calls" if flags else "bucket_calls"
    assert moved["batch"]["groups"] == 3 and moved["batch"]["members"] == 5
    assert moved["alg"][calls] == 3 * one["alg"][calls]


@pytest.mark.parametrize("flags", (0, 1))
def test_a_split_step_changes_no_byte(gpu, flags):
    """PROVE_BATCH_PAIRS below two members' pairs of every step that has ell pairs or more: those steps go out member by
    member, the small ones still together."""
    cm, ell, k = gpu, 12, 5
    with cm.knobs(PROVE_BATCH_PAIRS=ell):
        proofs, status, draws, moved = run_batch(cm, ell, k, flags)
    check_members(cm, ell, k, flags, proofs, status, draws)
    one = single(cm, ell, 0, flags)[2]
    calls, pairs = ("ct_calls", "ct_pairs") if flags else ("bucket_calls", "bucket_pairs")
    assert moved["alg"][calls] > one["alg"][calls], "a step was split"
    assert moved["alg"][pairs] == k * one["alg"][pairs]
    assert moved["batch"]["groups"] == 1


def test_refusals_with_a_device(gpu):
    cm, ell = gpu, 4
    crs = the_crs(cm, ell)
    ms = [member(cm, ell, i) for i in range(2)]
    rands = [cm.Rand(1), cm.Rand(1)]
    before = cm.stat_prove_batch()
    with pytest.raises(cm.CurdleError) as e:
        cm.prove_batch(crs, [ms[0] + (rands[0],), ms[1] + (rands[1],)], flags=2)
    assert e.value.code == cm.EINVAL and "flag" in e.value.msg
    with pytest.raises(cm.CurdleError) as e:
        cm.prove_batch(crs, [ms[0] + (rands[0],), ms[1] + (rands[0],)])
    assert e.value.code == cm.EINVAL and "share" in e.value.msg
    with pytest.raises(cm.CurdleError) as e:
        cm.prove_batch(the_crs(cm, 12), [ms[0] + (rands[0],), ms[1] + (rands[1],)])
    assert e.value.code == cm.EINVAL and "CRS" in e.value.msg
    with cm.knobs(PROVER_FOLD_BASES=1):
        with pytest.raises(cm.CurdleError) as e:
            cm.prove_batch(crs, [ms[0] + (rands[0],)], flags=cm.PROVE_BATCH_CONSTANT_TIME)
        assert e.value.code == cm.EINVAL and "FOLD_BASES" in e.value.msg
    assert cm.stat_prove_batch() == before
    assert (rands[0].get_frs(2) == cm.Rand(1).get_frs(2)).all(), "nothing was drawn"
    assert cm.prove_batch(crs, [], flags=1) == ([], [])


def test_a_batch_beside_an_msm_and_a_verification(gpu, oracle, coracle):
    """The switches live on the member threads: another thread's bucket MSM and verification are untouched meanwhile."""
    cm, ell, k = gpu, 12, 3
    crs = the_crs(cm, ell)
    Rs, Ss, Ts, Us, M = member(cm, ell, 1)[:5]
    plain = single(cm, ell, 1, 0)[0]
    a, q = oracle.Rand(1).get_frs(2)
    bases = coracle.points_walk(a, q, 4096)
    t = np.random.default_rng(4096).integers(0, 1 << 62, size=(4096, 4), dtype=np.uint64)
    exp = coracle.msm_pippenger(bases, t, threads=4)
    errors = []

    def worker():
        try:
            for _ in range(3):
                assert (cm.msm_g1(bases, t) == exp).all()
                assert cm.verify(crs, plain, Rs, Ss, Ts, Us, M, cm.Rand(43)) is True
        except BaseException as e:  # noqa: BLE001 - reported by the main thread
            errors.append(e)

    th = threading.Thread(target=worker)
    th.start()
    results = [run_batch(cm, ell, k, flags) for flags in (1, 0)]
    th.join()
    assert not errors, errors
    for flags, (proofs, status, draws, _) in zip((1, 0), results):
        check_members(cm, ell, k, flags, proofs, status, draws)
