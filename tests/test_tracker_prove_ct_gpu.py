"""CURDLE_TRACKER_PROVE_CONSTANT_TIME on the GPU: curdle_whisk_generate_tracker_proof_batch_blinders_ex / _ex with the flag
write byte for byte what the single call (GenerateWhiskTrackerProof, whisk.go:149), the big-integer model of
tests/tracker_prove_model.py and the batch without the flag write.  Under the flag kG and A = b G come from
k_fbase_mul_ct over the generator's table and B = b rG from k_g1_mul_ct over the decoded rG records; the counters
prove it: a pass of m members moves curdle_stat_fbase_ct by (2 m, 1) and curdle_stat_g1_mul_ct by (m, 1) and neither
curdle_stat_fbase[0..1] nor curdle_stat_normalize."""
import threading

import numpy as np
import pytest

import tracker_prove_model as tpm
from test_tracker_prove_gpu import ZERO, bad_records, limbs, model, pool, single, tiled  # noqa: F401  (model, pool: fixtures)
from test_transcript_status_gpu import T_ONE, fr_limbs, prove_pool, prover_case  # noqa: F401  (prove_pool: a fixture)

pytestmark = pytest.mark.gpu

CT = 1
PASS = 1 << 16


def stats(gpu):
    fb = gpu.stat_fbase()
    return dict(fbct=gpu.stat_fbase_ct(), mul=gpu.stat_g1_mul_ct(), fb=(fb["scalars"], fb["launches"]), nz=gpu.stat_normalize())


def moved_as_a_flagged_call(a, b, k):
    passes = (k + PASS - 1) // PASS
    assert (b["fbct"]["scalars"] - a["fbct"]["scalars"], b["fbct"]["launches"] - a["fbct"]["launches"]) == (2 * k, passes)
    assert (b["mul"]["scalars"] - a["mul"]["scalars"], b["mul"]["launches"] - a["mul"]["launches"]) == (k, passes)
    assert b["fb"] == a["fb"] and b["nz"] == a["nz"]


def generate(gpu, oracle, trackers, ks, bs, flags=CT):
    s0 = stats(gpu)
    proofs, res = gpu.whisk_generate_tracker_proof_batch(trackers, limbs(oracle, ks), blinders=limbs(oracle, bs), flags=flags)
    s1 = stats(gpu)
    assert proofs.shape == (len(trackers), 128) and res.dtype == np.int32
    if flags:
        moved_as_a_flagged_call(s0, s1, len(trackers))
    else:
        assert s1["fbct"] == s0["fbct"] and s1["mul"] == s0["mul"]
    return [p.tobytes() for p in proofs], res.tolist()


def test_case_families_against_the_single_call_the_model_and_the_unflagged_batch(gpu, oracle, model):  # noqa: F811
    cases = tpm.case_families(oracle)
    seeds = [500 + j for j in range(len(cases))]
    trackers = [model.tracker(k, r) for _, k, r in cases]
    ks = [k for _, k, _ in cases]
    bs = [oracle.Rand(s).get_fr() for s in seeds]
    proofs, res = generate(gpu, oracle, trackers, ks, bs)
    assert res == [gpu.OK] * len(cases)
    assert (proofs, res) == generate(gpu, oracle, trackers, ks, bs, flags=0)
    plain, plain_res = gpu.whisk_generate_tracker_proof_batch(trackers, limbs(oracle, ks), blinders=limbs(oracle, bs))
    assert proofs == [p.tobytes() for p in plain] and res == plain_res.tolist()
    for j, (name, k, r) in enumerate(cases):
        assert proofs[j] == single(gpu, oracle, trackers[j], k, seeds[j]), name
        assert proofs[j] == model.proof(k, r, bs[j]), name
    inf = oracle.compress(None)
    by_name = {c[0]: p for c, p in zip(cases, proofs)}
    assert by_name["tracker=inf"][48:96] == inf and by_name["tracker=inf"][:48] != inf    # rG at infinity: B = b inf
    assert "k=0" in by_name


def test_explicit_blinders_0_1_and_r_minus_1(gpu, oracle, model, pool):  # noqa: F811
    """b = 0: A and B at infinity (the mask of both kernels), s = -c k; b = r - 1: the walk's discarded P + (-P)."""
    bs = [0, 1, oracle.R - 1, 0]
    members = [pool[j] for j in range(4)]
    args = ([m[2] for m in members], [m[0] for m in members], bs)
    proofs, res = generate(gpu, oracle, *args)
    assert res == [gpu.OK] * 4
    assert (proofs, res) == generate(gpu, oracle, *args, flags=0)
    for (k, r, t, kc), b, p in zip(members, bs, proofs):
        assert p == model.proof(k, r, b), b
    assert proofs[0][:96] == oracle.compress(None) * 2
    assert gpu.whisk_is_valid_tracker_proof_batch([m[2] for m in members], [m[3] for m in members], proofs).tolist() == [1] * 4


@pytest.mark.parametrize("position", ["rG", "krG"])
def test_bad_trackers_between_honest_neighbours(gpu, oracle, model, pool, position):  # noqa: F811
    trackers, ks, seeds, bad_at = [], [], [], []
    for j, (name, rec) in enumerate(bad_records(oracle).items()):
        k, r, t, _ = pool[j]
        k2, _, t2, _ = pool[j + 5]
        trackers += [t, rec + t2[48:] if position == "rG" else t2[:48] + rec]
        ks += [k, k2]
        seeds += [700 + 2 * j, 701 + 2 * j]
        bad_at.append(2 * j + 1)
    k, r, t, _ = pool[11]
    trackers.append(t)
    ks.append(k)
    seeds.append(799)
    bs = [oracle.Rand(s).get_fr() for s in seeds]
    proofs, res = generate(gpu, oracle, trackers, ks, bs)
    assert len(bad_at) == 5
    for i in range(len(trackers)):
        want = single(gpu, oracle, trackers[i], ks[i], seeds[i])
        assert (want is None) == (i in bad_at), i
        if want is None:
            assert res[i] == gpu.EINVAL and proofs[i] == ZERO, i
        else:
            assert res[i] == gpu.OK and proofs[i] == want, i
    assert (proofs, res) == generate(gpu, oracle, trackers, ks, bs, flags=0)


def test_the_rand_form_leaves_rand_where_the_loop_of_single_calls_does(gpu, oracle, pool):  # noqa: F811
    bad = bad_records(oracle)
    trackers = [pool[i % 12][2] for i in range(20)]
    ks = [pool[i % 12][0] for i in range(20)]
    trackers[6] = bad["off subgroup"] + trackers[6][48:]
    trackers[13] = trackers[13][:48] + bad["off curve"]
    ra, rb, rc = gpu.Rand(31337), gpu.Rand(31337), gpu.Rand(31337)
    s0 = stats(gpu)
    proofs, res = gpu.whisk_generate_tracker_proof_batch(trackers, limbs(oracle, ks), rand=ra, flags=CT)
    moved_as_a_flagged_call(s0, stats(gpu), 20)
    for i in range(20):
        try:
            want = gpu.whisk_generate_tracker_proof(trackers[i], limbs(oracle, [ks[i]])[0], rb)
            assert res[i] == gpu.OK and proofs[i].tobytes() == want, i
        except gpu.CurdleError as e:
            assert e.code == gpu.EINVAL and i in (6, 13)
            assert res[i] == gpu.EINVAL and proofs[i].tobytes() == ZERO, i
    assert res.tolist().count(gpu.EINVAL) == 2
    plain, plain_res = gpu.whisk_generate_tracker_proof_batch(trackers, limbs(oracle, ks), rand=rc, flags=0)
    assert (plain == proofs).all() and (plain_res == res).all()
    nxt = rb.get_fr()
    assert (ra.get_fr() == nxt).all() and (rc.get_fr() == nxt).all()


def check_tiled(gpu, oracle, model, pool, k, seed, pinned=()):  # noqa: F811
    which, ks, bl = tiled(oracle, pool, k, seed, pinned)
    trackers = [pool[w][2] for w in which]
    before, s0 = gpu.stat_tracker_prove(), stats(gpu)
    proofs, res = gpu.whisk_generate_tracker_proof_batch(trackers, ks, blinders=bl, flags=CT)
    after, s1 = gpu.stat_tracker_prove(), stats(gpu)
    assert (res == gpu.OK).all()
    assert (after["device"] - before["device"], after["host"] - before["host"]) == (k, 0)
    moved_as_a_flagged_call(s0, s1, k)
    plist = [p.tobytes() for p in proofs]
    assert gpu.whisk_is_valid_tracker_proof_batch(trackers, [pool[w][3] for w in which], plist).tolist() == [1] * k
    rng = np.random.default_rng(seed + 1)
    sample = range(k) if k <= 64 else sorted(set(rng.integers(k, size=64).tolist()))
    for i in sample:
        kk, r = pool[which[i]][0], pool[which[i]][1]
        b = oracle.fr_from_mont_limbs([int(v) for v in bl[i]])
        assert plist[i] == model.proof(kk, r, b), i
    for i in pinned:
        assert plist[i] == single(gpu, oracle, trackers[i], pool[which[i]][0], 10_000 + i), i
    return trackers, ks, bl, proofs


@pytest.mark.parametrize("k", [1, 63, 64, 65, 257])
def test_sizes(gpu, oracle, model, pool, k):  # noqa: F811
    trackers, ks, bl, proofs = check_tiled(gpu, oracle, model, pool, k, k)
    plain, _ = gpu.whisk_generate_tracker_proof_batch(trackers, ks, blinders=bl)
    assert (plain == proofs).all()


@pytest.mark.timeout(600)
def test_the_pass_boundary(gpu, oracle, model, pool):  # noqa: F811
    """65,537 members are two passes, 65,536 and 1: every member verified by the batch verifier, 64 sampled against the
    model, the first and last member of each pass against the single call, the whole against the unflagged batch."""
    trackers, ks, bl, proofs = check_tiled(gpu, oracle, model, pool, 65537, 3, pinned=(0, 65535, 65536))
    plain, _ = gpu.whisk_generate_tracker_proof_batch(trackers, ks, blinders=bl)
    assert (plain == proofs).all()


@pytest.mark.parametrize("k", [3, 65])
def test_members_that_give_up_are_handed_to_the_host(gpu, oracle, prove_pool, k):  # noqa: F811
    """TRANSCRIPT_MAX_TRIES = 1: the members the model names are generated by the host single path, under the flag as
    without it, and curdle_stat_tracker_prove[1] moves by the model's count."""
    c = prover_case(gpu, oracle, prove_pool, k, T_ONE, seed=900 + k)
    want, n_back = c["want"], sum(c["back"])
    assert n_back >= 1
    ks = fr_limbs(oracle, c["ks"])
    with gpu.knobs(TRANSCRIPT_MAX_TRIES=T_ONE):
        s0, t0 = gpu.stat_tracker_prove(), stats(gpu)
        proofs, res = gpu.whisk_generate_tracker_proof_batch(c["trackers"], ks, blinders=fr_limbs(oracle, c["blinders"]), flags=CT)
        s1, t1 = gpu.stat_tracker_prove(), stats(gpu)
        ra = gpu.Rand(c["seed"])
        rproofs, rres = gpu.whisk_generate_tracker_proof_batch(c["trackers"], ks, rand=ra, flags=CT)
        s2 = gpu.stat_tracker_prove()
    moved_as_a_flagged_call(t0, t1, k)
    assert (ra.get_fr() == c["next_fr"]).all()
    for a, b in ((s0, s1), (s1, s2)):
        assert (b["host"] - a["host"], b["device"] - a["device"]) == (n_back, k - n_back)
    for got, gres in ((proofs, res), (rproofs, rres)):
        for i in range(k):
            if want[i] is None:
                assert gres[i] == gpu.EINVAL and got[i].tobytes() == ZERO, i
            else:
                assert gres[i] == gpu.OK and got[i].tobytes() == want[i], (i, c["back"][i])


def test_one_thread_beside_an_msm_and_a_verification(gpu, oracle, coracle, model, pool):  # noqa: F811
    which, ks, bl = tiled(oracle, pool, 300, 41)
    trackers = [pool[w][2] for w in which]
    kcs = [pool[w][3] for w in which]
    first, res = gpu.whisk_generate_tracker_proof_batch(trackers, ks, blinders=bl)          # the unflagged batch's bytes
    assert (res == gpu.OK).all()
    plist = [p.tobytes() for p in first]
    k0, q0 = oracle.Rand(1).get_frs(2)
    pts = coracle.points_walk(k0, q0, 2048)
    sc = np.random.default_rng(6).integers(0, 1 << 62, size=(2048, 4), dtype=np.uint64)
    msm_want = gpu.msm_g1(pts, sc)
    errors, results = [], []

    def prover():
        try:
            for _ in range(3):
                results.append(gpu.whisk_generate_tracker_proof_batch(trackers, ks, blinders=bl, flags=CT)[0].copy())
        except Exception as e:  # noqa: BLE001 - reported below
            errors.append(e)

    th = threading.Thread(target=prover)
    th.start()
    for _ in range(2):
        assert (gpu.msm_g1(pts, sc) == msm_want).all()
        assert gpu.whisk_is_valid_tracker_proof_batch(trackers, kcs, plist).tolist() == [1] * 300
    th.join()
    assert not errors, errors
    assert len(results) == 3 and all((got == first).all() for got in results)
