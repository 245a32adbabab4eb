"""curdle_whisk_generate_tracker_proof_batch / _blinders on the GPU: every member's 128 bytes equal what the single call
(curdle_whisk_generate_tracker_proof, GenerateWhiskTrackerProof at whisk.go:149) writes for the same tracker, k and
blinder, and what the big-integer model of tests/tracker_prove_model.py (pinned against the single call by
tests/test_tracker_prove_model.py) gives.  The single call draws its blinder from a Rand: a member that is compared
with it gets oracle.Rand(seed).get_fr() as its explicit blinder."""
import threading

import numpy as np
import pytest

import tracker_prove_model as tpm
from test_tracker_batch_gpu import off_curve_record, off_subgroup_point

pytestmark = pytest.mark.gpu

ZERO = bytes(128)


def limbs(oracle, values):
    return np.array([oracle.fr_to_mont_limbs(v % oracle.R) for v in values], dtype=np.uint64).reshape(-1, 4)


def single(cm, oracle, tracker, k, seed):
    """The single call's 128 bytes, or None where it returns CURDLE_EINVAL."""
    try:
        return cm.whisk_generate_tracker_proof(tracker, limbs(oracle, [k])[0], cm.Rand(seed))
    except cm.CurdleError as e:
        assert e.code == cm.EINVAL
        return None


def generate(cm, oracle, trackers, ks, bs):
    proofs, res = cm.whisk_generate_tracker_proof_batch(trackers, limbs(oracle, ks), blinders=limbs(oracle, bs))
    assert proofs.shape == (len(trackers), 128) and res.dtype == np.int32
    return [p.tobytes() for p in proofs], res.tolist()


@pytest.fixture(scope="module")
def model(oracle):
    return tpm.Model(oracle)


@pytest.fixture(scope="module")
def pool(gpu, oracle, model):
    """A dozen distinct (k, r) pairs with their trackers and k commitments."""
    rand = oracle.Rand(77)
    pairs = [(rand.get_fr(), rand.get_fr()) for _ in range(12)]
    return [(k, r, model.tracker(k, r), model.k_commitment(k, r)) for k, r in pairs]


def test_case_families_against_the_single_call_and_the_model(gpu, oracle, model):
    cases = tpm.case_families(oracle)
    seeds = [500 + j for j in range(len(cases))]
    trackers = [model.tracker(k, r) for _, k, r in cases]
    ks = [k for _, k, _ in cases]
    bs = [oracle.Rand(s).get_fr() for s in seeds]
    proofs, res = generate(gpu, oracle, trackers, ks, bs)
    assert res == [gpu.OK] * len(cases)
    for j, (name, k, r) in enumerate(cases):
        assert proofs[j] == single(gpu, oracle, trackers[j], k, seeds[j]), name
        assert proofs[j] == model.proof(k, r, bs[j]), name
    inf = oracle.compress(None)
    by_name = {c[0]: p for c, p in zip(cases, proofs)}
    assert by_name["tracker=inf"][48:96] == inf and by_name["tracker=inf"][:48] != inf    # B = b inf


def test_explicit_blinders_0_1_and_r_minus_1(gpu, oracle, model, pool):
    """No seed draws these, so the single call cannot produce them: the model is the reference, and the verifier
    accepts the result.  b = 0: A and B at infinity, s = -c k."""
    bs = [0, 1, oracle.R - 1, 0]
    members = [pool[j] for j in range(4)]
    proofs, res = generate(gpu, oracle, [m[2] for m in members], [m[0] for m in members], bs)
    assert res == [gpu.OK] * 4
    for (k, r, t, kc), b, p in zip(members, bs, proofs):
        assert p == model.proof(k, r, b), b
    assert proofs[0][:96] == oracle.compress(None) * 2
    assert gpu.whisk_is_valid_tracker_proof_batch([m[2] for m in members], [m[3] for m in members], proofs).tolist() == [1] * 4


def bad_records(oracle):
    x_ge_p = bytearray(oracle.P.to_bytes(48, "big"))
    x_ge_p[0] |= 0x80
    stray = bytearray(oracle.compress(None))
    stray[47] = 1
    return {"off curve": off_curve_record(oracle), "off subgroup": off_subgroup_point(oracle),
            "x >= p": bytes(x_ge_p), "infinity with stray bits": bytes(stray), "uncompressed form": b"\x01" * 48}


@pytest.mark.parametrize("position", ["rG", "krG"])
def test_bad_trackers_between_honest_neighbours(gpu, oracle, model, pool, position):
    trackers, ks, bs, seeds, bad_at = [], [], [], [], []
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
    for i in range(len(trackers)):
        want = single(gpu, oracle, trackers[i], ks[i], seeds[i])
        assert (want is None) == (i in bad_at), i
        if want is None:
            assert res[i] == gpu.EINVAL and proofs[i] == ZERO, i
        else:
            assert res[i] == gpu.OK and proofs[i] == want, i


def test_the_rand_form_draws_as_the_loop_of_single_calls_does(gpu, oracle, pool):
    """20 members, two that do not decode inside: a member the single call refuses before its draw draws nothing."""
    bad = bad_records(oracle)
    trackers = [pool[i % 12][2] for i in range(20)]
    ks = [pool[i % 12][0] for i in range(20)]
    trackers[6] = bad["off subgroup"] + trackers[6][48:]
    trackers[13] = trackers[13][:48] + bad["off curve"]
    ra, rb = gpu.Rand(31337), gpu.Rand(31337)
    proofs, res = gpu.whisk_generate_tracker_proof_batch(trackers, limbs(oracle, ks), rand=ra)
    for i in range(20):
        try:
            want = gpu.whisk_generate_tracker_proof(trackers[i], limbs(oracle, [ks[i]])[0], rb)
            assert res[i] == gpu.OK and proofs[i].tobytes() == want, i
        except gpu.CurdleError as e:
            assert e.code == gpu.EINVAL and i in (6, 13)
            assert res[i] == gpu.EINVAL and proofs[i].tobytes() == ZERO, i
    assert res.tolist().count(gpu.EINVAL) == 2
    assert (ra.get_fr() == rb.get_fr()).all()


def tiled(oracle, pool, k, seed, pinned=()):
    """k members over the pool with fresh blinders (Montgomery limbs below 2^254 < r taken as they are); the members in
    `pinned` get the first draw of oracle.Rand(seed of the member) so that the single call can be asked about them."""
    rng = np.random.default_rng(seed)
    which = rng.integers(len(pool), size=k)
    bl = rng.integers(0, 1 << 62, size=(k, 4), dtype=np.uint64)
    for i in pinned:
        bl[i] = oracle.fr_to_mont_limbs(oracle.Rand(10_000 + i).get_fr())
    ks = np.array([oracle.fr_to_mont_limbs(p[0]) for p in pool], dtype=np.uint64)[which]
    return which, ks, bl


def check_tiled(gpu, oracle, model, pool, k, seed, pinned=()):
    which, ks, bl = tiled(oracle, pool, k, seed, pinned)
    trackers = [pool[w][2] for w in which]
    before = gpu.stat_tracker_prove()
    proofs, res = gpu.whisk_generate_tracker_proof_batch(trackers, ks, blinders=bl)
    after = gpu.stat_tracker_prove()
    assert (res == gpu.OK).all()
    assert after["device"] + after["host"] - before["device"] - before["host"] == k     # the counters count the members
    assert after["host"] == before["host"]
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
    return trackers, ks, bl, plist


@pytest.mark.parametrize("k", [1, 15, 16, 17, 63, 64, 65, 129, 1025, 8193])
def test_sizes(gpu, oracle, model, pool, k):
    check_tiled(gpu, oracle, model, pool, k, k)


@pytest.mark.timeout(600)
def test_the_pass_boundary(gpu, oracle, model, pool):
    """65,537 members are two passes: 65,536 and 1.  The first and last member of each are held against the single call."""
    check_tiled(gpu, oracle, model, pool, 65537, 3, pinned=(0, 65535, 65536))


def test_the_same_inputs_give_the_same_bytes(gpu, oracle, model, pool):
    trackers, ks, bl, first = check_tiled(gpu, oracle, model, pool, 200, 8)
    proofs, res = gpu.whisk_generate_tracker_proof_batch(trackers, ks, blinders=bl)
    assert (res == gpu.OK).all() and [p.tobytes() for p in proofs] == first


def test_two_threads_beside_an_msm_and_a_verification(gpu, oracle, coracle, model, pool):
    jobs = []
    for t in range(2):
        which, ks, bl = tiled(oracle, pool, 300, 40 + t)
        trackers = [pool[w][2] for w in which]
        proofs, res = gpu.whisk_generate_tracker_proof_batch(trackers, ks, blinders=bl)
        assert (res == gpu.OK).all()
        jobs.append((trackers, ks, bl, proofs.copy(), [pool[w][3] for w in which]))
    k0, q0 = oracle.Rand(1).get_frs(2)
    pts = coracle.points_walk(k0, q0, 2048)
    sc = np.random.default_rng(6).integers(0, 1 << 62, size=(2048, 4), dtype=np.uint64)
    msm_want = gpu.msm_g1(pts, sc)
    errors, results = [], {}
    stop = threading.Event()

    def prover(t):
        try:
            trackers, ks, bl, _, _ = jobs[t]
            results[t] = [gpu.whisk_generate_tracker_proof_batch(trackers, ks, blinders=bl)[0].copy() for _ in range(3)]
        except Exception as e:  # noqa: BLE001 - reported below
            errors.append(e)

    def beside():
        try:
            while True:  # at least once, and for as long as the provers run
                assert (gpu.msm_g1(pts, sc) == msm_want).all()
                trackers, _, _, proofs, kcs = jobs[0]
                assert gpu.whisk_is_valid_tracker_proof_batch(trackers, kcs, [p.tobytes() for p in proofs]).tolist() == [1] * 300
                if stop.is_set():
                    break
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    other = threading.Thread(target=beside)
    other.start()
    threads = [threading.Thread(target=prover, args=(t,)) for t in range(2)]
    [t.start() for t in threads]
    [t.join() for t in threads]
    stop.set()
    other.join()
    assert not errors, errors
    for t in range(2):
        for got in results[t]:
            assert (got == jobs[t][3]).all()
