"""The tracker batches with exactly ONE free MSM slot, on the library's own stream: no second slot lends its stream, so
the side chain of a pass (the transcripts and the subgroup test, tracker_api.hip's decode_beside) runs behind the
square roots on the held slot's stream instead of beside them.  Only the enqueue order differs, so every call must give
what the same call gives with all slots free -- answers, proof bytes, the place a curdle_rand is left at, and the
movement of the counters -- for the host-hashed, the device-hashed and the combined check and for both forms of the
generator, with and without CURDLE_TRACKER_PROVE_CONSTANT_TIME.  k = 1 is a single lane, 65 one past a wave (and above
the size from which the default hashes on the device), 257 one past a block."""
import contextlib

import numpy as np
import pytest

from test_tracker_batch_gpu import pool  # noqa: F401  (pool: the module-scoped fixture of that file)
from test_tracker_combined_gpu import SEED, want_for

pytestmark = pytest.mark.gpu

SIZES = [1, 65, 257]
CT = 1  # CURDLE_TRACKER_PROVE_CONSTANT_TIME


@pytest.fixture(scope="module")
def parked(gpu, oracle, coracle):
    """A context manager: MSM_SLOTS - 1 pipelined MSMs of 2,048 pairs hold their slots until it is left."""
    import torch
    k, q = oracle.Rand(1).get_frs(2)
    n = 2048
    pts = coracle.points_walk(k, q, n)
    sc = np.random.default_rng(n).integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    sc[:, 3] &= np.uint64((1 << 62) - 1)
    d_pts = torch.from_numpy(pts.view(np.int64)).to("cuda:0")
    d_sc = torch.from_numpy(sc.view(np.int64)).to("cuda:0")
    torch.cuda.synchronize()

    @contextlib.contextmanager
    def hold():
        assert gpu.msm_free_slots() == gpu.MSM_SLOTS
        tickets = []
        try:
            for _ in range(gpu.MSM_SLOTS - 1):
                tickets.append(gpu.msm_g1_device_submit(d_pts.data_ptr(), d_sc.data_ptr(), n))
            assert gpu.msm_free_slots() == 1
            yield
        finally:
            waited = [gpu.msm_wait(tk) for tk in tickets]
        assert all((w == waited[0]).all() for w in waited)
        assert gpu.msm_free_slots() == gpu.MSM_SLOTS

    return hold


def with_stats(stat, call):
    before = stat()
    got = call()
    after = stat()
    return got, {name: after[name] - before[name] for name in after}


def verify_batches(pool, k):  # noqa: F811
    """Honest members with one that rejects, one S+1 and one with a record that does not decode among them; at k = 1
    each of the four kinds alone."""
    hon, cases = pool
    special = [cases[name][0] for name in ("A other", "S+1", "off curve")]
    if k == 1:
        return [[hon[0][0]]] + [[m] for m in special]
    members = [hon[j % len(hon)][0] for j in range(k)]
    for at, m in zip((0, k // 2, k - 1), special):
        members[at] = m
    return [members]


@pytest.mark.parametrize("k", SIZES)
def test_verification_with_one_free_slot(gpu, pool, parked, k):  # noqa: F811
    def plain(flags):
        return lambda t, kc, p: gpu.whisk_is_valid_tracker_proof_batch(t, kc, p, flags=flags).tolist()

    forms = [("host-hashed", plain(gpu.TRACKER_HASH_HOST), gpu.stat_tracker),
             ("device-hashed", plain(gpu.TRACKER_HASH_DEVICE), gpu.stat_tracker),
             ("combined", lambda t, kc, p: gpu.whisk_is_valid_tracker_proof_batch_combined(t, kc, p, SEED).tolist(),
              gpu.stat_tracker_combined)]
    for members in verify_batches(pool, k):
        want = want_for(gpu, members)
        t, kc, p = (list(x) for x in zip(*members))
        free = [with_stats(stat, lambda: call(t, kc, p)) for _, call, stat in forms]
        with parked():
            one = [with_stats(stat, lambda: call(t, kc, p)) for _, call, stat in forms]
        for (name, _, _), (got_free, moved_free), (got_one, moved_one) in zip(forms, free, one):
            assert got_one == want, name
            assert got_free == want, name
            assert moved_one == moved_free and any(moved_one.values()), name


def undecodable(pool):  # noqa: F811
    return pool[1]["off curve"][0][0]                   # a tracker whose krG is not on the curve


def prove_batches(oracle, pool, k):  # noqa: F811
    """(trackers, ks, blinders): the pool's honest trackers with one that does not decode among them; at k = 1 an honest
    one alone and the undecodable one alone."""
    hon, _ = pool
    bad = undecodable(pool)
    key = {h[0][0]: h[2] for h in hon}

    def batch(trackers):
        ks = np.array([oracle.fr_to_mont_limbs(key.get(t, 5)) for t in trackers], dtype=np.uint64).reshape(-1, 4)
        bl = np.random.default_rng(len(trackers)).integers(0, 1 << 62, size=(len(trackers), 4), dtype=np.uint64)
        return trackers, ks, bl

    if k == 1:
        return [batch([hon[0][0][0]]), batch([bad])]
    trackers = [hon[j % len(hon)][0][0] for j in range(k)]
    trackers[k // 2] = bad
    return [batch(trackers)]


@pytest.mark.parametrize("flags", [0, CT])
@pytest.mark.parametrize("k", SIZES)
def test_generation_with_one_free_slot(gpu, oracle, pool, parked, k, flags):  # noqa: F811
    bad = undecodable(pool)
    for trackers, ks, bl in prove_batches(oracle, pool, k):
        def blinders():
            proofs, res = gpu.whisk_generate_tracker_proof_batch(trackers, ks, blinders=bl, flags=flags)
            return proofs.tobytes(), res.tolist()

        def rand(r):
            proofs, res = gpu.whisk_generate_tracker_proof_batch(trackers, ks, rand=r, flags=flags)
            return proofs.tobytes(), res.tolist()

        ra, rb = gpu.Rand(4242 + k), gpu.Rand(4242 + k)
        free_b, moved_free_b = with_stats(gpu.stat_tracker_prove, blinders)
        free_r, moved_free_r = with_stats(gpu.stat_tracker_prove, lambda: rand(ra))
        with parked():
            one_b, moved_one_b = with_stats(gpu.stat_tracker_prove, blinders)
            one_r, moved_one_r = with_stats(gpu.stat_tracker_prove, lambda: rand(rb))
        assert one_b == free_b and one_r == free_r
        assert moved_one_b == moved_free_b == moved_one_r == moved_free_r == {"device": len(trackers), "host": 0}
        assert (ra.get_fr() == rb.get_fr()).all()
        # the undecodable member, and it alone, is refused with a proof of zeros
        assert one_b[1] == one_r[1] == [gpu.EINVAL if t == bad else gpu.OK for t in trackers]
        for i, t in enumerate(trackers):
            assert (one_b[0][128 * i:128 * i + 128] == bytes(128)) == (t == bad), i
