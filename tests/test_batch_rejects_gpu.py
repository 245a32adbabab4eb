"""The batch verifiers settle a failed group by ONE accumulation in member form (curdle_dacc_run_members), not by
verifying its members one by one: k = 96 committed proofs (the ell = 12 fixture, then the Whisk fixture) in groups of
32, with bad members that pass the direct checks -- a point swapped between Ts and Us, a proof scalar altered, another
instance's M -- as the first and the last member of a group (two in that group), a group that is all bad and a group
left clean.  Every accept bit equals the single verification of that proof under the seed the batch draws for it;
curdle_stat_dacc_members shows one member-form accumulation per failed group and nobody verified one by one.  With
BATCH_GROUP above the member form's limit the bits are the same and every member of the (one, failed) group is counted
as verified one by one.  One worker thread: the groups are then members 0..31, 32..63, 64..95."""
import os

import numpy as np
import pytest

from conftest import ROOT
from test_proof_fixtures import instance

pytestmark = pytest.mark.gpu

K, GROUP = 96, 32
BAD = {0: "swap", GROUP - 1: "scalar", **{GROUP + j: ("swap", "scalar", "M")[j % 3] for j in range(GROUP)}}
BATCH_SEED = 9


@pytest.fixture(scope="module")
def vectors():
    return np.load(os.path.join(ROOT, "tests", "golden", "proof_vectors.npz"))


def batch_seeds(gpu):
    """The seed VerifyBatchCore draws for member i: the low 64 bits of the i-th element of the batch's Rand."""
    rand = gpu.Rand(BATCH_SEED)
    return [int(rand.get_fr()[0]) for _ in range(K)]


def flip_last_scalar(proof: bytes, end: int) -> bytes:
    b = bytearray(proof)
    b[end - 20] ^= 0x10
    return bytes(b)


def settled_by_members(gpu, run, failed_groups):
    """run() under groups of 32, then under one group beyond the member form's limit: the same bits; the counters."""
    with gpu.knobs(BATCH_GROUP=GROUP):
        s0 = gpu.stat_dacc_members()
        got = run()
        s1 = gpu.stat_dacc_members()
    assert s1["runs"] - s0["runs"] == failed_groups, (s0, s1)
    assert s1["members"] - s0["members"] == failed_groups * GROUP and s1["one_by_one"] == s0["one_by_one"], (s0, s1)
    with gpu.knobs(BATCH_GROUP=K):                     # 96 members: beyond CURDLE_DACC_MAX_MEMBERS
        again = run()
        s2 = gpu.stat_dacc_members()
    assert again == got
    assert s2["runs"] == s1["runs"] and s2["one_by_one"] - s1["one_by_one"] == K, (s1, s2)
    return got


def test_verify_batch_settles_failed_groups_by_member_sums(gpu, vectors):
    seed = int(vectors["ell12_seed"][0])
    crs, Rs, Ss, Ts, Us, M, *_ = instance(gpu, 12, seed)
    proof = vectors["ell12_proof"].tobytes()
    other_M = instance(gpu, 12, seed + 1)[5]
    assert not (np.asarray(other_M) == np.asarray(M)).all()
    items = [[proof, Rs, Ss, Ts, Us, M] for _ in range(K)]
    for i, kind in BAD.items():
        if kind == "swap":
            T2, U2 = Ts.copy(), Us.copy()
            T2[0], U2[0] = Us[0], Ts[0]
            items[i][3], items[i][4] = T2, U2
        elif kind == "scalar":
            items[i][0] = flip_last_scalar(proof, len(proof))
        else:
            items[i][5] = other_M
    seeds = batch_seeds(gpu)

    def single(i):
        try:
            return gpu.verify(crs, *items[i], gpu.Rand(seeds[i]))
        except gpu.CurdleError:
            return False
    expect = [single(i) for i in range(K)]
    assert expect == [i not in BAD for i in range(K)]
    cols = [list(c) for c in zip(*items)]
    got = settled_by_members(gpu, lambda: gpu.verify_batch(crs, *cols, gpu.Rand(BATCH_SEED), nthreads=1), failed_groups=2)
    assert got == expect


def test_whisk_batch_settles_failed_groups_by_member_sums(gpu, vectors):
    pre, post, proof = (vectors[k].tobytes() for k in ("whisk_pre", "whisk_post", "whisk_proof"))
    pre_l = [pre[96 * i:96 * (i + 1)] for i in range(124)]
    post_l = [post[96 * i:96 * (i + 1)] for i in range(124)]
    crs = gpu.CRS(124, gpu.Rand(7))
    pres, posts, proofs = [pre_l] * K, [list(post_l) for _ in range(K)], [proof] * K
    for i, kind in BAD.items():
        if kind == "swap":                                   # post tracker 0 = T_0 || U_0
            posts[i][0] = post_l[0][48:] + post_l[0][:48]
        elif kind == "scalar":
            proofs[i] = flip_last_scalar(proof, 4536)        # the last scalar ends where the padding starts
        else:
            proofs[i] = pre_l[3][:48] + proof[48:]           # M: the proof's first point, here some other point of G1
    seeds = batch_seeds(gpu)

    def single(i):
        try:
            return gpu.whisk_is_valid_shuffle_proof(crs, pres[i], posts[i], proofs[i], gpu.Rand(seeds[i]))
        except gpu.CurdleError:
            return False
    expect = [single(i) for i in range(K)]
    assert expect == [i not in BAD for i in range(K)]
    got = settled_by_members(
        gpu, lambda: gpu.whisk_is_valid_shuffle_proof_batch(crs, pres, posts, proofs, gpu.Rand(BATCH_SEED), nthreads=1), failed_groups=2)
    assert got == expect
