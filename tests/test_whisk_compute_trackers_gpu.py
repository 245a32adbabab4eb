"""curdle_whisk_compute_trackers_batch on the GPU: computeTracker and getKComm (whisk/whisk_test.go:98-109) for n members
in one call, byte for byte what the two single host calls write -- over the k x r matrix of tests/test_fbase_abi.py, at
the edges of a wave and a block, across a pass, across the normalisation's switch to its wide lane rule (3 n crosses
65,536 between n = 21,845 and 21,846), and through the whole tracker life cycle: compute, prove, verify."""
import numpy as np
import pytest

import fbase_model as fm

pytestmark = pytest.mark.gpu

INF48 = bytes([0xC0]) + bytes(47)
ONE = np.array([0x00000001fffffffe, 0x5884b7fa00034802, 0x998c4fefecbc4ff5, 0x1824b159acc5056f], dtype=np.uint64)  # 1 as an fr.Element


def single(gpu, ks, rs):
    """The single host calls over limb arrays: (uint8[n, 96], uint8[n, 48])."""
    t, c = [], []
    for i in range(len(ks)):
        t.append(gpu.whisk_compute_tracker(ks[i], rs[i] if rs is not None else ONE))
        c.append(gpu.whisk_k_commitment(ks[i]))
    return (np.frombuffer(b"".join(t), dtype=np.uint8).reshape(-1, 96), np.frombuffer(b"".join(c), dtype=np.uint8).reshape(-1, 48))


def random_limbs(seed, n):
    """n Montgomery fr.Elements: any four words below r are one."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64((1 << 62) - 1)
    return a


def test_the_montgomery_one_of_this_file(oracle):
    assert oracle.fr_to_mont_limbs(1) == [int(v) for v in ONE]


def test_the_matrix_against_the_single_calls_and_the_model(gpu, oracle, coracle):
    vals = fm.whisk_scalars(oracle)
    pairs = [(k, r) for _, k in vals for _, r in vals]
    inv = vals[-1][1]
    pairs.append((inv, pow(inv, -1, oracle.R)))                                   # k r = 1
    ks, rs = fm.to_limbs(oracle, [k for k, _ in pairs]), fm.to_limbs(oracle, [r for _, r in pairs])
    a = gpu.stat_fbase()
    trk, com = gpu.whisk_compute_trackers_batch(ks, rs)
    b = gpu.stat_fbase()
    assert b["scalars"] - a["scalars"] == 3 * len(pairs) and b["launches"] - a["launches"] == 1    # ONE launch for all three columns
    want_t, want_c = single(gpu, ks, rs)
    assert (trk == want_t).all() and (com == want_c).all()
    for i in (0, 1, 20, 79, 200, len(pairs) - 1):                                 # ... and the model directly
        assert (bytes(trk[i]), bytes(com[i])) == fm.tracker_bytes(oracle, coracle, *pairs[i]), i
    assert bytes(trk[0]) == INF48 + INF48 and bytes(com[0]) == INF48              # k = r = 0
    assert bytes(trk[-1][48:]) == oracle.compress(oracle.G1)
    # rs null: r = 1, the fork's initial trackers (G, k G); k_commitments_out null: two columns, the same trackers
    t1, c1 = gpu.whisk_compute_trackers_batch(ks, None)
    assert (t1[:, :48] == np.frombuffer(oracle.compress(oracle.G1), dtype=np.uint8)).all()
    assert (t1[:, 48:] == com).all() and (c1 == com).all()
    a = gpu.stat_fbase()
    t2, c2 = gpu.whisk_compute_trackers_batch(ks, rs, commitments=False)
    b = gpu.stat_fbase()
    assert c2 is None and (t2 == trk).all()
    assert b["scalars"] - a["scalars"] == 2 * len(pairs) and b["launches"] - a["launches"] == 1
    t3, _ = gpu.whisk_compute_trackers_batch(ks, None, commitments=False)
    assert (t3 == t1).all()


@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_sizes_and_passes(gpu, n):
    ks, rs = random_limbs(n, n), random_limbs(1000 + n, n)
    ks[n // 2] = 0
    want_t, want_c = single(gpu, ks, rs)
    trk, com = gpu.whisk_compute_trackers_batch(ks, rs)
    assert (trk == want_t).all() and (com == want_c).all()
    with gpu.knobs(FBASE_PASS=256):                                               # 85 members a pass (128 without commitments)
        a = gpu.stat_fbase()
        trk, com = gpu.whisk_compute_trackers_batch(ks, rs)
        b = gpu.stat_fbase()
        assert (trk == want_t).all() and (com == want_c).all()
        assert b["launches"] - a["launches"] == (n + 84) // 85 and b["scalars"] - a["scalars"] == 3 * n
        trk, _ = gpu.whisk_compute_trackers_batch(ks, rs, commitments=False)
        assert (trk == want_t).all()
        assert gpu.stat_fbase()["launches"] - b["launches"] == (n + 127) // 128


@pytest.mark.parametrize("n", [21845, 21846])
def test_across_the_normalisations_wide_lane_rule(gpu, oracle, coracle, n):
    """3 n = 65,535 and 65,538: below and beyond kNormalizeWideMin.  64 sampled members, the first and the last against
    the model; ALL of them on the GPU: one key shared by every member owns every tracker, that key plus one owns none."""
    k = random_limbs(77, 1)[0]
    ks = np.tile(k, (n, 1))
    rs = random_limbs(n, n)
    rs[5] = 0                                                                      # a tracker of two infinities
    trk, com = gpu.whisk_compute_trackers_batch(ks, rs)
    kv = oracle.fr_from_mont_limbs([int(v) for v in k])
    sample = sorted({0, n - 1, 5} | {int(i) for i in np.random.default_rng(n).integers(0, n, size=64)})
    for i in sample:
        rv = oracle.fr_from_mont_limbs([int(v) for v in rs[i]])
        assert (bytes(trk[i]), bytes(com[i])) == fm.tracker_bytes(oracle, coracle, kv, rv), i
    assert (com == com[0]).all()
    k1 = np.array(oracle.fr_to_mont_limbs(kv + 1), dtype=np.uint64)
    owned = gpu.whisk_find_own_trackers(trk, np.stack([k, k1]))
    assert (owned[0] == gpu.TRACKER_OWNED).all()
    not_owned = owned[1] == gpu.TRACKER_NOT_OWNED
    assert not_owned.sum() == n - 1 and owned[1][5] == gpu.TRACKER_OWNED           # infinity | infinity is everybody's


def test_the_life_cycle(gpu):
    """300 members: trackers and commitments, proofs over them, all accepted; two commitments swapped: exactly those two
    rejected."""
    n = 300
    ks, rs, blinders = random_limbs(1, n), random_limbs(2, n), random_limbs(3, n)
    a = gpu.stat_fbase()
    trk, com = gpu.whisk_compute_trackers_batch(ks, rs)
    b = gpu.stat_fbase()
    assert (b["scalars"] - a["scalars"], b["launches"] - a["launches"]) == (3 * n, 1)
    trackers, comms = [bytes(t) for t in trk], [bytes(c) for c in com]
    proofs, results = gpu.whisk_generate_tracker_proof_batch(trackers, ks, blinders=blinders)
    assert (results == gpu.OK).all()
    proofs = [bytes(p) for p in proofs]
    assert (gpu.whisk_is_valid_tracker_proof_batch(trackers, comms, proofs) == 1).all()
    comms[7], comms[201] = comms[201], comms[7]
    ok = gpu.whisk_is_valid_tracker_proof_batch(trackers, comms, proofs)
    assert sorted(np.nonzero(ok != 1)[0].tolist()) == [7, 201] and (ok[[7, 201]] == 0).all()
