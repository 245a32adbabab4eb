"""The checked batch verifier (curdle_verify_batch_checked): every member's 4 ell instance points and its M are
checked on the GPU in chunks beside the verification; a member with a bad point is reported and never verified, every
other member gets the bit curdle_verify_batch gives it.

The batch is the committed ell = 12 proof k = 40 times -- two groups at the default group size of 32, and no multiple
of the chunk (16 members: chunks of 16, 16 and 8) -- with these members altered:
  (a) Ss[7]  a torsion-plus-G1 point of the fixture              -> Ss[7], not in the subgroup
  (b) Us[11] a point of another curve                            -> Us[11], not on the curve
  (c) M      off the curve, Z != 1 (Y scaled by another Z)       -> M, not on the curve
  (d) M      torsion plus G1, Z != 1                             -> M, not in the subgroup
  (e) Rs[0]  a coordinate >= p                                   -> Rs[0], not a field element
  (f) Rs[1]  infinity: no fault; the verifier's own bit
  (g) good points, one bit of the proof's last scalar flipped: no fault; fails in its group, settled by member sums
  (h) Ts[3] off the curve, Ss[5] not in the subgroup, M bad      -> Ss[5]: the first in the order Rs, Ss, Ts, Us, M"""
import os
import threading

import numpy as np
import pytest

import jac_check_cases as jc
from conftest import ROOT
from test_proof_fixtures import instance

pytestmark = pytest.mark.gpu

K, ELL, BATCH_SEED = 40, 12, 9
GOLDEN = os.path.join(ROOT, "tests", "golden")
MEMBER = {"a": 2, "f": 5, "g": 9, "b": 17, "c": 20, "d": 33, "e": 35, "h": 39}       # every chunk has a fault
FAULTS = {"a": ("Ss", 7, 4), "b": ("Us", 11, 3), "c": ("M", 0, 3), "d": ("M", 0, 4), "e": ("Rs", 0, 2), "h": ("Ss", 5, 4)}


class Material:
    def __init__(self, gpu, oracle):
        v = np.load(os.path.join(GOLDEN, "proof_vectors.npz"))
        self.proof = v["ell12_proof"].tobytes()
        self.crs, self.Rs, self.Ss, self.Ts, self.Us, self.M = instance(gpu, ELL, int(v["ell12_seed"][0]))[:6]
        a, d = np.load(os.path.join(GOLDEN, "affine_check_points.npz")), np.load(os.path.join(GOLDEN, "decode_edge_records.npz"))
        rows = np.nonzero(d["status_no_subgroup"] == 0)[0]
        mine = np.nonzero(a["family"] == b"from_decoder")[0]
        j = next(j for j in range(len(rows)) if d["family"][rows[j]] == b"torsion_plus_g1")
        self.tq = a["points"][mine[j]]
        assert a["status_subgroup"][mine[j]] == 4 and a["status_no_subgroup"][mine[j]] == 0
        i = next(i for i in range(len(a["points"])) if a["family"][i] == b"other_curve") + 5
        self.other = a["points"][i]
        assert a["status_subgroup"][i] == 3
        i = next(i for i in range(len(a["points"])) if a["family"][i] == b"range")
        self.range = a["points"][i]
        assert a["status_subgroup"][i] == 2
        # M off the curve: X scaled by z, Y by another; M outside G1: the torsion-plus-G1 point scaled by z
        x, y = oracle.jac_from_mont_limbs([int(w) for w in self.M])
        z, z2 = jc.seeded("batch/z"), jc.seeded("batch/z2")
        self.M_off = np.array(jc.words_of(jc.mont(x * z * z), jc.mont(y * pow(z2, 3, oracle.P)), jc.mont(z)), dtype=np.uint64)
        tx, ty = oracle.affine_from_mont_limbs([int(w) for w in self.tq])
        self.M_tq = np.array(jc.words_of(*jc.scaled(tx, ty, z)), dtype=np.uint64)
        assert jc.model_status(self.M_off.tolist()) == 3 and jc.model_status(self.M_tq.tolist()) == 4
        assert jc.raw(self.M_off[12:]) != oracle.R_FP

    def honest(self):
        return [self.proof, self.Rs.copy(), self.Ss.copy(), self.Ts.copy(), self.Us.copy(), self.M.copy()]

    def altered(self, kind):
        it = self.honest()
        if kind == "a":
            it[2][7] = self.tq
        elif kind == "b":
            it[4][11] = self.other
        elif kind == "c":
            it[5] = self.M_off
        elif kind == "d":
            it[5] = self.M_tq
        elif kind == "e":
            it[1][0] = self.range
        elif kind == "f":
            it[1][1] = 0
        elif kind == "g":
            b = bytearray(self.proof)
            b[len(b) - 20] ^= 0x10
            it[0] = bytes(b)
        elif kind == "h":
            it[3][3], it[2][5], it[5] = self.other, self.tq, self.M_tq
        return it


@pytest.fixture(scope="module")
def mat(gpu, oracle):
    return Material(gpu, oracle)


def columns(items):
    return [list(c) for c in zip(*items)]


def batch_seeds(gpu, k):
    """The seed VerifyBatchCore draws for member i: the low 64 bits of the i-th element of the batch's Rand."""
    rand = gpu.Rand(BATCH_SEED)
    return [int(rand.get_fr()[0]) for _ in range(k)]


def single_checked(gpu, crs, item, seed):
    """curdle_verify_checked of one member: its bit, or the (vector, index, code) of the point it refuses."""
    try:
        return bool(gpu.verify_checked(crs, *item, gpu.Rand(seed)))
    except gpu.CurdleError as e:
        for code, text in ((2, "not a field element"), (3, "not on the curve"), (4, "not in the prime-order subgroup")):
            if e.code == gpu.EINVAL and text in e.msg and ": " in e.msg:
                where = e.msg.split(": ")[0]
                return ("M", 0, code) if where == "M" else (where[:2], int(where[3:-1]), code)
        return False                                             # malformed proof: rejected in a batch


def test_fault_cases(gpu, mat):
    items = [mat.honest() for _ in range(K)]
    for kind, i in MEMBER.items():
        items[i] = mat.altered(kind)
    want_faults = [None] * K
    for kind, f in FAULTS.items():
        want_faults[MEMBER[kind]] = f
    faulty = {MEMBER[kind] for kind in FAULTS}
    cols = columns(items)
    c0, d0 = gpu.stat_batch_checked(), gpu.stat_dacc_members()
    oks, faults = gpu.verify_batch_checked(mat.crs, *cols, gpu.Rand(BATCH_SEED), nthreads=1)
    c1, d1 = gpu.stat_batch_checked(), gpu.stat_dacc_members()
    print("oks", [int(b) for b in oks], "faults", [f for f in faults if f])
    assert faults == want_faults
    assert all(not oks[i] for i in faulty)
    # chunks of 16, 16 and 8 members; six members rejected by the check
    assert {k: c1[k] - c0[k] for k in c1} == {"batches": 1, "rejected": 6, "chunks": 3}, (c0, c1)
    # One worker: the first group is the first 32 members that REACH a group, and holds (g): one failed group, settled
    # by one pass of member sums over its 32 members; the few clean members left make the second group, which
    # passes.  Had (a)-(e) or (h) entered a group, 40 members would have made two failed groups.
    assert (d1["runs"] - d0["runs"], d1["members"] - d0["members"], d1["one_by_one"] - d0["one_by_one"]) == (1, 32, 0), (d0, d1)
    plain = gpu.verify_batch(mat.crs, *cols, gpu.Rand(BATCH_SEED), nthreads=1)
    seeds = batch_seeds(gpu, K)
    for i in range(K):
        one = single_checked(gpu, mat.crs, items[i], seeds[i])
        if i in faulty:
            assert one == want_faults[i], (i, one)
        else:
            assert oks[i] == plain[i] == one, (i, oks[i], plain[i], one)
    assert [i for i in range(K) if not oks[i]] == sorted(faulty | {MEMBER["f"], MEMBER["g"]})
    # ... and the same on many threads
    again = gpu.verify_batch_checked(mat.crs, *cols, gpu.Rand(BATCH_SEED), nthreads=8)
    assert again == (oks, faults)


def small_batch(mat, k, bad):
    items = [mat.honest() for _ in range(k)]
    for i, kind in bad.items():
        items[i] = mat.altered(kind)
    return items


def test_a_whole_chunk_of_bad_members(gpu, mat):
    """Chunks and groups of four: members 4..7 are one chunk and all bad, the other chunks are clean."""
    bad = {4: "a", 5: "c", 6: "e", 7: "h"}
    items = small_batch(mat, 12, bad)
    with gpu.knobs(BATCH_CHUNK=4, BATCH_GROUP=4):
        c0 = gpu.stat_batch_checked()
        for threads in (1, 8):
            oks, faults = gpu.verify_batch_checked(mat.crs, *columns(items), gpu.Rand(BATCH_SEED), nthreads=threads)
            assert faults == [FAULTS[bad[i]] if i in bad else None for i in range(12)]
            assert oks == [i not in bad for i in range(12)]
        c1 = gpu.stat_batch_checked()
    assert {k: c1[k] - c0[k] for k in c1} == {"batches": 2, "rejected": 8, "chunks": 6}


@pytest.mark.parametrize("kind", [None, "d", "g"])
def test_a_batch_of_one(gpu, mat, kind):
    items = small_batch(mat, 1, {0: kind} if kind else {})
    oks, faults = gpu.verify_batch_checked(mat.crs, *columns(items), gpu.Rand(BATCH_SEED), nthreads=4)
    assert (oks, faults) == ([kind is None], [FAULTS.get(kind)])


def test_an_empty_batch(gpu, mat):
    c0 = gpu.stat_batch_checked()
    assert gpu.verify_batch_checked(mat.crs, [], [], [], [], [], [], gpu.Rand(1)) == ([], [])
    assert gpu.stat_batch_checked() == c0


def test_honest_input_gives_the_unchecked_bits(gpu, mat):
    """The control: nothing to find, and bit for bit curdle_verify_batch -- on honest members and on members that are
    wrong but in G1 (another instance's vectors, a truncated proof)."""
    items = [mat.honest() for _ in range(K)]
    items[3][1], items[3][2] = items[3][2], items[3][1]
    items[21][0] = items[21][0][:-9]
    items[38] = mat.altered("g")
    cols = columns(items)
    for threads in (1, 8):
        oks, faults = gpu.verify_batch_checked(mat.crs, *cols, gpu.Rand(BATCH_SEED), nthreads=threads)
        assert faults == [None] * K
        assert oks == gpu.verify_batch(mat.crs, *cols, gpu.Rand(BATCH_SEED), nthreads=threads) == [i not in (3, 21, 38) for i in range(K)]


def fault_batch(mat):
    items = [mat.honest() for _ in range(K)]
    for kind, i in MEMBER.items():
        items[i] = mat.altered(kind)
    want = [None] * K
    for kind, f in FAULTS.items():
        want[MEMBER[kind]] = f
    bits = [i not in MEMBER.values() for i in range(K)]
    return columns(items), bits, want


def test_with_every_decode_context_taken(gpu, mat):
    """All four decode contexts held by point decodings in flight: the chunks' checks (and the proofs' decodings) go
    through MSM slots, and the answers are the same."""
    cols, bits, want = fault_batch(mat)
    blob = np.load(os.path.join(GOLDEN, "decode_edge_records.npz"))["records"][:8].tobytes()
    tickets = [gpu.g1_decompress_start(blob) for _ in range(4)]
    try:
        assert gpu.verify_batch_checked(mat.crs, *cols, gpu.Rand(BATCH_SEED), nthreads=8) == (bits, want)
    finally:
        for t in tickets:
            gpu.g1_decompress_finish(t, 8)


def test_with_every_msm_slot_taken_while_the_batch_runs(gpu, mat, oracle, coracle):
    """As many threads as there are workspace slots run MSMs back to back while the batch runs: its groups and its
    checks queue for slots with them, and the answers are the same."""
    cols, bits, want = fault_batch(mat)
    k, q = oracle.Rand(5).get_frs(2)
    pts = coracle.points_walk(k, q, 4096)
    sc = np.random.default_rng(5).integers(0, 1 << 62, size=(4096, 4), dtype=np.uint64)
    slots = gpu.msm_free_slots()
    stop, started, lowest, errors = threading.Event(), threading.Barrier(slots + 1), [slots], []

    def load():
        try:
            first = gpu.msm_g1(pts, sc)
            started.wait(timeout=60)
            while not stop.is_set():
                assert (gpu.msm_g1(pts, sc) == first).all()
        except Exception as e:                                   # noqa: BLE001  (reported below)
            errors.append(e)
            stop.set()

    threads = [threading.Thread(target=load) for _ in range(slots)]
    for t in threads:
        t.start()
    try:
        started.wait(timeout=60)
        for threads_n in (8, 1):
            got = gpu.verify_batch_checked(mat.crs, *cols, gpu.Rand(BATCH_SEED), nthreads=threads_n)
            lowest[0] = min(lowest[0], gpu.msm_free_slots())
            assert got == (bits, want)
    finally:
        stop.set()
        for t in threads:
            t.join()
    print("workspace slots: %d, free right after a batch: %d" % (slots, lowest[0]))
    assert not errors, errors


def test_two_contexts_on_one_gpu(gpu, mat):
    """curdle_init_devices with a repeated id: the batch is sharded over two contexts, each shard's check on its own;
    bits and faults are those of one context."""
    cols, bits, want = fault_batch(mat)
    v = np.load(os.path.join(GOLDEN, "proof_vectors.npz"))
    one = gpu.verify_batch_checked(mat.crs, *cols, gpu.Rand(BATCH_SEED), nthreads=8)
    assert one == (bits, want)
    gpu.init_devices([0, 0])
    try:
        assert gpu.device_count() == 2
        crs = instance(gpu, ELL, int(v["ell12_seed"][0]))[0]
        c0 = gpu.stat_batch_checked()
        two = gpu.verify_batch_checked(crs, *cols, gpu.Rand(BATCH_SEED), nthreads=8)
        c1 = gpu.stat_batch_checked()
    finally:
        gpu.set_device(-1)
        gpu.shutdown()
        gpu.init(0)
    assert gpu.device_count() == 1
    assert two == one
    # two shards of 20 members: chunks of 16 and 4 each
    assert {k: c1[k] - c0[k] for k in c1} == {"batches": 1, "rejected": 6, "chunks": 4}
