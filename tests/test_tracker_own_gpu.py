"""curdle_whisk_find_own_trackers / _device on the GPU: owned[j, i] for m keys and n trackers equals, byte for byte,
what the big-integer model of tests/tracker_own_model.py says (pinned against the single call, host code, by
tests/test_tracker_own_abi.py) and what the single call answers.  The pool of distinct trackers is small and is tiled:
the kernel does not care that trackers repeat, and the model's verdicts are computed once per distinct (key, tracker)."""
import threading

import numpy as np
import pytest

import tracker_own_model as tom

pytestmark = pytest.mark.gpu

WAVE, BLOCK, PASS = 16, 64, 1 << 17      # trackers of one key per wave, per block, and per decoding pass
DEFAULT_PAIRS = 1 << 18


def limbs(oracle, values):
    return np.array([oracle.fr_to_mont_limbs(v % oracle.R) for v in values], dtype=np.uint64).reshape(-1, 4)


def launches(n, m, pairs=DEFAULT_PAIRS):
    """The launch rule of csrc/tracker_own_api.hip: per pass, every key's trackers padded to whole waves, the tracker
    dimension cut into chunks of min(that, pairs) quads, one chunk of up to pairs / chunk (<= 65,535) keys a launch."""
    pairs = max(WAVE, pairs // WAVE * WAVE)
    total = 0
    for lo in range(0, n, PASS):
        cnt = min(PASS, n - lo)
        tc = min(-(-cnt // WAVE) * WAVE, pairs)
        keys = min(65535, max(1, pairs // tc))
        total += -(-cnt // tc) * -(-m // keys)
    return total


class Plant:
    """Five keys, the distinct trackers around them and the model's verdict for every (key, distinct tracker)."""

    def __init__(self, oracle):
        o = self.o = oracle
        rand = o.Rand(2024)
        self.keys = [rand.get_fr() for _ in range(5)]
        bases = [o.scalar_mul(rand.get_fr(), o.G1) for _ in range(2)]
        strangers = [rand.get_fr() for _ in range(6)]

        def tracker(k, base):
            return o.compress(base) + o.compress(tom.product(o, k, base))

        self.filler = [tracker(k, bases[j % 2]) for j, k in enumerate(strangers)]          # owned by none of the keys
        self.honest = [tracker(k, bases[j % 2]) for j, k in enumerate(self.keys)]          # honest[j] is key j's
        x_ge_p = bytearray(o.P.to_bytes(48, "big"))
        x_ge_p[0] |= 0x80
        self.bad = [bytes(x_ge_p) + self.filler[0][48:], self.filler[1][:48] + b"\x01" * 48]
        self.distinct = self.filler + self.honest + self.bad
        self.table = np.array(tom.matrix(o, self.distinct, self.keys), dtype=np.uint8)     # [5][13]
        self.records = np.frombuffer(b"".join(self.distinct), dtype=np.uint8).reshape(-1, 96)
        self.key_limbs = limbs(o, self.keys)
        assert self.table[:, :6].sum() == 0 and (self.table[:, 6:11] == np.eye(5, dtype=np.uint8)).all()
        assert (self.table[:, 11:] == tom.BAD).all()

    def honest_of(self, j):
        return len(self.filler) + j

    def bad_at(self, j):
        return len(self.filler) + len(self.honest) + j

    def filled(self, n, seed):
        return np.random.default_rng(seed).integers(len(self.filler), size=n)

    def corners(self, n, m, seed):
        """Filler everywhere; the first key owns the first tracker and the last key the last one, and (from four
        trackers on) the last key the second and the first key the last but one: both keys own something at both ends
        of the tracker dimension, and nobody owns anything else."""
        idx = self.filled(n, seed)
        if n >= 4:
            idx[1], idx[n - 2] = self.honest_of(m - 1), self.honest_of(0)
        idx[0] = self.honest_of(0)
        idx[n - 1] = self.honest_of(m - 1)
        return idx

    def call(self, gpu, idx, m):
        return gpu.whisk_find_own_trackers(self.records[idx], self.key_limbs[:m])

    def want(self, idx, m):
        return self.table[:m][:, idx]


@pytest.fixture(scope="module")
def plant(gpu, oracle):
    return Plant(oracle)


@pytest.fixture(scope="module")
def families(gpu, oracle):
    keys, trackers = tom.case_families(oracle)
    want = np.array(tom.matrix(oracle, [t for _, t in trackers], [k for _, k in keys]), dtype=np.uint8)
    return keys, trackers, want


def test_every_case_family_as_a_matrix(gpu, oracle, families):
    keys, trackers, want = families
    kl = limbs(oracle, [k for _, k in keys])
    got = gpu.whisk_find_own_trackers([t for _, t in trackers], kl)
    assert got.shape == want.shape and got.dtype == np.uint8
    for j, i in zip(*np.nonzero(got != want)):
        raise AssertionError((keys[j][0], trackers[i][0], int(got[j, i]), int(want[j, i])))
    for j, (kname, _) in enumerate(keys):
        for i, (tname, t) in enumerate(trackers):
            try:
                one = tom.OWNED if gpu.whisk_is_own_tracker(t, kl[j]) else tom.NOT_OWNED
            except gpu.CurdleError as e:
                assert e.code == gpu.EINVAL
                one = tom.BAD
            assert got[j, i] == one, (kname, tname)
    # both exceptional endings of the final addition occur: opposite operands (an owned pair whose k rG is finite) and
    # equal operands (k rG against the negated krG)
    kn, tn = [n for n, _ in keys], [n for n, _ in trackers]
    assert got[kn.index("lambda"), tn.index("honest lambda")] == tom.OWNED
    assert got[kn.index("random 0"), tn.index("honest random 0")] == tom.OWNED
    for name in ("lambda", "random 0"):
        t = dict(trackers)["krG negated, " + name]
        k = dict(keys)[name]
        assert tom.product(oracle, k, tom.decompress(oracle, t[:48])) == oracle.neg(tom.decompress(oracle, t[48:]))
        assert got[kn.index(name), tn.index("krG negated, " + name)] == tom.NOT_OWNED
    assert (got[:, tn.index("rG = krG = infinity")] == tom.OWNED).all()
    assert (got[:, tn.index("rG = infinity, krG finite")] == tom.NOT_OWNED).all()
    assert got[:, tn.index("krG = infinity")].tolist() == [tom.OWNED if k == 0 else tom.NOT_OWNED for _, k in keys]


@pytest.mark.parametrize("position", ["rG", "krG"])
def test_bad_records_between_honest_neighbours(gpu, oracle, families, plant, position):
    _, trackers, _ = families
    bad = [t for n, t in trackers if n.startswith("bad %s: " % position)]
    assert len(bad) == 5
    m = 3
    row, idx = [], []
    for j, rec in enumerate(bad):
        row += [plant.distinct[plant.honest_of(j % m)], rec]
        idx += [plant.honest_of(j % m), None]
    row.append(plant.distinct[plant.honest_of(m - 1)])
    idx.append(plant.honest_of(m - 1))
    before = gpu.stat_tracker_own()
    got = gpu.whisk_find_own_trackers(row, plant.key_limbs[:m])
    after = gpu.stat_tracker_own()
    for i, d in enumerate(idx):
        if d is None:
            assert (got[:, i] == gpu.TRACKER_BAD).all(), i            # the column, for every key
        else:
            assert (got[:, i] == plant.table[:m, d]).all(), i         # the neighbours are exact
    assert after["bad"] - before["bad"] == 5 * m
    assert after["pairs"] - before["pairs"] == len(row) * m
    assert after["launches"] - before["launches"] == 1


@pytest.mark.parametrize("m", [1, 2, 3, 5])
@pytest.mark.parametrize("n", [1, WAVE - 1, WAVE, WAVE + 1, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 2])
def test_edges_of_waves_blocks_and_keys(gpu, plant, n, m):
    idx = plant.corners(n, m, 100 * n + m)
    want = plant.want(idx, m)
    planted = {(0, 0), (m - 1, n - 1)} | ({(m - 1, 1), (0, n - 2)} if n >= 4 else set())
    if n == 1:
        planted = {(m - 1, 0)}
    assert {(int(j), int(i)) for j, i in zip(*np.nonzero(want))} == planted
    got = plant.call(gpu, idx, m)
    assert got.shape == (m, n) and (got == want).all(), np.argwhere(got != want)[:8]


@pytest.mark.parametrize("n,m", [(17, 5), (64, 3)])
def test_launch_splitting_through_the_knob(gpu, plant, n, m):
    idx = plant.corners(n, m, n)
    idx[n // 2] = plant.bad_at(0)
    want = plant.want(idx, m)
    counts = {}
    for v in (None, 16, 32, 48, 1000):
        with gpu.knobs(**({} if v is None else {"TRACKER_OWN_PAIRS": v})):
            before = gpu.stat_tracker_own()
            got = plant.call(gpu, idx, m)
            after = gpu.stat_tracker_own()
        assert (got == want).all(), v
        counts[v] = after["launches"] - before["launches"]
        assert counts[v] == launches(n, m, DEFAULT_PAIRS if v is None else v), v
        assert after["bad"] - before["bad"] == m
    assert counts == ({None: 1, 16: 10, 32: 5, 48: 5, 1000: 1} if n == 17 else {None: 1, 16: 12, 32: 6, 48: 6, 1000: 1})


def test_two_launches_under_the_default_knob(gpu, oracle, plant):
    """65 DISTINCT keys: the five plant keys at rows 0, 31, 62 (the first launch's last), 63 and 64 (the second
    launch), sixty random keys between them; only the three planted pairs are non-zero."""
    n, m = 4100, 65
    assert launches(n, m) == 2
    rows = {0: 0, 31: 1, 62: 2, 63: 3, 64: 4}                 # row of the call -> plant key
    rand = oracle.Rand(4100)
    keys = [plant.keys[rows[j]] if j in rows else rand.get_fr() for j in range(m)]
    assert len(set(keys)) == m
    idx = plant.filled(n, 41)
    planted = {(0, 0), (63, n - 1), (64, 2049)}               # (row, tracker)
    for j, t in planted:
        idx[t] = plant.honest_of(rows[j])
    used = sorted(set(idx.tolist()))
    table = np.zeros((m, len(plant.distinct)), dtype=np.uint8)
    table[:, used] = np.array(tom.matrix(oracle, [plant.distinct[d] for d in used], keys), dtype=np.uint8)
    want = table[:, idx]
    assert {(int(j), int(i)) for j, i in zip(*np.nonzero(want))} == planted
    before = gpu.stat_tracker_own()
    got = gpu.whisk_find_own_trackers(plant.records[idx], limbs(oracle, keys))
    after = gpu.stat_tracker_own()
    assert after["launches"] - before["launches"] == 2 and after["pairs"] - before["pairs"] == n * m
    assert (got == want).all(), np.argwhere(got != want)[:8]


def test_the_tracker_pass_boundary(gpu, plant):
    n = PASS + 1
    assert launches(n, 1) == 2
    idx = plant.filled(n, 7)
    idx[PASS - 1], idx[PASS] = plant.honest_of(0), plant.honest_of(0)
    idx[PASS - 2], idx[0] = plant.bad_at(0), plant.bad_at(1)
    idx[5] = plant.honest_of(0)
    want = plant.want(idx, 1)
    assert (want[0, [0, 5, PASS - 2, PASS - 1, PASS]] == [2, 1, 2, 1, 1]).all() and int((want != 0).sum()) == 5
    got = plant.call(gpu, idx, 1)
    assert (got == want).all(), np.argwhere(got != want)[:8]
    # ... and the bad record on the far side of the boundary
    idx[PASS], idx[PASS - 2] = plant.bad_at(1), plant.filled(1, 1)[0]
    got = plant.call(gpu, idx, 1)
    assert (got == plant.want(idx, 1)).all() and got[0, PASS] == gpu.TRACKER_BAD and got[0, PASS - 1] == gpu.TRACKER_OWNED


@pytest.mark.parametrize("off", [0, 1, 3])
def test_resident_arrays_on_a_callers_stream_and_on_the_librarys(gpu, plant, off):
    import torch
    n, m = 130, 3
    idx = plant.corners(n, m, 900 + off)
    idx[70] = plant.bad_at(1)
    host = plant.call(gpu, idx, m)
    assert (host == plant.want(idx, m)).all()
    trk = torch.from_numpy(plant.records[idx].reshape(-1).copy()).pin_memory()
    ks = torch.from_numpy(plant.key_limbs[:m].view(np.int64).copy()).pin_memory()
    guard = 16
    for own_stream in (True, False):
        s = torch.cuda.Stream() if own_stream else None
        with torch.cuda.stream(s) if own_stream else torch.cuda.stream(torch.cuda.current_stream()):
            d_trk = torch.zeros_like(trk, device="cuda:0")
            d_ks = torch.zeros_like(ks, device="cuda:0")
            d_out = torch.full((guard + off + m * n + guard,), 0x5A, dtype=torch.uint8, device="cuda:0")
            d_trk.copy_(trk, non_blocking=True)          # written on the stream immediately before the call
            d_ks.copy_(ks, non_blocking=True)
            if not own_stream:
                torch.cuda.synchronize()
            gpu.whisk_find_own_trackers_device(d_trk.data_ptr(), n, d_ks.data_ptr(), m, d_out.data_ptr() + guard + off,
                                               stream=s.cuda_stream if own_stream else None)
            out = d_out.cpu().numpy()
        torch.cuda.synchronize()
        assert (out[:guard + off] == 0x5A).all() and (out[guard + off + m * n:] == 0x5A).all()
        assert (out[guard + off:guard + off + m * n].reshape(m, n) == host).all()
        assert (d_ks.cpu().numpy() == ks.numpy()).all()                     # the caller's keys are not touched


def test_beside_an_msm_and_a_tracker_verification(gpu, oracle, coracle, plant):
    n, m = 300, 5
    idx = plant.corners(n, m, 55)
    want = plant.want(idx, m)
    # an honest opening proof of plant key 0's tracker, verified in batches of 40 beside the search
    k = plant.keys[0]
    t = plant.distinct[plant.honest_of(0)]
    proofs, res = gpu.whisk_generate_tracker_proof_batch([t], limbs(oracle, [k]), blinders=limbs(oracle, [12345]))
    assert res.tolist() == [gpu.OK]
    kc = oracle.compress(oracle.scalar_mul(k, oracle.G1))
    members = ([t] * 40, [kc] * 40, [proofs[0].tobytes()] * 40)
    k0, q0 = oracle.Rand(1).get_frs(2)
    pts = coracle.points_walk(k0, q0, 2048)
    sc = np.random.default_rng(6).integers(0, 1 << 62, size=(2048, 4), dtype=np.uint64)
    msm_want = gpu.msm_g1(pts, sc)
    errors, results = [], []
    stop = threading.Event()

    def search():
        try:
            for _ in range(3):
                results.append(plant.call(gpu, idx, m))
        except Exception as e:  # noqa: BLE001 - reported below
            errors.append(e)

    def beside():
        try:
            while True:  # at least once, and for as long as the search runs
                assert (gpu.msm_g1(pts, sc) == msm_want).all()
                assert gpu.whisk_is_valid_tracker_proof_batch(*members).tolist() == [1] * 40
                if stop.is_set():
                    break
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    other = threading.Thread(target=beside)
    other.start()
    mine = threading.Thread(target=search)
    mine.start()
    mine.join()
    stop.set()
    other.join()
    assert not errors, errors
    assert len(results) == 3 and all((got == want).all() for got in results)


def test_the_owned_pairs_open_their_trackers(gpu, oracle, plant):
    """What the search finds goes to the generator: every owned (k, tracker) pair yields a proof the verifier accepts."""
    n, m = 65, 5
    idx = plant.corners(n, m, 100 * n + m)
    got = plant.call(gpu, idx, m)
    pairs = [(int(j), int(i)) for j, i in zip(*np.nonzero(got == gpu.TRACKER_OWNED))]
    assert sorted(pairs) == [(0, 0), (0, n - 2), (m - 1, 1), (m - 1, n - 1)]
    trackers = [plant.records[idx[i]].tobytes() for _, i in pairs]
    ks = [plant.keys[j] for j, _ in pairs]
    proofs, res = gpu.whisk_generate_tracker_proof_batch(trackers, limbs(oracle, ks),
                                                         blinders=limbs(oracle, [1000 + j for j in range(len(pairs))]))
    assert res.tolist() == [gpu.OK] * len(pairs)
    kcs = [oracle.compress(oracle.scalar_mul(k, oracle.G1)) for k in ks]
    assert gpu.whisk_is_valid_tracker_proof_batch(trackers, kcs, [p.tobytes() for p in proofs]).tolist() == [1] * len(pairs)
    # a pair the search did NOT report does not open: the proof of a stranger's tracker is rejected
    other = plant.records[idx[2]].tobytes()
    proofs, res = gpu.whisk_generate_tracker_proof_batch([other], limbs(oracle, [ks[0]]), blinders=limbs(oracle, [77]))
    assert res.tolist() == [gpu.OK]
    assert gpu.whisk_is_valid_tracker_proof_batch([other], [kcs[0]], [proofs[0].tobytes()]).tolist() == [0]
