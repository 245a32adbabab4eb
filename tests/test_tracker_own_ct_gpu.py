"""curdle_whisk_find_own_trackers_ex / _device_ex under CURDLE_TRACKER_OWN_CONSTANT_TIME on the GPU: the verdict bytes of
k_tracker_own_ct equal, byte for byte, the big-integer model of tests/tracker_own_model.py and the call without the
flag; the flattened (key, tracker) layout is held at waves and blocks that straddle keys, at the launch rule's cuts and
at the pass boundary; and the counters prove which kernel ran.  The plant (five keys, the distinct trackers around them
and the model's verdicts) is that of tests/test_tracker_own_gpu.py."""
import threading

import numpy as np
import pytest

import tracker_own_model as tom
from test_tracker_own_ct_model import PASS, launches
from test_tracker_own_gpu import Plant, limbs

pytestmark = pytest.mark.gpu

CT = 1


def stats(gpu):
    return {"ct": gpu.stat_tracker_own_ct(), "own": gpu.stat_tracker_own(), "mul": gpu.stat_g1_mul_ct(), "norm": gpu.stat_normalize()}


def moved(before, after, which):
    return {k: after[which][k] - before[which][k] for k in before[which]}


@pytest.fixture(scope="module")
def plant(gpu, oracle):
    return Plant(oracle)


@pytest.fixture(scope="module")
def nine(oracle, plant):
    """Nine keys: the plant's five and four strangers, with the model's verdicts over the plant's distinct trackers."""
    rand = oracle.Rand(2509)
    keys = plant.keys + [rand.get_fr() for _ in range(4)]
    assert len(set(keys)) == 9
    extra = np.array(tom.matrix(oracle, plant.distinct, keys[5:]), dtype=np.uint8)
    table = np.concatenate([plant.table, extra])
    assert table.shape == (9, len(plant.distinct)) and not (extra[:, :11] != 0).any()
    return limbs(oracle, keys), table


@pytest.fixture(scope="module")
def families(gpu, oracle):
    keys, trackers = tom.case_families(oracle)
    want = np.array(tom.matrix(oracle, [t for _, t in trackers], [k for _, k in keys]), dtype=np.uint8)
    return keys, trackers, want


def call(gpu, plant, idx, m, flags=CT):
    return gpu.whisk_find_own_trackers(plant.records[idx], plant.key_limbs[:m], flags=flags)


def test_every_case_family_as_a_matrix(gpu, oracle, families):
    keys, trackers, want = families
    assert want.shape == (66, 28)
    kl = limbs(oracle, [k for _, k in keys])
    recs = [t for _, t in trackers]
    before = stats(gpu)
    got = gpu.whisk_find_own_trackers(recs, kl, flags=CT)
    after = stats(gpu)
    assert got.shape == want.shape and got.dtype == np.uint8
    for j, i in zip(*np.nonzero(got != want)):
        raise AssertionError((keys[j][0], trackers[i][0], int(got[j, i]), int(want[j, i])))
    assert (got == gpu.whisk_find_own_trackers(recs, kl)).all()               # the call without the flag
    assert (got == gpu.whisk_find_own_trackers(recs, kl, flags=0)).all()
    assert moved(before, after, "ct") == {"pairs": 66 * 28, "launches": 1, "bad": 66 * 10}
    kn, tn = [n for n, _ in keys], [n for n, _ in trackers]
    # k = r - 1, whose last step discards P + (-P), owns its tracker; k = 0 owns exactly the krG = infinity ones
    assert got[kn.index("r-1"), tn.index("honest r-1")] == tom.OWNED
    assert got[kn.index("lambda"), tn.index("honest lambda")] == tom.OWNED
    for name in ("lambda", "random 0"):                                         # equal x, opposite y
        assert got[kn.index(name), tn.index("krG negated, " + name)] == tom.NOT_OWNED
    assert got[kn.index("r-lambda"), tn.index("krG negated, lambda")] == tom.OWNED
    assert (got[:, tn.index("rG = krG = infinity")] == tom.OWNED).all()
    assert (got[:, tn.index("rG = infinity, krG finite")] == tom.NOT_OWNED).all()
    assert got[:, tn.index("krG = infinity")].tolist() == [tom.OWNED if k == 0 else tom.NOT_OWNED for _, k in keys]
    assert sum(n.startswith("bad ") for n in tn) == 10 and (got[:, [n.startswith("bad ") for n in tn]] == tom.BAD).all()


@pytest.mark.parametrize("position", ["rG", "krG"])
def test_bad_records_between_honest_neighbours(gpu, families, plant, position):
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
    before = stats(gpu)
    got = gpu.whisk_find_own_trackers(row, plant.key_limbs[:m], flags=CT)
    after = stats(gpu)
    for i, d in enumerate(idx):
        if d is None:
            assert (got[:, i] == gpu.TRACKER_BAD).all(), i            # the column, for every key
        else:
            assert (got[:, i] == plant.table[:m, d]).all(), i         # the neighbours are exact
    assert moved(before, after, "ct") == {"pairs": len(row) * m, "launches": 1, "bad": 5 * m}
    assert after["own"] == before["own"]


@pytest.mark.parametrize("m", [1, 2, 3, 5])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 514])
def test_edges_of_waves_blocks_and_keys(gpu, plant, n, m):
    """Ownership at the four corners of the matrix and nowhere else.  n = 65 with m = 5 and n = 257 with m = 3 are the
    shapes at which a wave, and a block, hold the end of one key's row and the start of the next."""
    idx = plant.corners(n, m, 100 * n + m)
    want = plant.want(idx, m)
    planted = {(0, 0), (m - 1, n - 1)} | ({(m - 1, 1), (0, n - 2)} if n >= 4 else set())
    if n == 1:
        planted = {(m - 1, 0)}
    assert {(int(j), int(i)) for j, i in zip(*np.nonzero(want))} == planted
    got = call(gpu, plant, idx, m)
    assert got.shape == (m, n) and (got == want).all(), np.argwhere(got != want)[:8]


@pytest.mark.parametrize("n,m", [(300, 5), (64, 9)])
def test_launch_splitting_through_the_knob(gpu, plant, nine, n, m):
    key_limbs, table = nine
    idx = plant.corners(n, min(m, 5), n)
    idx[n // 2] = plant.bad_at(0)
    want = table[:m][:, idx]
    counts = {}
    for v in (256, 512, 1000):
        with gpu.knobs(TRACKER_OWN_PAIRS=v):
            before = stats(gpu)
            got = gpu.whisk_find_own_trackers(plant.records[idx], key_limbs[:m], flags=CT)
            after = stats(gpu)
        assert (got == want).all(), (v, np.argwhere(got != want)[:8])
        counts[v] = moved(before, after, "ct")["launches"]
        assert counts[v] == launches(n, m, v), v
        assert moved(before, after, "ct")["bad"] == m and moved(before, after, "ct")["pairs"] == n * m
    assert counts == ({256: 10, 512: 5, 1000: 3} if n == 300 else {256: 3, 512: 2, 1000: 1})


def test_two_launches_under_the_default_knob(gpu, plant):
    """A full pass of 2^17 trackers holds two keys a launch, so three keys are two launches; only the planted pairs
    are non-zero."""
    n, m = PASS, 3
    assert launches(n, m) == 2
    idx = plant.corners(n, m, 17)
    want = plant.want(idx, m)
    assert {(int(j), int(i)) for j, i in zip(*np.nonzero(want))} == {(0, 0), (m - 1, n - 1), (m - 1, 1), (0, n - 2)}
    before = stats(gpu)
    got = call(gpu, plant, idx, m)
    after = stats(gpu)
    assert moved(before, after, "ct") == {"pairs": n * m, "launches": 2, "bad": 0}
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
    before = stats(gpu)
    got = call(gpu, plant, idx, 1)
    assert moved(before, stats(gpu), "ct") == {"pairs": n, "launches": 2, "bad": 2}
    assert (got == want).all(), np.argwhere(got != want)[:8]
    # ... and the bad record on the far side of the boundary
    idx[PASS], idx[PASS - 2] = plant.bad_at(1), plant.filled(1, 1)[0]
    got = call(gpu, plant, idx, 1)
    assert (got == plant.want(idx, 1)).all() and got[0, PASS] == gpu.TRACKER_BAD and got[0, PASS - 1] == gpu.TRACKER_OWNED


@pytest.mark.parametrize("off", [0, 1, 3])
def test_resident_arrays_on_a_callers_stream_and_on_the_librarys(gpu, plant, off):
    import torch
    n, m = 130, 3
    idx = plant.corners(n, m, 900 + off)
    idx[70] = plant.bad_at(1)
    want = plant.want(idx, m)
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
            before = stats(gpu)
            gpu.whisk_find_own_trackers_device(d_trk.data_ptr(), n, d_ks.data_ptr(), m, d_out.data_ptr() + guard + off,
                                               stream=s.cuda_stream if own_stream else None, flags=CT)
            assert moved(before, stats(gpu), "ct") == {"pairs": n * m, "launches": 1, "bad": m}
            out = d_out.cpu().numpy()
        torch.cuda.synchronize()
        assert (out[:guard + off] == 0x5A).all() and (out[guard + off + m * n:] == 0x5A).all()
        assert (out[guard + off:guard + off + m * n].reshape(m, n) == want).all()
        assert (d_ks.cpu().numpy() == ks.numpy()).all()                     # the caller's keys are not touched


def test_the_counters_say_which_kernel_ran(gpu, plant):
    n, m = 70, 4
    idx = plant.corners(n, m, 70)
    want = plant.want(idx, m)
    before = stats(gpu)
    assert (call(gpu, plant, idx, m) == want).all()
    mid = stats(gpu)
    assert moved(before, mid, "ct") == {"pairs": m * n, "launches": 1, "bad": 0}
    assert mid["own"] == before["own"] and mid["mul"] == before["mul"] and mid["norm"] == before["norm"]
    for flags in (None, 0):                                                    # the reverse
        assert (call(gpu, plant, idx, m, flags=flags) == want).all()
        after = stats(gpu)
        assert moved(mid, after, "own") == {"pairs": m * n, "launches": 1, "bad": 0}
        assert after["ct"] == mid["ct"] and after["mul"] == mid["mul"] and after["norm"] == mid["norm"]
        mid = after


def test_beside_an_msm_and_a_tracker_verification(gpu, oracle, coracle, plant):
    n, m = 300, 5
    idx = plant.corners(n, m, 55)
    want = plant.want(idx, m)
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
                results.append(call(gpu, plant, idx, m))
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
