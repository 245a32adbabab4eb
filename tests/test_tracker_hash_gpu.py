"""The tracker batch with its transcripts hashed on the GPU (curdle_whisk_is_valid_tracker_proof_batch_ex with
CURDLE_TRACKER_HASH_DEVICE, and _batch_device over resident arrays): every member's answer equals the single call's
(curdle_whisk_is_valid_tracker_proof) on the same bytes and the host-hashed batch's -- over the case families of
tests/test_tracker_batch_gpu.py, S at its bounds, the sizes at which the packing of the transcript kernel and of the
gather kernel changes, one pass boundary, beside other callers, and on a caller's stream."""
import threading

import numpy as np
import pytest

import merlin_model as mm
from test_tracker_batch_gpu import pool, single  # noqa: F401  (pool: the module-scoped fixture of that file)

pytestmark = pytest.mark.gpu

_single = {}  # member -> the single call's answer, shared by every test here


def want_for(cm, members):
    out = []
    for m in members:
        if m not in _single:
            _single[m] = single(cm, m)
        out.append(_single[m])
    return out


def arrays(members):
    t, kc, p = zip(*members)
    return [np.frombuffer(b"".join(x), dtype=np.uint8) for x in (t, kc, p)]


def run_resident(cm, members, stream=0):
    import torch
    d = [torch.from_numpy(a.copy()).to("cuda:0") for a in arrays(members)]
    torch.cuda.synchronize()
    return cm.whisk_is_valid_tracker_proof_batch_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), len(members), stream)


def run_flag(cm, members, flags):
    t, kc, p = zip(*members)
    return cm.whisk_is_valid_tracker_proof_batch(list(t), list(kc), list(p), flags=flags)


def check_forms(cm, members, expected=None):
    """HASH_DEVICE and the resident form against HASH_HOST, the single call, and the expected values."""
    want = want_for(cm, members)
    host = run_flag(cm, members, cm.TRACKER_HASH_HOST)
    dev = run_flag(cm, members, cm.TRACKER_HASH_DEVICE)
    res = run_resident(cm, members)
    for got in (host, dev, res):
        assert got.dtype == np.int32 and len(got) == len(members)
    assert host.tolist() == want
    assert dev.tolist() == want
    assert res.tolist() == want
    if expected is not None:
        assert want == expected


def mixed(pool, k, seed):
    """k members from the 12 honest proofs, one in ten tampered (any case of the pool)."""
    hon, cases = pool
    rng = np.random.default_rng(seed)
    tampered = list(cases.values())
    members, expected = [], []
    for _ in range(k):
        if k > 1 and rng.random() < 0.1:
            m, want = tampered[rng.integers(len(tampered))]
        else:
            m, want = hon[rng.integers(len(hon))][0], 1
        members.append(m)
        expected.append(want)
    return members, expected


def test_every_case_between_honest_neighbours(gpu, pool):
    hon, cases = pool
    members, expected = [], []
    for j, (m, want) in enumerate(cases.values()):
        members += [hon[j % len(hon)][0], m]
        expected += [1, want]
    members.append(hon[-1][0])
    expected.append(1)
    assert sum(e == 1 for _, e in cases.values()) == 5 and sum(e == 0 for _, e in cases.values()) == 6
    check_forms(gpu, members, expected)


S_BOUNDS = {"r-1": (lambda R: R - 1, 0), "r": (lambda R: R, "E"), "r+1": (lambda R: R + 1, "E"),
            "2^256-1": (lambda R: (1 << 256) - 1, "E"), "0": (lambda R: 0, 0)}


@pytest.mark.parametrize("name", list(S_BOUNDS))
def test_s_at_its_bounds_alone_and_inside_a_wave(gpu, oracle, pool, name):
    hon, _ = pool
    value, want = S_BOUNDS[name]
    want = gpu.EINVAL if want == "E" else want
    t, kc, p = hon[0][0]
    m = (t, kc, p[:96] + value(oracle.R).to_bytes(32, "big"))
    check_forms(gpu, [m], [want])
    wave = [hon[j % len(hon)][0] for j in range(64)]
    for at in (0, 37, 63):
        members = list(wave)
        members[at] = m
        check_forms(gpu, members, [want if j == at else 1 for j in range(64)])


@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 128, 129, 256, 257, 4096, 4097, 8192, 8193])
def test_sizes_where_the_packing_changes(gpu, pool, k):
    members, expected = mixed(pool, k, seed=k)
    check_forms(gpu, members, expected)


def test_one_pass_boundary(gpu, pool):
    hon, cases = pool
    k = 65537
    members = [hon[j % len(hon)][0] for j in range(k)]
    expected = [1] * k
    for at, name in ((65535, "S+1"), (65536, "A other")):
        members[at], expected[at] = cases[name]
    check_forms(gpu, members, expected)


def test_counters(gpu, pool):
    members, _ = mixed(pool, 300, seed=3)
    s0 = gpu.stat_tracker()
    t0 = gpu.stat_transcript()
    run_flag(gpu, members, gpu.TRACKER_HASH_DEVICE)
    s1 = gpu.stat_tracker()
    assert s1["device"] - s0["device"] == 300 and s1["host"] == s0["host"]
    run_resident(gpu, members)
    s2 = gpu.stat_tracker()
    assert s2["device"] - s1["device"] == 300 and s2["host"] == s1["host"]
    # the tracker path hashes in its slot's own buffers: curdle_transcript_batch and its context saw none of it
    assert gpu.stat_transcript() == t0
    run_flag(gpu, members, gpu.TRACKER_HASH_HOST)
    s3 = gpu.stat_tracker()
    assert s3["host"] - s2["host"] == 300 and s3["device"] == s2["device"]
    assert s3["handed_back"] == s0["handed_back"]
    # the knob moves the plain call between the two
    with gpu.knobs(TRACKER_DEVICE_HASH=1):
        run_flag(gpu, members, None)
    s4 = gpu.stat_tracker()
    assert s4["device"] - s3["device"] == 300 and s4["host"] == s3["host"]
    with gpu.knobs(TRACKER_DEVICE_HASH=0):
        run_flag(gpu, members, gpu.TRACKER_HASH_DEFAULT)
    s5 = gpu.stat_tracker()
    assert s5["host"] - s4["host"] == 300 and s5["device"] == s4["device"]


def test_two_threads_beside_a_transcript_batch_and_an_msm(gpu, oracle, coracle, pool):
    batches = [mixed(pool, 700, seed=40 + t)[0] for t in range(2)]
    wants = [want_for(gpu, b) for b in batches]
    program = mm.prelude_program(16)
    data = np.random.default_rng(9).integers(0, 256, size=(300, mm.consumed_bytes(program)), dtype=np.uint8)
    want_ch, _, _ = gpu.transcript_batch(program, data, label=mm.PRELUDE_LABEL, host=True, nthreads=4)
    k, q = oracle.Rand(1).get_frs(2)
    n = 2048
    pts = coracle.points_walk(k, q, n)
    sc = np.random.default_rng(n).integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    sc[:, 3] &= np.uint64((1 << 62) - 1)
    want_msm = coracle.msm_pippenger(pts, sc, threads=4)
    results, errors = {}, []

    def guarded(name, fn):
        def run():
            try:
                results[name] = fn()
            except Exception as e:  # noqa: BLE001 - reported below
                errors.append((name, e))
        return threading.Thread(target=run)

    threads = [guarded(("tracker", t), lambda t=t: [run_flag(gpu, batches[t], gpu.TRACKER_HASH_DEVICE).tolist() for _ in range(3)])
               for t in range(2)]
    threads.append(guarded("transcript", lambda: [gpu.transcript_batch(program, data, label=mm.PRELUDE_LABEL)[0] for _ in range(3)]))
    threads.append(guarded("msm", lambda: [gpu.msm_g1(pts, sc) for _ in range(3)]))
    [t.start() for t in threads]
    [t.join() for t in threads]
    assert not errors, errors
    for t in range(2):
        assert results[("tracker", t)] == [wants[t]] * 3
    assert all((ch == want_ch).all() for ch in results["transcript"])
    assert all((got == want_msm).all() for got in results["msm"])


def test_a_callers_stream_orders_the_inputs(gpu, pool):
    import torch
    members, expected = mixed(pool, 1000, seed=8)
    want = want_for(gpu, members)
    assert want == expected
    host = [torch.from_numpy(a.copy()).pin_memory() for a in arrays(members)]
    dev = [torch.zeros(h.numel(), dtype=torch.uint8, device="cuda:0") for h in host]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        for d, h in zip(dev, host):
            d.copy_(h, non_blocking=True)  # written on the caller's stream immediately before the call
        got = gpu.whisk_is_valid_tracker_proof_batch_device(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(),
                                                            len(members), stream.cuda_stream)
    assert got.tolist() == want
    # and arrays that are not 8-byte aligned
    off = [torch.zeros(h.numel() + 3, dtype=torch.uint8, device="cuda:0") for h in host]
    for o, h in zip(off, host):
        o[3:].copy_(h)
    torch.cuda.synchronize()
    got = gpu.whisk_is_valid_tracker_proof_batch_device(off[0][3:].data_ptr(), off[1][3:].data_ptr(), off[2][3:].data_ptr(),
                                                        len(members), 0)
    assert got.tolist() == want
