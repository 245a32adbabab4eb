"""curdle_transcript_batch on the GPU (csrc/transcript_kernels.hip): challenges, exported states and status bytes bit
for bit against the pure-Python model (tests/merlin_model.py) at small shapes and against the host twin
(curdle_transcript_batch_host) at the Whisk shape; at every members-per-wave layout the launch has (knob
TRANSCRIPT_LANES: the library's own choice, which is one member per wave at these sizes, full waves of 64, and a
count that leaves the last wave ragged); continuation across the two implementations; concurrent callers; the
counters; the refusals."""
import threading

import numpy as np
import pytest

import merlin_model as mm
from test_merlin_model import raw_call, refused_calls, retry_fixture

pytestmark = pytest.mark.gpu

K_MAX = 257
LANES = (None, 64, 5)
_reference = {}


def data_for(program, k, seed=11):
    return np.random.default_rng(seed).integers(0, 256, size=(k, mm.consumed_bytes(program)), dtype=np.uint8)


def model_reference(name, program, label):
    """(data, challenges, states) of K_MAX members by the model, computed once; a batch of k members is its first k rows."""
    if name not in _reference:
        data = data_for(program, K_MAX)
        ch = np.zeros((K_MAX, mm.n_challenges(program), 32), dtype=np.uint8)
        st = np.zeros((K_MAX, mm.STATE_SIZE), dtype=np.uint8)
        for i in range(K_MAX):
            mc, _, mst, status, _ = mm.run_program(program, bytes(data[i]), label)
            assert status == 0
            ch[i] = np.frombuffer(b"".join(mc), dtype=np.uint8).reshape(-1, 32)
            st[i] = np.frombuffer(mst, dtype=np.uint8)
        for a in (data, ch, st):
            a.setflags(write=False)
        _reference[name] = (data, ch, st)
    return _reference[name]


def small_programs():
    progs = {"prelude4": (mm.prelude_program(4), mm.PRELUDE_LABEL)}
    for event, program in mm.boundary_programs().items():
        progs[event] = (program, mm.BOUNDARY_LABEL)
    return progs


@pytest.mark.parametrize("k", [1, 63, 64, 65, 257])
def test_boundary_programs_and_small_prelude_equal_the_model(gpu, k):
    for name, (program, label) in small_programs().items():
        data, want_ch, want_st = model_reference(name, program, label)
        for lanes in LANES:
            with gpu.knobs(TRANSCRIPT_LANES=lanes):
                ch, st, status = gpu.transcript_batch(program, data[:k], label=label)
            assert not status.any(), (name, lanes)
            assert (ch == want_ch[:k]).all(), (name, lanes, "challenges")
            assert (st == want_st[:k]).all(), (name, lanes, "states")
            # without states the challenges are the same
            ch2, none, _ = gpu.transcript_batch(program, data[:k], label=label, want_states=False)
            assert none is None and (ch2 == want_ch[:k]).all()


def test_whisk_prelude_equals_the_host_twin_and_the_model(gpu):
    program = mm.prelude_program(124)
    data = data_for(program, 257, seed=124)
    want_ch, want_st, want_status = gpu.transcript_batch(program, data, label=mm.PRELUDE_LABEL, host=True, nthreads=8)
    assert not want_status.any()
    for i in (0, 128, 256):
        mc, _, mst, _, _ = mm.run_program(program, bytes(data[i]), mm.PRELUDE_LABEL)
        assert bytes(want_ch[i].reshape(-1)) == b"".join(mc) and bytes(want_st[i]) == mst
    for lanes in LANES:
        with gpu.knobs(TRANSCRIPT_LANES=lanes):
            ch, st, status = gpu.transcript_batch(program, data, label=mm.PRELUDE_LABEL)
        assert not status.any()
        assert (ch == want_ch).all() and (st == want_st).all(), lanes
    # a stride wider than the program reads: the rest of a row is not hashed
    wide = np.concatenate([data, np.full((257, 13), 0xA5, dtype=np.uint8)], axis=1)
    ch, st, _ = gpu.transcript_batch(program, wide, label=mm.PRELUDE_LABEL)
    assert (ch == want_ch).all() and (st == want_st).all()


def test_retry_fixture_members_draw_their_recorded_challenges(gpu):
    fx = retry_fixture()
    data = np.array([list(mm.retry_member_data(int(s))) for s in fx["seeds"]], dtype=np.uint8)
    for lanes in LANES:
        with gpu.knobs(TRANSCRIPT_LANES=lanes):
            ch, _, status = gpu.transcript_batch(mm.RETRY_PROGRAM, data, label=mm.RETRY_LABEL)
        assert not status.any() and (ch == fx["challenges"]).all(), lanes


def test_resume_across_implementations(gpu):
    program = mm.prelude_program(8) + [(mm.TR_APPEND, b"more", 2, 33), (mm.TR_CHALLENGES, b"z", 3, 0), (mm.TR_APPEND, b"end", 1, 170)]
    data = data_for(program, 70, seed=5)
    whole_ch, whole_st, _ = gpu.transcript_batch(program, data, label=mm.PRELUDE_LABEL, host=True, nthreads=4)
    dev_ch, dev_st, _ = gpu.transcript_batch(program, data, label=mm.PRELUDE_LABEL)
    assert (dev_ch == whole_ch).all() and (dev_st == whole_st).all()
    for cut in (1, 2, 3, 4):
        c1 = mm.consumed_bytes(program[:cut])
        for first_host in (False, True):
            ch1, st1, s1 = gpu.transcript_batch(program[:cut], data[:, :c1], label=mm.PRELUDE_LABEL, host=first_host)
            ch2, st2, s2 = gpu.transcript_batch(program[cut:], data[:, c1:], init_states=st1, host=not first_host)
            assert not s1.any() and not s2.any()
            assert (np.concatenate([ch1, ch2], axis=1) == whole_ch).all(), (cut, first_host)
            assert (st2 == whole_st).all(), (cut, first_host)


def test_four_threads_calling_at_once(gpu):
    programs = [(mm.prelude_program(4), mm.PRELUDE_LABEL, 65), (mm.prelude_program(8), mm.PRELUDE_LABEL, 33),
                (mm.boundary_programs()["le32_straddles"], mm.BOUNDARY_LABEL, 130), (mm.RETRY_PROGRAM, mm.RETRY_LABEL, 257)]
    want = []
    for j, (program, label, k) in enumerate(programs):
        data = data_for(program, k, seed=40 + j)
        want.append((data,) + gpu.transcript_batch(program, data, label=label, host=True, nthreads=4))
    errors = []

    def caller(j):
        program, label, _ = programs[j]
        data, want_ch, want_st, _ = want[j]
        try:
            for _ in range(5):
                ch, st, status = gpu.transcript_batch(program, data, label=label)
                if status.any() or not (ch == want_ch).all() or not (st == want_st).all():
                    errors.append("thread %d: a wrong result" % j)
        except Exception as e:      # noqa: BLE001 -- reported below, on the test's thread
            errors.append("thread %d: %r" % (j, e))

    threads = [threading.Thread(target=caller, args=(j,)) for j in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


def test_stat_counters_count_device_members_only(gpu):
    program = mm.prelude_program(4)
    data = data_for(program, 37)
    before = gpu.stat_transcript()
    gpu.transcript_batch(program, data, label=mm.PRELUDE_LABEL, host=True)
    assert gpu.stat_transcript() == before
    gpu.transcript_batch(program, data, label=mm.PRELUDE_LABEL)
    gpu.transcript_batch(program, data[:5], label=mm.PRELUDE_LABEL)
    after = gpu.stat_transcript()
    assert after["members"] == before["members"] + 42 and after["handed_back"] == before["handed_back"]
    assert gpu.transcript_last_kernel_ms() > 0


def test_refusals_launch_nothing(gpu):
    good = [(mm.TR_APPEND, b"a", 2, 10), (mm.TR_CHALLENGES, b"c", 1, 0)]
    assert raw_call(gpu, False, good) == gpu.OK
    before, ms = gpu.stat_transcript(), gpu.transcript_last_kernel_ms()
    for what, kw in refused_calls(gpu):
        assert raw_call(gpu, False, **kw) == gpu.EINVAL, what
    assert raw_call(gpu, False, good, k=0) == gpu.OK
    # members x bytes beyond the device entry point's total
    big = [(mm.TR_APPEND, b"a", 1, gpu.TRANSCRIPT_MAX_BYTES)]
    assert raw_call(gpu, False, big, k=2048, fake=True) == gpu.EINVAL
    assert gpu.stat_transcript() == before and gpu.transcript_last_kernel_ms() == ms


def test_whisk_batch_takes_its_preludes_from_the_device_behind_the_knob(gpu):
    """curdle_whisk_is_valid_shuffle_proof_batch on k = 40 with bad members of the kinds tests/test_batch_rejects_gpu.py
    plants (a point swapped between T and U, a proof scalar altered, another point as M) and a proof that does not
    parse: knob GPU_PRELUDE on and off give the same bits; with it on every member's prelude is hashed on the device
    (chunks of 16, 16 and 8: curdle_stat_transcript counts 40 members), with it off none is."""
    import os
    from conftest import ROOT
    from test_batch_rejects_gpu import flip_last_scalar
    vectors = np.load(os.path.join(ROOT, "tests", "golden", "proof_vectors.npz"))
    pre, post, proof = (vectors[n].tobytes() for n in ("whisk_pre", "whisk_post", "whisk_proof"))
    pre_l = [pre[96 * i:96 * (i + 1)] for i in range(124)]
    post_l = [post[96 * i:96 * (i + 1)] for i in range(124)]
    crs = gpu.CRS(124, gpu.Rand(7))
    k = 40
    bad = {0: "swap", 15: "scalar", 16: "M", 17: "parse", 22: "swap", 39: "scalar"}
    pres, posts, proofs = [pre_l] * k, [list(post_l) for _ in range(k)], [proof] * k
    for i, kind in bad.items():
        if kind == "swap":
            posts[i][0] = post_l[0][48:] + post_l[0][:48]
        elif kind == "scalar":
            proofs[i] = flip_last_scalar(proof, 4536)
        elif kind == "M":
            proofs[i] = pre_l[3][:48] + proof[48:]
        else:
            proofs[i] = proof[:48] + b"\xff" * 48 + proof[96:]       # a record that is no field element
    expect = [i not in bad for i in range(k)]

    def run():
        return gpu.whisk_is_valid_shuffle_proof_batch(crs, pres, posts, proofs, gpu.Rand(9), nthreads=4)
    with gpu.knobs(BATCH_CHUNK=16):
        s0 = gpu.stat_transcript()
        off = run()
        s1 = gpu.stat_transcript()
        with gpu.knobs(GPU_PRELUDE=1):
            on = run()
        s2 = gpu.stat_transcript()
        with gpu.knobs(GPU_PRELUDE=0):
            off_again = run()
        s3 = gpu.stat_transcript()
    assert off == expect and on == off and off_again == off
    assert s1 == s0 and s3 == s2
    assert s2["members"] - s1["members"] == k and s2["handed_back"] == s1["handed_back"]
