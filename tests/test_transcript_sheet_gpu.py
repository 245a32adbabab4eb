"""The sheet kernel of the batched Merlin transcripts (csrc/transcript_sheet_kernels.hip: a STROBE state spread over
the lanes of a wave half, two members per wave) behind knob TRANSCRIPT_SHEET: challenges, exported states and status
bytes bit for bit against the model (tests/merlin_model.py), the host twin and the lane kernel -- at sizes that leave
a wave half empty, on the recorded retry cases (members that share a wave need different numbers of tries), across a
resumption from any implementation to any other, from four threads at once, through the tracker batches that hash on
the device and through the Whisk shuffle batch's prelude; and curdle_stat_transcript_paths, which says which kernel
hashed.

Not provoked here: the status byte after 256 rejected draws of one challenge (probability 0.547^256).  The bound in
k_transcript_sheet's retry loop (the status set on the half that still needs a draw, the other half keeping its state
and its challenge) is run by tests/test_transcript_status_gpu.py, which lowers it through the test hook
TRANSCRIPT_MAX_TRIES and puts every pair of the retry fixture's members on the two halves of a wave."""
import os
import threading

import numpy as np
import pytest

import merlin_model as mm
from test_merlin_model import retry_fixture
from test_tracker_batch_gpu import pool  # noqa: F401  (the module-scoped fixture of that file)
from test_tracker_hash_gpu import mixed, run_flag, run_resident, want_for
from test_transcript_batch_gpu import data_for, model_reference, small_programs

pytestmark = pytest.mark.gpu

SHEET, LANE = 1, 0


def moved(gpu, before):
    after = gpu.stat_transcript_paths()
    return after["lane"] - before["lane"], after["sheet"] - before["sheet"]


@pytest.mark.parametrize("k", [1, 2, 3, 63, 64, 65, 257])
def test_boundary_programs_and_small_prelude_equal_the_model(gpu, k):
    for name, (program, label) in small_programs().items():
        data, want_ch, want_st = model_reference(name, program, label)
        for knob in (SHEET, LANE):
            with gpu.knobs(TRANSCRIPT_SHEET=knob):
                p0 = gpu.stat_transcript_paths()
                ch, st, status = gpu.transcript_batch(program, data[:k], label=label)
                ch2, none, status2 = gpu.transcript_batch(program, data[:k], label=label, want_states=False)
                assert moved(gpu, p0) == ((0, 2 * k) if knob == SHEET else (2 * k, 0)), (name, knob)
            assert not status.any() and not status2.any(), (name, knob)
            assert (ch == want_ch[:k]).all(), (name, knob, "challenges")
            assert (st == want_st[:k]).all(), (name, knob, "states")
            assert none is None and (ch2 == want_ch[:k]).all(), (name, knob, "challenges without states")


def test_whisk_prelude_equals_the_host_twin(gpu):
    program = mm.prelude_program(124)
    data = data_for(program, 257, seed=124)
    want_ch, want_st, want_status = gpu.transcript_batch(program, data, label=mm.PRELUDE_LABEL, host=True, nthreads=8)
    assert not want_status.any()
    wide = np.concatenate([data, np.full((257, 13), 0xA5, dtype=np.uint8)], axis=1)
    with gpu.knobs(TRANSCRIPT_SHEET=SHEET):
        p0 = gpu.stat_transcript_paths()
        ch, st, status = gpu.transcript_batch(program, data, label=mm.PRELUDE_LABEL)
        # a stride wider than the program reads: the rest of a row is not hashed
        wch, wst, wstatus = gpu.transcript_batch(program, wide, label=mm.PRELUDE_LABEL)
        assert moved(gpu, p0) == (0, 514)
    assert not status.any() and (ch == want_ch).all() and (st == want_st).all()
    assert not wstatus.any() and (wch == want_ch).all() and (wst == want_st).all()


def test_retry_fixture_members_draw_their_recorded_challenges(gpu):
    fx = retry_fixture()
    tries = fx["tries"]
    # members 2 i and 2 i + 1 share a wave; they must need different numbers of tries for some challenge
    pairs = [(tries[i] != tries[i + 1]).any() for i in range(0, len(tries) - 1, 2)]
    assert sum(pairs) >= 2 and (tries[:-1] != tries[1:]).any(axis=1).sum() >= 2
    data = np.array([list(mm.retry_member_data(int(s))) for s in fx["seeds"]], dtype=np.uint8)
    for knob in (SHEET, LANE):
        with gpu.knobs(TRANSCRIPT_SHEET=knob):
            ch, st, status = gpu.transcript_batch(mm.RETRY_PROGRAM, data, label=mm.RETRY_LABEL)
            # ... and one place on, so that every member meets its other neighbour
            ch1, st1, status1 = gpu.transcript_batch(mm.RETRY_PROGRAM, data[1:], label=mm.RETRY_LABEL)
        assert not status.any() and (ch == fx["challenges"]).all(), knob
        assert not status1.any() and (ch1 == fx["challenges"][1:]).all() and (st1 == st[1:]).all(), knob
        if knob == SHEET:
            sheet_st = st
    assert (sheet_st == st).all()


def test_resume_across_kernels(gpu):
    program = mm.prelude_program(8) + [(mm.TR_APPEND, b"more", 2, 33), (mm.TR_CHALLENGES, b"z", 3, 0), (mm.TR_APPEND, b"end", 1, 170)]
    data = data_for(program, 70, seed=5)
    whole_ch, whole_st, _ = gpu.transcript_batch(program, data, label=mm.PRELUDE_LABEL, host=True, nthreads=4)

    def run(impl, *args, **kw):
        if impl == "host":
            return gpu.transcript_batch(*args, host=True, **kw)
        with gpu.knobs(TRANSCRIPT_SHEET=SHEET if impl == "sheet" else LANE):
            return gpu.transcript_batch(*args, **kw)
    for impl in ("lane", "sheet"):
        ch, st, _ = run(impl, program, data, label=mm.PRELUDE_LABEL)
        assert (ch == whole_ch).all() and (st == whole_st).all(), impl
    for cut in (1, 2, 3, 4):
        c1 = mm.consumed_bytes(program[:cut])
        for first in ("host", "lane", "sheet"):
            ch1, st1, s1 = run(first, program[:cut], data[:, :c1], label=mm.PRELUDE_LABEL)
            for second in ("host", "lane", "sheet"):
                if second == first:
                    continue
                ch2, st2, s2 = run(second, program[cut:], data[:, c1:], init_states=st1)
                assert not s1.any() and not s2.any()
                assert (np.concatenate([ch1, ch2], axis=1) == whole_ch).all(), (cut, first, second)
                assert (st2 == whole_st).all(), (cut, first, second)


def test_path_counters(gpu):
    program = mm.prelude_program(4)
    k = 37
    data = data_for(program, k)

    def call(**kw):
        p0, s0 = gpu.stat_transcript_paths(), gpu.stat_transcript()
        gpu.transcript_batch(program, data, label=mm.PRELUDE_LABEL, **kw)
        return moved(gpu, p0), gpu.stat_transcript()["members"] - s0["members"]
    with gpu.knobs(TRANSCRIPT_SHEET=SHEET):
        assert call() == ((0, k), k)
        with gpu.knobs(TRANSCRIPT_LANES=64):          # the sheet knob decides when it is set
            assert call() == ((0, k), k)
    with gpu.knobs(TRANSCRIPT_SHEET=LANE):
        assert call() == ((k, 0), k)
    with gpu.knobs(TRANSCRIPT_LANES=64):
        assert call() == ((k, 0), k)
    (lane, sheet), members = call()
    assert sorted((lane, sheet)) == [0, k] and members == k
    assert call(host=True) == ((0, 0), 0)


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

    with gpu.knobs(TRANSCRIPT_SHEET=SHEET):
        p0 = gpu.stat_transcript_paths()
        threads = [threading.Thread(target=caller, args=(j,)) for j in range(4)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert moved(gpu, p0) == (0, 5 * (65 + 33 + 130 + 257))
    assert not errors, errors


@pytest.mark.parametrize("k", [1, 65, 130])
def test_tracker_batches_hash_on_the_sheet_kernel(gpu, pool, k):  # noqa: F811
    members, expected = mixed(pool, k, seed=1000 + k)
    if k == 130:                                       # tampered members on both halves of a wave, and the last member
        hon, cases = pool
        for at, name in ((0, "S+1"), (1, "A other"), (129, "S+1")):
            members[at], expected[at] = cases[name]
    want = want_for(gpu, members)
    assert want == expected
    got = {}
    for knob in (LANE, SHEET):
        with gpu.knobs(TRANSCRIPT_SHEET=knob):
            p0 = gpu.stat_transcript_paths()
            flag = run_flag(gpu, members, gpu.TRACKER_HASH_DEVICE)
            p1 = gpu.stat_transcript_paths()
            resident = run_resident(gpu, members)
            assert moved(gpu, p0) == ((0, 2 * k) if knob == SHEET else (2 * k, 0))
            assert moved(gpu, p1) == ((0, k) if knob == SHEET else (k, 0))
        got[knob] = (flag.tolist(), resident.tolist())
    assert got[SHEET] == got[LANE] == (want, want)


def test_whisk_batch_preludes_on_the_sheet_kernel(gpu):
    """curdle_whisk_is_valid_shuffle_proof_batch on k = 40 in chunks of 16 with the bad members that
    tests/test_transcript_batch_gpu.py plants (a point swapped between T and U, a proof scalar altered, another point
    as M, a proof that does not parse): GPU_PRELUDE=1 under TRANSCRIPT_SHEET=1 gives the bits of GPU_PRELUDE=0, and all
    40 preludes are hashed by the sheet kernel."""
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
        p0 = gpu.stat_transcript_paths()
        with gpu.knobs(GPU_PRELUDE=0):
            off = run()
        p1 = gpu.stat_transcript_paths()
        with gpu.knobs(GPU_PRELUDE=1, TRANSCRIPT_SHEET=SHEET):
            on = run()
        p2 = gpu.stat_transcript_paths()
    assert off == expect and on == off
    assert p1 == p0
    assert (p2["lane"] - p1["lane"], p2["sheet"] - p1["sheet"]) == (0, k)
