"""The batched Merlin transcripts without a GPU: the pure-Python model (tests/merlin_model.py) against hashlib and
Merlin's published vector, the host's transcript and the host twin curdle_transcript_batch_host against the model, the
position invariant that lets one compiled tape serve every member, continuation through exported states, the refusals
of the interface, and the committed retry fixture against the model."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import merlin_model as mm
from conftest import ROOT


def _data(program, k, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(k, mm.consumed_bytes(program)), dtype=np.uint8)


def _against_model(cm, program, label, data, ch, st, status, members=None):
    for i in (range(len(data)) if members is None else members):
        mc, _, mst, mstatus, _ = mm.run_program(program, bytes(data[i]), label)
        assert status[i] == mstatus == 0, i
        assert bytes(ch[i].reshape(-1)) == b"".join(mc), ("challenges of member", i)
        assert bytes(st[i]) == mst, ("state of member", i)


@pytest.mark.parametrize("n", [0, 1, 135, 136, 137, 1000])
def test_model_permutation_under_sha3_and_shake_padding_equals_hashlib(n):
    msg = (bytes(range(251)) * 4)[:n]
    assert mm.sponge(msg, 136, 0x06, 32) == hashlib.sha3_256(msg).digest()
    assert mm.sponge(msg, 136, 0x1F, 300) == hashlib.shake_256(msg).digest(300)      # 300: the squeeze permutes too


def test_model_reproduces_merlins_published_vector():
    # merlin's "equivalence_simple", the vector of tests/test_protocol_host.py
    out = mm.merlin_test_vector(b"test protocol", b"some label", b"some data", b"challenge", 32)
    assert out.hex() == "d5a21972d0d5fe320c0d263fac7fffb8145aa640af6e9bca177c03c7efcf0615"


def test_model_equals_the_hosts_merlin_on_every_message_length_to_400(cm):
    msg = hashlib.shake_256(b"lengths").digest(400)
    for n in range(401):
        assert cm.merlin_test_vector(b"proto", b"lbl", msg[:n], b"chal", 40) == mm.merlin_test_vector(b"proto", b"lbl", msg[:n], b"chal", 40), n


@pytest.mark.parametrize("ell", [4, 8])
def test_host_twin_equals_the_model_on_the_prelude(cm, ell):
    program = mm.prelude_program(ell)
    data = _data(program, 6, ell)
    ch, st, status = cm.transcript_batch(program, data, label=mm.PRELUDE_LABEL, host=True, nthreads=3)
    assert ch.shape == (6, ell, 32)
    _against_model(cm, program, mm.PRELUDE_LABEL, data, ch, st, status)


def test_boundary_programs_hit_their_events_and_host_twin_equals_the_model(cm):
    programs = mm.boundary_programs()
    assert sorted(programs) == sorted(mm.BOUNDARY_EVENTS)
    for event, program in programs.items():
        _, events, _ = mm.positions(program, mm.BOUNDARY_LABEL)
        hits = [e for e in events if e[0] == event]
        assert hits, event
        if event == "header_ends_at_166_no_forced_f":
            assert any(e[1] == mm.FLAG_I | mm.FLAG_A | mm.FLAG_C for e in hits)      # a PRF's header
        data = _data(program, 4, 7)
        ch, st, status = cm.transcript_batch(program, data, label=mm.BOUNDARY_LABEL, host=True)
        _against_model(cm, program, mm.BOUNDARY_LABEL, data, ch, st, status)
        # the events are those of the hashing run too, not of the position replay alone
        _, _, _, _, m = mm.run_program(program, bytes(data[0]), mm.BOUNDARY_LABEL)
        assert any(e[0] == event for e in m.strobe.events), event


def test_positions_depend_on_the_program_alone():
    """pos and pos_begin after a challenge try are (32, 0) whatever came before, after a whole GetAndAppendChallenge
    under a label of L bytes (72 + L, 39 + L) -- (90, 57) for the prelude -- and the end position of a program is the
    same with real hashing (members that retry) as in the position replay (first draw accepted)."""
    for ell in (4, 5, 8, 31):
        assert mm.positions(mm.prelude_program(ell), mm.PRELUDE_LABEL)[0] == (90, 57, mm.FLAG_A)
    for L in (0, 1, 18, 32):
        for filler in (0, 50, 131, 165, 166, 167):
            prog = [(mm.TR_APPEND, b"fill", 1, filler), (mm.TR_CHALLENGES, b"c" * L, 1, 0)]
            assert mm.positions(prog, b"p")[0] == (72 + L, 39 + L, mm.FLAG_A), (L, filler)
            m = mm.Merlin(b"p", hashing=False)
            m.append_message(b"fill", bytes(filler))
            m.challenge_bytes(b"c" * L, 32)
            assert (m.strobe.pos, m.strobe.pos_begin) == (32, 0), (L, filler)
    program = mm.prelude_program(4) + [(mm.TR_APPEND, b"tail", 3, 5)]
    want = mm.positions(program, mm.PRELUDE_LABEL)[0]
    retried = 0
    for seed in range(6):
        data = bytes(_data(program, 1, seed)[0])
        _, tries, st, _, _ = mm.run_program(program, data, mm.PRELUDE_LABEL)
        retried += max(tries) > 1
        assert (st[200], st[201], st[202]) == want
    assert retried


def test_a_program_run_whole_equals_two_calls_through_states(cm):
    program = mm.prelude_program(4) + [(mm.TR_APPEND, b"more", 2, 33), (mm.TR_CHALLENGES, b"z", 3, 0)]
    data = _data(program, 5, 3)
    whole_ch, whole_st, _ = cm.transcript_batch(program, data, label=mm.PRELUDE_LABEL, host=True)
    for cut in (1, 2, 3):
        first, second = program[:cut], program[cut:]
        c1 = mm.consumed_bytes(first)
        ch1, st1, s1 = cm.transcript_batch(first, data[:, :c1], label=mm.PRELUDE_LABEL, host=True)
        ch2, st2, s2 = cm.transcript_batch(second, data[:, c1:], init_states=st1, host=True, nthreads=2)
        assert not s1.any() and not s2.any()
        assert (np.concatenate([ch1, ch2], axis=1) == whole_ch).all() and (st2 == whole_st).all(), cut
    # the model continues from an exported state as well
    c1 = mm.consumed_bytes(program[:2])
    _, _, mst, _, _ = mm.run_program(program[:2], bytes(data[0, :c1]), mm.PRELUDE_LABEL)
    mc, _, mst2, _, _ = mm.run_program(program[2:], bytes(data[0, c1:]), state=mst)
    assert mst2 == bytes(whole_st[0]) and b"".join(mc) == bytes(whole_ch[0, 4:].reshape(-1))


def refused_calls(cm):
    """(what, kwargs for _raw_call) of every malformed call of the interface."""
    good = [(mm.TR_APPEND, b"a", 2, 10), (mm.TR_CHALLENGES, b"c", 1, 0)]
    states = np.zeros((2, 208), dtype=np.uint8)
    states[:, 200] = 5
    moved = states.copy()
    moved[1, 200] = 6
    past = states.copy()
    past[:, 200] = 166
    return [
        ("an unknown op", dict(program=[(3, b"a", 1, 4)])),
        ("op 0", dict(program=[(0, b"a", 1, 4)])),
        ("label_len above 32", dict(program=good, label_len=33)),
        ("data_stride below what the program reads", dict(program=good, stride=19)),
        ("both a label and states", dict(program=good, states=states, label=b"x")),
        ("neither a label nor states", dict(program=good, label=None)),
        ("states at different positions", dict(program=good, states=moved, label=None)),
        ("a state whose position is past the rate", dict(program=good, states=past, label=None)),
        ("more challenges than the limit", dict(program=[(mm.TR_CHALLENGES, b"c", cm.TRANSCRIPT_MAX_CHALLENGES + 1, 0)])),
        ("more bytes per member than the limit", dict(program=[(mm.TR_APPEND, b"a", 2, cm.TRANSCRIPT_MAX_BYTES // 2 + 1)], stride=1 << 21, k=0)),
        ("more members than the limit", dict(program=good, k=cm.TRANSCRIPT_MAX_MEMBERS + 1, null_data=False, fake=True)),
    ]


def raw_call(cm, host, program, label=b"t", states=None, stride=None, label_len=None, k=2, fake=False, null_data=False):
    """The C entry point itself, so that a malformed call can be made at all.  Returns the return code."""
    steps, consumed, n_ch = cm.transcript_steps(program)
    if label_len is not None:
        steps[0].label_len = label_len
    stride = consumed if stride is None else stride
    kk = 2 if fake else k
    data = np.zeros(max(1, kk * max(stride, consumed)), dtype=np.uint8)
    ch = np.zeros(max(1, kk * n_ch * 32), dtype=np.uint8)
    status = np.zeros(max(1, kk), dtype=np.uint8)
    args = (label, None if states is None else cm._ptr(states), steps, len(program), cm._ptr(data), stride, k, cm._ptr(ch), None, cm._ptr(status))
    return cm._transcript_batch_host(*args, 1) if host else cm._transcript_batch(*args)


def test_malformed_calls_are_refused(cm):
    for what, kw in refused_calls(cm):
        assert raw_call(cm, True, **kw) == cm.EINVAL, what
        assert cm.last_error(), what
    good = [(mm.TR_APPEND, b"a", 2, 10), (mm.TR_CHALLENGES, b"c", 1, 0)]
    assert raw_call(cm, True, good) == cm.OK
    assert raw_call(cm, True, good, k=0) == cm.OK                     # k = 0 is CURDLE_OK
    # the device entry point refuses the same calls before it looks for a device ...
    for what, kw in refused_calls(cm):
        assert raw_call(cm, False, **kw) == cm.EINVAL, what
    assert raw_call(cm, False, good, k=0) == cm.OK
    # ... and without one a well-formed call fails loudly: the host twin is no fallback
    if not cm.device_available():
        assert raw_call(cm, False, good) == cm.ENODEV
        assert "no HIP device" in cm.last_error()


def test_step_struct_matches_the_header(cm):
    assert C.sizeof(cm._TranscriptStep) == 48
    text = open(os.path.join(ROOT, "include", "curdle_msm.h")).read()
    for name, value in (("STATE_SIZE", cm.TRANSCRIPT_STATE_SIZE), ("MAX_TRIES", cm.TRANSCRIPT_MAX_TRIES), ("MAX_MEMBERS", cm.TRANSCRIPT_MAX_MEMBERS),
                        ("MAX_BYTES", cm.TRANSCRIPT_MAX_BYTES), ("MAX_CHALLENGES", cm.TRANSCRIPT_MAX_CHALLENGES), ("MAX_MESSAGES", cm.TRANSCRIPT_MAX_MESSAGES)):
        assert "#define CURDLE_TRANSCRIPT_%s %d " % (name, value) in text.replace("\n", " \n"), name
    assert mm.MAX_TRIES == cm.TRANSCRIPT_MAX_TRIES and mm.STATE_SIZE == cm.TRANSCRIPT_STATE_SIZE


def retry_fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "transcript_retry_cases.npz"))


def test_retry_fixture_holds_its_cases_and_agrees_with_the_model_and_the_host_twin(cm):
    fx = retry_fixture()
    seeds, challenges, tries, kind = fx["seeds"], fx["challenges"], fx["tries"], fx["kind"]
    assert challenges.shape == (len(seeds), 8, 32) and tries.shape == (len(seeds), 8)
    for bit in (1, 2, 4):
        assert (kind & bit).astype(bool).sum() >= 3
    assert (tries.max(axis=1)[(kind & 4) != 0] >= 6).all()
    assert all((challenges[i, :, 0] == 0x73).any() for i in np.nonzero(kind & 2)[0])
    r_bytes = mm.R.to_bytes(32, "big")
    assert all(bytes(c) < r_bytes for c in challenges.reshape(-1, 32))
    # a sample against the model: one member of each kind
    for bit in (1, 2, 4):
        i = int(np.nonzero(kind & bit)[0][0])
        mc, mt, _, status, m = mm.run_program(mm.RETRY_PROGRAM, mm.retry_member_data(int(seeds[i])), mm.RETRY_LABEL)
        assert status == 0 and mt == list(tries[i]) and b"".join(mc) == bytes(challenges[i].reshape(-1))
        if bit == 1:
            rejected = [e[1] for e in m.strobe.events if e[0] == "rejected_draw" and e[1][0] == 0x73]
            assert rejected and all(r_bytes <= d for d in rejected)
    # every member against the host twin
    data = np.array([list(mm.retry_member_data(int(s))) for s in seeds], dtype=np.uint8)
    ch, _, status = cm.transcript_batch(mm.RETRY_PROGRAM, data, label=mm.RETRY_LABEL, host=True, nthreads=2)
    assert not status.any() and (ch == challenges).all()
