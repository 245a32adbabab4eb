"""The status byte of the batched Merlin transcripts without a GPU: the host twin curdle_transcript_batch_host under the
test hook TRANSCRIPT_MAX_TRIES (host/knobs.h: the retry bound lowered to min(256, value)) on the recorded retry cases
(tests/golden/transcript_retry_cases.npz: 12 members, 8 challenges each, the tries of every challenge recorded), against
the model (tests/merlin_model.py, run_program(max_tries=...)).  A member gives up exactly when one of its challenges needs
more than T draws; the members at exactly T and at exactly T + 1 are the off-by-one test of the bound.  Also the knob's
edges: 0 and values above 256 are "not set", and curdle_plan_override knows the name with and without CURDLE_."""
import functools

import numpy as np
import pytest

import merlin_model as mm
from test_merlin_model import retry_fixture

BOUNDS = (2, 5, 6, 8, 9, None)      # None: the knob unset
# bound -> (members with status 1, status-0 members that hold a challenge of exactly `bound` tries): counted on the fixture
FIXTURE_COUNTS = {1: (12, 0), 2: (10, 2), 5: (6, 2), 6: (3, 3), 8: (1, 0), 9: (0, 1)}


@functools.lru_cache(maxsize=None)
def retry_reference():
    """The fixture's members run through the model once at the library's own bound: (data uint8[12, 32], challenges
    uint8[12, 8, 32], tries int[12, 8], states uint8[12, 208]), shared by the tests here and the GPU tests."""
    fx = retry_fixture()
    data = np.array([list(mm.retry_member_data(int(s))) for s in fx["seeds"]], dtype=np.uint8)
    ch, tries, st = [], [], []
    for row in data:
        mc, mt, mst, status, _ = mm.run_program(mm.RETRY_PROGRAM, bytes(row), mm.RETRY_LABEL)
        assert status == 0
        ch.append(np.frombuffer(b"".join(mc), dtype=np.uint8).reshape(8, 32))
        tries.append(mt)
        st.append(np.frombuffer(mst, dtype=np.uint8))
    ch, tries, st = np.array(ch), np.array(tries), np.array(st)
    assert (ch == fx["challenges"]).all() and (tries == fx["tries"]).all()
    for a in (data, ch, tries, st):
        a.setflags(write=False)
    return data, ch, tries, st


def gives_up(tries, bound):
    """The model's status bytes under a bound from the tries of every challenge."""
    return (np.asarray(tries) > bound).any(axis=-1)


def first_failing(tries_row, bound):
    """(index, tries) of the challenge at which a member gives up."""
    j = int(np.argmax(np.asarray(tries_row) > bound))
    return j, int(tries_row[j])


def test_the_fixture_holds_members_at_the_bound_and_one_past_it():
    _, _, tries, _ = retry_reference()
    for bound, (n_status, n_exact) in FIXTURE_COUNTS.items():
        status = gives_up(tries, bound)
        exact = [i for i in range(12) if not status[i] and (tries[i] == bound).any()]
        assert (int(status.sum()), len(exact)) == (n_status, n_exact), bound
    # both kinds of neighbour of the bound, so that a changed fixture cannot hollow the tests below out: a member that
    # keeps going with a challenge of exactly T tries, and one that gives up at a challenge of exactly T + 1
    for bound in (2, 5, 6):
        status = gives_up(tries, bound)
        assert any(not status[i] and (tries[i] == bound).any() for i in range(12)), bound
        assert any(status[i] and first_failing(tries[i], bound)[1] == bound + 1 for i in range(12)), bound
    assert first_failing(tries[11], 8) == (5, 9) and gives_up(tries, 8).tolist() == [False] * 11 + [True]
    assert tries[11, 5] == 9 and not gives_up(tries, 9).any()


@pytest.mark.parametrize("bound", [1, 2, 5, 6, 8, 9])
def test_model_under_a_bound_stops_at_the_first_challenge_that_gives_up(bound):
    data, ch, tries, st = retry_reference()
    for i in range(12):
        mc, mt, mst, status, _ = mm.run_program(mm.RETRY_PROGRAM, bytes(data[i]), mm.RETRY_LABEL, max_tries=bound)
        assert status == int(gives_up(tries[i], bound)), i
        if status:
            j, _ = first_failing(tries[i], bound)
            assert mt == tries[i, :j].tolist() and b"".join(mc) == bytes(ch[i, :j].reshape(-1)), i
        else:
            assert mt == tries[i].tolist() and b"".join(mc) == bytes(ch[i].reshape(-1)) and mst == bytes(st[i]), i


@pytest.mark.parametrize("bound", BOUNDS + (1,))
@pytest.mark.parametrize("nthreads", [1, 3])
def test_host_twin_gives_up_exactly_where_the_model_does(cm, bound, nthreads):
    data, want_ch, tries, want_st = retry_reference()
    want_status = gives_up(tries, 256 if bound is None else bound)
    with cm.knobs(TRANSCRIPT_MAX_TRIES=bound):
        ch, st, status = cm.transcript_batch(mm.RETRY_PROGRAM, data, label=mm.RETRY_LABEL, host=True, nthreads=nthreads)
        ch2, none, status2 = cm.transcript_batch(mm.RETRY_PROGRAM, data, label=mm.RETRY_LABEL, host=True, want_states=False)
    assert status.dtype == np.uint8 and set(status.tolist()) <= {0, 1}
    assert (status.astype(bool) == want_status).all() and (status2 == status).all()
    keep = ~want_status
    assert (ch[keep] == want_ch[keep]).all() and (st[keep] == want_st[keep]).all()
    assert none is None and (ch2[keep] == want_ch[keep]).all()
    if bound is None:
        assert keep.all()


def test_a_lowered_bound_does_not_outlive_its_block(cm):
    data, want_ch, _, want_st = retry_reference()
    with cm.knobs(TRANSCRIPT_MAX_TRIES=1):
        _, _, status = cm.transcript_batch(mm.RETRY_PROGRAM, data, label=mm.RETRY_LABEL, host=True)
        assert status.all()
    ch, st, status = cm.transcript_batch(mm.RETRY_PROGRAM, data, label=mm.RETRY_LABEL, host=True)
    assert not status.any() and (ch == want_ch).all() and (st == want_st).all()


@pytest.mark.parametrize("value", [0, 257, 10 ** 6])
def test_values_outside_1_to_256_behave_as_unset(cm, value):
    data, want_ch, tries, want_st = retry_reference()
    assert tries.max() == 9             # under a bound taken from `value` modulo anything small, somebody would give up
    with cm.knobs(TRANSCRIPT_MAX_TRIES=value):
        ch, st, status = cm.transcript_batch(mm.RETRY_PROGRAM, data, label=mm.RETRY_LABEL, host=True)
    assert not status.any() and (ch == want_ch).all() and (st == want_st).all()


def test_256_is_accepted_and_is_the_default(cm):
    data, want_ch, _, want_st = retry_reference()
    with cm.knobs(TRANSCRIPT_MAX_TRIES=256):
        ch, st, status = cm.transcript_batch(mm.RETRY_PROGRAM, data, label=mm.RETRY_LABEL, host=True)
    assert not status.any() and (ch == want_ch).all() and (st == want_st).all()
    assert cm.TRANSCRIPT_MAX_TRIES == mm.MAX_TRIES == 256


def test_the_knob_is_known_under_both_names(cm):
    override = cm._lib.curdle_plan_override
    data, _, tries, _ = retry_reference()
    try:
        for name in (b"TRANSCRIPT_MAX_TRIES", b"CURDLE_TRANSCRIPT_MAX_TRIES"):
            assert override(name, 5) == cm.OK, name
            _, _, status = cm.transcript_batch(mm.RETRY_PROGRAM, data, label=mm.RETRY_LABEL, host=True)
            assert (status.astype(bool) == gives_up(tries, 5)).all(), name
            assert override(name, -1) == cm.OK, name
            _, _, status = cm.transcript_batch(mm.RETRY_PROGRAM, data, label=mm.RETRY_LABEL, host=True)
            assert not status.any(), name
        assert override(b"TRANSCRIPT_MAX_TRY", 5) == cm.EINVAL
    finally:
        override(b"TRANSCRIPT_MAX_TRIES", -1)


def test_the_single_host_transcript_ignores_the_knob(cm):
    """GetAndAppendChallenge of the host's own Transcript -- what the single calls that settle a handed-back member
    hash with -- has no bound of the batch's: a tracker proof generated and checked by the single calls under a bound of
    one draw is the proof of the unset bound and verifies."""
    import bls12381_ref as o
    k, r = 0x1234567, 0x89abcd
    rG = o.scalar_mul(r, o.G1)
    tracker = o.compress(rG) + o.compress(o.scalar_mul(k, rG))
    k_comm = o.compress(o.scalar_mul(k, o.G1))
    limbs = np.array(o.fr_to_mont_limbs(k), dtype=np.uint64)
    import tracker_prove_model as tpm
    proofs, retried = {}, 0
    for seed in range(6):
        proofs[seed] = cm.whisk_generate_tracker_proof(tracker, limbs, cm.Rand(seed))
        row = k_comm + o.compress(o.G1) + tracker[48:] + tracker[:48] + proofs[seed][:96]
        retried += mm.run_program(tpm.PROGRAM, row, tpm.LABEL)[1][0] > 1
    assert retried                # under a bound of one draw these transcripts would give up in the batch
    with cm.knobs(TRANSCRIPT_MAX_TRIES=1):
        for seed, want in proofs.items():
            assert cm.whisk_generate_tracker_proof(tracker, limbs, cm.Rand(seed)) == want, seed
            assert cm.whisk_is_valid_tracker_proof(tracker, k_comm, want), seed
