"""The status byte of the batched Merlin transcripts on the GPU, and everything that sits behind it.  With the library's
bound of 256 draws a member gives up with probability 0.547^256; the test hook TRANSCRIPT_MAX_TRIES (host/knobs.h) lowers
the bound to T, so that the give-up branches of k_transcript_batch and k_transcript_sheet, k_tracker_challenge's zeroing,
the hand-back loops of the tracker batches (plain, combined) and of the tracker prover, and the Whisk shuffle batch's
return to the host prelude all run here.

Which members give up is predicted by the Python model alone (tests/merlin_model.py: a member gives up under T exactly
when one of its challenges needs more than T draws); never by the library's host twin.  The single calls that settle a
handed-back member ignore the knob, so every answer and every proof is still the single call's.  Challenges and state
of a status-1 member are unspecified (include/curdle_msm.h) and are not asserted."""
import functools
import os

import numpy as np
import pytest

import merlin_model as mm
import tracker_combined_model as tc
import tracker_prove_model as tpm
from test_tracker_batch_gpu import off_subgroup_point, pool  # noqa: F401  (pool: the module-scoped fixture of that file)
from test_tracker_hash_gpu import arrays, mixed, run_flag, run_resident, want_for
from test_transcript_batch_gpu import data_for
from test_transcript_status_host import gives_up, retry_reference

pytestmark = pytest.mark.gpu

SHEET, LANE = 1, 0
BOUNDS = (2, 5, 6, 8)
# knob settings of a run: the sheet kernel; the lane kernel at the library's members per wave, at 1, 2 and 64
KERNELS = {"sheet": dict(TRANSCRIPT_SHEET=SHEET), "lane": dict(TRANSCRIPT_SHEET=LANE),
           "lane1": dict(TRANSCRIPT_SHEET=LANE, TRANSCRIPT_LANES=1), "lane2": dict(TRANSCRIPT_SHEET=LANE, TRANSCRIPT_LANES=2),
           "lane64": dict(TRANSCRIPT_SHEET=LANE, TRANSCRIPT_LANES=64)}
T_ONE, T_FEW = 1, 2          # the tracker tests' bounds: about half of the members give up, and about a third


# ---- a) curdle_transcript_batch ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pair_batch():
    """All 144 ordered pairs of the retry fixture's members, laid out consecutively: members 2 j and 2 j + 1 share a
    wave of the sheet kernel, so every kind of member sits beside every other kind, in either half.  (data, challenges,
    tries, states) by the model, from the twelve members' reference."""
    data, ch, tries, st = retry_reference()
    idx = np.array([m for a in range(12) for b in range(12) for m in (a, b)])
    return tuple(x[idx] for x in (data, ch, tries, st))


@functools.lru_cache(maxsize=None)
def random_batch():
    """257 members of random data under the retry program, by the model: four full waves and one member of the lane
    kernel at 64 members per wave, where some members give up at try T while their neighbours still draw."""
    data = data_for(mm.RETRY_PROGRAM, 257, seed=2024)
    ch = np.zeros((257, 8, 32), dtype=np.uint8)
    st = np.zeros((257, mm.STATE_SIZE), dtype=np.uint8)
    tries = np.zeros((257, 8), dtype=np.int64)
    for i in range(257):
        mc, mt, mst, status, _ = mm.run_program(mm.RETRY_PROGRAM, bytes(data[i]), mm.RETRY_LABEL)
        assert status == 0
        ch[i] = np.frombuffer(b"".join(mc), dtype=np.uint8).reshape(8, 32)
        st[i] = np.frombuffer(mst, dtype=np.uint8)
        tries[i] = mt
    return data, ch, tries, st


def batches():
    """name -> (data, challenges, tries, states)"""
    pairs = pair_batch()
    one = retry_reference()
    out = {"pairs 288": pairs, "pairs 289": tuple(np.concatenate([x, y[11:12]]) for x, y in zip(pairs, one)),
           "member 11 alone": tuple(x[11:12] for x in one), "member 4 alone": tuple(x[4:5] for x in one),
           "random 257": random_batch()}
    assert len(out["pairs 288"][0]) == 288 and len(out["pairs 289"][0]) == 289
    return out


def run_checked(gpu, name, batch, bound, knobs, twin_status=None):
    """One batch under one bound on one kernel, with and without the states: status bytes, the status-0 members'
    outputs and the counters against the model.  Returns the status bytes."""
    data, want_ch, tries, want_st = batch
    want_status = gives_up(tries, bound)
    k, n_up = len(data), int(want_status.sum())
    with gpu.knobs(TRANSCRIPT_MAX_TRIES=bound, **knobs):
        s0 = gpu.stat_transcript()
        ch, st, status = gpu.transcript_batch(mm.RETRY_PROGRAM, data, label=mm.RETRY_LABEL)
        s1 = gpu.stat_transcript()
        ch2, none, status2 = gpu.transcript_batch(mm.RETRY_PROGRAM, data, label=mm.RETRY_LABEL, want_states=False)
        s2 = gpu.stat_transcript()
    what = (name, bound, knobs)
    assert set(status.tolist()) <= {0, 1} and (status.astype(bool) == want_status).all(), what
    assert (status2 == status).all() and none is None, what
    keep = ~want_status
    assert (ch[keep] == want_ch[keep]).all(), (what, "challenges")
    assert (st[keep] == want_st[keep]).all(), (what, "states")
    assert (ch2[keep] == want_ch[keep]).all(), (what, "challenges without states")
    for a, b in ((s0, s1), (s1, s2)):
        assert (b["members"] - a["members"], b["handed_back"] - a["handed_back"]) == (k, n_up), what
    if twin_status is not None:
        assert (status == twin_status).all(), what
    return status


@pytest.mark.parametrize("bound", BOUNDS)
def test_both_kernels_give_up_exactly_where_the_model_does(gpu, bound):
    handed0 = gpu.stat_transcript()["handed_back"]
    expected_moves = 0
    for name, batch in batches().items():
        data, want_ch, tries, want_st = batch
        want_status = gives_up(tries, bound)
        if name in ("pairs 288", "random 257"):     # members that give up beside members that keep drawing
            assert 3 <= want_status.sum() <= len(data) - 3, (name, bound)
        if name == "member 11 alone":
            assert want_status.all()
        if name == "random 257":                    # full waves of the lane kernel with both kinds inside
            for w in range(4):
                assert 0 < want_status[64 * w:64 * w + 64].sum() < 64, (bound, w)
        # the host twin under the same bound: the same status bytes, the same outputs where the status is 0
        with gpu.knobs(TRANSCRIPT_MAX_TRIES=bound):
            tch, tst, twin_status = gpu.transcript_batch(mm.RETRY_PROGRAM, data, label=mm.RETRY_LABEL, host=True, nthreads=4)
        assert (twin_status.astype(bool) == want_status).all(), (name, bound)
        assert (tch[~want_status] == want_ch[~want_status]).all() and (tst[~want_status] == want_st[~want_status]).all()
        for kernel, knobs in KERNELS.items():
            run_checked(gpu, name, batch, bound, knobs, twin_status)
            expected_moves += 2 * int(want_status.sum())
    moved = gpu.stat_transcript()["handed_back"] - handed0
    assert moved == expected_moves and moved > 0      # curdle_stat_transcript out[1] is seen to move


def test_sheet_pairs_hold_every_kind_of_neighbour():
    """What the 288-member batch puts on the two halves of a wave, per bound: a member that gives up beside one that
    does not, beside one with a challenge of exactly T tries, beside one that gives up at another challenge index, in
    either half; and two members that give up at the same challenge (a member beside itself)."""
    _, _, tries, _ = pair_batch()
    for bound in (2, 5, 6):
        up = gives_up(tries, bound)
        first = [int(np.argmax(t > bound)) if u else -1 for t, u in zip(tries, up)]
        exact = [(not u) and (t == bound).any() for t, u in zip(tries, up)]
        kinds = set()
        for j in range(0, 288, 2):
            for a, b, half in ((j, j + 1, "low"), (j + 1, j, "high")):
                if up[a] and not up[b]:
                    kinds.add(("beside ordinary", half))
                if up[a] and exact[b]:
                    kinds.add(("beside exactly T", half))
                if up[a] and up[b] and first[a] < first[b]:
                    kinds.add(("gives up earlier than its neighbour", half))
            if up[j] and up[j + 1] and first[j] == first[j + 1]:
                kinds.add("both at the same challenge")
        assert len(kinds) == 7, (bound, kinds)


@pytest.mark.parametrize("kernel", ["sheet", "lane", "lane64"])
def test_a_state_exported_under_a_lowered_bound_continues_under_the_unset_one(gpu, kernel):
    data, _, tries, want_st = pair_batch()
    bound = 5
    keep = ~gives_up(tries, bound)
    assert 3 <= keep.sum() <= 285
    with gpu.knobs(TRANSCRIPT_MAX_TRIES=bound, **KERNELS[kernel]):
        _, st, status = gpu.transcript_batch(mm.RETRY_PROGRAM, data, label=mm.RETRY_LABEL)
    assert (status == 0).tolist() == keep.tolist() and (st[keep] == want_st[keep]).all()
    second = [(mm.TR_APPEND, b"more", 2, 33), (mm.TR_CHALLENGES, b"z", 3, 0)]
    members = np.nonzero(keep)[0][:24]                  # both halves of a wave among them
    assert (members % 2).any() and not (members % 2).all()
    more = data_for(second, len(members), seed=6)
    with gpu.knobs(**KERNELS[kernel]):
        ch2, st2, status2 = gpu.transcript_batch(second, more, init_states=st[members])
    assert not status2.any()
    for j, i in enumerate(members):                     # the model's two calls
        _, _, mst, s1, _ = mm.run_program(mm.RETRY_PROGRAM, bytes(data[i]), mm.RETRY_LABEL)
        mc, mt, mst2, s2, _ = mm.run_program(second, bytes(more[j]), state=mst)
        assert s1 == 0 and s2 == 0
        assert bytes(ch2[j].reshape(-1)) == b"".join(mc) and bytes(st2[j]) == mst2, i


# ---- the tracker members' transcripts by the model -------------------------------------------------------------
_tries = {}


def tracker_tries(oracle, member):
    """Draws the one challenge of a tracker member's transcript needs: tracker_prove_model.PROGRAM over the member's
    row kG | G | krG | rG | A | B, from the member's raw bytes as the device hashes them."""
    if member not in _tries:
        t, kc, p = member
        row = kc + oracle.compress(oracle.G1) + t[48:] + t[:48] + p[:96]
        _, tries, _, status, _ = mm.run_program(tpm.PROGRAM, row, tpm.LABEL)
        assert status == 0 and len(tries) == 1
        _tries[member] = tries[0]
    return _tries[member]


def handed_back(oracle, members, bound):
    return [tracker_tries(oracle, m) > bound for m in members]


# ---- b) the plain tracker batch ----------------------------------------------------------------------------------
def choose_mixed(oracle, pool, k, bound):  # noqa: F811
    """The first seed whose `mixed` batch holds, by the model, enough members of every kind for its size."""
    for seed in range(5000, 5400):
        members, expected = mixed(pool, k, seed)
        back = handed_back(oracle, members, bound)
        n_back, n_dev = sum(back), k - sum(back)
        bad_back = sum(b and e != 1 for b, e in zip(back, expected))
        if k == 1 and n_back == 1:
            return members, expected, back
        if k == 3 and n_back >= 1 and n_dev >= 1:
            return members, expected, back
        if k >= 64 and n_back >= 3 and n_dev >= 3 and bad_back >= 1:
            return members, expected, back
    raise AssertionError("no seed gives a batch of %d members with every kind under a bound of %d" % (k, bound))


@pytest.mark.parametrize("bound", [T_ONE, T_FEW])
@pytest.mark.parametrize("k", [1, 3, 64, 65, 257])
def test_plain_tracker_batch_hands_back_the_members_the_model_names(gpu, oracle, pool, k, bound):  # noqa: F811
    members, expected, back = choose_mixed(oracle, pool, k, bound)
    n_back = sum(back)
    if k >= 64:     # the counts the choice was made for
        assert n_back >= 3 and k - n_back >= 3
        assert any(b and e in (0, gpu.EINVAL) for b, e in zip(back, expected))
    want = want_for(gpu, members)
    assert want == expected
    for kernel in ("sheet", "lane"):
        with gpu.knobs(TRANSCRIPT_MAX_TRIES=bound, **KERNELS[kernel]):
            s0 = gpu.stat_tracker()
            dev = run_flag(gpu, members, gpu.TRACKER_HASH_DEVICE)
            s1 = gpu.stat_tracker()
            host = run_flag(gpu, members, gpu.TRACKER_HASH_HOST)
            s2 = gpu.stat_tracker()
        assert dev.tolist() == want, (kernel, "HASH_DEVICE")
        assert (s1["handed_back"] - s0["handed_back"], s1["device"] - s0["device"], s1["host"] - s0["host"]) == (n_back, k - n_back, 0)
        assert host.tolist() == want, (kernel, "HASH_HOST")
        assert (s2["handed_back"] - s1["handed_back"], s2["device"] - s1["device"], s2["host"] - s1["host"]) == (0, 0, k)
    assert n_back > 0


@pytest.mark.parametrize("k", [1, 65, 257])
def test_resident_tracker_batch_fails_the_call_on_a_member_that_gives_up(gpu, oracle, pool, k):  # noqa: F811
    """What the resident form does today (include/curdle_msm.h): no host copy of the member exists to settle it by, so
    the call fails with CURDLE_EHIP and names the first such member of the pass."""
    members, expected, back = choose_mixed(oracle, pool, k, T_FEW)
    first = back.index(True)
    with gpu.knobs(TRANSCRIPT_MAX_TRIES=T_FEW):
        with pytest.raises(gpu.CurdleError) as e:
            run_resident(gpu, members)
    assert e.value.code == gpu.EHIP and ("member %d " % first) in e.value.msg and "no canonical challenge" in e.value.msg
    # a bound under which nobody gives up: the answers are the single call's, as with the knob unset
    nobody = max(tracker_tries(oracle, m) for m in members)
    assert nobody > T_FEW
    with gpu.knobs(TRANSCRIPT_MAX_TRIES=nobody):
        s0 = gpu.stat_tracker()
        assert run_resident(gpu, members).tolist() == want_for(gpu, members) == expected
        s1 = gpu.stat_tracker()
    assert (s1["device"] - s0["device"], s1["handed_back"] - s0["handed_back"]) == (k, 0)
    assert run_resident(gpu, members).tolist() == expected


# ---- c) the combined tracker batch -------------------------------------------------------------------------------
SEED = bytes(range(7, 39))
ACCEPTED = ("k=1", "k=r-1", "k=0", "r=1", "tracker=inf")
BLOCK = 256   # members per block of k_tracker_combine


def honest_batch(pool, k, shift=0):  # noqa: F811
    hon, cases = pool
    acc = [h[0] for h in hon] + [cases[name][0] for name in ACCEPTED]
    return [acc[(j + shift) % len(acc)] for j in range(k)]


def run_combined(cm, members):
    t, kc, p = zip(*members)
    return cm.whisk_is_valid_tracker_proof_batch_combined(list(t), list(kc), list(p), SEED)


def combined_moved(cm, before):
    after = cm.stat_tracker_combined()
    return {name: after[name] - before[name] for name in after}


def rejects_by_kind(oracle, pool, bound):  # noqa: F811
    """(a rejected member that gives up under the bound, one that does not), from the pool's six rejects."""
    _, cases = pool
    rejects = [m for m, want in cases.values() if want == 0]
    up = [m for m in rejects if tracker_tries(oracle, m) > bound]
    stay = [m for m in rejects if tracker_tries(oracle, m) <= bound]
    assert up and stay, "the pool's rejects hold no member of each kind under a bound of %d" % bound
    return up[0], stay[0]


@pytest.mark.parametrize("bound", [T_ONE, T_FEW])
@pytest.mark.parametrize("k", [1, 3, 65, 257])
def test_combined_batch_settles_the_pass_without_the_members_that_give_up(gpu, oracle, pool, k, bound):  # noqa: F811
    shift = 2 if k == 1 else 0                       # k = 1: the one member gives up under both bounds
    members = honest_batch(pool, k, shift)
    back = handed_back(oracle, members, bound)
    n_back = sum(back)
    assert n_back >= 1 and (k == 1 or k - n_back >= 1)
    for kernel in ("sheet", "lane"):
        with gpu.knobs(TRANSCRIPT_MAX_TRIES=bound, **KERNELS[kernel]):
            before = gpu.stat_tracker_combined()
            got = run_combined(gpu, members)
            assert got.dtype == np.int32 and got.tolist() == [1] * k
            # settled by the sum: the members that gave up were kept out of it and answered on the host
            assert combined_moved(gpu, before) == {"settled": 1, "fell_back": 0, "accepted": k - n_back, "excluded": n_back}, kernel
    if k < 3:
        return
    gives_up_reject, settled_reject = rejects_by_kind(oracle, pool, bound)
    # a handed-back member tampered to a reject: it answers 0 on the host, and the pass is still settled by the sum
    tampered = list(members)
    at = back.index(True)
    tampered[at] = gives_up_reject
    with gpu.knobs(TRANSCRIPT_MAX_TRIES=bound):
        before = gpu.stat_tracker_combined()
        got = run_combined(gpu, tampered)
        assert got.tolist() == [0 if j == at else 1 for j in range(k)] == want_for(gpu, tampered)
        assert combined_moved(gpu, before) == {"settled": 1, "fell_back": 0, "accepted": k - n_back, "excluded": n_back}
    # a device-settled member tampered: the sum is not infinity, the chains answer, every answer is the single call's
    tampered = list(members)
    at = back.index(False)
    tampered[at] = settled_reject
    with gpu.knobs(TRANSCRIPT_MAX_TRIES=bound):
        before = gpu.stat_tracker_combined()
        got = run_combined(gpu, tampered)
        assert got.tolist() == [0 if j == at else 1 for j in range(k)] == want_for(gpu, tampered)
        assert combined_moved(gpu, before) == {"settled": 0, "fell_back": 1, "accepted": 0, "excluded": n_back}


@pytest.mark.parametrize("bound", [T_ONE, T_FEW])
@pytest.mark.parametrize("shift", [0, 1])
def test_combined_scalars_of_members_that_give_up_are_zero(gpu, oracle, pool, bound, shift):  # noqa: F811
    """curdle_whisk_tracker_combined_scalars on 257 members, two blocks of k_tracker_combine: a member that gives up
    has five zero scalars and the generator's total is the model's sum over the others.  shift = 1 puts a member that
    gives up alone into the second block (its block's sum is then zero), shift = 0 one that does not."""
    k = BLOCK + 1
    members = honest_batch(pool, k, shift)
    _, cases = pool
    members[100], members[101] = cases["S=r"][0], cases["rogue A"][0]      # the other kinds of exclusion beside them
    back = handed_back(oracle, members, bound)
    assert back[BLOCK] == (shift == 1) and sum(back[:BLOCK]) >= 3 and BLOCK - sum(back[:BLOCK]) >= 3
    want = want_for(gpu, members)
    model = [tc.member_from_bytes(oracle, *m, excluded=(w == gpu.EINVAL or b)) for m, w, b in zip(members, want, back)]
    scalars, want_g = tc.scalars_and_g(oracle, model, SEED)
    want_scalars = np.array(tc.mont_limbs(oracle, scalars), dtype=np.uint64)
    t, kc, p = zip(*members)
    for kernel in ("sheet", "lane"):
        with gpu.knobs(TRANSCRIPT_MAX_TRIES=bound, **KERNELS[kernel]):
            got, g = gpu.whisk_tracker_combined_scalars(list(t), list(kc), list(p), SEED)
        for j in range(k):
            if back[j]:
                assert not got[j].any(), (kernel, j)
        bad = np.nonzero((got != want_scalars).any(axis=(1, 2)))[0]
        assert bad.size == 0, (kernel, "members %s differ from the model" % bad[:8].tolist())
        assert [int(v) for v in g] == [int(v) for v in oracle.fr_to_mont_limbs(want_g)], kernel
    # the same members with the knob unset: the members that gave up take part again
    got, _ = gpu.whisk_tracker_combined_scalars(list(t), list(kc), list(p), SEED)
    assert all(got[j].any() for j in range(k) if back[j])


def test_resident_combined_batch_fails_the_call_on_a_member_that_gives_up(gpu, oracle, pool):  # noqa: F811
    import torch
    k = 65
    members = honest_batch(pool, k)
    back = handed_back(oracle, members, T_FEW)
    first = back.index(True)
    dev = [torch.from_numpy(a.copy()).to("cuda:0") for a in arrays(members)]
    torch.cuda.synchronize()
    ptrs = [d.data_ptr() for d in dev]
    with gpu.knobs(TRANSCRIPT_MAX_TRIES=T_FEW):
        with pytest.raises(gpu.CurdleError) as e:
            gpu.whisk_is_valid_tracker_proof_batch_combined_device(*ptrs, k, SEED)
    assert e.value.code == gpu.EHIP and ("member %d " % first) in e.value.msg and "no canonical challenge" in e.value.msg
    nobody = max(tracker_tries(oracle, m) for m in members)
    with gpu.knobs(TRANSCRIPT_MAX_TRIES=nobody):
        before = gpu.stat_tracker_combined()
        assert gpu.whisk_is_valid_tracker_proof_batch_combined_device(*ptrs, k, SEED).tolist() == [1] * k
        assert combined_moved(gpu, before) == {"settled": 1, "fell_back": 0, "accepted": k, "excluded": 0}
    assert gpu.whisk_is_valid_tracker_proof_batch_combined_device(*ptrs, k, SEED).tolist() == [1] * k


# ---- d) the tracker prover -----------------------------------------------------------------------------------------
def fr_limbs(oracle, values):
    return np.array([oracle.fr_to_mont_limbs(v % oracle.R) for v in values], dtype=np.uint64).reshape(-1, 4)


@pytest.fixture(scope="module")
def prove_pool(oracle):
    """A dozen (k, r) pairs: (k, tracker, k commitment)."""
    model = tpm.Model(oracle)
    rand = oracle.Rand(4242)
    pairs = [(rand.get_fr(), rand.get_fr()) for _ in range(12)]
    return [(k, model.tracker(k, r), model.k_commitment(k, r)) for k, r in pairs], model, pairs


def prover_case(cm, oracle, prove_pool, k, bound, seed):
    """k members over the pool, the member after the first one that gives up carrying a tracker record outside the
    subgroup (k >= 3).  The reference is the loop of single calls on a Rand of `seed`; the blinders are that Rand's
    draws, one per member that decodes; which members give up is the model's word on the single calls' A and B."""
    members, _, _ = prove_pool
    rogue = off_subgroup_point(oracle)
    for attempt in range(64):
        which = [(5 * i + attempt) % 12 for i in range(k)]
        trackers = [members[w][1] for w in which]
        ks = [members[w][0] for w in which]
        rb, draws = cm.Rand(seed + attempt), oracle.Rand(seed + attempt)
        want, blinders, back = [], [], []
        bad_at = None
        for i in range(k):
            if bad_at is None and k >= 3 and i >= 1 and back[i - 1]:
                bad_at = i
                trackers[i] = rogue + trackers[i][48:]
            try:
                proof = cm.whisk_generate_tracker_proof(trackers[i], fr_limbs(oracle, [ks[i]])[0], rb)
            except cm.CurdleError as e:
                assert e.code == cm.EINVAL and i == bad_at
                want.append(None)
                blinders.append(0)
                back.append(False)
                continue
            want.append(proof)
            blinders.append(draws.get_fr())
            back.append(tracker_tries(oracle, (trackers[i], members[which[i]][2], proof)) > bound)
        n_back = sum(back)
        enough = n_back >= 1 and (k < 3 or (bad_at is not None and k - n_back - 1 >= 1)) and (k < 65 or n_back >= 3)
        if enough:
            return dict(which=which, trackers=trackers, ks=ks, want=want, blinders=blinders, back=back, bad_at=bad_at,
                        seed=seed + attempt, next_fr=rb.get_fr())
    raise AssertionError("no arrangement of %d members with every kind under a bound of %d" % (k, bound))


@pytest.mark.parametrize("bound", [T_ONE, T_FEW])
@pytest.mark.parametrize("k", [1, 3, 65, 257])
def test_prover_generates_the_members_that_give_up_by_the_single_path(gpu, oracle, prove_pool, k, bound):
    c = prover_case(gpu, oracle, prove_pool, k, bound, seed=900 + k)
    members, model, pairs = prove_pool
    want, back, n_back = c["want"], c["back"], sum(c["back"])
    assert n_back >= 1 and (k < 3 or (c["bad_at"] is not None and back[c["bad_at"] - 1]))
    ks = fr_limbs(oracle, c["ks"])
    # the single calls' proofs are the big-integer model's: one member that gives up, one that does not
    settled = [i for i in range(k) if not back[i] and want[i] is not None]
    for i in [back.index(True)] + settled[:1]:
        kk, r = pairs[c["which"][i]]
        assert want[i] == model.proof(kk, r, c["blinders"][i]), i

    def check(proofs, res, what):
        for i in range(k):
            if want[i] is None:
                assert res[i] == gpu.EINVAL and proofs[i].tobytes() == bytes(128), (what, i)
            else:
                assert res[i] == gpu.OK and proofs[i].tobytes() == want[i], (what, i, back[i])

    for kernel in ("sheet", "lane"):
        with gpu.knobs(TRANSCRIPT_MAX_TRIES=bound, **KERNELS[kernel]):
            s0 = gpu.stat_tracker_prove()
            proofs, res = gpu.whisk_generate_tracker_proof_batch(c["trackers"], ks, blinders=fr_limbs(oracle, c["blinders"]))
            s1 = gpu.stat_tracker_prove()
            ra = gpu.Rand(c["seed"])
            rproofs, rres = gpu.whisk_generate_tracker_proof_batch(c["trackers"], ks, rand=ra)
            s2 = gpu.stat_tracker_prove()
        check(proofs, res, (kernel, "blinders"))
        check(rproofs, rres, (kernel, "rand"))
        assert (ra.get_fr() == c["next_fr"]).all(), kernel           # the two rands agree on their next draw
        for a, b in ((s0, s1), (s1, s2)):
            assert (b["host"] - a["host"], b["device"] - a["device"]) == (n_back, k - n_back), kernel
    for i in range(k):                                               # every generated proof verifies
        if want[i] is not None:
            assert gpu.whisk_is_valid_tracker_proof(c["trackers"][i], members[c["which"][i]][2], proofs[i].tobytes()), i


# ---- e) the Whisk shuffle batch's prelude ------------------------------------------------------------------------
def test_whisk_batch_returns_to_the_host_prelude_for_every_member_that_gives_up(gpu):
    """curdle_whisk_is_valid_shuffle_proof_batch with GPU_PRELUDE=1 on k = 8 in chunks of 4, three bad members of
    different kinds inside, under a bound of ONE draw: a prelude draws 124 challenges, so every hashed member gives up
    (a member keeps going with probability 0.453^124) and takes the host prelude.  The verdicts are those of
    GPU_PRELUDE=0, and curdle_stat_transcript counts every hashed member as handed back -- on either kernel."""
    from conftest import ROOT
    from test_batch_rejects_gpu import flip_last_scalar
    vectors = np.load(os.path.join(ROOT, "tests", "golden", "proof_vectors.npz"))
    pre, post, proof = (vectors[n].tobytes() for n in ("whisk_pre", "whisk_post", "whisk_proof"))
    pre_l = [pre[96 * i:96 * (i + 1)] for i in range(124)]
    post_l = [post[96 * i:96 * (i + 1)] for i in range(124)]
    crs = gpu.CRS(124, gpu.Rand(7))
    k = 8
    bad = {1: "swap", 3: "scalar", 4: "M"}
    pres, posts, proofs = [pre_l] * k, [list(post_l) for _ in range(k)], [proof] * k
    for i, kind in bad.items():
        if kind == "swap":
            posts[i][0] = post_l[0][48:] + post_l[0][:48]
        elif kind == "scalar":
            proofs[i] = flip_last_scalar(proof, 4536)
        else:
            proofs[i] = pre_l[3][:48] + proof[48:]
    expect = [i not in bad for i in range(k)]

    def run():
        return gpu.whisk_is_valid_shuffle_proof_batch(crs, pres, posts, proofs, gpu.Rand(9), nthreads=4)
    with gpu.knobs(BATCH_CHUNK=4):
        with gpu.knobs(GPU_PRELUDE=0):
            off = run()
        assert off == expect
        for kernel in ("sheet", "lane"):
            s0, p0 = gpu.stat_transcript(), gpu.stat_transcript_paths()
            with gpu.knobs(GPU_PRELUDE=1, TRANSCRIPT_MAX_TRIES=1, **KERNELS[kernel]):
                on = run()
            s1, p1 = gpu.stat_transcript(), gpu.stat_transcript_paths()
            assert on == off, kernel
            hashed = p1[kernel] - p0[kernel]
            assert hashed == k and p1["lane"] + p1["sheet"] - p0["lane"] - p0["sheet"] == k, kernel
            assert (s1["members"] - s0["members"], s1["handed_back"] - s0["handed_back"]) == (hashed, hashed), kernel
            # with the bound unset the same run hands nobody back
            s0 = gpu.stat_transcript()
            with gpu.knobs(GPU_PRELUDE=1, **KERNELS[kernel]):
                assert run() == off
            s1 = gpu.stat_transcript()
            assert (s1["members"] - s0["members"], s1["handed_back"] - s0["handed_back"]) == (k, 0), kernel
