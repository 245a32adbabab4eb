"""curdle_whisk_generate_shuffle_proof_batch on the GPU against the single calls of the same build
(curdle_whisk_generate_shuffle_proof without the flag, curdle_whisk_generate_shuffle_proof_ct under it): k = 1, 3, 8
members with their own trackers and seeds at n = 124, the only n the single call accepts, and at n = 125, which it
refuses behind its draws.  Per member the post-trackers, the 4,576 proof bytes and the rand's next draws are the single
call's and curdle_whisk_is_valid_shuffle_proof accepts.  One member with a tracker that does not decode -- placed first,
in the middle and last -- gets the single call's error code and rand state, and the others' bytes are unchanged."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K_MAX = 8


@pytest.fixture(scope="module")
def setup(gpu):
    """The CRS, K_MAX tracker sets of 125 trackers, and per flag the single calls' results on the first 124 (computed once)."""
    cm = gpu
    ell = cm.WHISK_ELL
    crs = cm.CRS(ell, cm.Rand(4))
    sets = []
    for i in range(K_MAX):
        r = cm.Rand(31 + i)
        trk, _ = cm.whisk_compute_trackers_batch(r.get_frs(ell + 1), r.get_frs(ell + 1), commitments=False)
        sets.append([trk[t].tobytes() for t in range(ell + 1)])
    singles = {}
    for flags, call in ((0, cm.whisk_generate_shuffle_proof), (1, cm.whisk_generate_shuffle_proof_ct)):
        for i in range(K_MAX):
            r = cm.Rand(600 + i)
            post, proof = call(crs, sets[i][:ell], r)
            singles[(flags, i)] = (post, proof, r.get_frs(2))
    return crs, sets, singles


def single_error(cm, crs, trackers, seed, flags):
    r = cm.Rand(seed)
    with pytest.raises(cm.CurdleError) as e:
        (cm.whisk_generate_shuffle_proof_ct if flags else cm.whisk_generate_shuffle_proof)(crs, trackers, r)
    return e.value.code, r.get_frs(2)


@pytest.mark.parametrize("flags", (0, 1))
@pytest.mark.parametrize("k", (1, 3, 8))
def test_a_batch_is_its_single_calls(gpu, setup, k, flags):
    cm = gpu
    crs, sets, singles = setup
    ell = cm.WHISK_ELL
    rands = [cm.Rand(600 + i) for i in range(k)]
    before = cm.stat_prove_batch()
    mul0 = cm.stat_host_point_mul()
    posts, proofs, status = cm.whisk_generate_shuffle_proof_batch(crs, [sets[i][:ell] for i in range(k)], rands, flags)
    mul1 = cm.stat_host_point_mul()
    after = cm.stat_prove_batch()
    assert status == [0] * k
    for i in range(k):
        post, proof, draws = singles[(flags, i)]
        assert posts[i] == post and proofs[i] == proof and len(proofs[i]) == 4576, (k, i)
        assert (rands[i].get_frs(2) == draws).all(), (k, i)
        assert cm.whisk_is_valid_shuffle_proof(crs, sets[i][:ell], posts[i], proofs[i], cm.Rand(43)) is True, (k, i)
    assert (after["calls"] - before["calls"], after["members"] - before["members"], after["groups"] - before["groups"]) == (1, k, 1)
    if flags:
        assert mul1 == mul0, "the calling thread multiplies no point on the host"


@pytest.mark.parametrize("flags", (0, 1))
def test_the_next_n_is_refused_per_member_behind_the_draws(gpu, setup, flags):
    cm = gpu
    crs, sets, _ = setup
    k, n = 3, cm.WHISK_ELL + 1
    rands = [cm.Rand(700 + i) for i in range(k)]
    posts, proofs, status = cm.whisk_generate_shuffle_proof_batch(crs, [sets[i][:n] for i in range(k)], rands, flags)
    for i in range(k):
        code, draws = single_error(cm, crs, sets[i][:n], 700 + i, flags)
        assert status[i] == code == cm.EINVAL and posts[i] is None and proofs[i] is None
        assert (rands[i].get_frs(2) == draws).all()


@pytest.mark.parametrize("flags", (0, 1))
@pytest.mark.parametrize("where", (0, 1, 2))
def test_a_tracker_that_does_not_decode_is_its_member_s_alone(gpu, setup, where, flags):
    cm = gpu
    crs, sets, singles = setup
    ell, k = cm.WHISK_ELL, 3
    pre = [list(sets[i][:ell]) for i in range(k)]
    pre[where][5] = bytes([0xFF]) * 96                          # x >= p: not an encoding
    rands = [cm.Rand(600 + i) for i in range(k)]
    posts, proofs, status = cm.whisk_generate_shuffle_proof_batch(crs, pre, rands, flags)
    code, draws = single_error(cm, crs, pre[where], 600 + where, flags)
    for i in range(k):
        if i == where:
            assert status[i] == code != 0 and posts[i] is None and proofs[i] is None
            assert (rands[i].get_frs(2) == draws).all()
            continue
        post, proof, want_draws = singles[(flags, i)]
        assert status[i] == 0 and posts[i] == post and proofs[i] == proof
        assert (rands[i].get_frs(2) == want_draws).all()


def test_fold_bases_is_refused_per_member_under_the_flag(gpu, setup):
    """With PROVER_FOLD_BASES set the flagged batch gives every member curdle_prove_ct's refusal where the single call
    meets it -- behind the shuffle step and its draws, before any prover work: the single call's code, text and rand
    state, and the call itself is CURDLE_OK.  Without the flag the knob refuses nothing and the bytes are the single
    calls' under the same knob."""
    cm = gpu
    crs, sets, _ = setup
    ell, k = cm.WHISK_ELL, 3
    with cm.knobs(PROVER_FOLD_BASES=1):
        rands = [cm.Rand(800 + i) for i in range(k)]
        walks0 = cm.stat_msm_ct()["walks"]
        posts, proofs, status = cm.whisk_generate_shuffle_proof_batch(crs, [sets[i][:ell] for i in range(k)], rands,
                                                                      cm.PROVE_BATCH_CONSTANT_TIME)
        text = cm.last_error()
        assert cm.stat_msm_ct()["walks"] - walks0 == 1, "the shuffle steps' one walk and no prover's"
        for i in range(k):
            r = cm.Rand(800 + i)
            with pytest.raises(cm.CurdleError) as e:
                cm.whisk_generate_shuffle_proof_ct(crs, sets[i][:ell], r)
            assert status[i] == e.value.code == cm.EINVAL and posts[i] is None and proofs[i] is None
            assert "PROVER_FOLD_BASES" in e.value.msg and e.value.msg in text
            assert (rands[i].get_frs(2) == r.get_frs(2)).all()
        rands = [cm.Rand(800 + i) for i in range(2)]
        posts, proofs, status = cm.whisk_generate_shuffle_proof_batch(crs, [sets[i][:ell] for i in range(2)], rands, 0)
        for i in range(2):
            r = cm.Rand(800 + i)
            assert status[i] == 0 and (posts[i], proofs[i]) == cm.whisk_generate_shuffle_proof(crs, sets[i][:ell], r)
            assert (rands[i].get_frs(2) == r.get_frs(2)).all()
