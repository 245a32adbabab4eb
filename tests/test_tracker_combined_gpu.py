"""The combined tracker batch on the GPU (curdle_whisk_is_valid_tracker_proof_batch_combined, _device): a pass settled
by ONE randomly weighted MSM.  The fallback to the per-member chains hides a broken sum behind correct answers, so the
tests pin the sum itself: the MSM scalars and the generator's total bit for bit against the big-integer model
(tests/tracker_combined_model.py, through curdle_whisk_tracker_combined_scalars), and the counters of
curdle_stat_tracker_combined -- an honest batch must be settled by sums with NO fallback.  Every honest batch is made
of the pool's twelve honest proofs and five accepted exceptional cases, each of which
tests/test_tracker_combined_model.py shows to sum to infinity."""
import threading

import numpy as np
import pytest

import tracker_combined_model as tc
from test_tracker_batch_gpu import pool, single  # noqa: F401  (pool: the module-scoped fixture of that file)

pytestmark = pytest.mark.gpu

SEED = bytes(range(1, 33))
SEED2 = bytes(range(101, 133))
ACCEPTED = ("k=1", "k=r-1", "k=0", "r=1", "tracker=inf")
PASS = 1 << 16
BLOCK = 256   # members per block of k_tracker_combine

_single = {}


def want_for(cm, members):
    out = []
    for m in members:
        if m not in _single:
            _single[m] = single(cm, m)
        out.append(_single[m])
    return out


def accepted_members(pool):
    """The seventeen members honest batches are made of."""
    hon, cases = pool
    return [h[0] for h in hon] + [cases[name][0] for name in ACCEPTED]


def honest_batch(pool, k):
    acc = accepted_members(pool)
    return [acc[j % len(acc)] for j in range(k)]


def run(cm, members, seed=SEED):
    t, kc, p = zip(*members)
    return cm.whisk_is_valid_tracker_proof_batch_combined(list(t), list(kc), list(p), seed)


def arrays(members):
    t, kc, p = zip(*members)
    return [np.frombuffer(b"".join(x), dtype=np.uint8) for x in (t, kc, p)]


def moved(cm, before):
    after = cm.stat_tracker_combined()
    return {name: after[name] - before[name] for name in after}


def model_members(cm, oracle, members):
    want = want_for(cm, members)
    return [tc.member_from_bytes(oracle, *m, excluded=(w == cm.EINVAL)) for m, w in zip(members, want)]


def check_scalars(cm, oracle, members, seed=SEED):
    """The kernel's 5 k scalars and the generator's total against the model, bit for bit."""
    t, kc, p = zip(*members)
    got, g = cm.whisk_tracker_combined_scalars(list(t), list(kc), list(p), seed)
    scalars, want_g = tc.scalars_and_g(oracle, model_members(cm, oracle, members), seed)
    want = np.array(tc.mont_limbs(oracle, scalars), dtype=np.uint64)
    assert got.shape == want.shape == (len(members), 5, 4)
    bad = np.nonzero((got != want).any(axis=(1, 2)))[0]
    assert bad.size == 0, "members %s differ from the model" % bad[:8].tolist()
    assert [int(v) for v in g] == [int(v) for v in oracle.fr_to_mont_limbs(want_g)]
    return got


def excluded_kinds(pool):
    """One member of every kind of exclusion: S >= r, a record that does not decode (off the curve, x >= p, stray
    bits), a record outside the subgroup in each of the five positions."""
    _, cases = pool
    names = ["S=r", "S=2^256-1", "all 0x01", "x>=p", "off curve", "inf stray bits", "rogue rG", "rogue krG", "rogue kG",
             "rogue A", "rogue B"]
    return [cases[n][0] for n in names]


@pytest.mark.parametrize("k", [1, 63, 64, 65, BLOCK + 1])
def test_scalars_and_g_match_the_model(gpu, oracle, pool, k):
    members = honest_batch(pool, k)
    check_scalars(gpu, oracle, members)
    # rejected members take part in the sum like honest ones: only refusals are excluded
    _, cases = pool
    if k > 2:
        members[k // 2] = cases["S+1"][0]
        members[k - 1] = cases["A other"][0]
        check_scalars(gpu, oracle, members)


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_scalars_of_excluded_members_are_zero(gpu, oracle, pool, where):
    k = 2 * BLOCK + 5                                                    # three blocks, the last one short
    at = {"first": 0, "middle": BLOCK, "last": k - 1}[where]             # (middle: the first lane of the second block)
    kinds = excluded_kinds(pool)
    for j, bad in enumerate(kinds):
        members = honest_batch(pool, k)
        members[at] = bad
        members[(at + 37) % k] = kinds[(j + 1) % len(kinds)]             # and a second kind somewhere inside a wave
        got = check_scalars(gpu, oracle, members)
        assert not got[at].any() and not got[(at + 37) % k].any()
        assert got[(at + 1) % k].any()


def test_two_seeds_give_different_scalars(gpu, oracle, pool):
    members = honest_batch(pool, 5)
    a = check_scalars(gpu, oracle, members, SEED)
    b = check_scalars(gpu, oracle, members, SEED2)
    assert (a != b).any(axis=(1, 2)).all()


@pytest.mark.parametrize("k", [1, 2, 64, 65, 4097])
def test_honest_batches_are_settled_by_the_sum(gpu, pool, k):
    members = honest_batch(pool, k)
    before = gpu.stat_tracker_combined()
    got = run(gpu, members)
    assert got.dtype == np.int32 and got.tolist() == [1] * k
    assert moved(gpu, before) == {"settled": 1, "fell_back": 0, "accepted": k, "excluded": 0}


def test_pass_boundary(gpu, pool):
    _, cases = pool
    k = PASS + 1
    members = honest_batch(pool, k)
    before = gpu.stat_tracker_combined()
    assert (run(gpu, members) == 1).all()
    assert moved(gpu, before) == {"settled": 2, "fell_back": 0, "accepted": k, "excluded": 0}
    expected = [1] * k
    for at, name in ((PASS - 1, "S+1"), (PASS, "A other")):
        members[at], expected[at] = cases[name]
    before = gpu.stat_tracker_combined()
    assert run(gpu, members).tolist() == expected
    assert moved(gpu, before) == {"settled": 0, "fell_back": 2, "accepted": 0, "excluded": 0}


def test_every_case_between_honest_neighbours(gpu, pool):
    hon, cases = pool
    errors = [(m, w) for m, w in cases.values() if w == gpu.EINVAL]
    others = [(m, w) for m, w in cases.values() if w != gpu.EINVAL]
    assert sum(w == 0 for _, w in others) == 6 and sum(w == 1 for _, w in others) == 5

    def between(group):
        members, expected = [], []
        for j, (m, want) in enumerate(group):
            members += [hon[j % len(hon)][0], m]
            expected += [1, want]
        return members + [hon[-1][0]], expected + [1]

    # errors only: the refused members are excluded and the sum still settles the pass
    members, expected = between(errors)
    before = gpu.stat_tracker_combined()
    got = run(gpu, members)
    assert got.tolist() == expected == want_for(gpu, members)
    assert moved(gpu, before) == {"settled": 1, "fell_back": 0, "accepted": len(errors) + 1, "excluded": len(errors)}
    # at least one reject: the chains answer
    members, expected = between(others + errors[:3])
    before = gpu.stat_tracker_combined()
    got = run(gpu, members)
    assert got.tolist() == expected == want_for(gpu, members)
    assert moved(gpu, before) == {"settled": 0, "fell_back": 1, "accepted": 0, "excluded": 3}


def test_adversarial_members_are_rejected(gpu, oracle, pool):
    """Members whose errors cancel under equal coefficients (the model test shows that they do)."""
    acc = accepted_members(pool)
    one, two = tc.cancelling_pair(oracle)
    lone = tc.self_cancelling(oracle)
    for bad in ([one.bytes, two.bytes], [lone.bytes]):
        assert want_for(gpu, bad) == [0] * len(bad)
        members = acc[:3] + bad[:1] + acc[3:5] + bad[1:] + acc[5:7]
        expected = [1] * 3 + [0] + [1] * 2 + [0] * (len(bad) - 1) + [1] * 2
        before = gpu.stat_tracker_combined()
        assert run(gpu, members).tolist() == expected
        assert moved(gpu, before) == {"settled": 0, "fell_back": 1, "accepted": 0, "excluded": 0}


def test_two_seeds_give_the_same_answers(gpu, pool):
    hon, cases = pool
    members = honest_batch(pool, 40)
    expected = [1] * 40
    for at, name in ((7, "S=r"), (20, "rogue A"), (33, "B other")):
        members[at], expected[at] = cases[name]
    assert run(gpu, members, SEED).tolist() == expected
    assert run(gpu, members, SEED2).tolist() == expected
    honest_only = honest_batch(pool, 40)
    before = gpu.stat_tracker_combined()
    assert run(gpu, honest_only, SEED).tolist() == run(gpu, honest_only, SEED2).tolist() == [1] * 40
    assert moved(gpu, before)["settled"] == 2


def test_resident_form(gpu, pool):
    import torch
    _, cases = pool
    mixed = honest_batch(pool, 300)
    for at, name in ((0, "rogue kG"), (150, "S+1"), (299, "x>=p")):
        mixed[at] = cases[name][0]
    honest_only = honest_batch(pool, 300)
    stream = torch.cuda.Stream()
    for members in (mixed, honest_only):
        want = run(gpu, members).tolist()
        assert want == want_for(gpu, members)
        host = arrays(members)
        for shift in (0, 1, 3):
            dev = [torch.zeros(len(a) + shift, dtype=torch.uint8, device="cuda:0") for a in host]
            for d, a in zip(dev, host):
                d[shift:].copy_(torch.from_numpy(a.copy()))
            torch.cuda.synchronize()
            ptrs = [d[shift:].data_ptr() for d in dev]
            before = gpu.stat_tracker_combined()
            got = gpu.whisk_is_valid_tracker_proof_batch_combined_device(*ptrs, len(members), SEED)
            assert got.tolist() == want
            with torch.cuda.stream(stream):
                got = gpu.whisk_is_valid_tracker_proof_batch_combined_device(*ptrs, len(members), SEED, stream.cuda_stream)
            assert got.tolist() == want
            if members is honest_only:   # on the caller's stream too the sum settles the pass
                assert moved(gpu, before) == {"settled": 2, "fell_back": 0, "accepted": 600, "excluded": 0}


def test_beside_other_work_and_with_one_free_slot(gpu, oracle, coracle, pool):
    import torch
    _, cases = pool
    members = honest_batch(pool, 700)
    members[123] = cases["A other"][0]
    want = want_for(gpu, members)
    honest_only = honest_batch(pool, 700)
    k, q = oracle.Rand(1).get_frs(2)
    n = 2048
    pts = coracle.points_walk(k, q, n)
    sc = np.random.default_rng(n).integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    sc[:, 3] &= np.uint64((1 << 62) - 1)
    want_msm = coracle.msm_pippenger(pts, sc, threads=4)
    results, errors = {}, []

    def guarded(name, fn):
        def body():
            try:
                results[name] = fn()
            except Exception as e:  # noqa: BLE001 - reported below
                errors.append((name, e))
        return threading.Thread(target=body)

    t, kc, p = (list(x) for x in zip(*members))
    threads = [guarded("combined", lambda: [run(gpu, members).tolist() for _ in range(3)] + [run(gpu, honest_only).tolist()]),
               guarded("plain", lambda: [gpu.whisk_is_valid_tracker_proof_batch(t, kc, p).tolist() for _ in range(3)]),
               guarded("msm", lambda: [gpu.msm_g1(pts, sc) for _ in range(3)])]
    [th.start() for th in threads]
    [th.join() for th in threads]
    assert not errors, errors
    assert results["combined"] == [want] * 3 + [[1] * 700]
    assert results["plain"] == [want] * 3
    assert all((got == want_msm).all() for got in results["msm"])

    # exactly one MSM slot free: the call runs everything, its MSM included, in the slot it holds
    d_pts = torch.from_numpy(pts.view(np.int64)).to("cuda:0")
    d_sc = torch.from_numpy(sc.view(np.int64)).to("cuda:0")
    torch.cuda.synchronize()
    tickets = [gpu.msm_g1_device_submit(d_pts.data_ptr(), d_sc.data_ptr(), n) for _ in range(gpu.MSM_SLOTS - 1)]
    try:
        before = gpu.stat_tracker_combined()
        assert run(gpu, members).tolist() == want
        assert run(gpu, honest_only).tolist() == [1] * 700
        assert moved(gpu, before) == {"settled": 1, "fell_back": 1, "accepted": 700, "excluded": 0}
    finally:
        waited = [gpu.msm_wait(tk) for tk in tickets]
    assert all((got == want_msm).all() for got in waited)
