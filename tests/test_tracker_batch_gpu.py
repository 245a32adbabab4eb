"""curdle_whisk_is_valid_tracker_proof_batch on the GPU: every member's answer equals the single
call's (curdle_whisk_is_valid_tracker_proof, IsValidWhiskTrackerProof at whisk.go:116) on the same
bytes -- 1, 0, or CurdleError with EINVAL -- with the interesting members sitting between honest
neighbours inside one batch."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


# --- helpers after tests/test_whisk.py ------------------------------------------------------------
def fr_limbs(oracle, k):
    return np.array(oracle.fr_to_mont_limbs(k % oracle.R), dtype=np.uint64)


def compute_tracker(oracle, k, r):
    # whisk_test.go:98-104: rG = r*G, krG = k*rG, both in gnark's compressed form
    rG = oracle.scalar_mul(r, oracle.G1)
    return oracle.compress(rG) + oracle.compress(oracle.scalar_mul(k, rG))


def k_comm(oracle, k):
    return oracle.compress(oracle.scalar_mul(k, oracle.G1))  # whisk_test.go:106-109


def off_subgroup_point(oracle):
    p = oracle.P
    x = 6
    while True:
        rhs = (x * x * x + 4) % p
        y = pow(rhs, (p + 1) // 4, p)
        if y * y % p == rhs and oracle.scalar_mul(oracle.R, (x, y)) is not None:
            return oracle.compress((x, y))
        x += 1


def off_curve_record(oracle):
    p = oracle.P
    x = 1
    while True:
        rhs = (x * x * x + 4) % p
        if pow(rhs, (p - 1) // 2, p) == p - 1:
            b = bytearray(x.to_bytes(48, "big"))
            b[0] |= 0x80
            return bytes(b)
        x += 1


def single(cm, member):
    """The single call's answer in the batch's encoding."""
    try:
        return 1 if cm.whisk_is_valid_tracker_proof(*member) else 0
    except cm.CurdleError as e:
        assert e.code == cm.EINVAL
        return cm.EINVAL


def honest(cm, oracle, k, r, seed):
    """(tracker, kComm, proof, blinder) of an honest opening proof."""
    tracker = compute_tracker(oracle, k, r)
    proof = cm.whisk_generate_tracker_proof(tracker, fr_limbs(oracle, k), cm.Rand(seed))
    return (tracker, k_comm(oracle, k), proof), oracle.Rand(seed).get_fr()  # the blinder is the proof's first draw


def run_batch(cm, members):
    t, kc, p = zip(*members) if members else ((), (), ())
    return cm.whisk_is_valid_tracker_proof_batch(list(t), list(kc), list(p))


def check_against_single(cm, members, expected=None, cache=None):
    got = run_batch(cm, members)
    assert got.dtype == np.int32 and len(got) == len(members)
    cache = {} if cache is None else cache
    want = []
    for m in members:
        if m not in cache:
            cache[m] = single(cm, m)
        want.append(cache[m])
    assert got.tolist() == want
    if expected is not None:
        assert want == expected
    return got


@pytest.fixture(scope="module")
def pool(gpu, oracle):
    """Distinct honest members (random k and r) and the tampered / exceptional ones, by name."""
    rand = oracle.Rand(77)
    hon = []
    for j in range(12):
        k, r = rand.get_fr(), rand.get_fr()
        m, b = honest(gpu, oracle, k, r, 100 + j)
        hon.append((m, b, k, r))
    R = oracle.R
    cases = {}
    # exceptional group cases inside the chain: all accepted
    # kG = +-G: the chain's running sum CAN meet the next addend or its negative, but only where the leading bits and
    # signs of the halves of s and c line up, which one seed leaves to chance (the tables' own sums P + phi(P) never
    # degenerate); tests/test_tracker_chain_events_gpu.py has members chosen for those branches
    cases["k=1"] = (honest(gpu, oracle, 1, 5, 201)[0], 1)          # kG = G, krG = rG
    cases["k=r-1"] = (honest(gpu, oracle, R - 1, 7, 202)[0], 1)    # kG = -G, krG = -rG
    cases["k=0"] = (honest(gpu, oracle, 0, 9, 203)[0], 1)          # kG, krG at infinity
    cases["r=1"] = (honest(gpu, oracle, 11, 1, 204)[0], 1)         # rG = G
    cases["tracker=inf"] = (honest(gpu, oracle, 13, 0, 205)[0], 1)  # rG = krG = inf: B = B' = inf
    (t, kc, p), b, k, r = hon[0]
    (t1, kc1, _), _, _, _ = hon[1]
    other_pt = oracle.compress(oracle.scalar_mul(12345, oracle.G1))
    s = int.from_bytes(p[96:], "big")
    # rejects
    cases["A other"] = ((t, kc, other_pt + p[48:]), 0)
    cases["B other"] = ((t, kc, p[:48] + other_pt + p[96:]), 0)
    cases["A = -A'"] = ((t, kc, oracle.compress(oracle.neg(oracle.scalar_mul(b, oracle.G1))) + p[48:]), 0)
    cases["S+1"] = ((t, kc, p[:96] + ((s + 1) % R).to_bytes(32, "big")), 0)
    cases["other kComm"] = ((t, kc1, p), 0)
    cases["other tracker"] = ((t1, kc, p), 0)
    # errors
    E = gpu.EINVAL
    rogue, off, inf = off_subgroup_point(oracle), off_curve_record(oracle), oracle.compress(None)
    x_ge_p = bytearray(oracle.P.to_bytes(48, "big"))
    x_ge_p[0] |= 0x80
    stray = bytearray(inf)
    stray[47] = 1
    cases["S=r"] = ((t, kc, p[:96] + R.to_bytes(32, "big")), E)
    cases["S=2^256-1"] = ((t, kc, p[:96] + b"\xff" * 32), E)
    cases["all 0x01"] = ((b"\x01" * 96, kc, p), E)
    cases["x>=p"] = ((t, kc, bytes(x_ge_p) + p[48:]), E)
    cases["off curve"] = ((t[:48] + off, kc, p), E)
    cases["inf stray bits"] = ((t, bytes(stray), p), E)
    cases["rogue rG"] = ((rogue + t[48:], kc, p), E)
    cases["rogue krG"] = ((t[:48] + rogue, kc, p), E)
    cases["rogue kG"] = ((t, rogue, p), E)
    cases["rogue A"] = ((t, kc, rogue + p[48:]), E)
    cases["rogue B"] = ((t, kc, p[:48] + rogue + p[96:]), E)
    # ... and the points an attacker would send (tests/golden/decode_edge_records.npz): small order, and small
    # order hidden behind a G1 point, in the same five positions
    from test_decode_edges_gpu import attack_records
    for name, bad in attack_records(oracle).items():
        cases[name + " rG"] = ((bad + t[48:], kc, p), E)
        cases[name + " krG"] = ((t[:48] + bad, kc, p), E)
        cases[name + " kG"] = ((t, bad, p), E)
        cases[name + " A"] = ((t, kc, bad + p[48:]), E)
        cases[name + " B"] = ((t, kc, p[:48] + bad + p[96:]), E)
    return hon, cases


def test_honest_proofs_accepted_and_match_the_protocol_equations(gpu, oracle, pool):
    hon, _ = pool
    check_against_single(gpu, [h[0] for h in hon], expected=[1] * len(hon))
    # an answer independent of both the host and the GPU path: A = b G, B = b rG, s = b - c k
    for (t, kc, p), b, k, r in hon[:3]:
        assert p[:48] == oracle.compress(oracle.scalar_mul(b, oracle.G1))
        assert p[48:96] == oracle.compress(oracle.scalar_mul(b, oracle.scalar_mul(r, oracle.G1)))
        s = int.from_bytes(p[96:], "big")
        c = (b - s) * pow(k, -1, oracle.R) % oracle.R
        assert oracle.add(oracle.scalar_mul(s, oracle.G1), oracle.scalar_mul(c * k % oracle.R, oracle.G1)) == \
            oracle.scalar_mul(b, oracle.G1)


def test_every_case_between_honest_neighbours(gpu, pool):
    hon, cases = pool
    members, expected = [], []
    for j, (m, want) in enumerate(cases.values()):
        members += [hon[j % len(hon)][0], m]
        expected += [1, want]
    members.append(hon[-1][0])
    expected.append(1)
    check_against_single(gpu, members, expected=expected)


@pytest.mark.parametrize("name", ["k=1", "k=r-1", "k=0", "r=1", "tracker=inf", "A = -A'", "S=r", "rogue kG"])
def test_case_alone(gpu, pool, name):
    m, want = pool[1][name]
    check_against_single(gpu, [m], expected=[want])


@pytest.mark.timeout(600)
@pytest.mark.parametrize("k", [1, 1024, 7000])
def test_sizes(gpu, pool, k):
    """7,000 members are 35,000 records, beyond the 32,768 of one two-kernel decoding."""
    hon, cases = pool
    rng = np.random.default_rng(k)
    tampered = list(cases.values())
    members, expected = [], []
    for i in range(k):
        if k > 1 and rng.random() < 0.1:
            m, want = tampered[rng.integers(len(tampered))]
        else:
            m, want = hon[rng.integers(len(hon))][0], 1
        members.append(m)
        expected.append(want)
    check_against_single(gpu, members, expected=expected, cache={})


@pytest.mark.timeout(600)
def test_concurrent_batches_beside_a_shuffle_batch(gpu, oracle, pool):
    hon, cases = pool
    rng = np.random.default_rng(5)
    pool_members = [h[0] for h in hon] + [m for m, _ in cases.values()]
    batches = [[pool_members[j] for j in rng.integers(len(pool_members), size=256)] for _ in range(4)]
    serial = [run_batch(gpu, b).tolist() for b in batches]
    cache = {}
    for b, s in zip(batches, serial):
        assert s == [cache.setdefault(m, single(gpu, m)) for m in b]

    rand = gpu.Rand(4)
    crs = gpu.CRS(gpu.WHISK_ELL, rand)
    pre = []
    r2 = gpu.Rand(31)
    for _ in range(gpu.WHISK_ELL):
        k = oracle.fr_from_mont_limbs([int(v) for v in r2.get_fr()])
        r = oracle.fr_from_mont_limbs([int(v) for v in r2.get_fr()])
        pre.append(compute_tracker(oracle, k, r))
    post, proof = gpu.whisk_generate_shuffle_proof(crs, pre, gpu.Rand(61))

    results, errors = {}, []
    stop = threading.Event()

    def tracker_worker(t):
        try:
            got = []
            for _ in range(3):
                got.append(run_batch(gpu, batches[t]).tolist())
            results[t] = got
        except Exception as e:  # noqa: BLE001 - reported below
            errors.append(e)

    def shuffle_worker():
        try:
            while True:  # at least once, and for as long as the tracker batches run
                assert gpu.whisk_is_valid_shuffle_proof_batch(crs, [pre, pre], [post, post], [proof, proof],
                                                              gpu.Rand(1), nthreads=2) == [True, True]
                if stop.is_set():
                    break
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    sh = threading.Thread(target=shuffle_worker)
    sh.start()
    threads = [threading.Thread(target=tracker_worker, args=(t,)) for t in range(4)]
    [t.start() for t in threads]
    [t.join() for t in threads]
    stop.set()
    sh.join()
    assert not errors, errors
    for t in range(4):
        assert results[t] == [serial[t]] * 3
