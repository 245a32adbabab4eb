"""k_tracker_check on members chosen for the branch its joint GLV chain takes (tests/golden/tracker_chain_cases.npz,
written by tests/golden/gen_tracker_chain_cases.py over tests/glv_chain_model.py): an addition of equal operands or of
opposite ones at the table of kG / krG or at the table of G / rG, a chain that goes on from infinity, a group whose
second chain runs on infinity throughout, a table that only ever adds infinity.  Every such member is an honest proof
and must be accepted wherever it sits in a wave, a block and a batch; every tampered twin must be rejected."""
import os
import sys

import pytest

import glv_chain_model as M
from test_tracker_batch_gpu import check_against_single, honest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import gen_tracker_chain_cases as gen  # noqa: E402

pytestmark = pytest.mark.gpu

WAVE, BLOCK = 8, 32          # members per wave and per block of k_tracker_check (eight lanes each, 256 lanes a block)
SIZES = [8, 9, 31, 32, 33, 65]
REQUIRED = (1, 2, 6, 7)      # reachable with k = +-1 / k = 0; classes 3..5 are kept as found


@pytest.fixture(scope="module")
def rows():
    found = {row["cls"] for row in ROWS}
    assert found >= set(REQUIRED), found
    return ROWS


@pytest.fixture(scope="module")
def hon(gpu, oracle):
    """The honest pool of tests/test_tracker_batch_gpu.py: twelve members of random k and r."""
    rand = oracle.Rand(77)
    out = []
    for j in range(12):
        k, r = rand.get_fr(), rand.get_fr()
        out.append(honest(gpu, oracle, k, r, 100 + j)[0])
    assert len(set(out)) == 12
    return out


@pytest.fixture(scope="module")
def singles(gpu):
    """The single call's answers, shared by every test of the module."""
    return {}


def test_the_members_still_take_their_branch_under_the_device_split(gpu, oracle, rows):
    """s and c of every member through the DEVICE build of the split (what k_tracker_check runs), then the
    model: the recorded step is there with its class, and the member still belongs to its class.  A change to
    the split cannot turn these into ordinary members unnoticed."""
    scal = [gen.member_scalars(oracle, row["member"], row["k"], row["seed"]) for row in rows]
    flat = [v for s, c, _ in scal for v in (s, c)]
    dev = M.splits(gpu, flat, True)
    assert dev == M.splits(gpu, flat, False)
    seen = set()
    for j, (row, (s, c, b)) in enumerate(zip(rows, scal)):
        k, r = row["k"], row["r"]
        events, u = M.joint_chain(dev[2 * j], dev[2 * j + 1], k, t=b)
        step = (row["bit"], row["site"], row["step"])
        assert u == b and step in events, (row["cls"], row["seed"])
        assert gen.classes_of(events, k, r).get(row["cls"]) == step, (row["cls"], row["seed"])
        if row["cls"] == 2 or (row["cls"] == 6 and row["step"] == M.OPPOSITE):
            after = events[events.index(step) + 1]
            assert after[2] == M.INTO_INF and after[0] < row["bit"]       # the chain doubles infinity, then adds into it
        if row["cls"] == 6:                                                # chain 1 of the group: infinity throughout
            other, u1 = M.joint_chain(dev[2 * j], dev[2 * j + 1], k, t=b, p_is_infinity=True)
            assert u1 == 0 and {e[2] for e in other} == {M.ADDS_INF}
        seen.add(row["cls"])
    assert seen >= set(REQUIRED)


ROWS = gen.load()[0]


@pytest.mark.parametrize("row", ROWS, ids=["class%d-%s-seed%d" % (row["cls"], row["step"], row["seed"]) for row in ROWS])
def test_every_member_alone_three_ways(gpu, oracle, singles, row):
    """Accepted by the batch, by the single call, and by the protocol's equations A = s G + c kG,
    B = s rG + c krG in the Python oracle."""
    m = row["member"]
    check_against_single(gpu, [m], expected=[1], cache=singles)
    s, c, b = gen.member_scalars(oracle, m, row["k"], row["seed"])
    G, k, r = oracle.G1, row["k"], row["r"]
    rG = oracle.scalar_mul(r, G)
    kG, krG = oracle.scalar_mul(k, G), oracle.scalar_mul(k, rG)
    assert m[0] == oracle.compress(rG) + oracle.compress(krG) and m[1] == oracle.compress(kG)
    assert oracle.compress(oracle.add(oracle.scalar_mul(s, G), oracle.scalar_mul(c, kG))) == m[2][:48]
    assert oracle.compress(oracle.add(oracle.scalar_mul(s, rG), oracle.scalar_mul(c, krG))) == m[2][48:96]


def positions(n):
    """Where the event member goes in a batch of n: the first and the last member of a wave and of a block, the
    last index, and between two ordinary members."""
    last_wave = WAVE * ((n - 1) // WAVE)
    want = {0, last_wave, WAVE - 1, last_wave - 1, n - 1, 3, BLOCK - 1, BLOCK, 2 * BLOCK - 1, 2 * BLOCK}
    return sorted(p for p in want if 0 <= p < n)


@pytest.mark.parametrize("n", SIZES)
def test_one_event_member_at_the_edges_of_waves_and_blocks(gpu, rows, hon, singles, n):
    """Every event member in turn, at every position of positions(n), among honest members: its quad pair takes
    the exceptional branch while the other quads of its wave do not.  Every verdict is the single call's, 1."""
    for p in positions(n):
        for j, row in enumerate(rows):
            members = [hon[(i + j) % len(hon)] for i in range(n)]
            members[p] = row["member"]
            check_against_single(gpu, members, expected=[1] * n, cache=singles)


def eight_of_different_classes(rows):
    """Eight event members: one of every class that has members, then second members."""
    firsts, seconds, seen = [], [], set()
    for row in rows:
        (seconds if row["cls"] in seen else firsts).append(row["member"])
        seen.add(row["cls"])
    return (firsts + seconds)[:WAVE]


def test_a_wave_of_event_members_and_a_batch_of_nothing_else(gpu, rows, hon, singles):
    """Neighbouring quads of one wave in different exceptional branches at once: a wave of eight event members
    (every class that has members, two of them twice) alone, behind and between honest waves, and shifted by
    one member so that it straddles two waves; then all event members as one batch."""
    wave = eight_of_different_classes(rows)
    assert len(wave) == WAVE and len(set(wave)) == WAVE
    check_against_single(gpu, wave, expected=[1] * WAVE, cache=singles)
    for lead in (WAVE, 1, BLOCK - WAVE, BLOCK - 1):
        members = [hon[i % len(hon)] for i in range(lead)] + wave + [hon[i % len(hon)] for i in range(WAVE)]
        check_against_single(gpu, members, expected=[1] * len(members), cache=singles)
    everyone = [row["member"] for row in rows]
    check_against_single(gpu, everyone, expected=[1] * len(everyone), cache=singles)
    check_against_single(gpu, everyone[::-1], expected=[1] * len(everyone), cache=singles)


def twins(oracle, member):
    """Four tampered copies of a member, every one a reject."""
    t, kc, p = member
    A, B, S = p[:48], p[48:96], p[96:]
    assert A != oracle.compress(None) and A[0] & 0x80
    minus_A = bytes([A[0] ^ 0x20]) + A[1:]                     # the sign bit of the compressed form
    s1 = ((int.from_bytes(S, "big") + 1) % oracle.R).to_bytes(32, "big")
    return {"A = inf": (t, kc, oracle.compress(None) + B + S),
            "A = -A": (t, kc, minus_A + B + S),
            "A, B swapped": (t, kc, B + A + S),
            "s + 1": (t, kc, A + B + s1)}


def test_reject_twins(gpu, oracle, rows, singles):
    """A chain that left early at a mid-chain infinity, or that lost its sum there, would accept A = infinity;
    the other twins are the plain rejects.  Alone and on either side of the untouched member."""
    for row in rows:
        m = row["member"]
        for name, bad in twins(oracle, m).items():
            assert bad != m, (row["cls"], name)
            check_against_single(gpu, [bad], expected=[0], cache=singles)
            check_against_single(gpu, [m, bad], expected=[1, 0], cache=singles)
            check_against_single(gpu, [bad, m], expected=[0, 1], cache=singles)
    # ... and all of them in one batch, every tampered member between untouched ones
    members, expected = [], []
    for row in rows:
        for bad in twins(oracle, row["member"]).values():
            members += [row["member"], bad]
            expected += [1, 0]
    check_against_single(gpu, members, expected=expected, cache=singles)
