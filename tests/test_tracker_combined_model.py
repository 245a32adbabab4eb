"""The combined tracker check on the CPU: the big-integer model (tests/tracker_combined_model.py) against the
protocol.  Honest members sum to infinity under the model's coefficients -- each of the seventeen accepted members
the GPU tests build their honest batches from; the adversarial members are what they claim (individually invalid,
cancelling under EQUAL coefficients, caught under the model's); an excluded member contributes nothing; one tampered
member leaves a non-zero sum.  The oracle's multiplications are slow, so every test takes a few members."""
import hashlib

import pytest

import tracker_combined_model as tc
from test_tracker_batch_gpu import honest

SEED = bytes(range(32))

# the accepted members of tests/test_tracker_batch_gpu.py's pool, by the recipe of that fixture: (k, r, seed of the proof)
EXCEPTIONAL = {"k=1": (1, 5, 201), "k=r-1": (-1, 7, 202), "k=0": (0, 9, 203), "r=1": (11, 1, 204), "tracker=inf": (13, 0, 205)}


def accepted_pool(cm, oracle):
    """[(name, model member)] of the pool's twelve honest proofs and its five accepted exceptional cases, with the
    bytes the library generated and the points from the discrete logs."""
    rand = oracle.Rand(77)
    recipe = []
    for j in range(12):
        k, r = rand.get_fr(), rand.get_fr()
        recipe.append(("honest %d" % j, k, r, 100 + j))
    recipe += [(name, k % oracle.R, r, seed) for name, (k, r, seed) in EXCEPTIONAL.items()]
    out = []
    for name, k, r, seed in recipe:
        (tracker, kc, proof), b = honest(cm, oracle, k, r, seed)
        pts = tc.honest_points(oracle, k, r, b)
        assert tracker == oracle.compress(pts[0]) + oracle.compress(pts[1]) and kc == oracle.compress(pts[2]), name
        assert proof[:96] == oracle.compress(pts[3]) + oracle.compress(pts[4]), name
        out.append((name, tc.member_from_bytes(oracle, tracker, kc, proof, False, pts)))
    return out


@pytest.fixture(scope="module")
def accepted(cm, oracle):
    return accepted_pool(cm, oracle)


def test_coefficients_are_the_shake_of_the_issue():
    rho, sigma = tc.coefficients(SEED, 0x0102030405060708)
    out = hashlib.shake_256(b"curdle/tracker-combine/v1" + SEED + bytes([8, 7, 6, 5, 4, 3, 2, 1])).digest(32)
    assert rho == int.from_bytes(out[:16], "little") and sigma == int.from_bytes(out[16:], "little")
    assert len(tc.DOMAIN) + 32 + 8 == 65 < 136                          # one rate block of SHAKE256
    assert tc.coefficients(SEED, 0) != tc.coefficients(SEED, 1)
    assert tc.coefficients(SEED, 0) != tc.coefficients(bytes(32), 0)


def test_every_accepted_pool_member_sums_to_infinity(oracle, accepted):
    """The condition on the GPU tests' honest batches: each member alone, at an index of its own, and the model's
    response equation for the library's bytes."""
    assert len(accepted) == 17
    for j, (name, m) in enumerate(accepted):
        assert m.s < oracle.R and not m.excluded, name
        assert tc.weighted_sum(oracle, [m], SEED, first=1000 * j + 3) is oracle.INF, name


def test_model_built_honest_members_sum_to_infinity_together(oracle):
    members = [tc.honest_member(oracle, 0x1111 + 7 * j, 0x2222 + j, 0x3333 + 5 * j) for j in range(3)]
    for m in members:
        assert tc.equation_errors(oracle, m) == (oracle.INF, oracle.INF)
    assert tc.weighted_sum(oracle, members, SEED) is oracle.INF
    assert tc.weighted_sum(oracle, members, SEED, coeff=tc.equal_coefficients) is oracle.INF


def test_the_cancelling_pair_is_what_it_claims(oracle):
    one, two = tc.cancelling_pair(oracle)
    e1, e2 = tc.equation_errors(oracle, one), tc.equation_errors(oracle, two)
    assert e1[0] is not oracle.INF and e2[0] is not oracle.INF           # each is invalid on its own
    assert e1[1] is oracle.INF and e2[1] is oracle.INF                   # ... in its first equation only
    assert e1[0] == oracle.neg(e2[0])
    assert one.s < oracle.R and two.s < oracle.R
    hon = tc.honest_member(oracle, 0x77, 0x55, 0x99)
    members = [hon, one, two]
    assert tc.weighted_sum(oracle, members, SEED, coeff=tc.equal_coefficients) is oracle.INF
    assert tc.weighted_sum(oracle, members, SEED) is not oracle.INF


def test_the_self_cancelling_member_is_what_it_claims(oracle):
    m = tc.self_cancelling(oracle)
    e1, e2 = tc.equation_errors(oracle, m)
    assert e1 is not oracle.INF and e1 == oracle.neg(e2)
    assert m.s < oracle.R
    hon = tc.honest_member(oracle, 0x77, 0x55, 0x99)
    assert tc.weighted_sum(oracle, [hon, m], SEED, coeff=tc.equal_coefficients) is oracle.INF
    assert tc.weighted_sum(oracle, [hon, m], SEED) is not oracle.INF


def test_an_excluded_member_has_zero_scalars_and_adds_nothing(oracle, accepted):
    hon = accepted[0][1]
    t, kc, p = hon.bytes
    s_ge_r = tc.member_from_bytes(oracle, t, kc, p[:96] + oracle.R.to_bytes(32, "big"), False)
    assert s_ge_r.excluded                                               # S >= r excludes by itself
    undecodable = tc.member_from_bytes(oracle, b"\x01" * 96, kc, p, True)
    for bad in (s_ge_r, undecodable):
        scalars, g = tc.scalars_and_g(oracle, [hon, bad, hon], SEED)
        assert scalars[1] == (0, 0, 0, 0, 0) and scalars[0] != (0, 0, 0, 0, 0)
        rho0, _ = tc.coefficients(SEED, 0)
        rho2, _ = tc.coefficients(SEED, 2)                               # the index counts the excluded member
        assert g == (rho0 + rho2) * hon.s % oracle.R
        assert tc.weighted_sum(oracle, [hon, bad, hon], SEED) is oracle.INF
    limbs = tc.mont_limbs(oracle, tc.scalars_and_g(oracle, [hon], SEED)[0])
    assert [oracle.fr_from_mont_limbs(x) for x in limbs[0]] == list(tc.scalars_and_g(oracle, [hon], SEED)[0][0])


def test_one_tampered_member_gives_a_non_zero_sum(oracle, accepted):
    hon = accepted[1][1]
    t, kc, p = hon.bytes
    tampered = tc.member_from_bytes(oracle, t, kc, p[:96] + ((hon.s + 1) % oracle.R).to_bytes(32, "big"), False, hon.points)
    assert tampered.c == hon.c                                           # S is not part of the transcript
    assert tc.weighted_sum(oracle, [accepted[0][1], tampered], SEED) is not oracle.INF
