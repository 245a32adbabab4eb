"""The constant-time ownership search (csrc/tracker_own_ct_kernels.hip) without a GPU: every key of
tracker_own_model.case_families walks to k under the model of the shared walk (tests/g1_mul_ct_model.py), the exactness
argument holds on every kept sum, the one exceptional DISCARDED sum over the whole key list is k = r - 1 at step 254 --
so the GPU matrix of tests/test_tracker_own_ct_gpu.py provably exercises it -- and the second launch rule of
csrc/tracker_own_api.hip, restated here, gives the counts worked out by hand below."""
import pytest

import g1_mul_ct_model as gm
import tracker_own_model as tom

PASS = 1 << 17
DEFAULT_PAIRS = 1 << 18
BLOCK = 256


def launches(n, m, pairs=DEFAULT_PAIRS):
    """The launch rule under CURDLE_TRACKER_OWN_CONSTANT_TIME: P = max(256, pairs / 256 * 256) lanes a launch; per pass
    of cnt trackers tc = min(cnt, P), kc = max(1, P / tc), and ceil(cnt / tc) * ceil(m / kc) launches."""
    p = max(BLOCK, pairs // BLOCK * BLOCK)
    total = 0
    for lo in range(0, n, PASS):
        cnt = min(PASS, n - lo)
        tc = min(cnt, p)
        kc = max(1, p // tc)
        total += -(-cnt // tc) * -(-m // kc)
    return total


@pytest.fixture(scope="module")
def families(oracle):
    return tom.case_families(oracle)


def test_every_key_walks_to_k_and_only_r_minus_1_discards_an_exceptional_sum(oracle, families):
    keys, trackers = families
    assert (len(keys), len(trackers)) == (66, 28)
    exceptional = []
    for name, k in keys:
        assert 0 <= k < gm.R == oracle.R, name
        m, steps, exc = gm.walk(k)                       # asserts the argument on every kept sum
        assert m == k and len(steps) == gm.STEPS, name
        kinds = [kind for _, _, kind in steps]
        assert kinds.count(gm.FIRST) == (1 if k else 0), name
        assert kinds.count(gm.KEPT) == max(0, bin(k).count("1") - 1), name
        assert all(kind == gm.IDLE for kind in kinds) == (k == 0), name
        exceptional += [(name, step, what) for step, what in exc]
    assert exceptional == [("r-1", 254, "P+(-P)")]
    assert dict(keys)["r-1"] == gm.R - 1 and dict(keys)["0"] == 0


def test_the_walk_on_a_trackers_own_points_ends_at_krG(oracle, families):
    """The point-level walk over the rG of honest trackers reaches their krG -- what the kernel's end compares -- and on
    k = r - 1 the discarded sum of the last step is exactly P + (-P) on those points."""
    keys, trackers = families
    kv, tv = dict(keys), dict(trackers)
    for name in ("1", "2", "r-1", "lambda", "random 0"):
        t = tv["honest " + name]
        rG, krG = tom.decompress(oracle, t[:48]), tom.decompress(oracle, t[48:])
        got, exc = gm.walk_points(oracle, kv[name], rG)
        assert got == krG, name
        assert exc == ([(254, "P+(-P)")] if name == "r-1" else []), name
    t = tv["krG negated, lambda"]
    got, _ = gm.walk_points(oracle, kv["lambda"], tom.decompress(oracle, t[:48]))
    assert got == oracle.neg(tom.decompress(oracle, t[48:]))      # equal x, opposite y: eq_x holds, eq_y decides
    assert gm.walk_points(oracle, 0, tom.decompress(oracle, tv["honest 1"][:48])) == (None, [])
    assert gm.walk_points(oracle, kv["random 0"], None) == (None, [])


def test_the_launch_rule_against_counts_worked_out_by_hand():
    # P = 256: 300 trackers are chunks of 256 + 44, one key a launch: 2 x 5
    assert launches(300, 5, 256) == 10
    # P = 512: tc = 300, kc = 512 / 300 = 1: 1 x 5
    assert launches(300, 5, 512) == 5
    # 1,000 rounds down to 768: tc = 300, kc = 2: 1 x ceil(5 / 2)
    assert launches(300, 5, 1000) == 3
    # 64 trackers: kc = 4, 8, 12 of 9 keys
    assert [launches(64, 9, p) for p in (256, 512, 1000)] == [3, 2, 1]
    # anything below 256 is 256
    assert [launches(300, 5, p) for p in (0, 1, 255, 257, 511)] == [10] * 5
    # the default, 2^18 lanes: 1,024 keys x 256 trackers are exactly one launch, one key more is two
    assert launches(256, 1024) == 1 and launches(256, 1025) == 2
    # 4,100 trackers: kc = 262,144 / 4,100 = 63 keys a launch
    assert launches(4100, 63) == 1 and launches(4100, 64) == 2 and launches(4100, 65) == 2
    # a full pass holds two keys a launch; one tracker more is a second pass of one tracker, every key in one launch
    assert launches(PASS, 2) == 1 and launches(PASS, 3) == 2
    assert launches(PASS + 1, 1) == 2 and launches(PASS + 1, 3) == 3
    # the largest calls: 2^20 trackers x 16 keys are eight passes of eight launches
    assert launches(1 << 20, 16) == 64
