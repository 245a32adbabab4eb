"""The bucket reduction of a pipelined MSM (submit / wait) at the segment lengths its plan now takes: a whole round
of lanes for the form without a scalar multiple (make_plan, msm_plan.hip), where it used to be a quarter round.

Submit / wait against the synchronous call and the C oracle, at small sizes whose pipelined plan has each shape --
read from the plan (curdle_msm_reduce_plan), not guessed: one-bucket segments, the flagship's eight windows of
32,768 buckets, window ranges of one and three windows -- on uniform and skewed scalars, and on inputs built so that
the segment walk itself doubles and returns to infinity at the top, in the middle and at the bottom of a segment."""
import os
import sys

import numpy as np
import pytest

from test_msm_gpu import rand_scalars

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = 16                      # the flagship's window width: eight windows of 32,768 buckets
N = 1 << 16                 # the smallest pair count whose plan at that width sorts in two passes, like the flagship


def _adversarial():
    tools = os.path.join(ROOT, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import adversarial_inputs
    return adversarial_inputs


@pytest.fixture(scope="module")
def inputs(gpu, oracle, coracle):
    """N + 1 walk points and uniform scalars, on the host and on the device; never modified."""
    import torch
    n = N + 1
    k, q = oracle.Rand(41).get_frs(2)
    pts = coracle.points_walk(k, q, n)
    sc = rand_scalars(np.random.default_rng(41), n, oracle)
    d_pts = torch.from_numpy(pts.view(np.int64)).to("cuda:0")
    d_sc = torch.from_numpy(sc.view(np.int64)).to("cuda:0")
    return {"pts": pts, "sc": sc, "d_pts": d_pts, "d_sc": d_sc}


def _both_ways(gpu, d_pts, d_sc, n, c=C, wb=0, we=-1):
    piped = gpu.msm_wait(gpu.msm_g1_device_submit(d_pts.data_ptr(), d_sc.data_ptr(), n, c, wb, we))
    sync = gpu.msm_g1_device(d_pts.data_ptr(), d_sc.data_ptr(), n, window_bits=c, win_begin=wb, win_end=we)
    return piped, sync


@pytest.mark.parametrize("n,c,seg", [(N, C, 8), (N + 1, C, 8), (N, 0, 4), (4096, 0, 1)])
def test_pipelined_call_equals_synchronous_call_and_oracle(gpu, coracle, inputs, n, c, seg):
    """The flagship's shape (eight-bucket segments: 32,768 quads, a whole round of lanes), that size + 1, and the two
    shapes below it that the quarter-round rule had at twice the length: 13-bit windows of unequal widths in
    four-bucket segments, 11-bit windows at one bucket per quad."""
    plan = gpu.msm_reduce_plan(n, c, pipelined=True)
    assert plan["reduce_bits"] == 1 and plan["seg"] == seg and plan["NS"] * 4 <= 131072, plan
    piped, sync = _both_ways(gpu, inputs["d_pts"], inputs["d_sc"], n, c)
    exp = coracle.msm_pippenger(inputs["pts"][:n], inputs["sc"][:n], threads=8)
    assert (piped == sync).all() and (piped == exp).all()


def test_window_ranges_of_one_and_three_windows(gpu, coracle, inputs):
    """One rank's share of the window split: one window and three, pipelined (four-bucket segments either way: the
    rule's starting point); with the rest of the eight windows they sum to the whole MSM."""
    W = gpu.num_windows(N, C)
    assert W == 8
    parts = []
    for wb, we in ((0, 1), (1, 4), (4, W)):
        assert gpu.msm_reduce_plan(N, C, wb, we, pipelined=True)["seg"] == 4
        piped, sync = _both_ways(gpu, inputs["d_pts"], inputs["d_sc"], N, C, wb, we)
        assert (piped == sync).all(), (wb, we)
        parts.append(piped)
    exp = coracle.msm_pippenger(inputs["pts"][:N], inputs["sc"][:N], threads=8)
    assert (gpu.g1_sum(np.stack(parts)) == exp).all()


@pytest.mark.parametrize("family", ["all_equal", "hot_window", "infinity_1pct", "small_9bit"])
def test_skewed_scalars(gpu, coracle, inputs, family):
    """all-equal scalars (two occupied buckets per window, both far beyond the merge limit: the walk reads them as one
    pre-merged fragment each), one hot window, 1 % bases at infinity, scalars of at most 9 bits."""
    import torch
    sc, dead = _adversarial().make_family(family, N, inputs["sc"], window_bits=C)
    sc = np.ascontiguousarray(sc)
    pts, d_pts = inputs["pts"][:N], inputs["d_pts"]
    if dead is not None:
        pts = pts.copy()
        pts[dead] = 0
        d_pts = torch.from_numpy(pts.view(np.int64)).to("cuda:0")
    d_sc = torch.from_numpy(sc.view(np.int64)).to("cuda:0")
    piped, sync = _both_ways(gpu, d_pts, d_sc, N)
    exp = coracle.msm_pippenger(pts, sc, threads=8)
    assert (piped == sync).all() and (piped == exp).all(), family


def test_segment_walk_doubles_and_returns_to_infinity(gpu, oracle, coracle):
    """Inputs built so that the WALK meets the exceptional additions: all scalars zero but a few small ones (the
    split leaves k1 = k, k2 = 0: checked), digit d of a window is bucket d - 1, and a segment of S buckets is walked
    from its top bucket down.  The same base in adjacent buckets makes the running sum equal the next fragment
    (doubling: at a segment's top, in its middle, at its bottom, and with a running sum P3 + P4 in XYZZ form
    meeting the affine-shaped fragment of the same point); P above -P returns the running sum to infinity
    mid-segment, and the walk goes on from there.  The same again in window 1."""
    import torch
    S = gpu.msm_reduce_plan(N, C, pipelined=True)["seg"]
    assert S >= 8
    k, q = oracle.Rand(43).get_frs(2)
    base = coracle.points_walk(k, q, 8)
    aff = [oracle.affine_from_mont_limbs([int(v) for v in row]) for row in base]
    P0, P1, P2, P3, P4, P5, P6, P7 = aff
    rows = []  # (point, bucket of the window)

    def put(pt, segment, u):
        rows.append((pt, S * segment + u))

    put(P0, 5, S - 2), put(P0, 5, S - 3), put(P0, 5, S - 4)   # P0 | + P0: doubling | + P0: 2 P0 + P0
    put(P1, 7, S - 1), put(P1, 7, S - 2)                      # doubling at the top of a segment
    put(P2, 9, 1), put(P2, 9, 0)                              # ... at its bottom
    put(P3, 11, 5), put(P4, 11, 5)                            # the fragments of P3 + P4, then the same point, affine-shaped
    put(oracle.add(P3, P4), 11, 4), put(P5, 11, 1)
    put(P6, 13, S - 1), put(oracle.neg(P6), 13, S - 2), put(P7, 13, 3), put(P7, 13, 2)   # back to infinity, on, doubling
    put(P5, 15, 4), put(oracle.neg(P5), 15, 3)                # the segment ends at infinity ...
    # ... and P, -P at a segment's two ends: the segment sum takes the running sum P in S - 1 times (the second time it
    # EQUALS it: the doubling of the other branch of the step) before the last fragment returns it to infinity
    put(P5, 16, S - 1), put(oracle.neg(P5), 16, 0)
    scal, points = [], []
    for pt, bucket in rows:
        for window in (0, 1):
            points.append(pt)
            scal.append((bucket + 1) << (16 * window))
    # the split of these scalars: k1 = k, k2 = 0, so that exactly these digits reach the buckets
    words = np.array([[(s >> (32 * i)) & 0xFFFFFFFF for i in range(8)] for s in scal], dtype=np.uint32)
    split = gpu.selftest_op(11, words, False)
    assert (split[:, :4] == words[:, :4]).all() and (split[:, 4:8] == 0).all() and (split[:, 8] == 0).all()
    pts = np.zeros((N, 12), dtype=np.uint64)
    pts[:] = base[0]
    sc = np.zeros((N, 4), dtype=np.uint64)
    at = np.random.default_rng(43).choice(N, len(points), replace=False)
    for i, pt, s in zip(at, points, scal):
        pts[i] = oracle.affine_to_mont_limbs(pt)
        sc[i] = oracle.fr_to_mont_limbs(s)
    d_pts = torch.from_numpy(pts.view(np.int64)).to("cuda:0")
    d_sc = torch.from_numpy(sc.view(np.int64)).to("cuda:0")
    piped, sync = _both_ways(gpu, d_pts, d_sc, N)
    exp = coracle.msm_pippenger(pts, sc, threads=8)
    assert (piped == sync).all() and (piped == exp).all()
