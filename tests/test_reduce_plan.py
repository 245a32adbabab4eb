"""The segment length of the bucket reduction as make_plan decides it, read through curdle_msm_reduce_plan (no device):
a pipelined single MSM sizes its segments for a whole round of lanes (131,072: 32,768 quads), a synchronous one for
three waves per SIMD (196,608), and both start from what the size rule gives."""
import pytest


def test_pipelined_single_msms_take_a_round_of_lanes(cm):
    whole = cm.msm_reduce_plan(1 << 20, pipelined=True)
    assert whole == {"reduce_bits": 1, "two_level": 1, "seg": 8, "G": 16, "NS": 32768, "window_bits": 16, "max_small": 8, "L": 128}
    assert cm.msm_reduce_plan(1 << 22, pipelined=True)["seg"] == 8
    # the ranks of the window split: 1, 2 and 4 of the eight windows (32,768 buckets each) start from 4 buckets and stay there
    for we in (1, 2, 4):
        p = cm.msm_reduce_plan(1 << 20, 0, 0, we, pipelined=True)
        assert (p["seg"], p["NS"]) == (4, 8192 * we)
    for logn in range(9, 25):
        for n in (1 << logn, (1 << logn) + 1, 3 << (logn - 1)):
            p = cm.msm_reduce_plan(n, pipelined=True)
            assert p["reduce_bits"] == 1 and p["seg"] & (p["seg"] - 1) == 0
            assert 4 * p["NS"] <= 131072 or p["seg"] == 64, (n, p)
            if p["seg"] > 4:       # lengthened: half the length would not have fitted the round
                assert 8 * p["NS"] > 131072, (n, p)


def test_synchronous_plans_are_what_they_were(cm):
    for n, seg in ((1268, 1), (1 << 16, 1), (1 << 18, 2), (1 << 20, 8), (1 << 24, 8)):
        assert cm.msm_reduce_plan(n)["seg"] == seg, n
    assert cm.msm_reduce_plan(1 << 20, 0, 0, 1)["seg"] == 1
    assert cm.msm_reduce_plan(100)["reduce_bits"] == 0          # below 300 pairs: the form with a scalar multiple


def test_the_knob_and_bad_arguments(cm):
    with cm.knobs(REDUCE_SEG=32):
        assert cm.msm_reduce_plan(1 << 20, pipelined=True)["seg"] == 32
    assert cm.msm_reduce_plan(1 << 20, pipelined=True)["seg"] == 8
    for bad in ((1 << 27) + 1, 0, 0, -1), (1 << 20, 3, 0, -1), (1 << 20, 17, 0, -1), (1 << 20, 16, 5, 3), (1 << 20, 16, 0, 9):
        with pytest.raises(cm.CurdleError):
            cm.msm_reduce_plan(*bad)
