"""The stream plan of pipelined MSMs (curdle_msm_stream_plan), without a device: which plan a context takes from the
hardware queues its process has (GPU_MAX_HW_QUEUES) and the STREAM_PLAN knob, and the streams the plan keeps busy."""
import pytest


@pytest.mark.parametrize("queues", [1, 2, 4, 8])
def test_fewer_than_sixteen_queues_take_the_compact_plan(cm, queues):
    whole = cm.msm_stream_plan(queues)
    assert whole["plan"] == "compact"
    # a whole pipelined MSM: main_stream, main_extra[0], pre_stream and the one shared tail stream
    assert (whole["main_streams"], whole["pre_streams"], whole["tail_streams"]) == (2, 1, 1)
    assert whole["busy_streams"] == 4
    rng = cm.msm_stream_plan(queues, window_range=True)
    assert rng["plan"] == "compact" and rng["tail_streams"] == 1 and rng["main_streams"] == 2
    assert rng["pre_streams"] == 1 and rng["busy_streams"] == 4      # measured: a second sort stream is a fifth busy stream


@pytest.mark.parametrize("queues", [16, 17, 32])
def test_from_sixteen_queues_the_wide_plan_stays(cm, queues):
    whole = cm.msm_stream_plan(queues)
    assert whole["plan"] == "wide"
    assert (whole["main_streams"], whole["pre_streams"], whole["tail_streams"]) == (2, 1, cm.MSM_SLOTS)
    assert cm.msm_stream_plan(queues, window_range=True)["pre_streams"] == 2


def test_the_boundary_is_sixteen(cm):
    assert cm.msm_stream_plan(15)["plan"] == "compact" and cm.msm_stream_plan(16)["plan"] == "wide"


def test_the_knob_forces_the_plan(cm):
    with cm.knobs(STREAM_PLAN=cm.STREAM_PLAN_WIDE):
        for queues in (1, 4, 16):
            assert cm.msm_stream_plan(queues)["plan"] == "wide"
    with cm.knobs(STREAM_PLAN=cm.STREAM_PLAN_COMPACT):
        for queues in (4, 16, 32):
            p = cm.msm_stream_plan(queues)
            assert p["plan"] == "compact" and p["busy_streams"] == 4
    with cm.knobs(STREAM_PLAN=cm.STREAM_PLAN_AUTO):
        assert cm.msm_stream_plan(4)["plan"] == "compact" and cm.msm_stream_plan(16)["plan"] == "wide"
    with cm.knobs(STREAM_PLAN=3):
        with pytest.raises(cm.CurdleError) as e:
            cm.msm_stream_plan(4)
        assert e.value.code == cm.EINVAL
    assert cm.msm_stream_plan(4)["plan"] == "compact" and cm.msm_stream_plan(16)["plan"] == "wide"   # unset again


def test_the_accumulate_stream_knob_shows_in_the_plan(cm):
    with cm.knobs(MAIN_STREAMS=1):
        assert cm.msm_stream_plan(4)["main_streams"] == 1 and cm.msm_stream_plan(4)["busy_streams"] == 3
    with cm.knobs(MAIN_STREAMS=4):
        assert cm.msm_stream_plan(4)["main_streams"] == 2          # the compact plan never has more than four busy streams
        assert cm.msm_stream_plan(16)["main_streams"] == 4


@pytest.mark.parametrize("queues", [0, -1, -16])
def test_a_queue_count_below_one_is_refused(cm, queues):
    with pytest.raises(cm.CurdleError) as e:
        cm.msm_stream_plan(queues)
    assert e.value.code == cm.EINVAL


def test_whole_or_range_is_checked(cm):
    import ctypes as C
    out = (C.c_uint32 * 4)()
    assert cm._msm_stream_plan(4, 2, out) == cm.EINVAL
    assert cm._msm_stream_plan(4, 0, None) == cm.EINVAL
