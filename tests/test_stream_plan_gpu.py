"""Pipelined MSMs under each stream plan on the GPU.  A context chooses its plan when it is created, so each plan runs
in a fresh child process (tests/stream_plan_child.py), three in all, one after the other, each under its own time
limit: the environment's queue count with the library's choice, the compact plan forced, and the wide plan forced with
16 hardware queues.  A child runs every check once; the tests below read its report."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

CHILD_LIMIT_S = 240
CONFIGS = {
    # name: (environment on top of the caller's, the plan the context must take)
    "auto": ({"CURDLE_STREAM_PLAN": ""}, None),            # by the environment's queue count
    "compact": ({"CURDLE_STREAM_PLAN": "2"}, "compact"),
    "wide16": ({"CURDLE_STREAM_PLAN": "1", "GPU_MAX_HW_QUEUES": "16"}, "wide"),
}
CHECKS = ["plan", "in_flight", "out_of_order", "slot_reuse", "mixed_calls", "two_threads", "second_context"]
_reports = {}
_stop = []            # a child died: nothing more is started on the GPU


def _expected(name):
    plan = CONFIGS[name][1]
    if plan is None:
        plan = "compact" if int(os.environ.get("GPU_MAX_HW_QUEUES") or 4) < 16 else "wide"
    return plan


def _report(name):
    if name in _reports:
        return _reports[name]
    if _stop:
        pytest.fail("not run: an earlier child process " + _stop[0])
    env = dict(os.environ)
    for k, v in CONFIGS[name][0].items():
        if v:
            env[k] = v
        else:
            env.pop(k, None)
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "stream_plan_child.py"), _expected(name)],
                           env=env, capture_output=True, text=True, timeout=CHILD_LIMIT_S, cwd=ROOT)
    except subprocess.TimeoutExpired:
        _stop.append(f"({name}) ran into its time limit")
        pytest.fail(f"child {name} ran into its time limit of {CHILD_LIMIT_S} s")
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("STREAM_PLAN_CHILD ")]
    if p.returncode != 0 or not lines:
        _stop.append(f"({name}) ended with status {p.returncode}")
        pytest.fail(f"child {name}: status {p.returncode}\n{p.stdout[-1500:]}\n{p.stderr[-2500:]}")
    _reports[name] = json.loads(lines[-1][len("STREAM_PLAN_CHILD "):])
    return _reports[name]


@pytest.mark.gpu
@pytest.mark.parametrize("check", CHECKS)
@pytest.mark.parametrize("config", list(CONFIGS))
def test_pipelined_calls_under_the_plan(gpu, config, check):
    """plan: the context took the expected plan (four busy streams when compact).  in_flight: 1, 4 and MSM_SLOTS - 1
    MSMs in flight at n = 300, 8,192, 65,537 and windows [0, 1) of 65,536 equal the synchronous call bit for bit, which
    equals the oracle at 300 and 8,192.  out_of_order: t5 first, then t0, then the rest.  slot_reuse: the freed slot
    takes a larger n at once beside three in flight.  mixed_calls: a synchronous call between submits; CURDLE_EBUSY
    with every slot taken, then recovery.  two_threads: three in flight each, ten MSMs each.  second_context: the
    in-flight set on a second context."""
    report = _report(config)
    assert report.get(check, "not run: an earlier check of this child failed") == "ok"
