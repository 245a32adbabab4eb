"""Child process of tests/test_stream_plan_gpu.py: the stream plan of pipelined MSMs is chosen when the context is
created, so every plan is exercised in a process of its own.

    python tests/stream_plan_child.py EXPECTED_PLAN

The environment decides the plan (GPU_MAX_HW_QUEUES, CURDLE_STREAM_PLAN).  Runs the checks in order, stops at the first
one that fails, and prints one JSON line {check name: "ok" | error text}.  Every comparison is on results, never on
timing."""
import json
import os
import sys
import threading
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "oracle", "py"), os.path.join(ROOT, "go-curdleproofs_amd")):
    sys.path.insert(0, p)

CHECKS = ["plan", "in_flight", "out_of_order", "slot_reuse", "mixed_calls", "two_threads", "second_context"]
N_BIG = 65537            # the first two-level shape
VARIANTS = 7             # scalar vectors per shape: MSM_SLOTS - 1 different MSMs in flight


def main():
    expected_plan = sys.argv[1]
    import torch
    import curdlemsm as cm
    import bls12381_ref as o
    import coracle as co

    results = {}
    cm.init(0)
    dev = torch.device("cuda:0")
    k, q = o.Rand(22).get_frs(2)
    pts = co.points_walk(k, q, N_BIG)                     # P_i = (k + i q) G: every shape is a prefix of the same walk
    d_pts = torch.from_numpy(pts.view(np.int64)).to(dev)
    rng = np.random.default_rng(22)
    sc = rng.integers(0, 1 << 64, size=(VARIANTS, N_BIG, 4), dtype=np.uint64)
    sc[:, :, 3] &= np.uint64((1 << 62) - 1)               # < r
    d_sc = [torch.from_numpy(sc[j].view(np.int64)).to(dev) for j in range(VARIANTS)]
    torch.cuda.synchronize()
    P = d_pts.data_ptr()

    # shape name -> (n, submit / sync keyword arguments)
    shapes = {"n300": (300, {}), "n8192": (8192, {}), "n65537": (N_BIG, {}), "range65536": (65536, {"win_begin": 0, "win_end": 1})}
    refs = {}                                             # (shape, variant) -> the synchronous call's result, computed once

    def ref(shape, j):
        if (shape, j) not in refs:
            n, kw = shapes[shape]
            refs[(shape, j)] = cm.msm_g1_device(P, d_sc[j].data_ptr(), n, **kw)
        return refs[(shape, j)]

    def submit(shape, j):
        n, kw = shapes[shape]
        return cm.msm_g1_device_submit(P, d_sc[j].data_ptr(), n, **kw)

    def same(got, shape, j, what):
        assert (got == ref(shape, j)).all(), f"{what}: {shape} variant {j} differs from the synchronous call"

    def in_flight_set(label):
        for shape in shapes:
            for j in range(VARIANTS):
                ref(shape, j)
            for m in (1, 4, cm.MSM_SLOTS - 1):
                tickets = [submit(shape, j) for j in range(m)]
                for j, t in enumerate(tickets):
                    same(cm.msm_wait(t), shape, j, f"{label} {m} in flight")

    def check_plan():
        queues = int(os.environ.get("GPU_MAX_HW_QUEUES") or 4)
        got = cm.msm_stream_plan(queues)
        assert got["plan"] == expected_plan, (queues, got)
        if expected_plan == "compact":
            assert got["busy_streams"] == 4, got

    def check_in_flight():
        in_flight_set("context 0")
        for shape in ("n300", "n8192"):                   # ... and the synchronous call itself against the oracle
            n = shapes[shape][0]
            for j in range(VARIANTS):
                exp = co.msm_pippenger(pts[:n], sc[j, :n], threads=4)
                assert (ref(shape, j) == exp).all(), f"{shape} variant {j}: the synchronous call differs from the oracle"

    def check_out_of_order():
        t = [submit("n8192", j) for j in range(6)]
        for j in (5, 0, 1, 2, 3, 4):                      # wait(t0) returns while later tails may still be queued
            same(cm.msm_wait(t[j]), "n8192", j, "out-of-order wait")
        t = [submit("n65537" if j & 1 else "n300", j) for j in range(6)]
        for j in (5, 0, 4, 1, 3, 2):
            same(cm.msm_wait(t[j]), "n65537" if j & 1 else "n300", j, "out-of-order wait, mixed sizes")

    def check_slot_reuse():
        t = [submit("n8192", j) for j in range(4)]
        same(cm.msm_wait(t[0]), "n8192", 0, "before reuse")
        big = submit("n65537", 5)                          # the freed slot, at once, with a larger n; three others in flight
        for j in (1, 2, 3):
            same(cm.msm_wait(t[j]), "n8192", j, "beside the reused slot")
        same(cm.msm_wait(big), "n65537", 5, "reused slot")

    def check_mixed_calls():
        a = submit("n8192", 1)
        n, kw = shapes["n65537"]
        sync = cm.msm_g1_device(P, d_sc[2].data_ptr(), n, **kw)   # a synchronous call between two submits
        b = submit("range65536", 3)
        same(sync, "n65537", 2, "synchronous call between submits")
        same(cm.msm_wait(b), "range65536", 3, "submit after a synchronous call")
        same(cm.msm_wait(a), "n8192", 1, "submit before a synchronous call")
        t = [submit("n300", j % VARIANTS) for j in range(cm.MSM_SLOTS)]
        try:
            submit("n300", 0)
            raise AssertionError("a submit with every slot taken succeeded")
        except cm.CurdleError as e:
            assert e.code == cm.EBUSY, e
        same(cm.msm_wait(t[3]), "n300", 3, "wait with every slot taken")
        extra = submit("n8192", 4)                         # recovery: the freed slot takes a call
        same(cm.msm_wait(extra), "n8192", 4, "submit after CURDLE_EBUSY")
        for j, tk in enumerate(t):
            if j != 3:
                same(cm.msm_wait(tk), "n300", j % VARIANTS, "draining after CURDLE_EBUSY")

    def check_two_threads():
        for j in range(VARIANTS):
            ref("n8192", j), ref("n300", j)
        errors = []

        def worker(shape, first):
            try:
                pending = []
                for i in range(10):
                    if len(pending) == 3:
                        j, tk = pending.pop(0)
                        same(cm.msm_wait(tk), shape, j, "two threads")
                    j = (first + i) % VARIANTS
                    pending.append((j, submit(shape, j)))
                for j, tk in pending:
                    same(cm.msm_wait(tk), shape, j, "two threads")
            except BaseException as e:                     # noqa: BLE001 -- handed to the main thread
                errors.append(e)

        th = [threading.Thread(target=worker, args=a) for a in (("n8192", 0), ("n300", 3))]
        for x in th:
            x.start()
        for x in th:
            x.join()
        if errors:
            raise errors[0]

    def check_second_context():
        devs = [int(x) for x in os.environ.get("CURDLE_TEST_DEVICES", "0,0").split(",")]
        cm.init_devices(devs)
        errors = []

        def run():
            try:
                cm.set_device(1)
                in_flight_set("context 1")                 # against context 0's synchronous results
            except BaseException as e:                     # noqa: BLE001
                errors.append(e)

        x = threading.Thread(target=run)
        x.start()
        x.join()
        cm.set_device(-1)
        cm.shutdown()
        if errors:
            raise errors[0]

    for name in CHECKS:
        try:
            locals()["check_" + name]()
            results[name] = "ok"
        except BaseException as e:                         # noqa: BLE001 -- reported; nothing more runs on the GPU after a failure
            results[name] = "".join(traceback.format_exception_only(type(e), e)).strip()[-1500:]
            break
    print("STREAM_PLAN_CHILD " + json.dumps(results), flush=True)


if __name__ == "__main__":
    main()
