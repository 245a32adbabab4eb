"""Wall time of curdle_whisk_is_valid_tracker_proof_batch against loops of the single call
(curdle_whisk_is_valid_tracker_proof) on 1 and 16 host threads, for k in {1, 64, 1024, 8192}
honest tracker proofs (a pool of 64 distinct members, cycled).  Every timed batch is checked
against the single call's answers.  Prints one JSON line.
    python tools/bench_tracker_batch.py [--reps 5] [--sizes 1024] [--batch-only]
--batch-only times the batch alone (the kernel-trace run: rocprofv3 --kernel-trace --stats -- python ...).
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "go-curdleproofs_amd"), os.path.join(ROOT, "oracle", "py")]
import numpy as np  # noqa: E402
import curdlemsm as cm  # noqa: E402
import bls12381_ref as o  # noqa: E402


def pool(n):
    rand = o.Rand(1)
    out = []
    for j in range(n):
        k, r = rand.get_fr(), rand.get_fr()
        rG = o.scalar_mul(r, o.G1)
        tracker = o.compress(rG) + o.compress(o.scalar_mul(k, rG))
        proof = cm.whisk_generate_tracker_proof(tracker, np.array(o.fr_to_mont_limbs(k), dtype=np.uint64), cm.Rand(j))
        out.append((tracker, o.compress(o.scalar_mul(k, o.G1)), proof))
    return out


def best(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1,64,1024,8192")
    ap.add_argument("--batch-only", action="store_true")
    a = ap.parse_args()
    if not cm.device_available():
        raise SystemExit("no HIP device visible: this benchmark measures the GPU path")
    cm.init(0)
    members = pool(64)
    single = [1 if cm.whisk_is_valid_tracker_proof(*m) else 0 for m in members]
    out = {"tool": "bench_tracker_batch", "reps": a.reps, "sizes": {}}
    with ThreadPoolExecutor(16) as ex:
        for k in (int(v) for v in a.sizes.split(",")):
            batch = [members[i % len(members)] for i in range(k)]
            want = [single[i % len(members)] for i in range(k)]
            t, kc, p = (list(c) for c in zip(*batch))
            for _ in range(2):  # warm-up: buffers grown, code objects loaded
                assert cm.whisk_is_valid_tracker_proof_batch(t, kc, p).tolist() == want

            def run_batch():
                assert cm.whisk_is_valid_tracker_proof_batch(t, kc, p).tolist() == want  # the call synchronises

            def loop1():
                assert [cm.whisk_is_valid_tracker_proof(*m) for m in batch] == [bool(w) for w in want]

            def loop16():
                assert list(ex.map(lambda m: cm.whisk_is_valid_tracker_proof(*m), batch)) == [bool(w) for w in want]

            tb = best(run_batch, a.reps)
            res = out["sizes"][str(k)] = {"batch_ms": round(tb * 1e3, 3), "batch_proofs_per_s": round(k / tb)}
            if not a.batch_only:
                reps_single = a.reps if k <= 1024 else 1
                t1 = best(loop1, reps_single)
                t16 = best(loop16, reps_single)
                res.update(single_1thread_ms=round(t1 * 1e3, 3), single_16threads_ms=round(t16 * 1e3, 3),
                           batch_vs_16threads=round(t16 / tb, 2))
            print(f"k={k}: {res}", file=sys.stderr, flush=True)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
