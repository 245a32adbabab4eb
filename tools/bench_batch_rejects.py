"""What bad proofs cost curdle_whisk_is_valid_shuffle_proof_batch: k = 1,024 Whisk shuffle proofs, 16 threads, the
members of bench.py's config-5 leg (eight seeded shuffles, repeated), three batches -- every member honest, 16 bad
members (at most one per group of 32), 32 bad members (one in every run of 32) -- a bad member being another shuffle's
post trackers, which passes the direct checks and fails its group's accumulation.  Medians of the timed repetitions
after warm-up, with the spread, and what curdle_stat_dacc_members counted over the timed repetitions (absent in a build
without the member form: null).  One JSON line.
    python tools/bench_batch_rejects.py [--reps 7] [--warmup 2] [--pkg DIR] [--label NAME]
--pkg: import curdlemsm from another tree's go-curdleproofs_amd (an A/B against another build on the same machine).
"""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--proofs", type=int, default=1024)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--pkg", default=None)
ap.add_argument("--label", default="this")
args = ap.parse_args()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, args.pkg or os.path.join(ROOT, "go-curdleproofs_amd"))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
import numpy as np  # noqa: E402
import curdlemsm as cm  # noqa: E402

cm.init(0)
ONE = np.array([0x760900000002fffd, 0xebf4000bc40c0002, 0x5f48985753c758ba, 0x77ce585370525745, 0x5c071a97a256ec6d,
                0x15f65ec3fa80e493], dtype=np.uint64)
compress = lambda aff: cm.g1_compress(np.concatenate([aff, ONE]))  # noqa: E731
crs = cm.CRS(cm.WHISK_ELL, cm.Rand(0))
sets = []
for j in range(8):                                      # bench.py, whisk_batch_leg: the same eight shuffles
    r = cm.Rand(10 + j)
    pts = r.get_g1_affines(2 * cm.WHISK_ELL)
    pre = [compress(pts[2 * i]) + compress(pts[2 * i + 1]) for i in range(cm.WHISK_ELL)]
    post, proof = cm.whisk_generate_shuffle_proof(crs, pre, r)
    sets.append((pre, post, proof))
k = args.proofs


def prepare(bad):
    pres, posts, proofs = [], [], []
    for i in range(k):
        pre, post, proof = sets[i % 8]
        if i in bad:
            post = sets[(i + 1) % 8][1]
        pres.append(pre), posts.append(post), proofs.append(proof)
    return cm.PreparedWhiskBatch(pres, posts, proofs), [i not in bad for i in range(k)]


# members are handed to the workers in index order, a group is 32 consecutive joins of ONE worker: bad members 64 apart
# cannot share a group; one in every run of 32 indices puts about one into every group
batches = {"honest": set(), "bad16": {64 * g + 21 for g in range(k // 64)}, "bad32": {32 * g + 13 for g in range(k // 32)}}
stat = getattr(cm, "stat_dacc_members", None)
seed = [100]
out = {"label": args.label, "proofs": k, "threads": args.threads, "reps": args.reps, "warmup": args.warmup,
       "lib": os.path.relpath(cm.LIB_PATH, ROOT), "batches": {}}
for name, bad in batches.items():
    prepared, expect = prepare(bad)

    def step():
        seed[0] += 1
        t0 = time.perf_counter()
        got = prepared.run(crs, cm.Rand(seed[0] * 1000), nthreads=args.threads)
        dt = (time.perf_counter() - t0) * 1e3
        assert list(got) == expect, f"{name}: accept bits differ"
        return dt
    for _ in range(args.warmup):
        step()
    s0 = stat() if stat else None
    ms = [step() for _ in range(args.reps)]
    s1 = stat() if stat else None
    out["batches"][name] = {"bad": len(bad), "ms_median": round(statistics.median(ms), 2), "ms_min": round(min(ms), 2),
                            "ms_max": round(max(ms), 2), "ms": [round(x, 2) for x in ms],
                            "stat_dacc_members_delta": {key: s1[key] - s0[key] for key in s1} if stat else None}
h = out["batches"]["honest"]["ms_median"]
out["bad16_over_honest"] = round(out["batches"]["bad16"]["ms_median"] / h, 3)
out["bad32_over_honest"] = round(out["batches"]["bad32"]["ms_median"] / h, 3)
print(json.dumps(out))
