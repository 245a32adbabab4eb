"""What the batched Merlin transcripts cost, in one run:
  (P) the primitive: curdle_transcript_batch against curdle_transcript_batch_host on --threads host threads for the
      verifier's prelude (4 ell + 1 encodings appended, ell challenges drawn) at ell = 124 and 252 and k = 64, 1,024 and
      8,192 members; the two agree bit for bit; the device call's wall time, and its kernel alone by HIP events
      (curdle_transcript_last_kernel_ms);
  (W) the Whisk batch of --proofs proofs (eight distinct honest shuffles, repeated, as bench.py's whisk-batch leg) on
      --threads threads with knob GPU_PRELUDE off and on.
Medians of the timed repetitions after warm-up, with min / max.  One JSON line.
    python tools/bench_transcript_batch.py [--reps 7] [--warmup 2] [--pkg DIR] [--label NAME] [--only-off]
--pkg: import curdlemsm from another tree's go-curdleproofs_amd (the parent's Whisk batch on the same machine);
--only-off: the Whisk batch with the knob off alone, which is all a build without the batched transcripts can run.
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
ap.add_argument("--ells", default="124,252")
ap.add_argument("--members", default="64,1024,8192")
ap.add_argument("--pkg", default=None)
ap.add_argument("--label", default="this")
ap.add_argument("--only-off", action="store_true")
ap.add_argument("--skip-whisk", action="store_true")
args = ap.parse_args()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, args.pkg or os.path.join(ROOT, "go-curdleproofs_amd"))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
import numpy as np  # noqa: E402
import curdlemsm as cm  # noqa: E402

cm.init(0)


def timed(fn):
    for _ in range(args.warmup):
        fn()
    ms = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": round(statistics.median(ms), 2), "ms_min": round(min(ms), 2), "ms_max": round(max(ms), 2),
            "ms": [round(x, 2) for x in ms]}


out = {"label": args.label, "threads": args.threads, "reps": args.reps, "warmup": args.warmup,
       "GPU_MAX_HW_QUEUES": os.environ.get("GPU_MAX_HW_QUEUES"), "CURDLE_TRANSCRIPT_LANES": os.environ.get("CURDLE_TRANSCRIPT_LANES"),
       "lib": os.path.relpath(cm.LIB_PATH, ROOT)}

if not args.only_off:
    out["primitive"] = {}
    for ell in [int(x) for x in args.ells.split(",")]:
        program = [(cm.TR_APPEND, b"curdleproofs_step1", 4 * ell + 1, 48), (cm.TR_CHALLENGES, b"curdleproofs_vec_a", ell, 0)]
        for k in [int(x) for x in args.members.split(",")]:
            data = np.random.default_rng(ell + k).integers(0, 256, size=(k, 48 * (4 * ell + 1)), dtype=np.uint8)
            want = cm.transcript_batch(program, data, label=b"curdleproofs", host=True, nthreads=args.threads)
            got = cm.transcript_batch(program, data, label=b"curdleproofs")
            assert all((a == b).all() for a, b in zip(want, got))
            kernel = []

            def device():
                cm.transcript_batch(program, data, label=b"curdleproofs")
                kernel.append(cm.transcript_last_kernel_ms())

            dev = timed(device)
            host = timed(lambda: cm.transcript_batch(program, data, label=b"curdleproofs", host=True, nthreads=args.threads))
            out["primitive"]["ell%d_k%d" % (ell, k)] = {
                "device": dev, "host_%d_threads" % args.threads: host,
                "kernel_ms_median": round(statistics.median(kernel[args.warmup:]), 3),
                "device_over_host": round(dev["ms_median"] / host["ms_median"], 3)}

if not args.skip_whisk:
    ONE = np.array([0x760900000002fffd, 0xebf4000bc40c0002, 0x5f48985753c758ba, 0x77ce585370525745, 0x5c071a97a256ec6d,
                    0x15f65ec3fa80e493], dtype=np.uint64)
    compress = lambda aff: cm.g1_compress(np.concatenate([aff, ONE]))  # noqa: E731
    crs = cm.CRS(cm.WHISK_ELL, cm.Rand(0))
    sets = []
    for j in range(8):
        r = cm.Rand(10 + j)
        pts = r.get_g1_affines(2 * cm.WHISK_ELL)
        pre = [compress(pts[2 * i]) + compress(pts[2 * i + 1]) for i in range(cm.WHISK_ELL)]
        post, proof = cm.whisk_generate_shuffle_proof(crs, pre, r)
        sets.append((pre, post, proof))
    k = args.proofs
    batch = cm.PreparedWhiskBatch([sets[i % 8][0] for i in range(k)], [sets[i % 8][1] for i in range(k)], [sets[i % 8][2] for i in range(k)])
    honest = [True] * k
    seed = [100]

    def run():
        seed[0] += 1
        assert list(batch.run(crs, cm.Rand(seed[0] * 1000), nthreads=args.threads)) == honest

    res = {"proofs": k, "knob_off": timed(run)}
    res["knob_off_spread_ms"] = round(res["knob_off"]["ms_max"] - res["knob_off"]["ms_min"], 2)
    if not args.only_off:
        s0 = cm.stat_transcript()
        with cm.knobs(GPU_PRELUDE=1):
            res["knob_on"] = timed(run)
        s1 = cm.stat_transcript()
        res["knob_on_members_hashed_on_device"] = int(s1["members"] - s0["members"])
        res["knob_off_again"] = timed(run)
        gain = res["knob_off"]["ms_median"] - res["knob_on"]["ms_median"]
        res["off_minus_on_ms"] = round(gain, 2)
        res["aim_on_beats_off_by_more_than_off_spread"] = bool(gain > res["knob_off_spread_ms"])
    out["whisk_batch"] = res
print(json.dumps(out))
