"""Generating Whisk tracker proofs in bulk: curdle_whisk_generate_tracker_proof_batch_blinders (one call, on the GPU)
against the only thing there was before it -- k calls of curdle_whisk_generate_tracker_proof (host code, one proof
each) spread over 1 and over 16 host threads -- in ONE process on one machine.

    python tools/bench_tracker_prove.py [--out profiles/r14_tracker_prove.json]

Per k (64, 1,024, 8,192, 65,536 members tiled over 12 distinct (tracker, k) pairs) and form: 2 warm-ups, then 7
repetitions; recorded are the median wall time, the spread (max - min) / median and members per second.  The calls go
through ctypes on prepared arrays; a loop thread runs `for i in its share: single call` in Python, whose overhead per
call (about a microsecond against 280) stays inside the figure.  ctypes releases the interpreter lock around every
call, so the 16 threads run on 16 cores.  Every batch is checked once, untimed: all members CURDLE_OK and accepted by
curdle_whisk_is_valid_tracker_proof_batch.

The compression kernel is also timed alone by HIP events, at the 3 k points a batch of k members compresses:
curdle_g1_compress_batch_device over resident Jacobian points on a stream, between two events on that stream (the
generator's own launch reads the XYZZ form; the inversion chain, which is all but a few products, is the same).
The last line printed is the JSON that --out also receives."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (64, 1024, 8192, 65536)
THREADS = (1, 16)
WARM, REPS = 2, 7


def timed(call):
    wall = []
    for rep in range(WARM + REPS):
        w0 = time.perf_counter()
        call()
        w1 = time.perf_counter()
        if rep >= WARM:
            wall.append(w1 - w0)
    return wall


def row(wall, k):
    med = statistics.median(wall)
    return {"wall_ms": round(med * 1e3, 4), "spread": round((max(wall) - min(wall)) / med, 4),
            "wall_min_ms": round(min(wall) * 1e3, 4), "wall_max_ms": round(max(wall) * 1e3, 4), "members_per_s": round(k / med)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default=",".join(str(s) for s in SIZES))
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    sys.path[:0] = [os.path.join(ROOT, "go-curdleproofs_amd"), os.path.join(ROOT, "oracle", "py")]
    import numpy as np
    import torch
    import curdlemsm as cm
    import bls12381_ref as o

    if not cm.device_available():
        raise SystemExit("no HIP device: this benchmark measures the GPU path")
    cm.init(0)
    lib, vp = cm._lib, C.c_void_p
    batch = lib.curdle_whisk_generate_tracker_proof_batch_blinders
    single = lib.curdle_whisk_generate_tracker_proof

    rand = o.Rand(1)
    pool = []
    for _ in range(12):
        k, r = rand.get_fr(), rand.get_fr()
        rG = o.scalar_mul(r, o.G1)
        pool.append((o.compress(rG) + o.compress(o.scalar_mul(k, rG)), o.fr_to_mont_limbs(k), o.compress(o.scalar_mul(k, o.G1))))
    kmax = max(sizes)
    rng = np.random.default_rng(14)
    which = rng.integers(len(pool), size=kmax)
    trackers = np.frombuffer(b"".join(pool[w][0] for w in which), dtype=np.uint8).copy()
    k_comms = np.frombuffer(b"".join(pool[w][2] for w in which), dtype=np.uint8).copy()
    ks = np.array([p[1] for p in pool], dtype=np.uint64)[which].copy()
    blinders = rng.integers(0, 1 << 62, size=(kmax, 4), dtype=np.uint64)   # Montgomery limbs below 2^254 < r, taken as they are
    rands = [cm.Rand(100 + t) for t in range(max(THREADS))]

    res = {"tool": "bench_tracker_prove", "warmups": WARM, "reps": REPS, "statistic": "median of the repetitions",
           "reference": "k single calls (curdle_whisk_generate_tracker_proof) over 1 and 16 host threads, same process",
           "cpus_seen": len(os.sched_getaffinity(0)), "sizes": {}}
    for k in sizes:
        proofs = np.zeros((k, 128), dtype=np.uint8)
        results = np.zeros(k, dtype=np.int32)
        out = res["sizes"][str(k)] = {}

        def run_batch():
            rc = batch(trackers.ctypes.data, ks.ctypes.data, blinders.ctypes.data, k, proofs.ctypes.data, results.ctypes.data)
            if rc != 0:
                raise SystemExit("batch k=%d: rc %d (%s)" % (k, rc, cm.last_error()))

        out["batch"] = row(timed(run_batch), k)
        if results.any():
            raise SystemExit("batch k=%d: a member failed" % k)
        plist = [p.tobytes() for p in proofs]
        tl = [trackers[96 * i: 96 * i + 96].tobytes() for i in range(k)]
        kl = [k_comms[48 * i: 48 * i + 48].tobytes() for i in range(k)]
        if not (cm.whisk_is_valid_tracker_proof_batch(tl, kl, plist) == 1).all():
            raise SystemExit("batch k=%d: a generated proof was not accepted" % k)

        loop_out = np.zeros((k, 128), dtype=np.uint8)
        t_ptr, k_ptr, o_ptr = trackers.ctypes.data, ks.ctypes.data, loop_out.ctypes.data
        for nt in THREADS:
            failed = []

            def share(t, nt=nt):
                h = rands[t]._h
                for i in range(t * k // nt, (t + 1) * k // nt):
                    if single(t_ptr + 96 * i, k_ptr + 32 * i, h, o_ptr + 128 * i) != 0:
                        failed.append(i)

            def run_loop(nt=nt):
                th = [threading.Thread(target=share, args=(t,)) for t in range(1, nt)]
                [t.start() for t in th]
                share(0)
                [t.join() for t in th]

            out["loop_%d_threads" % nt] = row(timed(run_loop), k)
            if failed:
                raise SystemExit("loop k=%d: a single call failed" % k)
        out["batch_over_loop_16"] = round(out["batch"]["wall_ms"] / out["loop_16_threads"]["wall_ms"], 4)

        # the compression kernel alone, 3 k resident Jacobian points
        n = 3 * k
        jac = np.tile(np.array([o.jac_to_mont_limbs(o.scalar_mul(7 + j, o.G1)) for j in range(8)], dtype=np.uint64), ((n + 7) // 8, 1))[:n]
        jac[:, 12:] = rng.integers(1, 1 << 62, size=(n, 6), dtype=np.uint64)   # some Z below p; the kernel checks nothing
        d_in = torch.from_numpy(jac.view(np.int64).copy()).to("cuda:0")
        d_out = torch.zeros(n * 48, dtype=torch.uint8, device="cuda:0")
        s = torch.cuda.Stream()
        kms = []
        for rep in range(WARM + REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(s):
                e0.record()
                cm.g1_compress_batch_device(d_in.data_ptr(), n, d_out.data_ptr(), stream=s.cuda_stream)
                e1.record()
            e1.synchronize()
            if rep >= WARM:
                kms.append(e0.elapsed_time(e1))
        out["compress_kernel_points"] = n
        out["compress_kernel_ms"] = round(statistics.median(kms), 4)
        out["compress_kernel_spread"] = round((max(kms) - min(kms)) / statistics.median(kms), 4)
        print("k=%d %s" % (k, json.dumps(out)), file=sys.stderr, flush=True)
    slower = [k for k in sizes if res["sizes"][str(k)]["batch_over_loop_16"] > 1]
    res["batch_slower_than_16_thread_loop_at"] = slower
    res["stat_tracker_prove"] = cm.stat_tracker_prove()
    text = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
