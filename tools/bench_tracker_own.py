"""curdle_whisk_find_own_trackers (k_tracker_own) against what a caller could do before it, in ONE process.

    python tools/bench_tracker_own.py [--out profiles/r16_tracker_own.json] [--kernel-stats kernel_stats.csv]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o own -- python tools/bench_tracker_own.py --kernels-only

At every shape (m keys, n trackers) the new call is timed in its host form (pageable arrays in, the (m, n) bytes out)
and its _device form (resident arrays, events on the caller's stream), against
(a) the composition the parent build offers: curdle_g1_decompress_batch over the 2 n records once, then for each key
    one curdle_g1_scalar_mul_batch_device with ONE shared scalar over the resident rG column, the n normalised records
    brought back and compared with the decoded krG column on the host (wall time from the tracker bytes to the matrix);
(b) the host single call curdle_whisk_is_own_tracker, on 1 and on 16 threads: timed over a SAMPLE of the pairs
    (2,048 per thread) and scaled to the shape -- the full grids are minutes to hours of CPU time.

2 warm-ups, then 7 repetitions of every arm in a loop of its own; recorded are the median and the spread
(max - min) / median.  Before anything is timed the results are checked: host form == _device form == the
composition's matrix, and the planted pairs are owned.

--kernels-only runs what the kernel-trace pass needs and nothing else: five _device calls at (64, 4,096) -- ONE launch
of exactly 2^18 quads, the default TRACKER_OWN_PAIRS -- and five curdle_g1_scalar_mul_batch_device calls over 2^18
points with per-point scalars.  --kernel-stats reads that pass's kernel_stats.csv into the JSON: the time of a full
default launch and the per-pair chain of k_tracker_own against k_scalar_mul_batch_quad, the only figure that says what
the wave-uniform key is worth.  The last line printed is the JSON that --out also receives."""
import argparse
import csv
import ctypes as C
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1, 8192), (1, 16384), (16, 16384), (64, 16384), (1024, 256), (1024, 8192))
WARM, REPS = 2, 7
FULL = (64, 4096)          # one launch of 2^18 quads
SAMPLE = 2048              # pairs per thread of the host single call


def stats(ms):
    med = statistics.median(ms)
    return {"ms": round(med, 4), "spread": round((max(ms) - min(ms)) / med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default=";".join("%d,%d" % s for s in SHAPES))
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split(",")) for s in a.shapes.split(";") if s]
    sys.path[:0] = [os.path.join(ROOT, "go-curdleproofs_amd"), os.path.join(ROOT, "oracle", "py")]
    import numpy as np
    import torch
    import curdlemsm as cm
    import bls12381_ref as o

    if not cm.device_available():
        raise SystemExit("no HIP device: this benchmark measures the GPU path")
    cm.init(0)
    rng = np.random.default_rng(16)
    s = torch.cuda.Stream()

    # eight keys with one honest tracker each, eight trackers of strangers; keys beyond the eight are random
    rand = o.Rand(16)
    pool_keys = [rand.get_fr() for _ in range(8)]
    bases = [o.scalar_mul(rand.get_fr(), o.G1) for _ in range(4)]
    trk = [o.compress(bases[j % 4]) + o.compress(o.scalar_mul(k, bases[j % 4])) for j, k in enumerate(pool_keys)]
    trk += [o.compress(bases[j % 4]) + o.compress(o.scalar_mul(rand.get_fr(), bases[j % 4])) for j in range(8)]
    pool = np.frombuffer(b"".join(trk), dtype=np.uint8).reshape(16, 96)
    pool_limbs = np.array([o.fr_to_mont_limbs(k) for k in pool_keys], dtype=np.uint64)

    def inputs(m, n):
        which = rng.integers(16, size=n)
        ks = rng.integers(0, 1 << 64, size=(m, 4), dtype=np.uint64)
        ks[:, 3] &= np.uint64((1 << 62) - 1)                      # Montgomery limbs below r, taken as they are
        ks[:min(m, 8)] = pool_limbs[:min(m, 8)]
        want = np.zeros((m, n), dtype=np.uint8)
        for j in range(min(m, 8)):
            want[j, which == j] = 1
        return np.ascontiguousarray(pool[which]), ks, want

    def events(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            e0.record()
            call()
            e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def wall(call):
        w0 = time.perf_counter()
        call()
        return (time.perf_counter() - w0) * 1e3

    def resident(trackers, ks, m, n):
        d_t = torch.from_numpy(trackers.reshape(-1)).to("cuda:0")
        d_k = torch.from_numpy(ks.view(np.int64)).to("cuda:0")
        d_o = torch.zeros(m * n, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        return d_t, d_k, d_o, lambda: cm.whisk_find_own_trackers_device(d_t.data_ptr(), n, d_k.data_ptr(), m, d_o.data_ptr(),
                                                                        stream=s.cuda_stream)

    if a.kernels_only:
        m, n = FULL
        trackers, ks, want = inputs(m, n)
        d_t, d_k, d_o, call = resident(trackers, ks, m, n)
        for _ in range(5):
            call()
        if not (d_o.cpu().numpy().reshape(m, n) == want).all():
            raise SystemExit("the full launch differs from the planted matrix")
        pts, st = cm.g1_decompress_batch(trackers[:, :48].tobytes())
        big = m * n
        d_p = torch.from_numpy(np.tile(pts, (m, 1)).view(np.int64)).to("cuda:0")
        sc = rng.integers(0, 1 << 64, size=(big, 4), dtype=np.uint64)
        sc[:, 3] &= np.uint64((1 << 62) - 1)
        d_s = torch.from_numpy(sc.view(np.int64)).to("cuda:0")
        d_r = torch.zeros(big * 12, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        for _ in range(5):
            cm.g1_scalar_mul_batch_device(d_p.data_ptr(), d_s.data_ptr(), big, 0, big, d_r.data_ptr())
        print("kernels-only: 5 x k_tracker_own over %d quads, 5 x k_scalar_mul_batch_quad over as many" % big)
        return

    res = {"tool": "bench_tracker_own", "warmups": WARM, "reps": REPS, "statistic": "median of the repetitions",
           "timing": "host form, composition and single call: wall time; _device form: torch (HIP) events on the caller's stream",
           "shapes": {}}
    single = cm._lib.curdle_whisk_is_own_tracker

    for m, n in shapes:
        trackers, ks, want = inputs(m, n)
        out = res["shapes"]["%dx%d" % (m, n)] = {"m": m, "n": n, "pairs": m * n}
        got = [None]

        def host():
            got[0] = cm.whisk_find_own_trackers(trackers, ks)

        d_t, d_k, d_o, dev = resident(trackers, ks, m, n)
        comp = np.zeros((m, n), dtype=np.uint8)
        t_back = torch.zeros((n, 12), dtype=torch.int64).pin_memory()      # a caller reads results back into pinned memory
        back = t_back.numpy().view(np.uint64)

        def composition():
            pts, st = cm.g1_decompress_batch(trackers.tobytes())
            if (st > cm.DECODE_INFINITY).any():
                raise SystemExit("a benchmark tracker did not decode")
            pts = pts.reshape(n, 2, 12)
            krg = np.ascontiguousarray(pts[:, 1])
            with torch.cuda.stream(s):
                d_p = torch.from_numpy(np.ascontiguousarray(pts[:, 0]).view(np.int64)).to("cuda:0", non_blocking=True)
                d_r = torch.empty(n * 12, dtype=torch.int64, device="cuda:0")
                for j in range(m):
                    cm.g1_scalar_mul_batch_device(d_p.data_ptr(), d_k.data_ptr() + 32 * j, 1, 0, n, d_r.data_ptr(),
                                                  stream=s.cuda_stream)
                    t_back.copy_(d_r.view(n, 12), non_blocking=True)
                    s.synchronize()
                    comp[j] = (back == krg).all(axis=1)

        host()
        dev()
        composition()
        if not (got[0] == want).all() or not (d_o.cpu().numpy().reshape(m, n) == want).all() or not (comp == want).all():
            raise SystemExit("%d x %d: the three matrices differ" % (m, n))
        # every arm in a loop of its own: interleaved, the composition's copies were seen to delay the call after them
        t_host = [wall(host) for rep in range(WARM + REPS)][WARM:]
        t_dev = [events(dev) for rep in range(WARM + REPS)][WARM:]
        t_comp = [wall(composition) for rep in range(WARM + REPS)][WARM:]
        out["host_form"], out["device_form"], out["composition"] = stats(t_host), stats(t_dev), stats(t_comp)
        out["host_form_pairs_per_s"] = round(m * n / out["host_form"]["ms"] * 1e3)
        out["device_form_pairs_per_s"] = round(m * n / out["device_form"]["ms"] * 1e3)
        out["composition_over_host_form"] = round(out["composition"]["ms"] / out["host_form"]["ms"], 3)

        # (b) the host single call over a sample of the grid
        kk = np.ascontiguousarray(ks)

        def sample(lo, count, flags):
            owned = C.c_int(0)
            for p in range(lo, lo + count):
                j, i = p % m, (p // m) % n
                if single(trackers[i].ctypes.data, kk[j].ctypes.data, C.byref(owned)) or owned.value != want[j, i]:
                    flags.append((j, i))

        for threads in (1, 16):
            ts = []
            for rep in range(WARM + REPS):
                wrong = []
                th = [threading.Thread(target=sample, args=(t * SAMPLE, SAMPLE, wrong)) for t in range(threads)]
                w0 = time.perf_counter()
                [t.start() for t in th]
                [t.join() for t in th]
                ts.append((time.perf_counter() - w0) * 1e3)
                if wrong:
                    raise SystemExit("%d x %d: the single call differs at %s" % (m, n, wrong[:3]))
            st_ = stats(ts[WARM:])
            per_pair_us = st_["ms"] * 1e3 / (threads * SAMPLE)
            out["single_call_%d_threads" % threads] = {"sample_pairs": threads * SAMPLE, "sample": st_,
                                                       "us_per_pair": round(per_pair_us, 3),
                                                       "scaled_to_the_shape_ms": round(per_pair_us * m * n / 1e3, 1)}
        print("%d x %d %s" % (m, n, json.dumps(out)), file=sys.stderr, flush=True)

    # one full default launch: (64, 4,096) is exactly 2^18 quads; the call's time includes decoding 8,192 records
    m, n = FULL
    trackers, ks, want = inputs(m, n)
    d_t, d_k, d_o, dev = resident(trackers, ks, m, n)
    before = cm.stat_tracker_own()
    ts = [events(dev) for rep in range(WARM + REPS)][WARM:]
    after = cm.stat_tracker_own()
    if not (d_o.cpu().numpy().reshape(m, n) == want).all() or after["launches"] - before["launches"] != WARM + REPS:
        raise SystemExit("the full launch is not one launch, or its matrix is wrong")
    res["full_default_launch"] = {"m": m, "n": n, "quads": m * n, "device_form_call": stats(ts)}
    if a.kernel_stats:
        rows = {}
        with open(a.kernel_stats) as f:
            for row in csv.DictReader(f):
                for key in ("k_tracker_own", "k_scalar_mul_batch_quad"):
                    if key in row["Name"]:
                        rows[key] = {"calls": int(row["Calls"]), "average_ms": round(float(row["AverageNs"]) / 1e6, 4),
                                     "min_ms": round(float(row["MinNs"]) / 1e6, 4), "max_ms": round(float(row["MaxNs"]) / 1e6, 4)}
        own, quad = rows.get("k_tracker_own"), rows.get("k_scalar_mul_batch_quad")
        res["kernel_trace"] = {"pairs_per_launch": m * n, "kernels": rows,
                               "source": "rocprofv3 --kernel-trace --stats over --kernels-only, a run of its own"}
        if own and quad:
            res["kernel_trace"]["ns_per_pair_k_tracker_own"] = round(own["average_ms"] * 1e6 / (m * n), 2)
            res["kernel_trace"]["ns_per_pair_k_scalar_mul_batch_quad"] = round(quad["average_ms"] * 1e6 / (m * n), 2)
            res["kernel_trace"]["per_point_over_uniform_key"] = round(quad["average_ms"] / own["average_ms"], 3)
    res["stat_tracker_own"] = cm.stat_tracker_own()
    text = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
