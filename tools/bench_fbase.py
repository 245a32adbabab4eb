"""The fixed-base multiplication (k_fbase_mul) and the bulk tracker computation against what the parent build offers,
in ONE process.

    python tools/bench_fbase.py [--out profiles/r17_fbase.json] [--kernel-stats N=kernel_stats.csv ...]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o fb -- python tools/bench_fbase.py --kernels-only N

Arm 1, n = 64 / 3,072 / 65,536 / 2^20 scalars: curdle_g1_fixed_base_mul_batch_device with affine output against
curdle_g1_scalar_mul_batch_device over the generator replicated n times (the GLV chain on quads), both resident, torch
(HIP) events on the caller's stream.  The records are compared first.  The compressed form is timed beside it, and at
2^20 curdle_g1_compress_batch_device (one Fermat inversion per point) over as many Jacobian points.
Arm 2, n members: curdle_whisk_compute_trackers_batch (host arrays in, bytes out, wall time) against the composition:
r G and k G from one curdle_g1_scalar_mul_batch_device over 2 n copies of the generator, k r G from a second one over
the resident r G, the three columns to Jacobian form with Z = 1 on the device and curdle_g1_compress_batch_device over
them, the bytes brought back; and against the single host calls on 1 and 16 threads over a sample, scaled.
2 warm-ups, then 7 repetitions of every arm in a loop of its own; recorded are the median and the spread
(max - min) / median.  `faster_by_more_than_the_spread` is the acceptance rule from 65,536 scalars up: the new arm's
median is below the composition's by more than the larger of the two arms' max - min.

--kernels-only N runs five resident affine calls at N scalars and nothing else, for a kernel-trace pass of its own;
--kernel-stats N=FILE reads such a pass's kernel_stats.csv into the JSON (k_fbase_mul alone, k_g1_normalize beside it).
The last line printed is the JSON that --out also receives."""
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
SIZES = (64, 3072, 65536, 1 << 20)
MEMBERS = (64, 1024, 21846, 349526)          # 3 n = 192 / 3,072 / 65,538 / 2^20 + 2
WARM, REPS = 2, 7
SAMPLE = 1024                                # members per thread of the single host calls


def stats(ms):
    med = statistics.median(ms)
    return {"ms": round(med, 4), "spread": round((max(ms) - min(ms)) / med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def verdict(new, old):
    gap = old["ms"] - new["ms"]
    return {"ratio_old_over_new": round(old["ms"] / new["ms"], 3),
            "faster_by_more_than_the_spread": bool(gap > max(new["max_ms"] - new["min_ms"], old["max_ms"] - old["min_ms"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default=",".join(str(v) for v in SIZES))
    ap.add_argument("--members", default=",".join(str(v) for v in MEMBERS))
    ap.add_argument("--kernels-only", type=int, default=0)
    ap.add_argument("--kernel-stats", action="append", default=[])
    a = ap.parse_args()
    sys.path[:0] = [os.path.join(ROOT, "go-curdleproofs_amd"), os.path.join(ROOT, "oracle", "py")]
    import numpy as np
    import torch
    import curdlemsm as cm
    import bls12381_ref as o

    if not cm.device_available():
        raise SystemExit("no HIP device: this benchmark measures the GPU path")
    cm.init(0)
    rng = np.random.default_rng(17)
    s = torch.cuda.Stream()
    gen = np.array(o.affine_to_mont_limbs(o.G1), dtype=np.uint64)
    one = np.array(o.fp_to_mont_limbs(1), dtype=np.uint64)

    def scalars(n):
        sc = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
        sc[:, 3] &= np.uint64((1 << 62) - 1)                      # Montgomery limbs below r, taken as they are
        return sc

    def dev(arr):
        return torch.from_numpy(np.ascontiguousarray(arr).view(np.int64).reshape(-1)).to("cuda:0")

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

    def timed(how, call):
        return stats([how(call) for _ in range(WARM + REPS)][WARM:])

    if a.kernels_only:
        n = a.kernels_only
        d_sc, d_out = dev(scalars(n)), torch.zeros(n * 12, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        for _ in range(5):
            cm.g1_fixed_base_mul_batch_device(d_sc.data_ptr(), 0, n, d_out.data_ptr())
        print("kernels-only: 5 x k_fbase_mul over %d scalars" % n)
        return

    res = {"tool": "bench_fbase", "warmups": WARM, "reps": REPS, "statistic": "median of the repetitions",
           "timing": "arm 1: torch (HIP) events on the caller's stream; arm 2: wall time", "arm1": {}, "arm2": {}}

    for n in [int(v) for v in a.sizes.split(",") if v]:
        out = res["arm1"][str(n)] = {"n": n}
        d_sc = dev(scalars(n))
        d_pts = dev(np.tile(gen, (n, 1)))
        d_new = torch.zeros(n * 12, dtype=torch.int64, device="cuda:0")
        d_old = torch.zeros(n * 12, dtype=torch.int64, device="cuda:0")
        d_comp = torch.zeros(n * 48, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        new = lambda: cm.g1_fixed_base_mul_batch_device(d_sc.data_ptr(), 0, n, d_new.data_ptr(), stream=s.cuda_stream)
        newc = lambda: cm.g1_fixed_base_mul_batch_device(d_sc.data_ptr(), 0, n, d_comp.data_ptr(), out_form=cm.G1_OUT_COMPRESSED,
                                                         stream=s.cuda_stream)
        old = lambda: cm.g1_scalar_mul_batch_device(d_pts.data_ptr(), d_sc.data_ptr(), n, 0, n, d_old.data_ptr(), stream=s.cuda_stream)
        new()
        old()
        if not torch.equal(d_new, d_old):
            raise SystemExit("n = %d: the fixed-base records differ from the chain's" % n)
        out["fixed_base_affine"] = timed(events, new)
        out["fixed_base_compressed"] = timed(events, newc)
        out["glv_chain_affine"] = timed(events, old)
        out["ns_per_scalar_fixed_base"] = round(out["fixed_base_affine"]["ms"] * 1e6 / n, 2)
        out["ns_per_scalar_glv_chain"] = round(out["glv_chain_affine"]["ms"] * 1e6 / n, 2)
        out["affine"] = verdict(out["fixed_base_affine"], out["glv_chain_affine"])
        out["compressed_over_affine_ms"] = round(out["fixed_base_compressed"]["ms"] - out["fixed_base_affine"]["ms"], 4)
        if n == 1 << 20:                                        # the per-point inversion the compressed form does not pay
            jac = torch.cat([d_new.view(n, 12), dev(np.tile(one, (n, 1))).view(n, 6)], dim=1).contiguous()
            torch.cuda.synchronize()
            out["k_g1_compress_per_point_inversion"] = timed(
                events, lambda: cm.g1_compress_batch_device(jac.data_ptr(), n, d_comp.data_ptr(), stream=s.cuda_stream))
            del jac
        print("arm 1 n = %d %s" % (n, json.dumps(out)), file=sys.stderr, flush=True)
        del d_sc, d_pts, d_new, d_old, d_comp

    single_t = cm._lib.curdle_whisk_compute_tracker
    single_c = cm._lib.curdle_whisk_k_commitment
    for n in [int(v) for v in a.members.split(",") if v]:
        out = res["arm2"][str(n)] = {"members": n, "scalars": 3 * n}
        ks, rs = scalars(n), scalars(n)
        got = [None, None]

        def new():
            got[0], got[1] = cm.whisk_compute_trackers_batch(ks, rs)

        t_back = torch.zeros(3 * n * 48, dtype=torch.uint8).pin_memory()
        d_gen = dev(np.tile(gen, (2 * n, 1)))
        d_one = dev(np.tile(one, (3 * n, 1))).view(3 * n, 6)
        torch.cuda.synchronize()
        comp = [None, None]

        def composition():
            with torch.cuda.stream(s):
                d_sc = torch.from_numpy(np.concatenate([rs, ks]).view(np.int64).reshape(-1)).to("cuda:0", non_blocking=True)
                d_aff = torch.empty(3 * n * 12, dtype=torch.int64, device="cuda:0")
                # r G | k G, then k (r G) behind them
                cm.g1_scalar_mul_batch_device(d_gen.data_ptr(), d_sc.data_ptr(), 2 * n, 0, 2 * n, d_aff.data_ptr(), stream=s.cuda_stream)
                cm.g1_scalar_mul_batch_device(d_aff.data_ptr(), d_sc.data_ptr() + 32 * n, n, 0, n, d_aff.data_ptr() + 96 * 2 * n,
                                              stream=s.cuda_stream)
                jac = torch.cat([d_aff.view(3 * n, 12), d_one], dim=1).contiguous()
                inf = (d_aff.view(3 * n, 12) == 0).all(dim=1)
                jac[inf, 12:] = 0                               # Z = 0 where the affine record is infinity
                d_c = torch.empty(3 * n * 48, dtype=torch.uint8, device="cuda:0")
                cm.g1_compress_batch_device(jac.data_ptr(), 3 * n, d_c.data_ptr(), stream=s.cuda_stream)
                t_back.copy_(d_c, non_blocking=True)
                s.synchronize()
            b = t_back.numpy().reshape(3, n, 48)
            comp[0] = np.concatenate([b[0], b[2]], axis=1)
            comp[1] = b[1].copy()

        new()
        composition()
        if not (got[0] == comp[0]).all() or not (got[1] == comp[1]).all():
            raise SystemExit("n = %d members: the batch differs from the composition" % n)
        out["batch"] = timed(wall, new)
        out["composition"] = timed(wall, composition)
        out["batch_vs_composition"] = verdict(out["batch"], out["composition"])
        out["us_per_member_batch"] = round(out["batch"]["ms"] * 1e3 / n, 3)

        def sample(lo, count, wrong):
            t, c = np.zeros(96, dtype=np.uint8), np.zeros(48, dtype=np.uint8)
            for i in range(lo, lo + count):
                i %= n
                if single_t(ks[i].ctypes.data, rs[i].ctypes.data, t.ctypes.data) or single_c(ks[i].ctypes.data, c.ctypes.data) \
                        or (t != got[0][i]).any() or (c != got[1][i]).any():
                    wrong.append(i)

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
                    raise SystemExit("n = %d members: the single calls differ at %s" % (n, wrong[:3]))
            st_ = stats(ts[WARM:])
            per_member_us = st_["ms"] * 1e3 / (threads * SAMPLE)
            out["single_calls_%d_threads" % threads] = {"sample_members": threads * SAMPLE, "sample": st_,
                                                        "us_per_member": round(per_member_us, 3),
                                                        "scaled_to_the_batch_ms": round(per_member_us * n / 1e3, 2)}
        print("arm 2 n = %d %s" % (n, json.dumps(out)), file=sys.stderr, flush=True)
        del d_gen, d_one, t_back

    for spec in a.kernel_stats:
        n, path = spec.split("=", 1)
        rows = {}
        with open(path) as f:
            for row in csv.DictReader(f):
                for key in ("k_fbase_mul", "k_g1_normalize"):
                    if key in row["Name"]:
                        rows[key] = {"calls": int(row["Calls"]), "average_ms": round(float(row["AverageNs"]) / 1e6, 4),
                                     "min_ms": round(float(row["MinNs"]) / 1e6, 4), "max_ms": round(float(row["MaxNs"]) / 1e6, 4)}
        entry = {"scalars": int(n), "kernels": rows, "source": "rocprofv3 --kernel-trace --stats over --kernels-only, a run of its own"}
        if "k_fbase_mul" in rows:
            ms = rows["k_fbase_mul"]["average_ms"]
            entry["ns_per_scalar_k_fbase_mul"] = round(ms * 1e6 / int(n), 2)
            # 255 of 256 digits are non-zero: 31.875 additions per uniform scalar; k_accumulate: 2^23 additions in 2.37 ms
            entry["additions_per_s"] = round(int(n) * 32 * 255 / 256 / ms * 1e3)
            entry["share_of_k_accumulate_rate"] = round(entry["additions_per_s"] / ((1 << 23) / 2.37e-3), 3)
        res.setdefault("kernel_trace", {})[n] = entry
    res["stat_fbase"] = cm.stat_fbase()
    text = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
