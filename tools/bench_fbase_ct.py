"""The constant-time fixed-base kernel (k_fbase_mul_ct, CURDLE_FBASE_CONSTANT_TIME) against the default kernel
(k_fbase_mul) in ONE process, same build, same run.

    python tools/bench_fbase_ct.py [--out profiles/r21_fbase_ct.json] [--kernel-stats N=kernel_stats.csv ...]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o ct -- python tools/bench_fbase_ct.py --kernels-only N

2 warm-ups, then 7 repetitions of every arm in a loop of its own; recorded are the median, the minimum and the maximum.
Resident arms: torch (HIP) events on the caller's stream around the _device_ex call with affine output.
Arm 1 (cost), random scalars at n = 65,536 / 2^18 / 2^20: flag on against flag off (the records are compared first), and
beside them curdle_g1_scalar_mul_batch_device over the generator replicated n times, the GLV chain a caller would use
otherwise.  There is no threshold: the ratio is written down.
Arm 2 (dependence on the scalars), n = 2^18, BOTH kernels on every family: all k = 0, all k = 1, all k = r - 1, random,
random with the low 128 bits zero.  Reported: each family's median, the largest difference between family medians, and
beside it the largest min-max spread of a single family.  The default kernel is the control: it must show k = 0 far below
random, or the arm cannot see anything (`control_sees_the_scalars`).
Arm 3: curdle_whisk_compute_trackers_batch_ex (host arrays in, bytes out, wall time) with the flag on and off at 65,536
members.

--kernels-only N runs five resident affine calls of each kernel at N random scalars and nothing else, for a kernel-trace
pass of its own; --kernel-stats N=FILE reads such a pass's kernel_stats.csv into the JSON.
The last line printed is the JSON that --out also receives."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (65536, 1 << 18, 1 << 20)
FAMILY_N = 1 << 18
MEMBERS = 65536
WARM, REPS = 2, 7
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def stats(ms):
    return {"ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default=",".join(str(v) for v in SIZES))
    ap.add_argument("--family-n", type=int, default=FAMILY_N)
    ap.add_argument("--members", type=int, default=MEMBERS)
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
    CT = cm.FBASE_CONSTANT_TIME
    rng = np.random.default_rng(21)
    s = torch.cuda.Stream()
    gen = np.array(o.affine_to_mont_limbs(o.G1), dtype=np.uint64)

    def random_limbs(n):
        sc = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
        sc[:, 3] &= np.uint64((1 << 62) - 1)                      # Montgomery limbs below r, taken as they are
        return sc

    def mont(ks):
        """Canonical scalars (Python integers) -> (n, 4) Montgomery limbs."""
        out = np.empty((len(ks), 4), dtype=np.uint64)
        for i, k in enumerate(ks):
            v = (k << 256) % R
            out[i] = [(v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(4)]
        return out

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

    def resident(d_sc, n, d_out, flags):
        return lambda: cm.g1_fixed_base_mul_batch_device(d_sc.data_ptr(), 0, n, d_out.data_ptr(), stream=s.cuda_stream, flags=flags)

    if a.kernels_only:
        n = a.kernels_only
        d_sc, d_out = dev(random_limbs(n)), torch.zeros(n * 12, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        for flags in (0, CT):
            for _ in range(5):
                cm.g1_fixed_base_mul_batch_device(d_sc.data_ptr(), 0, n, d_out.data_ptr(), flags=flags)
        print("kernels-only: 5 x k_fbase_mul and 5 x k_fbase_mul_ct over %d scalars" % n)
        return

    res = {"tool": "bench_fbase_ct", "warmups": WARM, "reps": REPS, "statistic": "median of the repetitions, min and max kept",
           "timing": "arms 1 and 2: torch (HIP) events on the caller's stream around the resident call, affine output; arm 3: wall time",
           "arm1_cost": {}, "arm2_scalar_dependence": {}, "arm3_tracker_batch": {}}

    for n in [int(v) for v in a.sizes.split(",") if v]:
        out = res["arm1_cost"][str(n)] = {"n": n}
        d_sc = dev(random_limbs(n))
        d_pts = dev(np.tile(gen, (n, 1)))
        d_ct = torch.zeros(n * 12, dtype=torch.int64, device="cuda:0")
        d_def = torch.zeros(n * 12, dtype=torch.int64, device="cuda:0")
        d_glv = torch.zeros(n * 12, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        on, off = resident(d_sc, n, d_ct, CT), resident(d_sc, n, d_def, 0)
        glv = lambda: cm.g1_scalar_mul_batch_device(d_pts.data_ptr(), d_sc.data_ptr(), n, 0, n, d_glv.data_ptr(), stream=s.cuda_stream)
        on()
        off()
        glv()
        torch.cuda.synchronize()
        if not torch.equal(d_ct, d_def) or not torch.equal(d_ct, d_glv):
            raise SystemExit("n = %d: the records of the three paths differ" % n)
        out["constant_time"] = timed(events, on)
        out["default"] = timed(events, off)
        out["glv_chain"] = timed(events, glv)
        out["constant_time_over_default"] = round(out["constant_time"]["ms"] / out["default"]["ms"], 3)
        out["constant_time_over_glv_chain"] = round(out["constant_time"]["ms"] / out["glv_chain"]["ms"], 3)
        out["ns_per_scalar"] = {k: round(out[k]["ms"] * 1e6 / n, 2) for k in ("constant_time", "default", "glv_chain")}
        print("arm 1 n = %d %s" % (n, json.dumps(out)), file=sys.stderr, flush=True)
        del d_sc, d_pts, d_ct, d_def, d_glv

    n = a.family_n
    if n:
        low_zero = [int(v) for v in rng.integers(1, 1 << 62, size=n)]
        families = {
            "all k = 0": np.zeros((n, 4), dtype=np.uint64),
            "all k = 1": np.tile(mont([1]), (n, 1)),
            "all k = r - 1": np.tile(mont([R - 1]), (n, 1)),
            "random": random_limbs(n),
            # canonical k = (a 126-bit random value) << 128: the 32 low 4-bit windows (16 low 8-bit ones) are zero
            "random, low 128 bits zero": mont([((v << 64 | w) % (R >> 128)) << 128 for v, w in zip(low_zero, reversed(low_zero))]),
        }
        arm = res["arm2_scalar_dependence"] = {"n": n, "constant_time": {}, "default": {}}
        d_out = torch.zeros(n * 12, dtype=torch.int64, device="cuda:0")
        d_ref = torch.zeros(n * 12, dtype=torch.int64, device="cuda:0")
        for name, limbs in families.items():
            d_sc = dev(limbs)
            torch.cuda.synchronize()
            resident(d_sc, n, d_out, CT)()
            resident(d_sc, n, d_ref, 0)()
            torch.cuda.synchronize()
            if not torch.equal(d_out, d_ref):
                raise SystemExit("family %s: the two kernels differ" % name)
            arm["constant_time"][name] = timed(events, resident(d_sc, n, d_out, CT))
            arm["default"][name] = timed(events, resident(d_sc, n, d_ref, 0))
            del d_sc
        for which in ("constant_time", "default"):
            meds = {k: v["ms"] for k, v in arm[which].items()}
            arm[which + "_summary"] = {
                "largest_difference_between_family_medians_ms": round(max(meds.values()) - min(meds.values()), 4),
                "slowest_family": max(meds, key=meds.get), "fastest_family": min(meds, key=meds.get),
                "largest_min_max_spread_of_one_family_ms": round(max(v["max_ms"] - v["min_ms"] for v in arm[which].values()), 4)}
        d = arm["default"]
        arm["control_sees_the_scalars"] = bool(d["all k = 0"]["ms"] < 0.5 * d["random"]["ms"])
        c = arm["constant_time_summary"]
        arm["constant_time_difference_beyond_the_repetition_spread"] = bool(
            c["largest_difference_between_family_medians_ms"] > c["largest_min_max_spread_of_one_family_ms"])
        print("arm 2 %s" % json.dumps(arm), file=sys.stderr, flush=True)
        del d_out, d_ref

    n = a.members
    if n:
        ks, rs = random_limbs(n), random_limbs(n)
        got = {}

        def batch(flags):
            def call():
                got[flags] = cm.whisk_compute_trackers_batch(ks, rs, flags=flags)
            return call

        batch(CT)()
        batch(0)()
        if not (got[CT][0] == got[0][0]).all() or not (got[CT][1] == got[0][1]).all():
            raise SystemExit("the tracker batch differs between the two kernels")
        arm = res["arm3_tracker_batch"] = {"members": n, "scalars": 3 * n, "constant_time": timed(wall, batch(CT)),
                                           "default": timed(wall, batch(0))}
        arm["constant_time_over_default"] = round(arm["constant_time"]["ms"] / arm["default"]["ms"], 3)
        print("arm 3 %s" % json.dumps(arm), file=sys.stderr, flush=True)

    for spec in a.kernel_stats:
        n, path = spec.split("=", 1)
        rows = {}
        with open(path) as f:
            for row in csv.DictReader(f):
                for key in ("k_fbase_mul_ct", "k_fbase_mul", "k_g1_normalize"):
                    if key in row["Name"]:
                        rows[key] = {"calls": int(row["Calls"]), "average_ms": round(float(row["AverageNs"]) / 1e6, 4),
                                     "min_ms": round(float(row["MinNs"]) / 1e6, 4), "max_ms": round(float(row["MaxNs"]) / 1e6, 4)}
                        break
        entry = {"scalars": int(n), "kernels": rows, "source": "rocprofv3 --kernel-trace --stats over --kernels-only, a run of its own"}
        if "k_fbase_mul_ct" in rows and "k_fbase_mul" in rows:
            entry["k_fbase_mul_ct_over_k_fbase_mul"] = round(rows["k_fbase_mul_ct"]["average_ms"] / rows["k_fbase_mul"]["average_ms"], 3)
            entry["ns_per_scalar"] = {k: round(rows[k]["average_ms"] * 1e6 / int(n), 2) for k in ("k_fbase_mul_ct", "k_fbase_mul")}
        res.setdefault("kernel_trace", {})[n] = entry
    res["stat_fbase"] = cm.stat_fbase()
    res["stat_fbase_ct"] = cm.stat_fbase_ct()
    text = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
