"""The constant-time variable-base kernel (k_g1_mul_ct, CURDLE_G1_MUL_CONSTANT_TIME) against the default GLV chain
(k_scalar_mul_batch_quad + k_g1_normalize), and the tracker-proof generator with CURDLE_TRACKER_PROVE_CONSTANT_TIME
against the one without, in ONE process, same build, same run.

    python tools/bench_g1_mul_ct.py [--out profiles/r24_g1_mul_ct.json] [--kernel-stats N=kernel_stats.csv ...]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o ct -- python tools/bench_g1_mul_ct.py --kernels-only N

2 warm-ups, then 7 repetitions of every arm in a loop of its own; recorded are the median, the minimum and the maximum.
Resident arms: torch (HIP) events on the caller's stream around the _device_ex call.
Cost arm, random scalars over random subgroup points at n = 64 / 1,024 / 65,536 / 2^18: flag on against flag off, the
records compared first.  There is no threshold: the ratio is written down.
Dependence arm, n = 2^16, BOTH paths on every family, per-pair scalars and ONE shared scalar: all k = 0, all k = 1, all
k = r - 1, random, random with the low 128 bits zero.  Reported: each family's median, the largest difference between
family medians and beside it the largest min-max spread of a single family.  The flagged call passes when the former lies
within the latter.  The default path is the control: its largest difference must be more than three times its largest
spread, or the arm cannot see a dependence where there is one (`control_sees_the_scalars`).
Prover arm: curdle_whisk_generate_tracker_proof_batch_blinders_ex (host arrays in, bytes out, wall time) with the flag on
and off at k = 64 / 1,024 / 8,192 / 65,536, the proofs compared first.

--kernels-only N runs five resident calls of each path at N random pairs and nothing else, for a kernel-trace pass of its
own; --kernel-stats N=FILE reads such a pass's kernel_stats.csv into the JSON.
The last line printed is the JSON that --out also receives."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (64, 1024, 65536, 1 << 18)
FAMILY_N = 1 << 16
MEMBERS = (64, 1024, 8192, 65536)
WARM, REPS = 2, 7
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
KERNELS = ("k_g1_mul_ct", "k_scalar_mul_batch_quad", "k_g1_normalize")


def stats(ms):
    return {"ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default=",".join(str(v) for v in SIZES))
    ap.add_argument("--family-n", type=int, default=FAMILY_N)
    ap.add_argument("--members", default=",".join(str(v) for v in MEMBERS))
    ap.add_argument("--kernels-only", type=int, default=0)
    ap.add_argument("--kernel-stats", action="append", default=[])
    a = ap.parse_args()
    sys.path[:0] = [os.path.join(ROOT, "go-curdleproofs_amd"), os.path.join(ROOT, "oracle", "py")]
    import numpy as np
    import torch
    import curdlemsm as cm

    if not cm.device_available():
        raise SystemExit("no HIP device: this benchmark measures the GPU path")
    cm.init(0)
    CT = cm.G1_MUL_CONSTANT_TIME
    rng = np.random.default_rng(24)
    s = torch.cuda.Stream()

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

    def random_points(n):
        """n random points of the subgroup as affine records: random multiples of the generator."""
        return cm.g1_fixed_base_mul_batch(random_limbs(n))

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

    def resident(d_pts, d_sc, ns, n, d_out, flags):
        return lambda: cm.g1_scalar_mul_batch_device(d_pts.data_ptr(), d_sc.data_ptr(), ns, 0, n, d_out.data_ptr(),
                                                     stream=s.cuda_stream, flags=flags)

    if a.kernels_only:
        n = a.kernels_only
        d_pts, d_sc = dev(random_points(n)), dev(random_limbs(n))
        d_out = torch.zeros(n * 12, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        for flags in (0, CT):
            for _ in range(5):
                cm.g1_scalar_mul_batch_device(d_pts.data_ptr(), d_sc.data_ptr(), n, 0, n, d_out.data_ptr(), flags=flags)
        print("kernels-only: 5 x the GLV chain with its normalisation and 5 x k_g1_mul_ct over %d pairs" % n)
        return

    res = {"tool": "bench_g1_mul_ct", "warmups": WARM, "reps": REPS, "statistic": "median of the repetitions, min and max kept",
           "timing": "cost and dependence arms: torch (HIP) events on the caller's stream around the resident call; prover arm: wall time",
           "arm_cost": {}, "arm_scalar_dependence": {}, "arm_prover": {}}

    for n in [int(v) for v in a.sizes.split(",") if v]:
        out = res["arm_cost"][str(n)] = {"n": n}
        d_pts, d_sc = dev(random_points(n)), dev(random_limbs(n))
        d_ct = torch.zeros(n * 12, dtype=torch.int64, device="cuda:0")
        d_def = torch.zeros(n * 12, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        on, off = resident(d_pts, d_sc, n, n, d_ct, CT), resident(d_pts, d_sc, n, n, d_def, 0)
        on()
        off()
        torch.cuda.synchronize()
        if not torch.equal(d_ct, d_def):
            raise SystemExit("n = %d: the records of the two paths differ" % n)
        out["constant_time"] = timed(events, on)
        out["default"] = timed(events, off)
        out["constant_time_over_default"] = round(out["constant_time"]["ms"] / out["default"]["ms"], 3)
        out["ns_per_pair"] = {k: round(out[k]["ms"] * 1e6 / n, 2) for k in ("constant_time", "default")}
        print("cost n = %d %s" % (n, json.dumps(out)), file=sys.stderr, flush=True)
        del d_pts, d_sc, d_ct, d_def

    n = a.family_n
    if n:
        low_zero = [int(v) for v in rng.integers(1, 1 << 62, size=n)]
        families = {
            "all k = 0": np.zeros((n, 4), dtype=np.uint64),
            "all k = 1": np.tile(mont([1]), (n, 1)),
            "all k = r - 1": np.tile(mont([R - 1]), (n, 1)),
            "random": random_limbs(n),
            # canonical k = (a 126-bit random value) << 128
            "random, low 128 bits zero": mont([((v << 64 | w) % (R >> 128)) << 128 for v, w in zip(low_zero, reversed(low_zero))]),
        }
        d_pts = dev(random_points(n))
        d_out = torch.zeros(n * 12, dtype=torch.int64, device="cuda:0")
        d_ref = torch.zeros(n * 12, dtype=torch.int64, device="cuda:0")
        arm = res["arm_scalar_dependence"] = {"n": n}
        for form in ("per_pair", "shared_scalar"):
            ns = n if form == "per_pair" else 1
            part = arm[form] = {"constant_time": {}, "default": {}}
            for name, limbs in families.items():
                d_sc = dev(limbs)                                  # the shared form reads its first scalar
                torch.cuda.synchronize()
                resident(d_pts, d_sc, ns, n, d_out, CT)()
                resident(d_pts, d_sc, ns, n, d_ref, 0)()
                torch.cuda.synchronize()
                if not torch.equal(d_out, d_ref):
                    raise SystemExit("%s, family %s: the two paths differ" % (form, name))
                part["constant_time"][name] = timed(events, resident(d_pts, d_sc, ns, n, d_out, CT))
                part["default"][name] = timed(events, resident(d_pts, d_sc, ns, n, d_ref, 0))
                del d_sc
            for which in ("constant_time", "default"):
                meds = {k: v["ms"] for k, v in part[which].items()}
                part[which + "_summary"] = {
                    "largest_difference_between_family_medians_ms": round(max(meds.values()) - min(meds.values()), 4),
                    "slowest_family": max(meds, key=meds.get), "fastest_family": min(meds, key=meds.get),
                    "largest_min_max_spread_of_one_family_ms": round(max(v["max_ms"] - v["min_ms"] for v in part[which].values()), 4)}
            c, d = part["constant_time_summary"], part["default_summary"]
            part["control_sees_the_scalars"] = bool(
                d["largest_difference_between_family_medians_ms"] > 3 * d["largest_min_max_spread_of_one_family_ms"])
            part["constant_time_difference_within_the_repetition_spread"] = bool(
                c["largest_difference_between_family_medians_ms"] <= c["largest_min_max_spread_of_one_family_ms"])
            if not part["control_sees_the_scalars"]:
                part["verdict"] = "the control shows no dependence beyond its spread: this arm proves nothing"
            elif part["constant_time_difference_within_the_repetition_spread"]:
                part["verdict"] = "no dependence of the flagged call on the scalars beyond the repetition spread; the control shows one"
            else:
                part["verdict"] = "the flagged call's family medians differ by MORE than the repetition spread"
            print("dependence %s %s" % (form, json.dumps(part)), file=sys.stderr, flush=True)
        del d_pts, d_out, d_ref

    for k in [int(v) for v in a.members.split(",") if v]:
        ks, rs, bl = random_limbs(k), random_limbs(k), random_limbs(k)
        trk, _ = cm.whisk_compute_trackers_batch(ks, rs)
        trackers = [t.tobytes() for t in trk]
        got = {}

        def batch(flags):
            def call():
                got[flags] = cm.whisk_generate_tracker_proof_batch(trackers, ks, blinders=bl, flags=flags)
            return call

        batch(cm.TRACKER_PROVE_CONSTANT_TIME)()
        batch(0)()
        if not (got[1][0] == got[0][0]).all() or got[1][1].any() or got[0][1].any():
            raise SystemExit("k = %d: the proofs differ between the two paths" % k)
        out = res["arm_prover"][str(k)] = {"members": k, "constant_time": timed(wall, batch(cm.TRACKER_PROVE_CONSTANT_TIME)),
                                           "default": timed(wall, batch(0))}
        out["constant_time_over_default"] = round(out["constant_time"]["ms"] / out["default"]["ms"], 3)
        print("prover k = %d %s" % (k, json.dumps(out)), file=sys.stderr, flush=True)

    for spec in a.kernel_stats:
        n, path = spec.split("=", 1)
        rows = {}
        with open(path) as f:
            for row in csv.DictReader(f):
                for key in KERNELS:
                    if key in row["Name"]:
                        rows[key] = {"calls": int(row["Calls"]), "average_ms": round(float(row["AverageNs"]) / 1e6, 4),
                                     "min_ms": round(float(row["MinNs"]) / 1e6, 4), "max_ms": round(float(row["MaxNs"]) / 1e6, 4)}
                        break
        entry = {"pairs": int(n), "kernels": rows, "source": "rocprofv3 --kernel-trace --stats over --kernels-only, a run of its own"}
        if "k_g1_mul_ct" in rows:
            entry["ns_per_pair_k_g1_mul_ct"] = round(rows["k_g1_mul_ct"]["average_ms"] * 1e6 / int(n), 2)
        if all(k in rows for k in KERNELS):
            chain = rows["k_scalar_mul_batch_quad"]["average_ms"] + rows["k_g1_normalize"]["average_ms"]
            entry["k_g1_mul_ct_over_chain_and_normalisation"] = round(rows["k_g1_mul_ct"]["average_ms"] / chain, 3)
        res.setdefault("arm_kernel", {})[n] = entry
    res["stat_g1_mul_ct"] = cm.stat_g1_mul_ct()
    res["stat_fbase_ct"] = cm.stat_fbase_ct()
    text = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
