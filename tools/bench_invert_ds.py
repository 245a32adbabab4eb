"""The division-step inversion (csrc/invert_ds.h) against the Fermat chain (csrc/invert28.h) in ONE process, same build,
same run.  The control is always the Fermat build, which is the parent's code untouched; no figure is compared with the
code under test.

    python tools/bench_invert_ds.py [--out profiles/r37_invert_ds.json] [--finish-trace DIR]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_invert_ds.py --finish-only

2 warm-ups, then 7 repetitions of every arm; recorded are the median, the minimum and the maximum.  Every arm's results
are compared before anything is timed.
  (a) curdle_fp_invert_batch_device at n = 64 / 4,096 / 65,536 / 2^20 with and without CURDLE_FP_INVERT_FERMAT: HIP events
      on the caller's stream around the resident call.
  (b) the finish alone: curdle_msm_g1_ct_batch_device over 1 segment of 256 terms and over 4,096 segments of 16 with knob
      CT_FINISH_DIVSTEPS at 0 and at 1.  The kernels' own durations come from a kernel-trace run of its own (--finish-only
      under the profiler, no counters in that run); --finish-trace DIR reads that run's *kernel_trace.csv and puts the
      medians of k_msm_ct_finish_seg and k_msm_ct_finish_seg_ds per shape into the JSON.  Without it (b) holds the calls'
      event times only and the rule below counts as not met.
  (c) curdle_prover_ct_prove at ell = 124 / 252 with the knob at 0 and at 1: wall time.
  (d) dependence on the values (evidence to record, not a gate): curdle_msm_g1_ct_device on 256 pairs with the knob at 1
      over the families all 0 / all 1 / all r - 1 / random / random with the low 128 bits zero, every repetition visiting
      every family and every arm in turn, beside the bucket MSM as the control that does move.
THE RULE FOR THE DEFAULT, fixed beforehand: the library takes the _ds finish when the knob is unset only if the knob-1
median is below the knob-0 median by more than the SUM of the two arms' min-max spreads, in both (b) shapes (kernel
durations) and in (c) at ell = 124; the JSON says whether it held.  The last line printed is the JSON that --out also
receives."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
INVERT_SIZES = (64, 4096, 65536, 1 << 20)
FINISH_SHAPES = ((1, 256), (4096, 16))
PROVE_ELLS = (124, 252)
FAMILY_PAIRS = 256
WARM, REPS = 2, 7
FERMAT = 1


def stats(ms):
    return {"ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def spread(row):
    return row["max_ms"] - row["min_ms"]


def beats(new, base):
    """The rule's comparison: below the control by more than the sum of the two arms' min-max spreads."""
    return bool(base["ms"] - new["ms"] > spread(new) + spread(base))


def compare(new, base):
    return {"divsteps_over_fermat": round(new["ms"] / base["ms"], 3), "sum_of_spreads_ms": round(spread(new) + spread(base), 4),
            "below_fermat_by_more_than_the_sum_of_spreads": beats(new, base)}


def read_finish_trace(directory):
    """Per (kernel, blocks): the durations of the last REPS dispatches in the profiler's kernel trace."""
    rows = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                name = r.get("Kernel_Name", "")
                if "k_msm_ct_finish_seg" not in name:
                    continue
                kernel = "k_msm_ct_finish_seg_ds" if "finish_seg_ds" in name else "k_msm_ct_finish_seg"
                grid = int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0)
                wg = int(r.get("Workgroup_Size_X") or r.get("Workgroup_Size") or 256)
                blocks = grid // wg if grid >= wg else grid
                rows.setdefault((kernel, blocks), []).append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6))
    return {key: [ms for _, ms in sorted(v)][-REPS:] for key, v in rows.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--finish-only", action="store_true", help="run arm (b) alone: the program of a kernel-trace run")
    ap.add_argument("--finish-trace", default=None, help="directory of that run's output")
    a = ap.parse_args()
    sys.path[:0] = [os.path.join(ROOT, "go-curdleproofs_amd"), os.path.join(ROOT, "oracle", "py")]
    import numpy as np
    import torch
    import curdlemsm as cm

    if not cm.device_available():
        raise SystemExit("no HIP device: this benchmark measures the GPU path")
    cm.init(0)
    rng = np.random.default_rng(37)
    s = torch.cuda.Stream()

    def random_limbs(n):
        sc = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
        sc[:, 3] &= np.uint64((1 << 62) - 1)                      # Montgomery limbs below r, taken as they are
        return sc

    def mont(ks):
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

    def timed(call):
        return stats([events(call) for _ in range(WARM + REPS)][WARM:])

    def wall(call):
        ms = []
        for _ in range(WARM + REPS):
            w0 = time.perf_counter()
            call()
            ms.append((time.perf_counter() - w0) * 1e3)
        return stats(ms[WARM:])

    res = {"tool": "bench_invert_ds", "warmups": WARM, "reps": REPS, "library": "this build",
           "statistic": "median of the repetitions, min and max kept",
           "control": "the Fermat build (CURDLE_FP_INVERT_FERMAT; CT_FINISH_DIVSTEPS = 0): the parent's code, in the same process",
           "arm_a_fp_invert_batch_device": {}, "arm_b_finish": {}, "arm_c_prover_ct_prove": {}, "arm_d_value_dependence": {}}

    points = cm.g1_fixed_base_mul_batch(random_limbs(4096))

    # --- (b) the finish ------------------------------------------------------------------------------------------------
    for k, n in FINISH_SHAPES:
        total = k * n
        offs = np.arange(k + 1, dtype=np.uint64) * np.uint64(n)
        d_pts, d_sc = dev(points[np.arange(total) % len(points)]), dev(random_limbs(total))
        torch.cuda.synchronize()

        def call():
            return cm.msm_g1_ct_batch_device(d_pts.data_ptr(), d_sc.data_ptr(), offs, 255, stream=s.cuda_stream)

        row = res["arm_b_finish"]["%dx%d" % (k, n)] = {"segments": k, "terms_per_segment": n}
        with cm.knobs(CT_FINISH_DIVSTEPS=0):
            want = call()
        with cm.knobs(CT_FINISH_DIVSTEPS=1):
            if not (call() == want).all():
                raise SystemExit("%d x %d: the two finish builds differ" % (k, n))
            row["call_divsteps"] = timed(call)
        with cm.knobs(CT_FINISH_DIVSTEPS=0):
            row["call_fermat"] = timed(call)
        row["call"] = compare(row["call_divsteps"], row["call_fermat"])
        print("finish %d x %d %s" % (k, n, json.dumps(row)), file=sys.stderr, flush=True)
        del d_pts, d_sc
    if a.finish_only:
        print(json.dumps(res["arm_b_finish"]), flush=True)
        return
    traced = False
    if a.finish_trace:
        t = read_finish_trace(a.finish_trace)
        for k, n in FINISH_SHAPES:
            row = res["arm_b_finish"]["%dx%d" % (k, n)]
            ds, fm = t.get(("k_msm_ct_finish_seg_ds", k)), t.get(("k_msm_ct_finish_seg", k))
            if ds and fm and len(ds) == REPS and len(fm) == REPS:
                row["kernel_divsteps"], row["kernel_fermat"] = stats(ds), stats(fm)
                row["kernel"] = compare(row["kernel_divsteps"], row["kernel_fermat"])
                traced = True
            else:
                traced = False
                break
    res["arm_b_finish"]["kernel_durations"] = ("from a kernel-trace run of its own (--finish-only under the profiler)" if traced
                                               else "not measured: the call times above are HIP events around the whole call")

    # --- (a) the public call -------------------------------------------------------------------------------------------
    for n in INVERT_SIZES:
        vals = [int.from_bytes(rng.bytes(48), "little") % P for _ in range(min(n, 4096))]
        rows = np.array([[(v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(6)] for v in vals], dtype=np.uint64)
        rows = rows[np.arange(n) % len(rows)]
        d_in, d_out = dev(rows), dev(np.zeros_like(rows))
        torch.cuda.synchronize()
        out = {}
        for name, flags in (("divsteps", 0), ("fermat", FERMAT)):
            def call(flags=flags):
                cm.fp_invert_batch_device(d_in.data_ptr(), n, d_out.data_ptr(), flags=flags, stream=s.cuda_stream)
            call()
            torch.cuda.synchronize()
            out[name + "_words"] = d_out.cpu().numpy().copy()
            out[name] = timed(call)
        if not (out.pop("divsteps_words") == out.pop("fermat_words")).all():
            raise SystemExit("n = %d: the two inversions differ" % n)
        out.update(compare(out["divsteps"], out["fermat"]))
        res["arm_a_fp_invert_batch_device"]["n_%d" % n] = out
        print("fp_invert n = %d %s" % (n, json.dumps(out)), file=sys.stderr, flush=True)
        del d_in, d_out

    # --- (c) the prover handle -----------------------------------------------------------------------------------------
    for ell in PROVE_ELLS:
        rand = cm.Rand(ell)
        crs = cm.CRS(ell, rand)
        perm = np.asarray(cm.Rand(42).generate_permutation(ell), dtype=np.uint32)
        k = rand.get_fr()
        Rs, Ss = rand.get_g1_affines(ell), rand.get_g1_affines(ell)
        Ts, Us, M, rs_m = cm.shuffle_permute_commit(crs, Rs, Ss, perm, k, rand)
        prover = cm.ProverCt(crs)

        def prove():
            return prover.prove(Rs, Ss, Ts, Us, M, perm, k, rs_m, cm.Rand(7))

        row = res["arm_c_prover_ct_prove"]["ell_%d" % ell] = {}
        with cm.knobs(CT_FINISH_DIVSTEPS=0):
            want = prove()
        with cm.knobs(CT_FINISH_DIVSTEPS=1):
            if prove() != want:
                raise SystemExit("ell = %d: the proofs differ" % ell)
            row["divsteps"] = wall(prove)
        with cm.knobs(CT_FINISH_DIVSTEPS=0):
            row["fermat"] = wall(prove)
        row.update(compare(row["divsteps"], row["fermat"]))
        prover.free()
        print("prove ell = %d %s" % (ell, json.dumps(row)), file=sys.stderr, flush=True)

    # --- (d) dependence on the values ----------------------------------------------------------------------------------
    n = FAMILY_PAIRS
    low_zero = [int(v) for v in rng.integers(1, 1 << 62, size=n)]
    families = {
        "all 0": np.zeros((n, 4), dtype=np.uint64),
        "all 1": np.tile(mont([1]), (n, 1)),
        "all r - 1": np.tile(mont([R - 1]), (n, 1)),
        "random": random_limbs(n),
        "random, low 128 bits zero": mont([((v << 64 | w) % (R >> 128)) << 128 for v, w in zip(low_zero, reversed(low_zero))]),
    }
    d_pts = dev(points[:n])
    d_fam = {name: dev(limbs) for name, limbs in families.items()}
    torch.cuda.synchronize()
    arms = {"default": lambda d_sc: cm.msm_g1_device(d_pts.data_ptr(), d_sc.data_ptr(), n, stream=s.cuda_stream),
            "msm_g1_ct_divsteps_finish": lambda d_sc: cm.msm_g1_ct_device(d_pts.data_ptr(), d_sc.data_ptr(), n, 255, stream=s.cuda_stream)}
    part = res["arm_d_value_dependence"] = {"n": n, "order": "every repetition visits every family and every arm in turn"}
    with cm.knobs(CT_FINISH_DIVSTEPS=1):
        for name, d_sc in d_fam.items():
            if not (arms["msm_g1_ct_divsteps_finish"](d_sc) == arms["default"](d_sc)).all():
                raise SystemExit("family %s: the two paths differ" % name)
        ms = {arm: {name: [] for name in families} for arm in arms}
        for _ in range(WARM + REPS):
            for name, d_sc in d_fam.items():
                for arm, call in arms.items():
                    ms[arm][name].append(events(lambda: call(d_sc)))
    for arm in arms:
        part[arm] = {name: stats(v[WARM:]) for name, v in ms[arm].items()}
        meds = {name: v["ms"] for name, v in part[arm].items()}
        part[arm + "_summary"] = {
            "largest_difference_between_family_medians_ms": round(max(meds.values()) - min(meds.values()), 4),
            "largest_min_max_spread_of_one_family_ms": round(max(spread(v) for v in part[arm].values()), 4)}
    d, c = part["default_summary"], part["msm_g1_ct_divsteps_finish_summary"]
    part["control_sees_the_values"] = bool(d["largest_difference_between_family_medians_ms"] > 3 * d["largest_min_max_spread_of_one_family_ms"])
    c["difference_within_the_repetition_spread"] = bool(
        c["largest_difference_between_family_medians_ms"] <= c["largest_min_max_spread_of_one_family_ms"])

    # --- the rule ------------------------------------------------------------------------------------------------------
    b = res["arm_b_finish"]
    parts = {"finish_1x256": traced and b["1x256"]["kernel"]["below_fermat_by_more_than_the_sum_of_spreads"],
             "finish_4096x16": traced and b["4096x16"]["kernel"]["below_fermat_by_more_than_the_sum_of_spreads"],
             "prove_ell_124": res["arm_c_prover_ct_prove"]["ell_124"]["below_fermat_by_more_than_the_sum_of_spreads"]}
    res["the_rule_for_unset"] = dict(parts, kernel_durations_measured=traced, met=bool(all(parts.values())),
                                     what="unset takes the _ds finish only if all three hold; otherwise it keeps Fermat")
    res["stat_fp_invert"] = cm.stat_fp_invert()
    text = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
