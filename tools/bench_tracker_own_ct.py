"""The constant-time ownership search (k_tracker_own_ct, CURDLE_TRACKER_OWN_CONSTANT_TIME) against the default search
(k_tracker_own) and against the composition a caller had before it, in ONE process, same build, same run.

    python tools/bench_tracker_own_ct.py [--out profiles/r25_tracker_own_ct.json] [--kernel-stats kernel_stats.csv]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o ownct -- python tools/bench_tracker_own_ct.py --kernels-only

2 warm-ups, then 7 repetitions of every arm in a loop of its own; recorded are the median, the minimum and the maximum.
Every side is timed by torch (HIP) events on the caller's stream around the resident call(s); every arm's matrix is
compared before anything is timed.

Arm 1, cost, at (m keys, n trackers) = (1, 8,192), (1, 16,384), (16, 16,384), (64, 16,384), (1,024, 256): the _device_ex
call with the flag, without it, and THE COMPOSITION: for each key one curdle_g1_scalar_mul_batch_device_ex with
CURDLE_G1_MUL_CONSTANT_TIME and ONE shared scalar over the decoded rG column, the n records copied back to pinned memory
and compared with the decoded krG column on the host.  The composition's decoding is done once OUTSIDE its timed region
(the two calls decode inside theirs), which favours the composition.  From 1,024 keys the composition is timed over its
first 64 keys and scaled by m / 64; the entry says so.  The acceptance rule is in the output as a boolean: at every shape
with m >= 16 the flagged call's median is below the composition's by more than the larger of the two min-max spreads.
The ratio to the call without the flag has no bar and is written down.

Arm 2, dependence on the keys, at (16, 16,384): key families all 0, all 1, all r - 1, random, random with the low 128 bits
zero, BOTH paths on every family.  Reported: each family's median, the largest difference between family medians and
beside it the largest min-max spread of a single family.  The flagged call passes when the former lies within the
latter.  The call without the flag is the control: its largest difference must be more than three times its largest
spread, or the arm cannot see a dependence where there is one.

--kernels-only runs five flagged _device_ex calls at (64, 4,096) -- ONE launch of exactly 2^18 lanes, the default
TRACKER_OWN_PAIRS -- and nothing else, for a kernel-trace pass of its own; --kernel-stats reads that pass's
kernel_stats.csv into the JSON.  The last line printed is the JSON that --out also receives."""
import argparse
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1, 8192), (1, 16384), (16, 16384), (64, 16384), (1024, 256))
FAMILY_SHAPE = (16, 16384)
FULL = (64, 4096)          # one launch of 2^18 lanes
COMPOSITION_KEYS = 64      # the composition is timed over at most this many keys and scaled
WARM, REPS = 2, 7
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
K_G1_MUL_CT_2P18_MS = 18.39  # profiles/r24_g1_mul_ct_kernel_stats_262144.csv


def stats(ms):
    return {"ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def spread(st):
    return st["max_ms"] - st["min_ms"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default=";".join("%d,%d" % s for s in SHAPES))
    ap.add_argument("--family-shape", default="%d,%d" % FAMILY_SHAPE)
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
    CT = cm.TRACKER_OWN_CONSTANT_TIME
    rng = np.random.default_rng(25)
    s = torch.cuda.Stream()

    # eight keys with one honest tracker each, eight trackers of strangers; keys beyond the eight are random
    rand = o.Rand(25)
    pool_keys = [rand.get_fr() for _ in range(8)]
    bases = [o.scalar_mul(rand.get_fr(), o.G1) for _ in range(4)]
    trk = [o.compress(bases[j % 4]) + o.compress(o.scalar_mul(k, bases[j % 4])) for j, k in enumerate(pool_keys)]
    trk += [o.compress(bases[j % 4]) + o.compress(o.scalar_mul(rand.get_fr(), bases[j % 4])) for j in range(8)]
    pool = np.frombuffer(b"".join(trk), dtype=np.uint8).reshape(16, 96)
    pool_limbs = np.array([o.fr_to_mont_limbs(k) for k in pool_keys], dtype=np.uint64)

    def random_limbs(m):
        ks = rng.integers(0, 1 << 64, size=(m, 4), dtype=np.uint64)
        ks[:, 3] &= np.uint64((1 << 62) - 1)                      # Montgomery limbs below r, taken as they are
        return ks

    def mont(ks):
        out = np.empty((len(ks), 4), dtype=np.uint64)
        for i, k in enumerate(ks):
            v = (k << 256) % R
            out[i] = [(v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(4)]
        return out

    def inputs(m, n):
        which = rng.integers(16, size=n)
        ks = random_limbs(m)
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

    def timed(call):
        return stats([events(call) for _ in range(WARM + REPS)][WARM:])

    def resident(trackers, ks, m, n, flags):
        d_t = torch.from_numpy(trackers.reshape(-1)).to("cuda:0")
        d_k = torch.from_numpy(np.ascontiguousarray(ks).view(np.int64)).to("cuda:0")
        d_o = torch.zeros(m * n, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        return d_k, d_o, lambda: cm.whisk_find_own_trackers_device(d_t.data_ptr(), n, d_k.data_ptr(), m, d_o.data_ptr(),
                                                                   stream=s.cuda_stream, flags=flags)

    def matrix(d_o, m, n):
        return d_o.cpu().numpy().reshape(m, n)

    if a.kernels_only:
        m, n = FULL
        trackers, ks, want = inputs(m, n)
        _, d_o, call = resident(trackers, ks, m, n, CT)
        before = cm.stat_tracker_own_ct()
        for _ in range(5):
            call()
        after = cm.stat_tracker_own_ct()
        if not (matrix(d_o, m, n) == want).all() or after["launches"] - before["launches"] != 5:
            raise SystemExit("the full launch is not one launch, or its matrix is wrong")
        print("kernels-only: 5 x k_tracker_own_ct over %d lanes" % (m * n))
        return

    res = {"tool": "bench_tracker_own_ct", "warmups": WARM, "reps": REPS,
           "statistic": "median of the repetitions, min and max kept",
           "timing": "torch (HIP) events on the caller's stream around the resident call(s); the composition's decoding is outside its timed region",
           "arm_cost": {}, "arm_key_dependence": {}}

    for m, n in shapes:
        trackers, ks, want = inputs(m, n)
        out = res["arm_cost"]["%dx%d" % (m, n)] = {"m": m, "n": n, "pairs": m * n}
        d_k, d_on, on = resident(trackers, ks, m, n, CT)
        _, d_off, off = resident(trackers, ks, m, n, 0)
        pts, st = cm.g1_decompress_batch(trackers.tobytes())
        if (st > cm.DECODE_INFINITY).any():
            raise SystemExit("a benchmark tracker did not decode")
        pts = pts.reshape(n, 2, 12)
        krg = np.ascontiguousarray(pts[:, 1])
        d_p = torch.from_numpy(np.ascontiguousarray(pts[:, 0]).view(np.int64).reshape(-1)).to("cuda:0")
        d_r = torch.empty(n * 12, dtype=torch.int64, device="cuda:0")
        t_back = torch.zeros((n, 12), dtype=torch.int64).pin_memory()
        back = t_back.numpy().view(np.uint64)
        mc = min(m, COMPOSITION_KEYS)
        comp = np.zeros((mc, n), dtype=np.uint8)
        torch.cuda.synchronize()

        def composition():
            for j in range(mc):
                cm.g1_scalar_mul_batch_device(d_p.data_ptr(), d_k.data_ptr() + 32 * j, 1, 0, n, d_r.data_ptr(),
                                              stream=s.cuda_stream, flags=cm.G1_MUL_CONSTANT_TIME)
                with torch.cuda.stream(s):
                    t_back.copy_(d_r.view(n, 12), non_blocking=True)
                s.synchronize()
                comp[j] = (back == krg).all(axis=1)

        on()
        off()
        composition()
        if not (matrix(d_on, m, n) == want).all() or not (matrix(d_off, m, n) == want).all() or not (comp == want[:mc]).all():
            raise SystemExit("%d x %d: the three matrices differ" % (m, n))
        out["constant_time"] = timed(on)
        out["default"] = timed(off)
        timed_comp = timed(composition)
        scale = m / mc
        out["composition"] = {k: round(v * scale, 4) for k, v in timed_comp.items()}
        out["composition_timed_over_keys"] = mc
        out["composition_scaled_by"] = scale
        out["constant_time_over_default"] = round(out["constant_time"]["ms"] / out["default"]["ms"], 3)
        out["composition_over_constant_time"] = round(out["composition"]["ms"] / out["constant_time"]["ms"], 3)
        out["ns_per_pair"] = {k: round(out[k]["ms"] * 1e6 / (m * n), 2) for k in ("constant_time", "default", "composition")}
        margin = max(spread(out["constant_time"]), spread(out["composition"]))
        out["larger_min_max_spread_ms"] = round(margin, 4)
        out["faster_than_the_composition_by_more_than_the_spread"] = bool(
            out["composition"]["ms"] - out["constant_time"]["ms"] > margin)
        print("cost %d x %d %s" % (m, n, json.dumps(out)), file=sys.stderr, flush=True)
        del d_p, d_r, d_on, d_off, d_k
    judged = [v for v in res["arm_cost"].values() if v["m"] >= 16]
    res["arm_cost_accepted"] = bool(judged) and all(v["faster_than_the_composition_by_more_than_the_spread"] for v in judged)

    m, n = [int(v) for v in a.family_shape.split(",")]
    if m and n:
        trackers, _, _ = inputs(m, n)
        lows = [int(v) for v in rng.integers(1, 1 << 62, size=2 * m)]
        families = {
            "all k = 0": np.zeros((m, 4), dtype=np.uint64),
            "all k = 1": np.tile(mont([1]), (m, 1)),
            "all k = r - 1": np.tile(mont([R - 1]), (m, 1)),
            "random": random_limbs(m),
            # canonical k = (a 126-bit random value) << 128
            "random, low 128 bits zero": mont([((v << 64 | w) % (R >> 128)) << 128 for v, w in zip(lows[:m], lows[m:])]),
        }
        arm = res["arm_key_dependence"] = {"m": m, "n": n, "constant_time": {}, "default": {}}
        for name, limbs in families.items():
            _, d_on, on = resident(trackers, limbs, m, n, CT)
            _, d_off, off = resident(trackers, limbs, m, n, 0)
            on()
            off()
            if not torch.equal(d_on, d_off):
                raise SystemExit("family %s: the two paths differ" % name)
            arm["constant_time"][name] = timed(on)
            arm["default"][name] = timed(off)
        for which in ("constant_time", "default"):
            meds = {k: v["ms"] for k, v in arm[which].items()}
            arm[which + "_summary"] = {
                "largest_difference_between_family_medians_ms": round(max(meds.values()) - min(meds.values()), 4),
                "slowest_family": max(meds, key=meds.get), "fastest_family": min(meds, key=meds.get),
                "largest_min_max_spread_of_one_family_ms": round(max(spread(v) for v in arm[which].values()), 4)}
        c, d = arm["constant_time_summary"], arm["default_summary"]
        arm["control_sees_the_keys"] = bool(
            d["largest_difference_between_family_medians_ms"] > 3 * d["largest_min_max_spread_of_one_family_ms"])
        arm["constant_time_difference_within_the_repetition_spread"] = bool(
            c["largest_difference_between_family_medians_ms"] <= c["largest_min_max_spread_of_one_family_ms"])
        if not arm["control_sees_the_keys"]:
            arm["verdict"] = "the control shows no dependence beyond its spread: this arm proves nothing"
        elif arm["constant_time_difference_within_the_repetition_spread"]:
            arm["verdict"] = "no dependence of the flagged call on the keys beyond the repetition spread; the control shows one"
        else:
            arm["verdict"] = "the flagged call's family medians differ by MORE than the repetition spread"
        print("dependence %s" % json.dumps(arm), file=sys.stderr, flush=True)

    if a.kernel_stats:
        m, n = FULL
        rows = {}
        with open(a.kernel_stats) as f:
            for row in csv.DictReader(f):
                if "k_tracker_own_ct" in row["Name"]:
                    rows["k_tracker_own_ct"] = {"calls": int(row["Calls"]), "average_ms": round(float(row["AverageNs"]) / 1e6, 4),
                                                "min_ms": round(float(row["MinNs"]) / 1e6, 4), "max_ms": round(float(row["MaxNs"]) / 1e6, 4)}
        entry = res["arm_kernel"] = {"lanes": m * n, "kernels": rows,
                                     "source": "rocprofv3 --kernel-trace --stats over --kernels-only, a run of its own"}
        if rows:
            avg = rows["k_tracker_own_ct"]["average_ms"]
            entry["ns_per_pair_k_tracker_own_ct"] = round(avg * 1e6 / (m * n), 2)
            entry["k_g1_mul_ct_at_as_many_pairs_ms"] = K_G1_MUL_CT_2P18_MS
            entry["dropping_the_inversion_is_worth_ms"] = round(K_G1_MUL_CT_2P18_MS - avg, 4)
    res["stat_tracker_own_ct"] = cm.stat_tracker_own_ct()
    res["stat_tracker_own"] = cm.stat_tracker_own()
    text = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
