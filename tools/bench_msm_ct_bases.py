"""The constant-time MSM over a resident base set, the walk split into chunks (curdle_ct_bases, curdle_msm_g1_ct_bases_device
/ _batch_device: k_msm_ct_walk_rows and the segmented sum) against the constant-time MSM whose lanes walk whole scalars
(curdle_msm_g1_ct_device / _batch_device, unchanged from the parent: the baseline) on the same pairs, in ONE process,
same build, same run.

    python tools/bench_msm_ct_bases.py [--out profiles/r33_msm_ct_bases.json]

2 warm-ups, then 7 repetitions of every arm in a loop of its own; recorded are the median, the minimum and the maximum.
Resident arms: torch (HIP) events on the caller's stream around the _device call.  The table build returns a handle
and waits for it: wall time.  Every arm's results are compared before anything is timed.
Per chunk_bits 8 / 16 / 32 / 64:
  build     curdle_ct_bases_create at n = 128, 512 and 2,048 (freed again outside the timed part);
  single    255 and 9 bits over 4, 129, 256 and 2,048 pairs through a built handle of as many bases, rows null;
  batch     4 x 129, 6 x 128 and 64 x 64 at 255 bits; a shape beyond n Cb <= 65,536 is recorded as refused.
THE ONE CONDITION: at chunk_bits = 16 the 255-bit MSM over 256 pairs takes LESS THAN HALF the time of
curdle_msm_g1_ct_device on the same pairs, with the medians apart by more than the min-max spread of either arm; the
JSON says whether it held.
Dependence arm (evidence to record, not a gate): 256 pairs at 255 bits over the families all 0 / all 1 / all r - 1 /
random / random with the low 128 bits zero, per chunk_bits, reported as tools/bench_msm_ct_batch.py reports it, with the
bucket MSM as the control.  Unlike the other arms, every repetition visits every family and every arm in turn: a call of
1 ms sees the clocks the calls before it left, and a loop per family would hand each family a different past.
The last line printed is the JSON that --out also receives."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK_BITS = (8, 16, 32, 64)
BUILD_SIZES = (128, 512, 2048)
SINGLE_SIZES = (4, 129, 256, 2048)
BATCH_SHAPES = ((4, 129), (6, 128), (64, 64))
BITS = (255, 9)
FAMILY_PAIRS = 256
MAX_TERMS = 65536
WARM, REPS = 2, 7
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def stats(ms):
    return {"ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def spread(row):
    return row["max_ms"] - row["min_ms"]


def summarise(part):
    meds = {k: v["ms"] for k, v in part.items()}
    return {"largest_difference_between_family_medians_ms": round(max(meds.values()) - min(meds.values()), 4),
            "slowest_family": max(meds, key=meds.get), "fastest_family": min(meds, key=meds.get),
            "largest_min_max_spread_of_one_family_ms": round(max(spread(v) for v in part.values()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path[:0] = [os.path.join(ROOT, "go-curdleproofs_amd"), os.path.join(ROOT, "oracle", "py")]
    import numpy as np
    import torch
    import curdlemsm as cm

    if not cm.device_available():
        raise SystemExit("no HIP device: this benchmark measures the GPU path")
    cm.init(0)
    rng = np.random.default_rng(33)
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

    def limbs_for(n, bits):
        return random_limbs(n) if bits == 255 else mont([int(v) for v in rng.integers(0, 1 << bits, size=n)])

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

    def ratio(new, base):
        return {"new_over_baseline": round(new["ms"] / base["ms"], 3),
                "medians_apart_by_more_than_either_spread": bool(abs(base["ms"] - new["ms"]) > max(spread(new), spread(base)))}

    res = {"tool": "bench_msm_ct_bases", "warmups": WARM, "reps": REPS, "library": "this build",
           "statistic": "median of the repetitions, min and max kept",
           "timing": "MSM arms: torch (HIP) events on the caller's stream around the resident call; table build: wall time",
           "baseline": "curdle_msm_g1_ct_device / curdle_msm_g1_ct_batch_device on the same pairs, unchanged from the parent build",
           "arm_build": {}, "arm_single": {}, "arm_batch": {}, "arm_secret_dependence": {}}

    points = cm.g1_fixed_base_mul_batch(random_limbs(max(SINGLE_SIZES + tuple(k * n for k, n in BATCH_SHAPES))))

    # --- the table build ---------------------------------------------------------------------------------------------
    for c in CHUNK_BITS:
        out = res["arm_build"]["chunk_bits_%d" % c] = {}
        for n in BUILD_SIZES:
            ms = []
            for _ in range(WARM + REPS):
                w0 = time.perf_counter()
                h = cm.CtBases(points[:n], c)
                ms.append((time.perf_counter() - w0) * 1e3)
                h.free()
            out["n_%d" % n] = dict(stats(ms[WARM:]), table_bytes=96 * n * ((255 + c - 1) // c))
        print("build c = %d %s" % (c, json.dumps(out)), file=sys.stderr, flush=True)

    # --- the single call ---------------------------------------------------------------------------------------------
    for n in SINGLE_SIZES:
        d_pts = dev(points[:n])
        handles = {c: cm.CtBases(points[:n], c) for c in CHUNK_BITS}
        out = res["arm_single"]["n_%d" % n] = {"n": n}
        for bits in BITS:
            d_sc = dev(limbs_for(n, bits))
            torch.cuda.synchronize()

            def base_call():
                return cm.msm_g1_ct_device(d_pts.data_ptr(), d_sc.data_ptr(), n, bits, stream=s.cuda_stream)

            want = cm.msm_g1_device(d_pts.data_ptr(), d_sc.data_ptr(), n, stream=s.cuda_stream)
            if not (base_call() == want).all():
                raise SystemExit("n = %d, bits = %d: the constant-time MSM and the bucket MSM differ" % (n, bits))
            row = out["bits_%d" % bits] = {}
            for c in CHUNK_BITS:
                def new_call(h=handles[c]):
                    return h.msm_device(d_sc.data_ptr(), n, None, bits, stream=s.cuda_stream)
                if not (new_call() == want).all():
                    raise SystemExit("n = %d, bits = %d, chunk_bits = %d: the chunked MSM and the bucket MSM differ" % (n, bits, c))
                row["chunk_bits_%d" % c] = timed(new_call)
            row["baseline_msm_g1_ct_device"] = timed(base_call)
            for c in CHUNK_BITS:
                row["chunk_bits_%d" % c].update(ratio(row["chunk_bits_%d" % c], row["baseline_msm_g1_ct_device"]))
            del d_sc
        for h in handles.values():
            h.free()
        print("single n = %d %s" % (n, json.dumps(out)), file=sys.stderr, flush=True)
        del d_pts

    new, base = res["arm_single"]["n_256"]["bits_255"]["chunk_bits_16"], res["arm_single"]["n_256"]["bits_255"]["baseline_msm_g1_ct_device"]
    res["the_one_condition"] = {
        "what": "chunk_bits = 16, 255 bits, 256 pairs through a built handle: less than half of curdle_msm_g1_ct_device on the "
                "same pairs, the medians apart by more than the min-max spread of either arm",
        "new_ms": new["ms"], "baseline_ms": base["ms"], "half_of_baseline_ms": round(base["ms"] / 2, 4),
        "new_spread_ms": round(spread(new), 4), "baseline_spread_ms": round(spread(base), 4),
        "met": bool(new["ms"] < base["ms"] / 2 and base["ms"] - new["ms"] > max(spread(new), spread(base)))}
    best = min(CHUNK_BITS, key=lambda c: res["arm_single"]["n_256"]["bits_255"]["chunk_bits_%d" % c]["ms"])
    res["fastest_chunk_bits_at_256_pairs_255_bits"] = best

    # --- the batch ---------------------------------------------------------------------------------------------------
    for k, n in BATCH_SHAPES:
        total = k * n
        offs = np.arange(k + 1, dtype=np.uint64) * np.uint64(n)
        d_pts, d_sc = dev(points[:total]), dev(random_limbs(total))
        torch.cuda.synchronize()

        def base_call():
            return cm.msm_g1_ct_batch_device(d_pts.data_ptr(), d_sc.data_ptr(), offs, 255, stream=s.cuda_stream)

        want = cm.msm_g1_batch_device(d_pts.data_ptr(), d_sc.data_ptr(), offs, stream=s.cuda_stream)
        if not (base_call() == want).all():
            raise SystemExit("%d x %d: the constant-time batch and the bucket batch differ" % (k, n))
        row = res["arm_batch"]["%dx%d" % (k, n)] = {"k": k, "n": n}
        for c in CHUNK_BITS:
            cb = (255 + c - 1) // c
            if total * cb > MAX_TERMS:
                row["chunk_bits_%d" % c] = {"refused": "%d pairs x %d chunks exceed 65,536 terms" % (total, cb)}
                continue
            h = cm.CtBases(points[:total], c)

            def new_call():
                return h.msm_batch_device(d_sc.data_ptr(), offs, None, 255, stream=s.cuda_stream)

            if not (new_call() == want).all():
                raise SystemExit("%d x %d, chunk_bits = %d: the chunked batch and the bucket batch differ" % (k, n, c))
            row["chunk_bits_%d" % c] = timed(new_call)
            h.free()
        row["baseline_msm_g1_ct_batch_device"] = timed(base_call)
        for c in CHUNK_BITS:
            if "ms" in row["chunk_bits_%d" % c]:
                row["chunk_bits_%d" % c].update(ratio(row["chunk_bits_%d" % c], row["baseline_msm_g1_ct_batch_device"]))
        print("batch %d x %d %s" % (k, n, json.dumps(row)), file=sys.stderr, flush=True)
        del d_pts, d_sc

    # --- dependence on the secrets -----------------------------------------------------------------------------------
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
    handles = {c: cm.CtBases(points[:n], c) for c in CHUNK_BITS}
    part = res["arm_secret_dependence"]["single_%d" % n] = {
        "n": n, "order": "every repetition visits every family and every arm in turn, so that a drift of the clocks over the "
                         "run reaches all families alike"}
    d_fam = {name: dev(limbs) for name, limbs in families.items()}
    torch.cuda.synchronize()
    arms = {"default": lambda d_sc: cm.msm_g1_device(d_pts.data_ptr(), d_sc.data_ptr(), n, stream=s.cuda_stream)}
    for c in CHUNK_BITS:
        arms["chunk_bits_%d" % c] = lambda d_sc, h=handles[c]: h.msm_device(d_sc.data_ptr(), n, None, 255, stream=s.cuda_stream)
    for name, d_sc in d_fam.items():
        want = arms["default"](d_sc)
        for arm, call in arms.items():
            if not (call(d_sc) == want).all():
                raise SystemExit("family %s, %s: the two paths differ" % (name, arm))
    ms = {arm: {name: [] for name in families} for arm in arms}
    for _ in range(WARM + REPS):
        for name, d_sc in d_fam.items():
            for arm, call in arms.items():
                ms[arm][name].append(events(lambda: call(d_sc)))
    for arm in arms:
        part[arm] = {name: stats(v[WARM:]) for name, v in ms[arm].items()}
    for which in ["default"] + ["chunk_bits_%d" % c for c in CHUNK_BITS]:
        part[which + "_summary"] = summarise(part[which])
    d = part["default_summary"]
    part["control_sees_the_secrets"] = bool(
        d["largest_difference_between_family_medians_ms"] > 3 * d["largest_min_max_spread_of_one_family_ms"])
    for c in CHUNK_BITS:
        m = part["chunk_bits_%d_summary" % c]
        m["difference_within_the_repetition_spread"] = bool(
            m["largest_difference_between_family_medians_ms"] <= m["largest_min_max_spread_of_one_family_ms"])
    print("dependence %s" % json.dumps(part), file=sys.stderr, flush=True)
    for h in handles.values():
        h.free()
    res["stat_msm_ct_bases"] = cm.stat_msm_ct_bases()
    res["stat_msm_ct"] = cm.stat_msm_ct()
    res["stat_msm_ct_batch"] = cm.stat_msm_ct_batch()
    text = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
