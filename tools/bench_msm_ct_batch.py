"""The batched constant-time MSM (curdle_msm_g1_ct_batch_device: ONE k_msm_ct_walk, k_g1_sum_ct_seg, k_msm_ct_finish_seg)
against a loop of single constant-time calls over the same MSMs and against the bucket batch
(curdle_msm_g1_batch_device), and Prove with CURDLE_PROVE_MSM_CONSTANT_TIME against Prove without, in ONE process, same
build, same run.

    python tools/bench_msm_ct_batch.py [--out profiles/r28_msm_ct_batch.json] [--merge-parent FILE]
    python tools/bench_msm_ct_batch.py --parent-arms-only --package <an older build's go-curdleproofs_amd> --out FILE

2 warm-ups, then 7 repetitions of every arm in a loop of its own; recorded are the median, the minimum and the maximum.
Resident arms: torch (HIP) events on the caller's stream around the _device call(s).  Prove takes host arrays and returns
bytes: wall time.  Every arm's results are compared before anything is timed.
Batch arm: k x n = 4 x 129, 2 x 256, 6 x 128, 64 x 64 and 4,096 x 16 at 255 and at 9 bits.  The loop of single calls runs
over at most 64 of the k MSMs (4,096 single calls at 5.5 ms would be 22 s a repetition); where k is larger the row says so
and scales the loop's time by k / 64.  THE ONE CONDITION: the batch of 4 x 129 at 255 bits is below TWO single calls of
129 pairs (one chain and four one-lane inversions in parallel blocks against four chains); the JSON says whether it held.
Prove arm: ell = 124 and 252, a random permutation, flag on against flag off, with the calls and pairs of one run from
curdle_stat_alg_msm, and the batch arm's prices put on them: each funnel call at the measured 255-bit batch time.
Dependence arm: the batch at 4 x 129 and 4,096 x 16 over the families all 0 / all 1 / all r - 1 / random / random with the
low 128 bits zero, and the flagged Prove at ell = 124 over the identity, the reversal and a random permutation.  Reported
as tools/bench_msm_ct.py reports it: each family's median, the largest difference between family medians and beside it
the largest min-max spread of a single family; the bucket path is the control and must show a difference of more than
three times its spread, or the row proves nothing.  Evidence to record, not a gate.
--parent-arms-only measures what a build without the batched call has (the loop of single calls, the bucket batch, the
unflagged Prove); --merge-parent puts such a file under "parent_build".
The last line printed is the JSON that --out also receives."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((4, 129), (2, 256), (6, 128), (64, 64), (4096, 16))
BITS = (255, 9)
ELLS = (124, 252)
FAMILY_SHAPES = ((4, 129), (4096, 16))
FAMILY_ELL = 124
SINGLES_MAX = 64
WARM, REPS = 2, 7
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def stats(ms):
    return {"ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def summarise(part):
    meds = {k: v["ms"] for k, v in part.items()}
    return {"largest_difference_between_family_medians_ms": round(max(meds.values()) - min(meds.values()), 4),
            "slowest_family": max(meds, key=meds.get), "fastest_family": min(meds, key=meds.get),
            "largest_min_max_spread_of_one_family_ms": round(max(v["max_ms"] - v["min_ms"] for v in part.values()), 4)}


def verdict(part):
    c, d = part["constant_time_summary"], part["default_summary"]
    part["control_sees_the_secrets"] = bool(
        d["largest_difference_between_family_medians_ms"] > 3 * d["largest_min_max_spread_of_one_family_ms"])
    part["constant_time_difference_within_the_repetition_spread"] = bool(
        c["largest_difference_between_family_medians_ms"] <= c["largest_min_max_spread_of_one_family_ms"])
    if not part["control_sees_the_secrets"]:
        part["verdict"] = "the control shows no dependence beyond its spread: this row proves nothing"
    elif part["constant_time_difference_within_the_repetition_spread"]:
        part["verdict"] = "no dependence of the constant-time call on the secrets beyond the repetition spread; the control shows one"
    else:
        part["verdict"] = "the constant-time call's family medians differ by MORE than the repetition spread"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-arms-only", action="store_true")
    ap.add_argument("--merge-parent", default=None)
    ap.add_argument("--package", default=os.path.join(ROOT, "go-curdleproofs_amd"),
                    help="the directory that holds curdlemsm/ and libcurdlemsm.so (an older build's, with --parent-arms-only)")
    a = ap.parse_args()
    sys.path[:0] = [a.package, os.path.join(ROOT, "oracle", "py")]
    import numpy as np
    import torch
    import curdlemsm as cm

    if not cm.device_available():
        raise SystemExit("no HIP device: this benchmark measures the GPU path")
    cm.init(0)
    new = not a.parent_arms_only
    rng = np.random.default_rng(28)
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

    def random_points(n):
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

    def batch(d_pts, d_sc, offs, bits):
        return lambda: cm.msm_g1_ct_batch_device(d_pts.data_ptr(), d_sc.data_ptr(), offs, bits, stream=s.cuda_stream)

    def bucket(d_pts, d_sc, offs):
        return lambda: cm.msm_g1_batch_device(d_pts.data_ptr(), d_sc.data_ptr(), offs, stream=s.cuda_stream)

    def singles(d_pts, d_sc, n, count, bits):
        def call():
            return np.array([cm.msm_g1_ct_device(d_pts.data_ptr() + 96 * n * j, d_sc.data_ptr() + 32 * n * j, n, bits,
                                                 stream=s.cuda_stream) for j in range(count)])
        return call

    res = {"tool": "bench_msm_ct_batch", "warmups": WARM, "reps": REPS, "library": "the older build given with --package" if a.parent_arms_only else "this build",
           "statistic": "median of the repetitions, min and max kept",
           "timing": "MSM arms: torch (HIP) events on the caller's stream around the resident call(s); Prove arms: wall time",
           "arm_batch": {}, "arm_prove": {}, "arm_secret_dependence": {}}

    for k, n in SHAPES:
        offs = np.arange(k + 1, dtype=np.uint64) * np.uint64(n)
        out = res["arm_batch"]["%dx%d" % (k, n)] = {"k": k, "n": n}
        d_pts = dev(random_points(k * n))
        count = min(k, SINGLES_MAX)
        for bits in BITS:
            limbs = random_limbs(k * n) if bits == 255 else mont([int(v) for v in rng.integers(0, 1 << bits, size=k * n)])
            d_sc = dev(limbs)
            torch.cuda.synchronize()
            one, off = singles(d_pts, d_sc, n, count, bits), bucket(d_pts, d_sc, offs)
            want = off()
            if not (one() == want[:count]).all():
                raise SystemExit("%d x %d, bits = %d: the single calls and the bucket batch differ" % (k, n, bits))
            if new and not (batch(d_pts, d_sc, offs, bits)() == want).all():
                raise SystemExit("%d x %d, bits = %d: the batched call and the bucket batch differ" % (k, n, bits))
            row = out["bits_%d" % bits] = {}
            if new:
                row["batch"] = timed(events, batch(d_pts, d_sc, offs, bits))
            row["single_calls"] = timed(events, one)
            row["single_calls_measured_msms"] = count
            row["single_calls_scaled_to_k_ms"] = round(row["single_calls"]["ms"] * k / count, 4)
            row["one_single_call_ms"] = round(row["single_calls"]["ms"] / count, 4)
            row["bucket_batch"] = timed(events, off)
            if new:
                row["batch_over_one_single_call"] = round(row["batch"]["ms"] / row["one_single_call_ms"], 3)
                row["batch_over_bucket_batch"] = round(row["batch"]["ms"] / row["bucket_batch"]["ms"], 3)
            del d_sc
        print("batch %d x %d %s" % (k, n, json.dumps(out)), file=sys.stderr, flush=True)
        del d_pts
    if new:
        row = res["arm_batch"]["4x129"]["bits_255"]
        res["the_one_condition"] = {
            "what": "the batch of 4 x 129 at 255 bits is below two single calls of 129 pairs, measured in this process",
            "batch_ms": row["batch"]["ms"], "two_single_calls_ms": round(2 * row["one_single_call_ms"], 4),
            "met": bool(row["batch"]["ms"] < 2 * row["one_single_call_ms"])}

    def prove_setup(ell, perm=None):
        rand = cm.Rand(ell)
        crs = cm.CRS(ell, rand)
        if perm is None:
            perm = cm.Rand(1000 + ell).generate_permutation(ell)
        k, Rs, Ss = rand.get_fr(), rand.get_g1_affines(ell), rand.get_g1_affines(ell)
        Ts, Us, M, rs_m = cm.shuffle_permute_commit(crs, Rs, Ss, perm, k, rand)
        return crs, Rs, Ss, Ts, Us, M, perm, k, rs_m

    def prove_call(inst, flags):
        return lambda: cm.prove(*inst, cm.Rand(42), flags=flags)

    def prove_same(inst, what):
        if prove_call(inst, cm.PROVE_MSM_CONSTANT_TIME)() != prove_call(inst, None)():
            raise SystemExit("%s: the proofs of the two paths differ" % what)

    for ell in ELLS:
        inst = prove_setup(ell)
        out = res["arm_prove"][str(ell)] = {"ell": ell}
        if new:
            prove_same(inst, "ell = %d" % ell)
            before = cm.stat_alg_msm()
            prove_call(inst, None)()
            after = cm.stat_alg_msm()
            out["one_run_from_curdle_stat_alg_msm"] = {"calls": after["bucket_calls"] - before["bucket_calls"],
                                                       "pairs": after["bucket_pairs"] - before["bucket_pairs"]}
            out["constant_time"] = timed(wall, prove_call(inst, cm.PROVE_MSM_CONSTANT_TIME))
        out["default"] = timed(wall, lambda: cm.prove(*inst, cm.Rand(42)))
        if new:
            out["constant_time_over_default"] = round(out["constant_time"]["ms"] / out["default"]["ms"], 3)
            out["constant_time_ms_per_funnel_call"] = round(
                out["constant_time"]["ms"] / out["one_run_from_curdle_stat_alg_msm"]["calls"], 3)
        print("prove ell = %d %s" % (ell, json.dumps(out)), file=sys.stderr, flush=True)
    if new:
        p = res["arm_prove"]["252"]
        res["pricing_restated"] = {
            "round_27_pricing": "558 ms for one Prove at ell = 252 with 96 untraced calls of 6,378 pairs routed ONE BY ONE, against 23 ms",
            "counted_calls": p["one_run_from_curdle_stat_alg_msm"]["calls"],
            "counted_pairs": p["one_run_from_curdle_stat_alg_msm"]["pairs"],
            "measured_constant_time_ms": p["constant_time"]["ms"], "measured_default_ms": p["default"]["ms"]}

    if new:
        for k, n in FAMILY_SHAPES:
            total = k * n
            offs = np.arange(k + 1, dtype=np.uint64) * np.uint64(n)
            low_zero = [int(v) for v in rng.integers(1, 1 << 62, size=total)]
            families = {
                "all 0": np.zeros((total, 4), dtype=np.uint64),
                "all 1": np.tile(mont([1]), (total, 1)),
                "all r - 1": np.tile(mont([R - 1]), (total, 1)),
                "random": random_limbs(total),
                "random, low 128 bits zero": mont([((v << 64 | w) % (R >> 128)) << 128 for v, w in zip(low_zero, reversed(low_zero))]),
            }
            d_pts = dev(random_points(total))
            part = res["arm_secret_dependence"]["batch_%dx%d" % (k, n)] = {"k": k, "n": n, "constant_time": {}, "default": {}}
            for name, limbs in families.items():
                d_sc = dev(limbs)
                torch.cuda.synchronize()
                if not (batch(d_pts, d_sc, offs, 255)() == bucket(d_pts, d_sc, offs)()).all():
                    raise SystemExit("%d x %d, family %s: the two paths differ" % (k, n, name))
                part["constant_time"][name] = timed(events, batch(d_pts, d_sc, offs, 255))
                part["default"][name] = timed(events, bucket(d_pts, d_sc, offs))
                del d_sc
            for which in ("constant_time", "default"):
                part[which + "_summary"] = summarise(part[which])
            verdict(part)
            print("dependence %d x %d %s" % (k, n, json.dumps(part)), file=sys.stderr, flush=True)
            del d_pts

        ell = FAMILY_ELL
        ident = np.arange(ell, dtype=np.uint32)
        families = {"identity": ident, "reversal": ident[::-1].copy(), "random": cm.Rand(1000 + ell).generate_permutation(ell)}
        part = res["arm_secret_dependence"]["prove_%d" % ell] = {"ell": ell, "constant_time": {}, "default": {}}
        for name, perm in families.items():
            inst = prove_setup(ell, perm)
            prove_same(inst, "ell = %d, %s" % (ell, name))
            part["constant_time"][name] = timed(wall, prove_call(inst, cm.PROVE_MSM_CONSTANT_TIME))
            part["default"][name] = timed(wall, prove_call(inst, None))
        for which in ("constant_time", "default"):
            part[which + "_summary"] = summarise(part[which])
        verdict(part)
        part["note"] = ("wall time of a whole Prove: the host part, which the flag does not change, is in both columns; the "
                        "control's MSM scalars are challenge multiples of the permuted vector and show little of the permutation")
        print("dependence prove %s" % json.dumps(part), file=sys.stderr, flush=True)
        res["stat_msm_ct"] = cm.stat_msm_ct()
        res["stat_msm_ct_batch"] = cm.stat_msm_ct_batch()
        res["stat_alg_msm"] = cm.stat_alg_msm()
    if a.merge_parent:
        with open(a.merge_parent) as f:
            res["parent_build"] = json.loads(f.read().strip().splitlines()[-1])
    text = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
