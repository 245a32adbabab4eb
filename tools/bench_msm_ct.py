"""The constant-time MSM (curdle_msm_g1_ct_device: k_msm_ct_walk, k_g1_sum_ct, k_msm_ct_finish) against the bucket MSM
(curdle_msm_g1_device), and the shuffle step with CURDLE_SHUFFLE_CONSTANT_TIME against the one without, in ONE process,
same build, same run.

    python tools/bench_msm_ct.py [--out profiles/r27_msm_ct.json]

2 warm-ups, then 7 repetitions of every arm in a loop of its own; recorded are the median, the minimum and the maximum.
Resident arms: torch (HIP) events on the caller's stream around the _device call.  The shuffle step takes host arrays and
returns host arrays: wall time.
Cost arm: random subgroup points at n = 4 / 64 / 256 / 512 / 4,096 / 65,536, random scalars below 2^9 walked at 9 steps
and random scalars below r walked at 255, against curdle_msm_g1_device on the same inputs, the results compared first.
Shuffle arm: ell = 124 / 252 / 508, random permutation and k, flag on against flag off, the outputs compared first.
Dependence arm: the MSM at n = 512 and 65,536 over the families all 0 / all 1 / all r - 1 / random / random with the low
128 bits zero, and the shuffle step at ell = 252 over the identity, the reversal and a random permutation.  Reported: each
family's median, the largest difference between family medians and beside it the largest min-max spread of a single
family.  The constant-time call passes when the former lies within the latter; the default call is the control: its
largest difference must be more than three times its largest spread, or the arm cannot see a dependence where there is
one.  Evidence to record, not a gate.
Pricing arm: one curdleproof.Prove at ell = 252 (n = 256, 8 halving rounds) routed through the primitive: the prover's
MultiExp call sites and their sizes as SURVEY.md lists them from the reference's sources, each priced at the measured
255-step time of the next measured size.  tools/prove_trace.py, which would count the calls of a run, needs a preloaded
shim and was not run for this.
The last line printed is the JSON that --out also receives."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (4, 64, 256, 512, 4096, 65536)
BITS = (9, 255)
ELLS = (124, 252, 508)
FAMILY_NS = (512, 65536)
FAMILY_ELL = 252
WARM, REPS = 2, 7
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def stats(ms):
    return {"ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def prove_msm_sizes(ell):
    """The MultiExp calls of one Prove ("Call graph"): curdleproof.go 4, samepermutationargument 1,
    grandproductargument 6, innerproductargument 2 + 4 a round, samemultiscalarargument 3 + 6 a round."""
    n = ell + 4
    rounds = n.bit_length() - 1
    sizes = [ell, 4, ell, ell] + [ell] + [n] * 6 + [n] * 2 + [n] * 3
    for k in range(1, rounds + 1):
        sizes += [n >> k] * (4 + 6)
    return sizes


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
        part["verdict"] = "the control shows no dependence beyond its spread: this arm proves nothing"
    elif part["constant_time_difference_within_the_repetition_spread"]:
        part["verdict"] = "no dependence of the constant-time call on the secrets beyond the repetition spread; the control shows one"
    else:
        part["verdict"] = "the constant-time call's family medians differ by MORE than the repetition spread"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default=",".join(str(v) for v in SIZES))
    ap.add_argument("--ells", default=",".join(str(v) for v in ELLS))
    ap.add_argument("--family-ns", default=",".join(str(v) for v in FAMILY_NS))
    ap.add_argument("--family-ell", type=int, default=FAMILY_ELL)
    a = ap.parse_args()
    sys.path[:0] = [os.path.join(ROOT, "go-curdleproofs_amd"), os.path.join(ROOT, "oracle", "py")]
    import numpy as np
    import torch
    import curdlemsm as cm

    if not cm.device_available():
        raise SystemExit("no HIP device: this benchmark measures the GPU path")
    cm.init(0)
    rng = np.random.default_rng(27)
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

    def ct(d_pts, d_sc, n, bits):
        return lambda: cm.msm_g1_ct_device(d_pts.data_ptr(), d_sc.data_ptr(), n, bits, stream=s.cuda_stream)

    def default(d_pts, d_sc, n):
        return lambda: cm.msm_g1_device(d_pts.data_ptr(), d_sc.data_ptr(), n, stream=s.cuda_stream)

    res = {"tool": "bench_msm_ct", "warmups": WARM, "reps": REPS, "statistic": "median of the repetitions, min and max kept",
           "timing": "MSM arms: torch (HIP) events on the caller's stream around the resident call; shuffle arms: wall time",
           "arm_cost": {}, "arm_shuffle": {}, "arm_secret_dependence": {}, "arm_prove_pricing": {}}

    for n in [int(v) for v in a.sizes.split(",") if v]:
        out = res["arm_cost"][str(n)] = {"n": n}
        d_pts = dev(random_points(n))
        for bits in BITS:
            limbs = random_limbs(n) if bits == 255 else mont([int(v) for v in rng.integers(0, 1 << bits, size=n)])
            d_sc = dev(limbs)
            torch.cuda.synchronize()
            on, off = ct(d_pts, d_sc, n, bits), default(d_pts, d_sc, n)
            if not (on() == off()).all():
                raise SystemExit("n = %d, bits = %d: the results of the two paths differ" % (n, bits))
            row = out["bits_%d" % bits] = {"constant_time": timed(events, on), "default": timed(events, off)}
            row["constant_time_over_default"] = round(row["constant_time"]["ms"] / row["default"]["ms"], 3)
            del d_sc
        print("cost n = %d %s" % (n, json.dumps(out)), file=sys.stderr, flush=True)
        del d_pts

    def shuffle_setup(ell):
        rand = cm.Rand(ell)
        crs = cm.CRS(ell, rand)
        return crs, rand.get_g1_affines(ell), rand.get_g1_affines(ell), rand.get_fr()

    def shuffle_call(crs, Rs, Ss, perm, k, flags, keep=None):
        def call():
            got = cm.shuffle_permute_commit(crs, Rs, Ss, perm, k, cm.Rand(5), flags=flags)
            if keep is not None:
                keep[flags] = got
        return call

    def shuffle_same(crs, Rs, Ss, perm, k, what):
        got = {}
        shuffle_call(crs, Rs, Ss, perm, k, cm.SHUFFLE_CONSTANT_TIME, got)()
        shuffle_call(crs, Rs, Ss, perm, k, 0, got)()
        if not all((x == y).all() for x, y in zip(got[1], got[0])):
            raise SystemExit("%s: the outputs of the two paths differ" % what)

    for ell in [int(v) for v in a.ells.split(",") if v]:
        crs, Rs, Ss, k = shuffle_setup(ell)
        perm = cm.Rand(1000 + ell).generate_permutation(ell)
        shuffle_same(crs, Rs, Ss, perm, k, "ell = %d" % ell)
        out = res["arm_shuffle"][str(ell)] = {
            "ell": ell, "constant_time": timed(wall, shuffle_call(crs, Rs, Ss, perm, k, cm.SHUFFLE_CONSTANT_TIME)),
            "default": timed(wall, shuffle_call(crs, Rs, Ss, perm, k, 0))}
        out["constant_time_over_default"] = round(out["constant_time"]["ms"] / out["default"]["ms"], 3)
        print("shuffle ell = %d %s" % (ell, json.dumps(out)), file=sys.stderr, flush=True)

    for n in [int(v) for v in a.family_ns.split(",") if v]:
        low_zero = [int(v) for v in rng.integers(1, 1 << 62, size=n)]
        families = {
            "all 0": np.zeros((n, 4), dtype=np.uint64),
            "all 1": np.tile(mont([1]), (n, 1)),
            "all r - 1": np.tile(mont([R - 1]), (n, 1)),
            "random": random_limbs(n),
            "random, low 128 bits zero": mont([((v << 64 | w) % (R >> 128)) << 128 for v, w in zip(low_zero, reversed(low_zero))]),
        }
        d_pts = dev(random_points(n))
        part = res["arm_secret_dependence"]["msm_%d" % n] = {"n": n, "constant_time": {}, "default": {}}
        for name, limbs in families.items():
            d_sc = dev(limbs)
            torch.cuda.synchronize()
            if not (ct(d_pts, d_sc, n, 255)() == default(d_pts, d_sc, n)()).all():
                raise SystemExit("n = %d, family %s: the two paths differ" % (n, name))
            part["constant_time"][name] = timed(events, ct(d_pts, d_sc, n, 255))
            part["default"][name] = timed(events, default(d_pts, d_sc, n))
            del d_sc
        for which in ("constant_time", "default"):
            part[which + "_summary"] = summarise(part[which])
        verdict(part)
        print("dependence n = %d %s" % (n, json.dumps(part)), file=sys.stderr, flush=True)
        del d_pts

    if a.family_ell:
        ell = a.family_ell
        crs, Rs, Ss, k = shuffle_setup(ell)
        ident = np.arange(ell, dtype=np.uint32)
        families = {"identity": ident, "reversal": ident[::-1].copy(), "random": cm.Rand(1000 + ell).generate_permutation(ell)}
        part = res["arm_secret_dependence"]["shuffle_%d" % ell] = {"ell": ell, "constant_time": {}, "default": {}}
        for name, perm in families.items():
            shuffle_same(crs, Rs, Ss, perm, k, "ell = %d, %s" % (ell, name))
            part["constant_time"][name] = timed(wall, shuffle_call(crs, Rs, Ss, perm, k, cm.SHUFFLE_CONSTANT_TIME))
            part["default"][name] = timed(wall, shuffle_call(crs, Rs, Ss, perm, k, 0))
        for which in ("constant_time", "default"):
            part[which + "_summary"] = summarise(part[which])
        verdict(part)
        print("dependence shuffle %s" % json.dumps(part), file=sys.stderr, flush=True)

    measured = sorted((int(n), row["bits_255"]) for n, row in res["arm_cost"].items())
    if measured:
        sizes = prove_msm_sizes(252)
        total = {"constant_time": 0.0, "default": 0.0}
        for size in sizes:
            row = next((r for n, r in measured if n >= size), measured[-1][1])
            for which in total:
                total[which] += row[which]["ms"]
        res["arm_prove_pricing"] = {
            "ell": 252, "msm_calls": len(sizes), "largest": max(sizes), "pairs": sum(sizes),
            "source_of_the_calls": "SURVEY.md call graph of the reference's Prove; not a traced run",
            "rule": "each call at the measured 255-step time of the next measured size; calls one after another",
            "constant_time_ms": round(total["constant_time"], 2), "default_ms": round(total["default"], 2)}
    res["stat_msm_ct"] = cm.stat_msm_ct()
    res["stat_g1_mul_ct"] = cm.stat_g1_mul_ct()
    text = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
