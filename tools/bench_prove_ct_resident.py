"""What the constant-time prover over resident tables costs: curdle_prover_ct_prove against curdle_prove_ct and curdle_prove
at ell = 124 and 252 in the same run, curdle_prover_ct_create, the Whisk form against curdle_whisk_generate_shuffle_proof_ct,
curdle_msm_g1_ct_bases_sets_batch against the single-handle batch on the same pairs, and the handle's Prove by permutation
family (identity / reversal / random: evidence only), in ONE process on one device.

    python tools/bench_prove_ct_resident.py [--out profiles/r35_prove_ct_resident.json]
    python tools/bench_prove_ct_resident.py --proofs 20      # only N handle Proves at ell = 124, for a kernel trace

2 warm-ups, then 7 repetitions of every arm in a loop of its own; recorded are the median, the minimum and the maximum.
Every call takes host arrays and returns bytes or words: wall time.  Every arm's results are compared before anything
is timed.  The condition, set beforehand: at ell = 124 the handle's Prove is below HALF of curdle_prove_ct measured in
this process, by more than both repetition spreads (max - min).  The JSON says whether it held; the tool does not fail
when it does not.  The last line printed is the JSON that --out also receives."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ELLS = (124, 252)
WARM, REPS = 2, 7


def stats(ms):
    return {"ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r35_prove_ct_resident.json"))
    ap.add_argument("--proofs", type=int, default=0)
    a = ap.parse_args()
    sys.path[:0] = [os.path.join(ROOT, "go-curdleproofs_amd"), os.path.join(ROOT, "oracle", "py")]
    import numpy as np
    import curdlemsm as cm

    if not cm.device_available():
        raise SystemExit("no HIP device: this benchmark measures the GPU path")
    cm.init(0)

    def wall(call):
        w0 = time.perf_counter()
        call()
        return (time.perf_counter() - w0) * 1e3

    def timed(call):
        return stats([wall(call) for _ in range(WARM + REPS)][WARM:])

    def instance(ell, family):
        rand = cm.Rand(ell)
        crs = cm.CRS(ell, rand)
        perm = {"identity": np.arange(ell, dtype=np.uint32), "reversal": np.arange(ell, dtype=np.uint32)[::-1].copy(),
                "random": np.asarray(cm.Rand(1000 + ell).generate_permutation(ell), dtype=np.uint32)}[family]
        k, Rs, Ss = rand.get_fr(), rand.get_g1_affines(ell), rand.get_g1_affines(ell)
        Ts, Us, M, rs_m = cm.shuffle_permute_commit(crs, Rs, Ss, perm, k, rand)
        return crs, Rs, Ss, Ts, Us, M, perm, k, rs_m

    if a.proofs:
        inst = instance(124, "random")
        prover = cm.ProverCt(inst[0])
        want = cm.prove_ct(*inst, cm.Rand(42))
        for _ in range(a.proofs):
            if prover.prove(*inst[1:], cm.Rand(42)) != want:
                raise SystemExit("the handle's proof differs")
        print(json.dumps({"tool": "bench_prove_ct_resident", "proofs": a.proofs, "ell": 124}))
        return

    res = {"tool": "bench_prove_ct_resident", "warmups": WARM, "reps": REPS,
           "statistic": "median of the repetitions, min and max kept", "timing": "wall time of the host call, one process",
           "arm_prove": {}, "arm_whisk": {}, "arm_sets_call": {}, "arm_families": {}}

    for ell in ELLS:
        inst = instance(ell, "random")
        crs, rest = inst[0], inst[1:]
        create = []
        for _ in range(WARM + REPS):
            w0 = time.perf_counter()
            p = cm.ProverCt(crs)
            create.append((time.perf_counter() - w0) * 1e3)
            p.free()
        prover = cm.ProverCt(crs)
        plain = lambda: cm.prove(*inst, cm.Rand(42))
        ct = lambda: cm.prove_ct(*inst, cm.Rand(42))
        handle = lambda: prover.prove(*rest, cm.Rand(42))
        if not (plain() == ct() == handle()):
            raise SystemExit("ell = %d: the proofs of the three paths differ" % ell)
        out = res["arm_prove"][str(ell)] = {"ell": ell, "curdle_prover_ct_create": stats(create[WARM:])}
        s0 = cm.stat_alg_msm(), cm.stat_alg_msm_resident(), cm.stat_msm_ct_bases(), cm.stat_msm_ct()
        handle()
        s1 = cm.stat_alg_msm(), cm.stat_alg_msm_resident(), cm.stat_msm_ct_bases(), cm.stat_msm_ct()
        d = [{n: y[n] - x[n] for n in x} for x, y in zip(s0, s1)]
        out["one_handle_prove"] = {"constant_time_calls": d[0]["ct_calls"], "constant_time_pairs": d[0]["ct_pairs"],
                                   "resident_calls": d[1]["resident_calls"], "fallback_calls": d[1]["fallback_calls"],
                                   "tables_built": d[2]["tables"], "chunk_lanes": d[2]["lanes"], "unchunked_walks": d[3]["walks"]}
        out["curdle_prove"] = timed(plain)
        out["curdle_prove_ct"] = timed(ct)
        out["curdle_prover_ct_prove"] = timed(handle)
        h, c = out["curdle_prover_ct_prove"], out["curdle_prove_ct"]
        out["handle_over_prove_ct"] = round(h["ms"] / c["ms"], 4)
        out["per_funnel_call_ms"] = {"curdle_prove_ct": round(c["ms"] / d[0]["ct_calls"], 4),
                                     "curdle_prover_ct_prove": round(h["ms"] / d[0]["ct_calls"], 4)}
        prover.free()
        print("prove ell = %d %s" % (ell, json.dumps(out)), file=sys.stderr, flush=True)

    # the condition, set before anything was measured
    p124 = res["arm_prove"]["124"]
    h, c = p124["curdle_prover_ct_prove"], p124["curdle_prove_ct"]
    spreads = (h["max_ms"] - h["min_ms"]) + (c["max_ms"] - c["min_ms"])
    res["condition"] = {"text": "at ell = 124 curdle_prover_ct_prove is below half of curdle_prove_ct by more than both repetition spreads",
                        "half_of_prove_ct_ms": round(c["ms"] / 2, 4), "handle_ms": h["ms"], "both_spreads_ms": round(spreads, 4),
                        "held": bool(c["ms"] / 2 - h["ms"] > spreads)}

    # by permutation family at ell = 124: evidence only, the shapes are public
    for family in ("identity", "reversal", "random"):
        inst = instance(124, family)
        prover = cm.ProverCt(inst[0])
        if prover.prove(*inst[1:], cm.Rand(42)) != cm.prove_ct(*inst, cm.Rand(42)):
            raise SystemExit("family %s: the proofs differ" % family)
        res["arm_families"][family] = timed(lambda: prover.prove(*inst[1:], cm.Rand(42)))
        prover.free()

    # the Whisk form
    crs = cm.CRS(cm.WHISK_ELL, cm.Rand(4))
    r = cm.Rand(31)
    trk, _ = cm.whisk_compute_trackers_batch(r.get_frs(cm.WHISK_ELL), r.get_frs(cm.WHISK_ELL), commitments=False)
    pre = [trk[i].tobytes() for i in range(cm.WHISK_ELL)]
    prover = cm.ProverCt(crs)
    ct = lambda: cm.whisk_generate_shuffle_proof_ct(crs, pre, cm.Rand(61))
    handle = lambda: prover.whisk_shuffle_proof(pre, cm.Rand(61))
    if ct() != handle():
        raise SystemExit("whisk: the two calls differ")
    res["arm_whisk"]["curdle_whisk_generate_shuffle_proof_ct"] = timed(ct)
    res["arm_whisk"]["curdle_prover_ct_whisk_shuffle_proof"] = timed(handle)
    prover.free()
    print("whisk %s" % json.dumps(res["arm_whisk"]), file=sys.stderr, flush=True)

    # the sets call against the single-handle batch on the same pairs: 256 and 2,048 pairs in 4 MSMs over 132 + 496 points
    rng = np.random.default_rng(35)
    limbs = rng.integers(0, 1 << 64, size=(628, 4), dtype=np.uint64)
    limbs[:, 3] &= np.uint64((1 << 62) - 1)
    pts = cm.g1_fixed_base_mul_batch(limbs)
    one = cm.CtBases(pts)
    two = [cm.CtBases(np.ascontiguousarray(pts[:132])), cm.CtBases(np.ascontiguousarray(pts[132:]))]
    for n in (256, 2048):
        sc = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
        sc[:, 3] &= np.uint64((1 << 62) - 1)
        rows = rng.integers(0, 628, size=n).astype(np.uint32)
        offs = [0, n // 4, n // 2, 3 * n // 4, n]
        single = lambda: one.msm_batch(sc, offs, rows)
        sets = lambda: cm.msm_g1_ct_bases_sets_batch(two, rows, sc, offs)
        if not (single() == sets()).all():
            raise SystemExit("sets call, n = %d: the results differ" % n)
        res["arm_sets_call"][str(n)] = {"pairs": n, "curdle_msm_g1_ct_bases_batch": timed(single),
                                        "curdle_msm_g1_ct_bases_sets_batch": timed(sets)}
    print("sets call %s" % json.dumps(res["arm_sets_call"]), file=sys.stderr, flush=True)

    text = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
