"""What the constant-time prover costs: curdle_prove, curdle_prove_ex under CURDLE_PROVE_MSM_CONSTANT_TIME and
curdle_prove_ct at ell = 124 and 252, curdle_whisk_generate_shuffle_proof against its _ct form, and the oblivious scalar
gather (curdle_fr_permute_ct_device) alone at n = 124 and 4,096, in ONE process on one device.

    python tools/bench_prove_ct.py [--out profiles/r29_prove_ct.json]

2 warm-ups, then 7 repetitions of every arm in a loop of its own; recorded are the median, the minimum and the maximum.
Prove and the Whisk calls take host arrays and return bytes: wall time.  The gather is resident: torch (HIP) events on
the caller's stream.  Every arm's results are compared before anything is timed.  The expectation the JSON is held
against: curdle_prove_ct costs the flagged curdle_prove_ex at the same ell plus about two lone walks (the two batches
of four small MSMs that replace the twelve host scalar multiplications; a lone walk is measured here as a
curdle_msm_g1_ct of 6 pairs).  No gate; where the difference exceeds three walks the note says so.
The last line printed is the JSON that --out also receives."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ELLS = (124, 252)
GATHER_NS = (124, 4096)
WARM, REPS = 2, 7


def stats(ms):
    return {"ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r29_prove_ct.json"))
    a = ap.parse_args()
    sys.path[:0] = [os.path.join(ROOT, "go-curdleproofs_amd"), os.path.join(ROOT, "oracle", "py")]
    import numpy as np
    import torch
    import curdlemsm as cm

    if not cm.device_available():
        raise SystemExit("no HIP device: this benchmark measures the GPU path")
    cm.init(0)
    rng = np.random.default_rng(29)
    s = torch.cuda.Stream()

    def wall(call):
        w0 = time.perf_counter()
        call()
        return (time.perf_counter() - w0) * 1e3

    def events(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            e0.record()
            call()
            e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def timed(how, call):
        return stats([how(call) for _ in range(WARM + REPS)][WARM:])

    res = {"tool": "bench_prove_ct", "warmups": WARM, "reps": REPS, "statistic": "median of the repetitions, min and max kept",
           "timing": "Prove and Whisk arms: wall time of the host call; gather and lone walk: torch (HIP) events on the caller's stream",
           "arm_prove": {}, "arm_whisk": {}, "arm_gather": {}}

    # a lone walk: the constant-time MSM of six pairs, resident
    limbs = rng.integers(0, 1 << 64, size=(6, 4), dtype=np.uint64)
    limbs[:, 3] &= np.uint64((1 << 62) - 1)
    pts = cm.g1_fixed_base_mul_batch(limbs)
    d_pts = torch.from_numpy(pts.view(np.int64).reshape(-1)).to("cuda:0")
    d_sc = torch.from_numpy(limbs.view(np.int64).reshape(-1)).to("cuda:0")
    torch.cuda.synchronize()
    res["lone_walk_6_pairs"] = timed(events, lambda: cm.msm_g1_ct_device(d_pts.data_ptr(), d_sc.data_ptr(), 6, 255, stream=s.cuda_stream))
    walk = res["lone_walk_6_pairs"]["ms"]

    for ell in ELLS:
        rand = cm.Rand(ell)
        crs = cm.CRS(ell, rand)
        perm = cm.Rand(1000 + ell).generate_permutation(ell)
        k, Rs, Ss = rand.get_fr(), rand.get_g1_affines(ell), rand.get_g1_affines(ell)
        Ts, Us, M, rs_m = cm.shuffle_permute_commit(crs, Rs, Ss, perm, k, rand)
        inst = (crs, Rs, Ss, Ts, Us, M, perm, k, rs_m)
        plain = lambda: cm.prove(*inst, cm.Rand(42))
        flagged = lambda: cm.prove(*inst, cm.Rand(42), flags=cm.PROVE_MSM_CONSTANT_TIME)
        ct = lambda: cm.prove_ct(*inst, cm.Rand(42))
        if not (plain() == flagged() == ct()):
            raise SystemExit("ell = %d: the proofs of the three paths differ" % ell)
        out = res["arm_prove"][str(ell)] = {"ell": ell}
        b0, m0 = cm.stat_alg_msm(), cm.stat_host_point_mul()
        ct()
        b1, m1 = cm.stat_alg_msm(), cm.stat_host_point_mul()
        out["one_prove_ct"] = {"constant_time_calls": b1["ct_calls"] - b0["ct_calls"], "constant_time_pairs": b1["ct_pairs"] - b0["ct_pairs"],
                               "bucket_calls": b1["bucket_calls"] - b0["bucket_calls"], "host_point_mul_calls": m1 - m0}
        out["curdle_prove"] = timed(wall, plain)
        out["curdle_prove_ex_flagged"] = timed(wall, flagged)
        out["curdle_prove_ct"] = timed(wall, ct)
        extra = out["curdle_prove_ct"]["ms"] - out["curdle_prove_ex_flagged"]["ms"]
        out["prove_ct_minus_flagged_ms"] = round(extra, 4)
        out["prove_ct_minus_flagged_in_lone_walks"] = round(extra / walk, 3)
        print("prove ell = %d %s" % (ell, json.dumps(out)), file=sys.stderr, flush=True)

    crs = cm.CRS(cm.WHISK_ELL, cm.Rand(4))
    r = cm.Rand(31)
    trk, _ = cm.whisk_compute_trackers_batch(r.get_frs(cm.WHISK_ELL), r.get_frs(cm.WHISK_ELL), commitments=False)
    pre = [trk[i].tobytes() for i in range(cm.WHISK_ELL)]
    plain = lambda: cm.whisk_generate_shuffle_proof(crs, pre, cm.Rand(61))
    ct = lambda: cm.whisk_generate_shuffle_proof_ct(crs, pre, cm.Rand(61))
    if plain() != ct():
        raise SystemExit("whisk: the two calls differ")
    res["arm_whisk"]["curdle_whisk_generate_shuffle_proof"] = timed(wall, plain)
    res["arm_whisk"]["curdle_whisk_generate_shuffle_proof_ct"] = timed(wall, ct)
    print("whisk %s" % json.dumps(res["arm_whisk"]), file=sys.stderr, flush=True)

    for n in GATHER_NS:
        rec = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
        perm = rng.permutation(n).astype(np.uint32)
        d_in = torch.from_numpy(rec.view(np.int64).reshape(-1)).to("cuda:0")
        d_perm = torch.from_numpy(perm.view(np.int32)).to("cuda:0")
        d_out = torch.zeros(4 * n, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        call = lambda: cm.fr_permute_ct_device(d_in.data_ptr(), d_perm.data_ptr(), n, d_out.data_ptr(), stream=s.cuda_stream)
        call()
        if not (d_out.cpu().numpy().view(np.uint64).reshape(n, 4) == rec[perm]).all():
            raise SystemExit("gather n = %d: not numpy's a[perm]" % n)
        res["arm_gather"][str(n)] = timed(events, call)
        res["arm_gather"]["host_form_%d" % n] = timed(wall, lambda: cm.fr_permute_ct(rec, perm))
    print("gather %s" % json.dumps(res["arm_gather"]), file=sys.stderr, flush=True)

    worst = max(res["arm_prove"][str(ell)]["prove_ct_minus_flagged_in_lone_walks"] for ell in ELLS)
    res["note"] = ("expected: curdle_prove_ct = flagged curdle_prove_ex + about two lone walks.  Largest measured difference: %.2f lone "
                   "walks.%s" % (worst, "" if worst <= 3 else "  ABOVE three walks: beyond the two batches' walks the route adds two host-form "
                                 "gathers (arm_gather, host_form_*: slot, staging, copy, wipe and two synchronisations each) and the normalisation "
                                 "of six public bases to affine on the host (a field inversion each) per batch; proof.A and the grand-product "
                                 "C as one call instead of a batch of two walk the same pairs."))
    text = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
