"""What proving in batches buys: curdle_prove_batch at ell = 124 and 252 with k = 1, 8, 64 members, without the flag and
under CURDLE_PROVE_BATCH_CONSTANT_TIME, against a loop of k single calls (curdle_prove / curdle_prove_ct) and against
the same k single calls spread over 16 threads, and curdle_whisk_generate_shuffle_proof_batch (n = 128: 124 trackers and
the four blinders) against its single calls the same way -- in ONE process on one device, the single calls being the
code they were before the batch existed.

    python tools/bench_prove_batch.py [--out profiles/r30_prove_batch.json] [--ells 124,252] [--ks 1,8,64]

2 warm-ups, then 7 repetitions of every arm in a loop of its own; recorded are the median, the minimum and the maximum
of the wall time of the whole arm (k proofs), and the median per proof.  Every arm's proofs are compared before
anything is timed.  The expectations the JSON is held against, none of them a gate: a constant-time batch that fits one
pass per step costs roughly ONE single curdle_prove_ct, since a walk's time does not depend on its pairs
(batch_over_one_single); the default form's time per proof at k = 64 falls below the 16-thread loop's.
The last line printed is the JSON that --out also receives."""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM, REPS, THREADS = 2, 7, 16


def stats(ms, k):
    med = statistics.median(ms)
    return {"ms": round(med, 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "ms_per_proof": round(med / k, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r30_prove_batch.json"))
    ap.add_argument("--ells", default="124,252")
    ap.add_argument("--ks", default="1,8,64")
    ap.add_argument("--no-whisk", action="store_true")
    a = ap.parse_args()
    ells = [int(v) for v in a.ells.split(",") if v]
    ks = [int(v) for v in a.ks.split(",") if v]
    sys.path[:0] = [os.path.join(ROOT, "go-curdleproofs_amd"), os.path.join(ROOT, "oracle", "py")]
    import numpy as np
    import curdlemsm as cm

    if not cm.device_available():
        raise SystemExit("no HIP device: this benchmark measures the GPU path")
    cm.init(0)
    pool = ThreadPoolExecutor(max_workers=THREADS)

    def timed(call, k):
        out = []
        for _ in range(WARM + REPS):
            w0 = time.perf_counter()
            call()
            out.append((time.perf_counter() - w0) * 1e3)
        return stats(out[WARM:], k)

    def arms(label, k, batch, one, forms):
        """batch(flags) -> k results; one(i, flags) -> member i's single result."""
        out = {}
        for flags, form in forms:
            loop = lambda: [one(i, flags) for i in range(k)]
            threads = lambda: list(pool.map(lambda i: one(i, flags), range(k)))
            want = loop()
            if batch(flags) != want or threads() != want:
                raise SystemExit("%s k = %d %s: the batch, the loop and the threads differ" % (label, k, form))
            s0 = cm.stat_prove_batch()
            batch(flags)
            s1 = cm.stat_prove_batch()
            r = out[form] = {"k": k, "coalesced_device_calls": s1["device_calls"] - s0["device_calls"], "groups": s1["groups"] - s0["groups"],
                             "batch": timed(lambda: batch(flags), k), "loop_of_single_calls": timed(loop, k),
                             "single_calls_on_%d_threads" % THREADS: timed(threads, k)}
            r["batch_over_loop"] = round(r["batch"]["ms"] / r["loop_of_single_calls"]["ms"], 4)
            r["batch_over_threads"] = round(r["batch"]["ms"] / r["single_calls_on_%d_threads" % THREADS]["ms"], 4)
            print("%s k = %d %s %s" % (label, k, form, json.dumps(r)), file=sys.stderr, flush=True)
        return out

    forms = ((0, "default"), (cm.PROVE_BATCH_CONSTANT_TIME, "constant_time"))
    res = {"tool": "bench_prove_batch", "warmups": WARM, "reps": REPS, "threads": THREADS,
           "statistic": "median of the repetitions of the whole arm (k proofs), min and max kept; ms_per_proof = median / k",
           "timing": "wall time of the host calls, one process, one device", "arm_prove": {}, "arm_whisk": {}}

    for ell in ells:
        crs = cm.CRS(ell, cm.Rand(ell))
        members = []
        for i in range(max(ks)):
            rand = cm.Rand(7000 + 100 * ell + i)
            perm = np.asarray(cm.Rand(1000 + ell + i).generate_permutation(ell), dtype=np.uint32)
            k_i, Rs, Ss = rand.get_fr(), rand.get_g1_affines(ell), rand.get_g1_affines(ell)
            Ts, Us, M, rs_m = cm.shuffle_permute_commit(crs, Rs, Ss, perm, k_i, rand)
            members.append((Rs, Ss, Ts, Us, M, perm, k_i, rs_m))
        one = lambda i, flags: (cm.prove_ct if flags else cm.prove)(crs, *members[i], cm.Rand(42 + i))
        res["arm_prove"][str(ell)] = {}
        for k in ks:
            batch = lambda flags: cm.prove_batch(crs, [members[i] + (cm.Rand(42 + i),) for i in range(k)], flags)[0]
            res["arm_prove"][str(ell)][str(k)] = arms("prove ell = %d" % ell, k, batch, one, forms)
        single_ct = res["arm_prove"][str(ell)][str(min(ks))]["constant_time"]["loop_of_single_calls"]["ms_per_proof"]
        for k in ks:
            r = res["arm_prove"][str(ell)][str(k)]["constant_time"]
            r["batch_over_one_single"] = round(r["batch"]["ms"] / single_ct, 3)

    if not a.no_whisk:
        n = cm.WHISK_ELL
        crs = cm.CRS(n, cm.Rand(4))
        sets = []
        for i in range(max(ks)):
            r = cm.Rand(31 + i)
            trk, _ = cm.whisk_compute_trackers_batch(r.get_frs(n), r.get_frs(n), commitments=False)
            sets.append([trk[t].tobytes() for t in range(n)])
        one = lambda i, flags: (cm.whisk_generate_shuffle_proof_ct if flags else cm.whisk_generate_shuffle_proof)(crs, sets[i], cm.Rand(61 + i))
        for k in ks:
            def batch(flags, k=k):
                posts, proofs, status = cm.whisk_generate_shuffle_proof_batch(crs, sets[:k], [cm.Rand(61 + i) for i in range(k)], flags)
                return list(zip(posts, proofs))
            res["arm_whisk"][str(k)] = arms("whisk n = 128", k, batch, one, forms)

    notes = []
    for ell in ells:
        for k in ks:
            r = res["arm_prove"][str(ell)][str(k)]
            notes.append("ell %d k %d: constant-time batch = %.2f x one single curdle_prove_ct; default batch %.2f ms a proof against %.2f ms on "
                         "%d threads" % (ell, k, r["constant_time"]["batch_over_one_single"], r["default"]["batch"]["ms_per_proof"],
                                         r["default"]["single_calls_on_%d_threads" % THREADS]["ms_per_proof"], THREADS))
    res["note"] = "; ".join(notes)
    text = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
