"""What checking a batch's points costs: k = 1,024 proofs (eight distinct proofs and instances, repeated, as
bench.py's batch leg), 16 host threads, for ell = 124 and ell = 252, in one run:
  (A) curdle_verify_batch
  (B) the recipe curdle_verify_batch's caller had before: ONE curdle_g1_check_batch over all k * 4 ell instance points
      (already gathered into one array: the gathering is not timed) and k host subgroup tests of M
      (curdle_host_in_subgroup; no inversion and no curve equation -- the honest Ms have Z = 1), spread over the same
      --threads host threads the batch gets and run beside the GPU's check, then (A).  (B1) is the same with the k tests of M on ONE thread, beside it
      for comparison only: the aim is judged against (B)
  (C) curdle_verify_batch_checked
  (C16) the same with a point of another curve planted in 16 of the 1,024 members
Medians of the timed repetitions after warm-up; (A) also with its spread.  Then curdle_g1_check_jac_batch against
curdle_g1_check_batch on as many points at n = 1,024, 32,768, 32,769 and 2^20.  One JSON line.
    python tools/bench_batch_checked.py [--reps 7] [--warmup 2] [--pkg DIR] [--label NAME] [--only-a]
--pkg: import curdlemsm from another tree's go-curdleproofs_amd (the parent's (A) on the same machine); --only-a: (A) alone,
which is all a build without the checked batch can run.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--proofs", type=int, default=1024)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--ells", default="124,252")
ap.add_argument("--pkg", default=None)
ap.add_argument("--label", default="this")
ap.add_argument("--only-a", action="store_true")
args = ap.parse_args()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, args.pkg or os.path.join(ROOT, "go-curdleproofs_amd"))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
import numpy as np  # noqa: E402
import curdlemsm as cm  # noqa: E402

cm.init(0)
k = args.proofs
ONE = np.array([0x760900000002fffd, 0xebf4000bc40c0002, 0x5f48985753c758ba, 0x77ce585370525745, 0x5c071a97a256ec6d,
                0x15f65ec3fa80e493], dtype=np.uint64)
lib = C.CDLL(cm.LIB_PATH)
lib.curdle_host_in_subgroup.argtypes = [C.c_void_p]
pool = ThreadPoolExecutor(max_workers=args.threads)
seed = [100]


def timed(fn, reps=None):
    for _ in range(args.warmup):
        fn()
    ms = []
    for _ in range(reps or args.reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": round(statistics.median(ms), 2), "ms_min": round(min(ms), 2), "ms_max": round(max(ms), 2),
            "ms": [round(x, 2) for x in ms]}


def next_rand():
    seed[0] += 1
    return cm.Rand(seed[0] * 1000)


out = {"label": args.label, "proofs": k, "threads": args.threads, "reps": args.reps, "warmup": args.warmup,
       "GPU_MAX_HW_QUEUES": os.environ.get("GPU_MAX_HW_QUEUES"), "CURDLE_BATCH_CHECKERS": os.environ.get("CURDLE_BATCH_CHECKERS"),
       "lib": os.path.relpath(cm.LIB_PATH, ROOT), "ell": {}}
for ell in [int(x) for x in args.ells.split(",")]:
    rand = cm.Rand(0)
    crs = cm.CRS(ell, rand)
    distinct = []
    for j in range(8):
        pj = cm.Rand(50 + j).generate_permutation(ell)
        kj = rand.get_fr()
        Rj, Sj = rand.get_g1_affines(ell), rand.get_g1_affines(ell)
        Tj, Uj, Mj, rsj = cm.shuffle_permute_commit(crs, Rj, Sj, pj, kj, rand)
        distinct.append((cm.prove(crs, Rj, Sj, Tj, Uj, Mj, pj, kj, rsj, cm.Rand(60 + j)), Rj, Sj, Tj, Uj, Mj))
    cols = [[distinct[i % 8][c] for i in range(k)] for c in range(6)]
    batch = cm.PreparedVerifyBatch(*cols)
    honest = [True] * k

    def run_a():
        assert batch.run(crs, next_rand(), nthreads=args.threads) == honest

    res = {"A_verify_batch": timed(run_a)}
    res["A_spread_ms"] = round(res["A_verify_batch"]["ms_max"] - res["A_verify_batch"]["ms_min"], 2)
    if not args.only_a:
        every = np.ascontiguousarray(np.concatenate([np.asarray(cols[c][i]) for i in range(k) for c in (1, 2, 3, 4)]))
        xyzz = [np.ascontiguousarray(np.concatenate([np.asarray(m)[:12], ONE, ONE])) for m in cols[5]]
        assert all((np.asarray(m)[12:] == ONE).all() for m in cols[5])

        def test_ms(part):
            return all(lib.curdle_host_in_subgroup(m.ctypes.data) == 1 for m in part)   # ctypes drops the GIL in the call

        parts = [xyzz[t::args.threads] for t in range(args.threads)]

        def check_first(threaded=True):
            futures = [pool.submit(test_ms, part) for part in parts] if threaded else []   # beside the GPU's check
            st = cm.g1_check_batch(every, True)
            assert not st.any()
            assert all(f.result() for f in futures) if threaded else test_ms(xyzz)

        def run_b():
            check_first()
            run_a()

        def run_b1():
            check_first(False)
            run_a()

        def run_c():
            oks, faults = batch.run_checked(crs, next_rand(), nthreads=args.threads)
            assert oks == honest and not faults["code"].any()

        res["B_check_then_verify_batch"] = timed(run_b)
        res["B_check_alone"] = timed(check_first)
        res["B1_check_on_one_thread_then_verify_batch"] = timed(run_b1)
        res["B1_check_alone"] = timed(lambda: check_first(False))
        res["C_verify_batch_checked"] = timed(run_c)
        # 16 members with a point of another curve (y^2 = x^3 + 1: (0, 1)) in Us, 64 apart
        bad = {64 * g + 21 for g in range(k // 64)}
        other = np.concatenate([np.zeros(6, dtype=np.uint64), ONE])
        cols16 = [list(c) for c in cols]
        for i in bad:
            u = np.asarray(cols[4][i]).copy()
            u[i % ell] = other
            cols16[4][i] = u
        batch16 = cm.PreparedVerifyBatch(*cols16)
        s0 = cm.stat_batch_checked()

        def run_c16():
            oks, faults = batch16.run_checked(crs, next_rand(), nthreads=args.threads)
            assert oks == [i not in bad for i in range(k)]
            assert {i for i in range(k) if faults["code"][i] > 1} == bad and all(faults["code"][i] == 3 for i in bad)

        res["C16_verify_batch_checked_16_bad"] = timed(run_c16)
        s1 = cm.stat_batch_checked()
        res["C16_stat_batch_checked_delta"] = {key: int(s1[key] - s0[key]) for key in s1}
        a, b, c = (res[n]["ms_median"] for n in ("A_verify_batch", "B_check_then_verify_batch", "C_verify_batch_checked"))
        res["C_minus_B_ms"] = round(c - b, 2)
        res["C_over_A"] = round(c / a, 3)
        res["aim_C_below_B_by_more_than_A_spread"] = bool(b - c > res["A_spread_ms"])
    out["ell"][str(ell)] = res

if not args.only_a:
    rand = cm.Rand(1)
    base = rand.get_g1_affines(1024)
    out["check_kernels"] = {}
    for n in (1024, 32768, 32769, 1 << 20):
        aff = np.ascontiguousarray(np.tile(base, ((n + 1023) // 1024, 1))[:n])
        jac = np.ascontiguousarray(np.concatenate([aff, np.tile(ONE, (n, 1))], axis=1))

        def run_aff():
            assert not cm.g1_check_batch(aff, True).any()

        def run_jac():
            assert not cm.g1_check_jac_batch(jac, True).any()

        ta, tj = timed(run_aff, 5), timed(run_jac, 5)
        out["check_kernels"][str(n)] = {"affine_ms": ta["ms_median"], "jac_ms": tj["ms_median"],
                                        "jac_over_affine": round(tj["ms_median"] / ta["ms_median"], 3)}
print(json.dumps(out))
