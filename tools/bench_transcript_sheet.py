"""The sheet kernel of the batched Merlin transcripts (knob TRANSCRIPT_SHEET) against the lane kernel, in four parts,
each a process of its own so that a caller can give each its own time limit and stop at the first that fails:

    cd <repository> && mkdir -p bench_outputs/sheet && P=bench_outputs/sheet && T=tools/bench_transcript_sheet.py && \
    timeout -k 10 300 python $T --part chain   --out $P/chain.json && \
    timeout -k 10 420 python $T --part prelude --out $P/prelude.json && \
    timeout -k 10 300 python $T --part tracker --out $P/tracker.json && \
    timeout -k 10 300 python $T --part whisk --cpus 16 --out $P/whisk16.json && \
    timeout -k 10 300 python $T --part whisk --cpus 4  --out $P/whisk4.json && \
    python $T --merge $P/chain.json $P/prelude.json $P/tracker.json $P/whisk16.json $P/whisk4.json \
        --out profiles/r20_transcript_sheet.json

Every figure is a median of 7 repetitions after 2 warm-ups, recorded with the repetitions' min, max and spread
(max - min).  The reference of every comparison is the untouched lane kernel (knob 0) in the same process.

  chain    (A) curdle_keccak_permute_batch, 512 dependent permutations, the kernel's time by HIP events: form 0 (a state
           per lane, one state per wave) against form 1 (a state spread over lanes, two per wave) at n = 1 .. 65,536:
           us per dependent permutation on a lone wave and on a full chip.
  prelude  (A) curdle_transcript_batch over the verifier's prelude at ell = 124 and 252, knob 0 against knob 1: kernel
           time and wall time per k; the host twin on 1 thread (to k = 1,024) and on 16 (to k = 8,192) beside it.  A k
           whose rows exceed CURDLE_TRANSCRIPT_MAX_TOTAL is recorded as refused.  The two knobs' outputs are compared.
  tracker  (B) the tracker batch with CURDLE_TRACKER_HASH_DEVICE and the combined form, knob 0 against knob 1, wall.
  whisk    (C) 1,024 Whisk shuffle proofs with GPU_PRELUDE off, on with knob 0, on with knob 1, the process confined
           to --cpus CPUs before the library loads; wall ms and time.process_time().

--merge applies the rule of choose_transcript_kernel (csrc/transcript_api.hip) to the ell = 124 wall times: the sheet
kernel up to the largest measured k at which its wall time is below the lane kernel's by more than the larger of the
two spreads; no such k at 64 or above means "lane kernel"."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM, REPS = 2, 7
CHAIN_REPS = 512
CHAIN_N = (1, 64, 1024, 8192, 65536)
PRELUDE_K = (1, 64, 256, 1024, 4096, 8192, 65536)
TRACKER_K = (64, 1024, 8192)
HOST_1_MAX, HOST_16_MAX = 1024, 8192


def stats(xs, digits=3):
    med = statistics.median(xs)
    return {"median": round(med, digits), "min": round(min(xs), digits), "max": round(max(xs), digits),
            "spread": round(max(xs) - min(xs), digits)}


def timed(fn, extra=None):
    """fn() WARM + REPS times -> wall ms statistics (and those of extra(), read after every call)."""
    wall, ex = [], []
    for rep in range(WARM + REPS):
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        if rep >= WARM:
            wall.append((t1 - t0) * 1e3)
            if extra:
                ex.append(extra())
    return (stats(wall), stats(ex)) if extra else stats(wall)


def confine(cpus):
    for tid in os.listdir("/proc/self/task"):
        try:
            os.sched_setaffinity(int(tid), cpus)
        except OSError:
            pass


def load():
    sys.path[:0] = [os.path.join(ROOT, "go-curdleproofs_amd"), os.path.join(ROOT, "oracle", "py"), os.path.join(ROOT, "tools")]
    import numpy as np
    import curdlemsm as cm
    cm.init(0)
    return np, cm


def part_chain():
    np, cm = load()
    out = {"reps": CHAIN_REPS, "n": {}}
    for n in CHAIN_N:
        a = np.random.default_rng(n).integers(0, 1 << 64, size=(n, 25), dtype=np.uint64)
        row, res = {}, {}
        for form, name in ((0, "lane"), (1, "sheet")):
            ms = []
            for rep in range(WARM + REPS):
                res[name], t = cm.keccak_permute_batch(a, form, CHAIN_REPS, want_ms=True)
                if rep >= WARM:
                    ms.append(t)
            row[name + "_kernel_ms"] = stats(ms)
            row[name + "_us_per_permutation"] = round(statistics.median(ms) * 1e3 / CHAIN_REPS, 3)
        assert (res["lane"] == res["sheet"]).all()
        row["lane_over_sheet"] = round(row["lane_kernel_ms"]["median"] / row["sheet_kernel_ms"]["median"], 3)
        out["n"][str(n)] = row
    return {"chain": out}


def part_prelude():
    np, cm = load()
    out = {}
    for ell in (124, 252):
        program = [(cm.TR_APPEND, b"curdleproofs_step1", 4 * ell + 1, 48), (cm.TR_CHALLENGES, b"curdleproofs_vec_a", ell, 0)]
        width = 48 * (4 * ell + 1)
        for k in PRELUDE_K:
            row = out.setdefault("ell%d" % ell, {})
            if k * (width + 16) > (1 << 30):
                row[str(k)] = {"refused": "k x (bytes per member + 16) exceeds CURDLE_TRANSCRIPT_MAX_TOTAL"}
                continue
            data = np.random.default_rng(ell + k).integers(0, 256, size=(k, width), dtype=np.uint8)
            r, got = {}, {}
            for knob, name in ((0, "lane"), (1, "sheet")):
                with cm.knobs(TRANSCRIPT_SHEET=knob):
                    got[name] = cm.transcript_batch(program, data, label=b"curdleproofs")
                    r[name + "_wall_ms"], r[name + "_kernel_ms"] = timed(
                        lambda: cm.transcript_batch(program, data, label=b"curdleproofs"), cm.transcript_last_kernel_ms)
            assert all((a == b).all() for a, b in zip(got["lane"], got["sheet"]))
            for threads, limit in ((1, HOST_1_MAX), (16, HOST_16_MAX)):
                if k <= limit:
                    r["host_%d_threads_wall_ms" % threads] = timed(
                        lambda: cm.transcript_batch(program, data, label=b"curdleproofs", host=True, nthreads=threads))
            row[str(k)] = r
    return {"prelude": out}


def part_tracker():
    np, cm = load()
    import tempfile
    import bench_tracker_hash as bth
    vp = C.c_void_p
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "members.npz")
        bth.make_members(path)
        z = {n: v.copy() for n, v in np.load(path).items()}
    ex = cm._lib.curdle_whisk_is_valid_tracker_proof_batch_ex
    ex.argtypes, ex.restype = [vp, vp, vp, C.c_size_t, C.c_uint, vp], C.c_int
    comb = cm._lib.curdle_whisk_is_valid_tracker_proof_batch_combined
    comb.argtypes, comb.restype = [vp, vp, vp, C.c_size_t, vp, vp], C.c_int
    seed = np.arange(32, dtype=np.uint8)
    out = {}
    for k in TRACKER_K:
        t, kc, p = z["trackers"][:96 * k].copy(), z["k_comms"][:48 * k].copy(), z["proofs"][:128 * k].copy()
        res = np.zeros(k, dtype=np.int32)
        forms = {"hash_device": lambda: ex(t.ctypes.data, kc.ctypes.data, p.ctypes.data, k, 2, res.ctypes.data),
                 "combined": lambda: comb(t.ctypes.data, kc.ctypes.data, p.ctypes.data, k, seed.ctypes.data, res.ctypes.data)}
        row = out[str(k)] = {}
        for name, f in forms.items():
            seen = {}
            for knob, kname in ((0, "lane"), (1, "sheet")):
                with cm.knobs(TRANSCRIPT_SHEET=knob):
                    def call():
                        if f() != 0:
                            raise SystemExit("%s k=%d: the call failed" % (name, k))
                    row["%s_%s_wall_ms" % (name, kname)] = timed(call)
                    seen[kname] = res.copy()
            assert (seen["lane"] == seen["sheet"]).all()
    return {"tracker": out}


def part_whisk(cpus):
    want = set(sorted(os.sched_getaffinity(0))[:cpus])
    confine(want)
    np, cm = load()
    confine(want)  # loading the HIP runtime has been seen to widen the main thread's set
    if os.sched_getaffinity(0) != want or len(want) != cpus:
        raise SystemExit("the CPU set did not hold")
    ONE = np.array([0x760900000002fffd, 0xebf4000bc40c0002, 0x5f48985753c758ba, 0x77ce585370525745, 0x5c071a97a256ec6d,
                    0x15f65ec3fa80e493], dtype=np.uint64)
    compress = lambda aff: cm.g1_compress(np.concatenate([aff, ONE]))  # noqa: E731
    crs = cm.CRS(cm.WHISK_ELL, cm.Rand(0))
    sets = []
    for j in range(8):
        r = cm.Rand(10 + j)
        pts = r.get_g1_affines(2 * cm.WHISK_ELL)
        pre = [compress(pts[2 * i]) + compress(pts[2 * i + 1]) for i in range(cm.WHISK_ELL)]
        post, proof = cm.whisk_generate_shuffle_proof(crs, pre, r)
        sets.append((pre, post, proof))
    k = 1024
    batch = cm.PreparedWhiskBatch([sets[i % 8][0] for i in range(k)], [sets[i % 8][1] for i in range(k)], [sets[i % 8][2] for i in range(k)])
    seed = [100]
    cpu = []

    def run():
        seed[0] += 1
        c0 = time.process_time()
        ok = batch.run(crs, cm.Rand(seed[0] * 1000), nthreads=cpus)
        cpu.append((time.process_time() - c0) * 1e3)
        assert all(ok)

    res = {"proofs": k, "cpus": cpus}
    for name, kn in (("prelude_off", {"GPU_PRELUDE": 0}), ("prelude_on_lane", {"GPU_PRELUDE": 1, "TRANSCRIPT_SHEET": 0}),
                     ("prelude_on_sheet", {"GPU_PRELUDE": 1, "TRANSCRIPT_SHEET": 1})):
        del cpu[:]
        p0 = cm.stat_transcript_paths()
        with cm.knobs(**kn):
            wall = timed(run)
        p1 = cm.stat_transcript_paths()
        res[name] = {"wall_ms": wall, "process_time_ms": stats(cpu[WARM:]),
                     "members_on_lane_kernel": p1["lane"] - p0["lane"], "members_on_sheet_kernel": p1["sheet"] - p0["sheet"]}
    return {"whisk_%d_cpus" % cpus: res}


def rule(prelude):
    """The chooser's threshold from the ell = 124 wall times (see the module's docstring)."""
    best, table = 0, {}
    for k, r in sorted(((int(k), r) for k, r in prelude.items() if "refused" not in r)):
        lane, sheet = r["lane_wall_ms"], r["sheet_wall_ms"]
        ahead = lane["median"] - sheet["median"] > max(lane["spread"], sheet["spread"])
        table[str(k)] = {"lane_wall_ms": lane["median"], "sheet_wall_ms": sheet["median"],
                         "larger_spread_ms": max(lane["spread"], sheet["spread"]), "sheet_ahead": bool(ahead)}
        if ahead:
            best = k
    ahead_at_64 = table.get("64", {}).get("sheet_ahead", False)
    return {"sheet_up_to_k": best if ahead_at_64 else 0, "sheet_ahead_at_64": bool(ahead_at_64), "by_k": table}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("chain", "prelude", "tracker", "whisk"))
    ap.add_argument("--cpus", type=int, default=16)
    ap.add_argument("--merge", nargs="+")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    if a.merge:
        res = {"note": "tools/bench_transcript_sheet.py: medians of %d after %d warm-ups; spread = max - min of the repetitions; "
                       "lane = knob TRANSCRIPT_SHEET=0 (the reference), sheet = TRANSCRIPT_SHEET=1" % (REPS, WARM)}
        for path in a.merge:
            res.update(json.load(open(path)))
        if "prelude" in res:
            res["rule"] = rule(res["prelude"]["ell124"])
    else:
        os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
        res = {"chain": part_chain, "prelude": part_prelude, "tracker": part_tracker, "whisk": lambda: part_whisk(a.cpus)}[a.part]()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
