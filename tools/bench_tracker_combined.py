"""The combined tracker batch (curdle_whisk_is_valid_tracker_proof_batch_combined, _device) against the per-member form
it falls back to, in one process on one GPU.

    python tools/bench_tracker_combined.py [--out profiles/r19_tracker_combined.json]

The comparison arm is curdle_whisk_is_valid_tracker_proof_batch_ex(..., CURDLE_TRACKER_HASH_DEVICE) for host arrays and
curdle_whisk_is_valid_tracker_proof_batch_device for resident ones: code the combined form did not change, so it stands
for the parent commit in the same run.  Per k (64, 1,024, 8,192, 65,536 members, from 12 honest proofs) and form (host
arrays, resident arrays): an all-honest batch and the same batch with exactly ONE rejected member (S + 1, in the
middle), 2 warm-ups and then 7 repetitions each; recorded are the median wall time of a call, its spread
(max - min) / median, and the fastest and slowest repetition.  The calls go through ctypes on prepared arrays: no Python
work is inside a timed call.  Every timed result is compared with the comparison arm's, an honest combined call must
have been settled by its sums (curdle_stat_tracker_combined) and a one-bad call must have fallen back.

k_tracker_combine alone is timed by HIP events around the kernel inside curdle_whisk_tracker_combined_scalars
(curdle_tracker_combined_last_kernel_ms), median of 7 after 2 warm-ups.

`honest_ahead_from_k`, per form: the smallest measured k at which the honest combined call is faster than the
comparison arm by more than the spread of the repetitions there (the larger of the two arms' spreads) -- and at every
larger measured k too; null if there is none.  No routing rule follows from it.  The last line printed is the JSON that
--out also receives."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (64, 1024, 8192, 65536)
WARM, REPS = 2, 7


def make_members():
    """12 honest members and member 0 with S + 1."""
    import numpy as np
    import curdlemsm as cm
    import bls12381_ref as o
    rand = o.Rand(1)
    hon = []
    for j in range(12):
        k, r = rand.get_fr(), rand.get_fr()
        rG = o.scalar_mul(r, o.G1)
        tracker = o.compress(rG) + o.compress(o.scalar_mul(k, rG))
        proof = cm.whisk_generate_tracker_proof(tracker, np.array(o.fr_to_mont_limbs(k), dtype=np.uint64), cm.Rand(j))
        hon.append((tracker, o.compress(o.scalar_mul(k, o.G1)), proof))
    t, kc, p = hon[0]
    s = int.from_bytes(p[96:], "big")
    return hon, (t, kc, p[:96] + ((s + 1) % o.R).to_bytes(32, "big"))


def timed(call, out, k):
    wall = []
    for rep in range(WARM + REPS):
        out[:] = -99
        w0 = time.perf_counter()
        rc = call()
        w1 = time.perf_counter()
        if rc != 0:
            raise SystemExit("k=%d: rc %d" % (k, rc))
        if rep >= WARM:
            wall.append(w1 - w0)
    med = statistics.median(wall)
    return {"wall_ms": round(med * 1e3, 4), "spread": round((max(wall) - min(wall)) / med, 4),
            "wall_min_ms": round(min(wall) * 1e3, 4), "wall_max_ms": round(max(wall) * 1e3, 4), "members_per_s": round(k / med)}


def ahead_from(rows, form):
    def ahead(k):
        c, p = rows[str(k)][form]["honest"]["combined"], rows[str(k)][form]["honest"]["per_member"]
        return c["wall_ms"] < p["wall_ms"] * (1 - max(c["spread"], p["spread"]))
    return next((k for i, k in enumerate(SIZES) if all(ahead(j) for j in SIZES[i:])), None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path[:0] = [os.path.join(ROOT, "go-curdleproofs_amd"), os.path.join(ROOT, "oracle", "py")]
    import numpy as np
    import torch
    import curdlemsm as cm
    if not cm.device_available():
        raise SystemExit("this benchmark measures the GPU path")
    cm.init(0)
    lib, vp = cm._lib, C.c_void_p
    ex = lib.curdle_whisk_is_valid_tracker_proof_batch_ex
    dev = lib.curdle_whisk_is_valid_tracker_proof_batch_device
    comb = lib.curdle_whisk_is_valid_tracker_proof_batch_combined
    comb_dev = lib.curdle_whisk_is_valid_tracker_proof_batch_combined_device
    hon, bad = make_members()
    seed = np.frombuffer(os.urandom(32), dtype=np.uint8).copy()
    rows = {}
    for k in SIZES:
        row = rows[str(k)] = {"host": {}, "resident": {}}
        for batch in ("honest", "one_bad"):
            members = [hon[j % len(hon)] for j in range(k)]
            if batch == "one_bad":
                members[k // 2] = bad
            t, kc, p = (np.frombuffer(b"".join(c), dtype=np.uint8).copy() for c in zip(*members))
            d = [torch.from_numpy(x).to("cuda:0") for x in (t, kc, p)]
            torch.cuda.synchronize()
            out, want = np.zeros(k, dtype=np.int32), np.ones(k, dtype=np.int32)
            if batch == "one_bad":
                want[k // 2] = 0
            hp = (t.ctypes.data, kc.ctypes.data, p.ctypes.data)
            dp = tuple(x.data_ptr() for x in d)
            arms = {"host": {"per_member": lambda: ex(*hp, k, cm.TRACKER_HASH_DEVICE, out.ctypes.data),
                             "combined": lambda: comb(*hp, k, seed.ctypes.data, out.ctypes.data)},
                    "resident": {"per_member": lambda: dev(*dp, k, out.ctypes.data, None),
                                 "combined": lambda: comb_dev(*dp, k, seed.ctypes.data, out.ctypes.data, None)}}
            for form, pair in arms.items():
                cell = row[form][batch] = {}
                for arm, call in pair.items():
                    before = cm.stat_tracker_combined()
                    cell[arm] = timed(call, out, k)
                    if not (out == want).all():
                        raise SystemExit("%s %s %s k=%d: wrong results" % (form, batch, arm, k))
                    if arm == "combined":
                        after = cm.stat_tracker_combined()
                        passes = (WARM + REPS) * ((k + 65535) // 65536)
                        moved = (after["settled"] - before["settled"], after["fell_back"] - before["fell_back"])
                        if moved != ((passes, 0) if batch == "honest" else (0, passes)):
                            raise SystemExit("%s %s k=%d: settled / fell back %s" % (form, batch, k, moved))
        # the kernel alone
        members = [hon[j % len(hon)] for j in range(k)]
        kms = []
        for rep in range(WARM + REPS):
            cm.whisk_tracker_combined_scalars(*[list(c) for c in zip(*members)], seed.tobytes())
            if rep >= WARM:
                kms.append(cm.tracker_combined_last_kernel_ms())
        row["k_tracker_combine_ms"] = round(statistics.median(kms), 4)
        row["k_tracker_combine_spread"] = round((max(kms) - min(kms)) / statistics.median(kms), 4)
        print(k, json.dumps(row), file=sys.stderr, flush=True)
    res = {"tool": "bench_tracker_combined", "warmups": WARM, "reps": REPS, "statistic": "median of the repetitions",
           "reference": "arm 'per_member' (curdle_whisk_is_valid_tracker_proof_batch_ex with CURDLE_TRACKER_HASH_DEVICE / "
                        "_batch_device), same process", "sizes": rows,
           "honest_ahead_from_k": {form: ahead_from(rows, form) for form in ("host", "resident")}}
    text = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
