"""The membership check for points in memory (curdle_g1_check_batch) beside its yardstick, the
batched decoder on as many records (curdle_g1_decompress_batch with the subgroup test: the same
subgroup chain plus a square root, 48 bytes fewer per point), and what the checked verifier costs
over the unchecked one at ell = 252.  One process, the calls of a size interleaved, medians.
    python tools/bench_affine_check.py [--out profiles/r08_affine_check.json]
Every point is a G1 point, so every lane runs the whole chain: the most a check can cost.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "go-curdleproofs_amd"))
import numpy as np
import torch
import curdlemsm as cm

WARMUP, REPS = 5, 20
SIZES = (1009, 1 << 14, 32768, 32769, 1 << 17, 1 << 20)
MONT_ONE = [0x760900000002fffd, 0xebf4000bc40c0002, 0x5f48985753c758ba, 0x77ce585370525745, 0x5c071a97a256ec6d,
            0x15f65ec3fa80e493]


def interleaved(calls, warmup=WARMUP, reps=REPS):
    """Median milliseconds of each call, the calls alternating inside every repetition; each ends in a device synchronise."""
    for _ in range(warmup):
        for f in calls.values():
            f()
    ts = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            t0 = time.perf_counter()
            f()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_affine_check.json"))
    args = ap.parse_args()
    if not cm.device_available():
        raise SystemExit("no HIP device: nothing is measured without one")
    cm.init(0)
    rand = cm.Rand(1)
    base = rand.get_g1_affines(256)
    enc = np.stack([np.frombuffer(cm.g1_compress(np.concatenate([p, np.array(MONT_ONE, dtype=np.uint64)])), dtype=np.uint8)
                    for p in base])
    out = {"device": torch.cuda.get_device_name(0), "warmup": WARMUP, "reps": REPS, "timing": "host clock around synchronous calls",
           "points": "G1 points (256 distinct, tiled): every point runs the whole subgroup chain", "sizes": {}}
    for n in SIZES:
        idx = np.arange(n) % 256
        pts = np.ascontiguousarray(base[idx])
        blob = enc[idx].tobytes()
        d_pts = torch.from_numpy(pts.view(np.int64)).to("cuda:0")
        torch.cuda.synchronize()
        assert not cm.g1_check_batch(pts, True).any() and not cm.g1_check_batch_device(d_pts.data_ptr(), n, True).any()
        assert not cm.g1_decompress_batch(blob, True)[1].any()
        r = interleaved({"check_host": lambda: cm.g1_check_batch(pts, True),
                         "check_device": lambda: cm.g1_check_batch_device(d_pts.data_ptr(), n, True),
                         "check_host_no_subgroup": lambda: cm.g1_check_batch(pts, False),
                         "decompress_subgroup": lambda: cm.g1_decompress_batch(blob, True)})
        r["check_host_over_decompress"] = r["check_host"]["median_ms"] / r["decompress_subgroup"]["median_ms"]
        r["check_device_over_decompress"] = r["check_device"]["median_ms"] / r["decompress_subgroup"]["median_ms"]
        out["sizes"][str(n)] = r
        print("n=%d: check host %.3f ms, device %.3f ms, without the subgroup test %.3f ms; decoder %.3f ms (check / decoder %.3f, %.3f)"
              % (n, r["check_host"]["median_ms"], r["check_device"]["median_ms"], r["check_host_no_subgroup"]["median_ms"],
                 r["decompress_subgroup"]["median_ms"], r["check_host_over_decompress"], r["check_device_over_decompress"]), flush=True)
        del d_pts

    # the verifier, ell = 252, on a decoded proof
    ell = 252
    rand = cm.Rand(0)
    crs = cm.CRS(ell, rand)
    perm = cm.Rand(42).generate_permutation(ell)
    k = rand.get_fr()
    Rs, Ss = rand.get_g1_affines(ell), rand.get_g1_affines(ell)
    Ts, Us, M, rs_m = cm.shuffle_permute_commit(crs, Rs, Ss, perm, k, rand)
    proof = cm.Proof(cm.prove(crs, Rs, Ss, Ts, Us, M, perm, k, rs_m, cm.Rand(42)))
    inst = np.concatenate([Rs, Ss, Ts, Us])
    seeds = iter(range(1000, 100000))

    def plain():
        assert cm.verify_proof(crs, proof, Rs, Ss, Ts, Us, M, cm.Rand(next(seeds)))

    def checked():
        assert cm.verify_proof_checked(crs, proof, Rs, Ss, Ts, Us, M, cm.Rand(next(seeds)))

    v = interleaved({"verify_proof": plain, "verify_proof_checked": checked,
                     "check_alone_n1008": lambda: cm.g1_check_batch(inst, True)}, warmup=10, reps=60)
    v["checked_minus_unchecked_ms"] = v["verify_proof_checked"]["median_ms"] - v["verify_proof"]["median_ms"]
    v["overlap_holds"] = v["checked_minus_unchecked_ms"] <= v["check_alone_n1008"]["median_ms"]
    v["check_paths"] = cm.stat_check_paths()
    out["verify_ell252"] = v
    print("ell=252: verify_proof %.3f ms, verify_proof_checked %.3f ms (+%.3f), the check alone at n = 1,008 %.3f ms"
          % (v["verify_proof"]["median_ms"], v["verify_proof_checked"]["median_ms"], v["checked_minus_unchecked_ms"],
             v["check_alone_n1008"]["median_ms"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
