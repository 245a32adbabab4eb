#!/usr/bin/env python3
"""Search points whose constant-time exit takes the SUBTRACTING arm of the masked canonical step (g1_exit_ct.h) inside
the shipped kernels, and write them to tests/golden/ct_exit_edges.json.  CPU only.

With a scalar k in {1, 2, 3} the walk of g1_walk_ct.h is deterministic in the words of the point: k = 1 ends on the
`first` arm, the accumulator is (x2, y2, one, one) exactly; k = 2 adds one doubling, k = 3 one doubling and one kept
sum.

How rare the arm is.  A Montgomery product t = a b / 2^392 is tau or tau + p (tau the canonical residue) and it is
tau + p exactly when tau 2^392 < a b.  The exit product of a coordinate is t = ix kToExt / 2^392 with tau the
coordinate's gnark value and ix the operand affine_words_ct hands over, itself a product below 2p.  When ix is its own
canonical residue it equals 2^8 tau mod p, and for small tau the condition reads 2^392 < 2^8 kToExt, which is false:
the arm needs ix in [p, 2p) -- about 1.4e-3 of the products whose first factor is an X3 or Y3 of up to 10p, 1e-4 for
k = 1 -- AND tau below ix kToExt / 2^392, about p / 1000.  That is of the order 1e-6 per coordinate, not the 3e-4 of
inputs uniform below 2p, so 2^15 points find nothing (measured: 98,304 pairs, 130 integer candidates, 0 hits) and the
default here is 2^21.  "Both coordinates" is of the order 1e-12 and is not expected.

The search decides tau <= 2p kToExt / 2^392 on plain integers for every point (k j) G, and the limb-exact model of
tests/g1_ct_model.py (the walk, the inversion chain, the products) then decides the candidates exactly.

k_fbase_mul_ct is different: it hands the canonical step the accumulator's X (an x3_fused output below 10p) and Y
(below 2p) themselves, through kToExtX16 and kToExtY64, not a product's result, so the estimate for uniform inputs
holds: about 2e-4 a lane for X and 2e-5 for Y.  `--fbase-lanes` scalars (uniform below r, a fixed seed) are walked
against the generator's table by the model of its 64-window walk (g1_ct_model.fbase_walk_ct; the table's words are
d28::from_gnark_iso of the multiples, no product), and the scalars whose X or Y exit subtracts are kept.

    python tools/find_ct_exit_edges.py [--points 2097152] [--fbase-lanes 131072] [--keep 4] [--only points|fbase]
"""
import argparse
import multiprocessing
import random
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "oracle", "py"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import bls12381_ref as oracle  # noqa: E402
import fp28_model as m  # noqa: E402
import g1_ct_model as g  # noqa: E402

P = m.P
KS = (1, 2, 3)


FBASE_SEED, FBASE_CHUNK = 2032, 1 << 12


def fbase_scalars(n):
    rnd = random.Random(FBASE_SEED)
    return [rnd.randrange(oracle.R) for _ in range(n)]


def _fbase_chunk(ks):
    tab = g.fbase_window_table(oracle.add, (oracle.GX, oracle.GY))
    acc, started = g.fbase_walk_ct(g.scalar_words(ks), tab)
    sx, sy = g.exit_subtracts(acc[0], "kToExtX16"), g.exit_subtracts(acc[1], "kToExtY64")
    szz = g.exit_subtracts(acc[2]) | g.exit_subtracts(acc[3])
    return [(k, bool(a), bool(b), bool(c)) for k, a, b, c in zip(ks, sx, sy, szz) if a or b or c]


def search_fbase(lanes, keep):
    ks = fbase_scalars(lanes)
    chunks = [ks[i:i + FBASE_CHUNK] for i in range(0, lanes, FBASE_CHUNK)]
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        hits = [h for part in pool.map(_fbase_chunk, chunks) for h in part]
    kinds = {"x": [h for h in hits if h[1] and not h[2]], "y": [h for h in hits if h[2] and not h[1]],
             "both": [h for h in hits if h[1] and h[2]], "zz_or_zzz": [h for h in hits if h[3]]}
    entries = [{"k": hex(h[0]), "kind": kind} for kind in ("x", "y", "both", "zz_or_zzz") for h in kinds[kind][:keep]]
    return {"what": "scalars k (uniform below r, random.Random(%d)) whose k G through k_fbase_mul_ct takes t - p in the exit of X "
                    "(kToExtX16), of Y (kToExtY64), of both, or of ZZ / ZZZ (kToExt)" % FBASE_SEED,
            "searched": lanes, "found": {kind: len(v) for kind, v in kinds.items()}, "entries": entries}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1 << 21)
    ap.add_argument("--keep", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ct_exit_edges.json"))
    ap.add_argument("--fbase-lanes", type=int, default=1 << 17)
    ap.add_argument("--only", choices=["points", "fbase"], default=None)
    a = ap.parse_args()
    if a.only == "fbase":                              # keep the point search of the file as it is
        doc = json.load(open(a.out))
        doc["fbase"] = search_fbase(a.fbase_lanes, a.keep)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        print(json.dumps({k: doc["fbase"][k] for k in ("searched", "found")}))
        return
    G = (oracle.GX, oracle.GY)
    bound = (2 * P * m.value1(m._T["kToExt"])) >> 392
    r384 = (1 << 384) % P
    steps = {k: oracle.scalar_mul(k, G) for k in KS}
    cur = dict(steps)                                   # cur[k] = (k j) G, j = 1, 2, ...
    cand = {k: [] for k in KS}
    for j in range(1, a.points + 1):
        for k in KS:
            x, y = cur[k]
            if x * r384 % P <= bound or y * r384 % P <= bound:
                cand[k].append((j, cur[1], cur[k]))
        for k in KS:
            cur[k] = oracle.add(cur[k], steps[k])
    found = {"x": [], "y": [], "both": []}
    candidates = sum(len(v) for v in cand.values())
    for k in KS:
        for lo in range(0, len(cand[k]), 4096):
            chunk = cand[k][lo:lo + 4096]
            gx, gy, acc = g.mul_ct_exit(k, [pt for _, pt, _ in chunk])
            assert m.affine(acc) == [res for _, _, res in chunk]
            for (j, _, _), sx, sy in zip(chunk, gx, gy):
                kind = "both" if sx and sy else ("x" if sx else ("y" if sy else None))
                if kind:
                    found[kind].append({"k": k, "j": j, "kind": kind})
    entries = []
    for kind in ("x", "y", "both"):
        for k in KS:                                   # a few of each kind, spread over the scalars
            entries += [e for e in found[kind] if e["k"] == k][: a.keep]
    doc = {"what": "points j G whose constant-time exit with scalar k takes t - p in the canonical step of x, of y, or of both "
                   "(tools/find_ct_exit_edges.py)",
           "searched": {"points_j": a.points, "scalars_k": list(KS), "pairs": a.points * len(KS), "integer_candidates": candidates},
           "found": {kind: len(v) for kind, v in found.items()},
           "entries": entries}
    if a.only == "points" and os.path.exists(a.out):
        old = json.load(open(a.out))
        if "fbase" in old:
            doc["fbase"] = old["fbase"]
    else:
        doc["fbase"] = search_fbase(a.fbase_lanes, a.keep)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({k: doc[k] for k in ("searched", "found")}), len(entries), "entries written")


if __name__ == "__main__":
    main()
