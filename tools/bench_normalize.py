"""The shared-inversion normalisation (k_g1_normalize) against what there was before it, in ONE process on one machine.

    python tools/bench_normalize.py [--out profiles/r15_normalize.json]

(a) curdle_g1_normalize_batch_device against curdle_g1_compress_batch_device -- the only device-side normalisation of
    the parent -- on the SAME resident Jacobian points, n = 64, 3,072, 24,576, 196,608 and 2^20: each call between two
    events on the caller's stream, the two calls alternating inside every repetition.  Beside the library's rule
    (one point per lane up to 65,536 points, eight beyond) both builds are timed at every size (knob
    NORMALIZE_LANE_POINTS), and the XYZZ form under the rule.
(b) curdle_g1_scalar_mul_batch (host arrays in, host arrays out, as it is) against upload + curdle_g1_scalar_mul_batch_device
    + download of the 96-byte records, n = 512, 65,536 and 2^20, both as wall time around work that ends in a
    synchronise, from the same pageable arrays; and the resident call alone between two events.

2 warm-ups, then 7 repetitions; recorded are the median, the spread (max - min) / median, and the ratios.  Before
anything is timed the outputs are checked: the two builds agree on every record and with the oracle, and the
resident scalar multiplications equal the host call's.  The last line printed is the JSON that --out also receives."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES_A = (64, 3072, 24576, 196608, 1 << 20)
SIZES_B = (512, 65536, 1 << 20)
WARM, REPS = 2, 7


def stats(ms):
    med = statistics.median(ms)
    return {"ms": round(med, 4), "spread": round((max(ms) - min(ms)) / med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes-a", default=",".join(str(s) for s in SIZES_A))
    ap.add_argument("--sizes-b", default=",".join(str(s) for s in SIZES_B))
    a = ap.parse_args()
    sizes_a = [int(s) for s in a.sizes_a.split(",") if s]
    sizes_b = [int(s) for s in a.sizes_b.split(",") if s]
    sys.path[:0] = [os.path.join(ROOT, "go-curdleproofs_amd"), os.path.join(ROOT, "oracle", "py")]
    import numpy as np
    import torch
    import curdlemsm as cm
    import bls12381_ref as o
    import coracle as co

    if not cm.device_available():
        raise SystemExit("no HIP device: this benchmark measures the GPU path")
    cm.init(0)
    rng = np.random.default_rng(15)
    s = torch.cuda.Stream()
    res = {"tool": "bench_normalize", "warmups": WARM, "reps": REPS, "statistic": "median of the repetitions",
           "timing": "torch (HIP) events on the caller's stream around each call; (b) host/composed: wall time around work that ends in a synchronise",
           "normalize_vs_compress": {}, "scalar_mul_batch": {}}

    def events(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            e0.record()
            call()
            e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    # ---- (a) -------------------------------------------------------------------------------------------------------
    base = [o.scalar_mul(7 + j, o.G1) for j in range(8)]
    for n in sizes_a:
        # (x z^2, y z^3, z) with 8 distinct z per base point: real Jacobian representatives, so the outputs can be checked
        rows, aff = [], []
        for j, pt in enumerate(base):
            for t in range(8):
                z = int.from_bytes(rng.bytes(47), "big") + 2
                rows.append(o.fp_to_mont_limbs(pt[0] * z * z % o.P) + o.fp_to_mont_limbs(pt[1] * z * z * z % o.P) + o.fp_to_mont_limbs(z))
                aff.append(o.affine_to_mont_limbs(pt))
        which = rng.integers(len(rows), size=n)
        jac = np.array(rows, dtype=np.uint64)[which]
        want = np.array(aff, dtype=np.uint64)[which]
        d_jac = torch.from_numpy(jac.view(np.int64).copy()).to("cuda:0")
        d_aff = torch.zeros(n * 12, dtype=torch.int64, device="cuda:0")
        d_enc = torch.zeros(n * 48, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        out = res["normalize_vs_compress"][str(n)] = {}

        def norm(form=cm.G1_FORM_JAC, d_in=d_jac):
            cm.g1_normalize_batch_device(d_in.data_ptr(), form, n, d_aff.data_ptr(), stream=s.cuda_stream)

        def comp():
            cm.g1_compress_batch_device(d_jac.data_ptr(), n, d_enc.data_ptr(), stream=s.cuda_stream)

        got = {}
        for lp in (1, 8):
            with cm.knobs(NORMALIZE_LANE_POINTS=lp):
                events(norm)
                got[lp] = d_aff.cpu().numpy().view(np.uint64).reshape(n, 12).copy()
        if not (got[1] == got[8]).all() or not (got[1] == want).all():
            raise SystemExit("n=%d: a normalised record differs from the oracle" % n)
        out["lane_points_by_rule"] = 1 if n <= 65536 else 8

        t_norm, t_comp = [], []
        for rep in range(WARM + REPS):
            x, y = events(norm), events(comp)
            if rep >= WARM:
                t_norm.append(x)
                t_comp.append(y)
        out["normalize"], out["compress"] = stats(t_norm), stats(t_comp)
        out["normalize_over_compress"] = round(out["normalize"]["ms"] / out["compress"]["ms"], 4)
        for lp in (1, 8):
            with cm.knobs(NORMALIZE_LANE_POINTS=lp):
                out["normalize_lane_points_%d" % lp] = stats([events(norm) for rep in range(WARM + REPS)][WARM:])
        # the XYZZ form: ZZ = Z^2, ZZZ = Z^3 of the same representatives (X and Y as they are)
        P = o.P
        zs = [o.fp_from_mont_limbs(r[12:18]) for r in rows]
        xrows = np.array([r[:12] + o.fp_to_mont_limbs(z * z % P) + o.fp_to_mont_limbs(z * z * z % P) for r, z in zip(rows, zs)], dtype=np.uint64)
        d_xyzz = torch.from_numpy(xrows[which].view(np.int64).copy()).to("cuda:0")
        torch.cuda.synchronize()
        nx = lambda: norm(cm.G1_FORM_XYZZ, d_xyzz)
        events(nx)
        if not (d_aff.cpu().numpy().view(np.uint64).reshape(n, 12) == want).all():
            raise SystemExit("n=%d: a record normalised from XYZZ differs from the oracle" % n)
        out["normalize_xyzz"] = stats([events(nx) for rep in range(WARM + REPS)][WARM:])
        print("a n=%d %s" % (n, json.dumps(out)), file=sys.stderr, flush=True)

    # ---- (b) -------------------------------------------------------------------------------------------------------
    k, q = o.Rand(15).get_frs(2)
    for n in sizes_b:
        pts = co.points_walk(k, q, n)
        sc = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
        sc[:, 3] &= np.uint64((1 << 62) - 1)                       # Montgomery limbs below r, taken as they are
        out = res["scalar_mul_batch"][str(n)] = {}
        host_out = [None]

        def host():
            host_out[0] = cm.g1_scalar_mul_batch(pts, sc)

        dev_out = np.zeros((n, 12), dtype=np.uint64)
        t_out = torch.from_numpy(dev_out.view(np.int64))

        def composed():
            with torch.cuda.stream(s):
                d_p = torch.from_numpy(pts.view(np.int64)).to("cuda:0", non_blocking=True)
                d_s = torch.from_numpy(sc.view(np.int64)).to("cuda:0", non_blocking=True)
                cm.g1_scalar_mul_batch_device(d_p.data_ptr(), d_s.data_ptr(), n, 0, n, d_p.data_ptr(), stream=s.cuda_stream)
                t_out.copy_(d_p.view(n, 12), non_blocking=True)
            s.synchronize()

        def wall(call):
            w0 = time.perf_counter()
            call()
            return (time.perf_counter() - w0) * 1e3

        host()
        composed()
        if not (host_out[0] == dev_out).all():
            raise SystemExit("n=%d: the resident scalar multiplications differ from the host call's" % n)
        t_host, t_dev = [], []
        for rep in range(WARM + REPS):
            x, y = wall(host), wall(composed)
            if rep >= WARM:
                t_host.append(x)
                t_dev.append(y)
        out["host_call"], out["upload_device_call_download"] = stats(t_host), stats(t_dev)
        out["composed_over_host_call"] = round(out["upload_device_call_download"]["ms"] / out["host_call"]["ms"], 4)
        d_p = torch.from_numpy(pts.view(np.int64)).to("cuda:0")
        d_s = torch.from_numpy(sc.view(np.int64)).to("cuda:0")
        d_o = torch.zeros(n * 12, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        resident = lambda: cm.g1_scalar_mul_batch_device(d_p.data_ptr(), d_s.data_ptr(), n, 0, n, d_o.data_ptr(), stream=s.cuda_stream)
        out["resident_call"] = stats([events(resident) for rep in range(WARM + REPS)][WARM:])
        print("b n=%d %s" % (n, json.dumps(out)), file=sys.stderr, flush=True)

    res["stat_normalize"] = cm.stat_normalize()
    text = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
