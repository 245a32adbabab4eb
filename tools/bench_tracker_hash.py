"""Where the tracker batch hashes its transcripts: the parent build's curdle_whisk_is_valid_tracker_proof_batch (host
hashing, the reference of every figure) against this build's CURDLE_TRACKER_HASH_HOST, CURDLE_TRACKER_HASH_DEVICE and
curdle_whisk_is_valid_tracker_proof_batch_device over resident arrays, in one run on one machine.

    python tools/bench_tracker_hash.py --parent-lib PATH/libcurdlemsm.so [--out profiles/r13_tracker_device_hash.json]

For every CPU set (1, 4 and 16 CPUs) the two builds run in turn, each in a fresh child process that confines itself
with os.sched_setaffinity BEFORE the library (and torch) is loaded, and again after the device is initialised, so
the library's thread pool sees that many cores; a child whose set did not hold fails.  Per k (64, 1,024, 8,192,
65,536 members: 12 honest proofs, one member in ten tampered) and form: 2 warm-ups, then 7 repetitions; recorded are
the median wall time of a call, the median of time.process_time() over a call (the CPU seconds the call burns, every
thread of the process), and the spread (max - min) / median of the repetitions.  The calls go through ctypes on
prepared arrays: no Python work is inside a timed call.  Every timed result is compared with the parent's.

This build's child also times the transcript kernel by HIP events -- NOT the launch the tracker path makes (that one
uses the slot's buffers on the second slot's stream, beside the square roots), but curdle_transcript_batch over the
same program and as many members of random bytes: the same kernel, tape and launch rule, alone on the GPU.  The field
is named for that: transcript_kernel_proxy_ms.

Two rules are applied to the 16-CPU runs.  `rule_as_issued_from_k`: the smallest measured k at
which device hashing is not slower than the parent's host hashing by more than the spread of the repetitions there
(the larger of the two forms' spreads).  `default_rule_from_k`, which the library's default follows (kDeviceHashFrom,
csrc/tracker_api.hip): the smallest measured k such that the same holds at k AND at every larger measured k -- a
threshold sends every batch above it to the device, so a size at which the device loses must lie below it.  The last
line printed is the JSON that --out also receives.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (64, 1024, 8192, 65536)
CPUS = (1, 4, 16)
WARM, REPS = 2, 7
LABEL = b"whisk_opening_proof"


def make_members(path):
    """12 honest members and 5 tampered ones -> npz of the three byte arrays of a 65,536-member batch."""
    sys.path[:0] = [os.path.join(ROOT, "go-curdleproofs_amd"), os.path.join(ROOT, "oracle", "py")]
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
    bad = [(t, kc, p[:96] + ((s + 1) % o.R).to_bytes(32, "big")), (t, kc, p[:96] + o.R.to_bytes(32, "big")),
           (hon[1][0], kc, p), (t, hon[1][1], p), (t, kc, hon[2][2][:48] + p[48:])]
    rng = np.random.default_rng(13)
    members = [bad[rng.integers(len(bad))] if rng.random() < 0.1 else hon[rng.integers(len(hon))] for _ in range(max(SIZES))]
    cols = [np.frombuffer(b"".join(c), dtype=np.uint8) for c in zip(*members)]
    np.savez(path, trackers=cols[0], k_comms=cols[1], proofs=cols[2])


def confine(cpus):
    """Every thread the process has so far onto `cpus`; threads started later inherit their creator's set."""
    for tid in os.listdir("/proc/self/task"):
        try:
            os.sched_setaffinity(int(tid), cpus)
        except OSError:
            pass  # a thread that ended meanwhile


def child(a):
    cpus = set(sorted(os.sched_getaffinity(0))[:a.cpus])
    confine(cpus)
    import numpy as np
    import torch
    lib = C.CDLL(a.lib)
    vp = C.c_void_p
    lib.curdle_init.argtypes = [C.c_int]
    plain = lib.curdle_whisk_is_valid_tracker_proof_batch
    plain.argtypes = [vp, vp, vp, C.c_size_t, vp]
    forms = {}
    if a.build == "parent":
        forms["host"] = lambda t, kc, p, k, out: plain(t, kc, p, k, out)
    else:
        ex = lib.curdle_whisk_is_valid_tracker_proof_batch_ex
        ex.argtypes = [vp, vp, vp, C.c_size_t, C.c_uint, vp]
        dev = lib.curdle_whisk_is_valid_tracker_proof_batch_device
        dev.argtypes = [vp, vp, vp, C.c_size_t, vp, vp]
        forms["host"] = lambda t, kc, p, k, out: ex(t, kc, p, k, 1, out)
        forms["device"] = lambda t, kc, p, k, out: ex(t, kc, p, k, 2, out)
        forms["resident"] = None
    if lib.curdle_init(0) != 0:
        raise SystemExit("curdle_init failed: this benchmark measures the GPU path")
    confine(cpus)  # again: loading torch or the HIP runtime has been seen to widen the main thread's set
    if os.sched_getaffinity(0) != cpus:
        raise SystemExit("the CPU set did not hold")
    z = np.load(a.members)
    want_all = np.load(a.want) if a.want and os.path.exists(a.want) else None
    res = {"build": a.build, "cpus": a.cpus, "cpus_seen": len(os.sched_getaffinity(0)), "sizes": {}}
    first_results = None
    for k in SIZES:
        t, kc, p = z["trackers"][:96 * k].copy(), z["k_comms"][:48 * k].copy(), z["proofs"][:128 * k].copy()
        d = [torch.from_numpy(x).to("cuda:0") for x in (t, kc, p)]
        torch.cuda.synchronize()
        out = np.zeros(k, dtype=np.int32)
        row = res["sizes"][str(k)] = {}
        for name in forms:
            if name == "resident":
                def call():
                    return dev(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), k, out.ctypes.data, None)
            else:
                def call(f=forms[name]):
                    return f(t.ctypes.data, kc.ctypes.data, p.ctypes.data, k, out.ctypes.data)
            wall, cpu = [], []
            for rep in range(WARM + REPS):
                out[:] = -99
                c0, w0 = time.process_time(), time.perf_counter()
                rc = call()
                w1, c1 = time.perf_counter(), time.process_time()
                if rc != 0:
                    raise SystemExit("%s %s k=%d: rc %d" % (a.build, name, k, rc))
                if rep >= WARM:
                    wall.append(w1 - w0)
                    cpu.append(c1 - c0)
            if k == max(SIZES) and first_results is None:
                first_results = out.copy()
            if want_all is not None and not (out == want_all[:k]).all():
                raise SystemExit("%s %s k=%d: results differ from the parent's" % (a.build, name, k))
            med = statistics.median(wall)
            row[name] = {"wall_ms": round(med * 1e3, 4), "cpu_ms": round(statistics.median(cpu) * 1e3, 4),
                         "spread": round((max(wall) - min(wall)) / med, 4), "wall_min_ms": round(min(wall) * 1e3, 4),
                         "wall_max_ms": round(max(wall) * 1e3, 4), "members_per_s": round(k / med)}
        if a.build != "parent":  # the transcript kernel alone
            class Step(C.Structure):
                _fields_ = [("op", C.c_uint32), ("count", C.c_uint32), ("len", C.c_uint32), ("label_len", C.c_uint32),
                            ("label", C.c_char * 32)]
            steps = (Step * 2)()
            for s, (op, label, count, ln) in zip(steps, ((1, b"tracker_opening_proof", 6, 48),
                                                         (2, b"tracker_opening_proof_challenge", 1, 0))):
                s.op, s.count, s.len, s.label_len, s.label = op, count, ln, len(label), label
            rows = np.random.default_rng(k).integers(0, 256, size=(k, 288), dtype=np.uint8)
            ch, status, ms = np.zeros((k, 32), np.uint8), np.zeros(k, np.uint8), C.c_double()
            tb = lib.curdle_transcript_batch
            tb.argtypes = [C.c_char_p, vp, vp, C.c_size_t, vp, C.c_size_t, C.c_size_t, vp, vp, vp]
            lib.curdle_transcript_last_kernel_ms.argtypes = [C.POINTER(C.c_double)]
            kms = []
            for rep in range(WARM + REPS):
                if tb(LABEL, None, steps, 2, rows.ctypes.data, 288, k, ch.ctypes.data, None, status.ctypes.data) != 0:
                    raise SystemExit("curdle_transcript_batch failed")
                lib.curdle_transcript_last_kernel_ms(C.byref(ms))
                if rep >= WARM:
                    kms.append(ms.value)
            row["transcript_kernel_proxy_ms"] = round(statistics.median(kms), 4)
            row["transcript_kernel_proxy_spread"] = round((max(kms) - min(kms)) / statistics.median(kms), 4)
    if a.build == "parent" and a.want and not os.path.exists(a.want):
        np.save(a.want, first_results)
    print("RESULT " + json.dumps(res), flush=True)


def not_slower(runs, k):
    """On 16 CPUs at k: device hashing within the spread of the repetitions (the larger of the two forms') of the parent."""
    by = {(r["build"], r["cpus"]): r for r in runs}
    p, d = by[("parent", 16)]["sizes"][str(k)]["host"], by[("this", 16)]["sizes"][str(k)]["device"]
    return d["wall_ms"] <= p["wall_ms"] * (1 + max(p["spread"], d["spread"]))


def rule_as_issued(runs):
    """The smallest measured k at which not_slower holds; None if there is none."""
    return next((k for k in SIZES if not_slower(runs, k)), None)


def default_rule(runs):
    """The smallest measured k from which not_slower holds at every measured size; None if there is none."""
    return next((k for i, k in enumerate(SIZES) if all(not_slower(runs, j) for j in SIZES[i:])), None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libcurdlemsm.so of the parent commit")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--lib")
    ap.add_argument("--build")
    ap.add_argument("--cpus", type=int)
    ap.add_argument("--members")
    ap.add_argument("--want")
    a = ap.parse_args()
    if a.child:
        return child(a)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        raise SystemExit("--parent-lib: the parent commit's libcurdlemsm.so is the reference of every figure")
    this_lib = os.path.join(ROOT, "go-curdleproofs_amd", "libcurdlemsm.so")
    runs = []
    with tempfile.TemporaryDirectory() as tmp:
        members, want = os.path.join(tmp, "members.npz"), os.path.join(tmp, "want.npy")
        make_members(members)
        for cpus in CPUS:
            for build, lib in (("parent", os.path.abspath(a.parent_lib)), ("this", this_lib)):
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--lib", lib, "--build", build, "--cpus", str(cpus),
                       "--members", members, "--want", want]
                # a fresh process per build and CPU set; a child that fails or runs long ends the whole run
                r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=300)
                if r.returncode != 0:
                    raise SystemExit("child %s on %d CPUs ended with %d" % (build, cpus, r.returncode))
                line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
                runs.append(json.loads(line[7:]))
                print(line[7:], file=sys.stderr, flush=True)
    out = {"tool": "bench_tracker_hash", "warmups": WARM, "reps": REPS, "statistic": "median of the repetitions",
           "reference": "build 'parent', form 'host', same run and CPU set", "runs": runs, "rule_as_issued_from_k": rule_as_issued(runs),
           "default_rule_from_k": default_rule(runs)}
    text = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
