"""The device accumulator's kernels called directly (curdle_dacc_begin / _run / _submit / _wait with
export_scalars) against the big-integer model of tests/dacc_model.py, bit for bit: every case of every
generated family -- all four builds of the evaluation (k_dacc_front staged in LDS and reading global
memory, k_dacc_scalars<true> and <false>), exponents and gamma products up to 31 bits, segments that
overlap and straddle, special constants, degenerate totals.  The verifier's own tests
(test_device_accumulator.py) reach this code only at the few shapes a verification emits.

Which family reaches which build: `routes` all four, on both sides of the 16,384-pair border and of each
LDS budget; `totals` the staged front and the staged separate kernels (n = 16,385, and 16,384 loose pairs
behind 70 slots); every other family the staged front.  tests/test_dacc_model.py proves these claims and
the model itself without a GPU.  That the build path() names is the build that ran is asserted call by call
on the library's launch counters (curdle_stat_dacc_builds): the four builds compute the same scalars, so a
wrong choice between them shows nowhere else."""
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np
import pytest

import dacc_model as M
from conftest import ROOT
from dacc_model import R, as_map

pytestmark = pytest.mark.gpu

CASES = {f: M.family(f) for f in M.FAMILIES}


@pytest.fixture(scope="module")
def base_pts(gpu):
    return gpu.Rand(2024).get_g1_affines(257)


@pytest.fixture(scope="module")
def resident(gpu, base_pts):
    """One resident set per size (the CRS points of a case are the first n_crs of the tiling)."""
    sets = {}

    def get(c):
        if c.n_crs not in sets:
            sets[c.n_crs] = gpu.DBases(M.case_points(c._replace(n_inst=0, n_extra=0, inf_inst=-1, inf_extra=-1), base_pts)[0])
        return sets[c.n_crs]
    yield get
    for b in sets.values():
        b.free()


def expected(c, base_pts, oracle, coracle):
    """(model slot scalars, the C oracle's sum over all bases of model scalars ++ loose scalars)."""
    want = M.slots(c.checks, c.pool, c.n_crs, c.n_inst)
    crs, inst, loose = M.case_points(c, base_pts)
    pts, sc = np.concatenate([crs, inst, loose]), want + list(c.extra_scalars)
    if not len(pts):
        pts, sc = np.zeros((1, 12), dtype=np.uint64), [0]
    return want, coracle.msm_pippenger(pts, M.pack_fr(sc, oracle), threads=4)


def call_args(c, base_pts, oracle):
    _, inst, loose = M.case_points(c, base_pts)
    return inst, M.pack_checks(c.checks), M.pack_fr(c.pool, oracle), loose, M.pack_fr(c.extra_scalars, oracle)


def check_scalars(c, scalars, want, oracle):
    raw = M.raw_ints(scalars)
    assert len(raw) == c.n_res, c.name
    assert all(v < R for v in raw), (c.name, "an exported element is not canonical")
    got = [v * oracle.R_FR_INV % R for v in raw]
    if got != want:
        bad = [i for i in range(c.n_res) if got[i] != want[i]]
        pytest.fail(f"{c.name} ({c.what}): {len(bad)} of {c.n_res} slot scalars differ from the model, first at slot {bad[0]} "
                    f"(n_crs = {c.n_crs}): got {got[bad[0]]:#x}, want {want[bad[0]]:#x}")


def ran(gpu, c, calls, before):
    """The launch counters moved by `calls` on the build path() names for this case, and on no other."""
    now = gpu.stat_dacc_builds()
    want = dict(before)
    build = M.path(c.n_total, len(c.pool), len(c.checks))
    if build != "none" and not (build.startswith("split") and c.n_res == 0):
        want[build] += calls
    assert now == want, (c.name, c.what, build, before, now)
    return now


def wait_polling(gpu, job):
    deadline = time.time() + 120
    while not gpu.dacc_poll(job):
        assert time.time() < deadline, "the accumulation never finished"
    return gpu.dacc_wait(job)


@pytest.mark.parametrize("fam", M.FAMILIES)
def test_kernels_match_the_model_bit_for_bit(gpu, oracle, coracle, base_pts, resident, fam):
    """Every case of the family: 1. exported scalars == the model, canonical; 2. the sum == the C oracle's MSM of the
    model's scalars ++ the loose scalars; 3. the same sum without export_scalars; 4. (routes, totals) the two-step
    form, with and without the export; and each call launched the build path() names.  Up to three cases of a
    family with at most 12 pairs are also summed by the Python oracle (a cross-check of the C oracle, which judges
    every case)."""
    python_sums = 0
    for c in CASES[fam]:
        want, exp = expected(c, base_pts, oracle, coracle)
        args = call_args(c, base_pts, oracle)
        counters = gpu.stat_dacc_builds()
        out, scalars = gpu.dacc_run(resident(c), *args, export=True)
        check_scalars(c, scalars, want, oracle)                                   # 1. the slot scalars
        assert (out == exp).all(), (c.name, c.what, "the sum differs from the oracle's MSM of the model's scalars")  # 2.
        out2, none = gpu.dacc_run(resident(c), *args, export=False)               # 3. without the export
        assert none is None and (out2 == exp).all(), (c.name, c.what, "the sum differs without export_scalars")
        counters = ran(gpu, c, 2, counters)
        if fam in ("routes", "totals"):                                           # 4. the two-step form
            out3, sc3 = wait_polling(gpu, gpu.dacc_submit(resident(c), *args, export=True))
            check_scalars(c, sc3, want, oracle)
            assert (out3 == exp).all(), (c.name, c.what, "the sum differs in the two-step form")
            out4, _ = wait_polling(gpu, gpu.dacc_submit(resident(c), *args, export=False))
            assert (out4 == exp).all(), (c.name, c.what, "the sum differs in the two-step form without export_scalars")
            ran(gpu, c, 2, counters)
        if 0 < c.n_total <= 12 and python_sums < 3:                               # the Python oracle's textbook sum
            python_sums += 1
            crs, inst, loose = M.case_points(c, base_pts)
            acc = oracle.INF
            for p, s in zip(np.concatenate([crs, inst, loose]), want + list(c.extra_scalars)):
                if p.any():
                    acc = oracle.add(acc, oracle.scalar_mul(s, oracle.affine_from_mont_limbs([int(v) for v in p])))
            assert (out == coracle.jac_normalise(np.array(oracle.jac_to_mont_limbs(acc), dtype=np.uint64))).all(), c.name


def test_eight_accumulations_open_at_once_keep_their_own_results(gpu, oracle, coracle, base_pts):
    """Eight accumulations (all the workspace slots) submitted before any is waited for, collected in reverse
    order: each gets the scalars and the sum of its own description -- no job buffer, scalar array or pinned
    stage shared by mistake."""
    pick = [c for c in CASES["random"] if c.n_res >= 20 and c.n_extra and len(c.checks) >= 3][:6] + \
           [c for c in CASES["overlap"] if c.n_res >= 300][:1] + [c for c in CASES["totals"] if c.n_res == 257][:1]
    assert len(pick) == 8 == gpu.MSM_SLOTS
    sets = [gpu.DBases(M.case_points(c, base_pts)[0]) for c in pick]
    jobs = []
    try:
        for b, c in zip(sets, pick):
            jobs.append(gpu.dacc_submit(b, *call_args(c, base_pts, oracle), export=True))
        for c, job in reversed(list(zip(pick, jobs))):
            want, exp = expected(c, base_pts, oracle, coracle)
            out, scalars = gpu.dacc_wait(job)
            check_scalars(c, scalars, want, oracle)
            assert (out == exp).all(), c.name
    finally:
        for job in jobs:                                 # a failure above must not keep workspace slots
            gpu.dacc_abort(job)
        for b in sets:
            b.free()


def test_ignored_fields_have_no_effect(gpu, oracle, base_pts, resident):
    """The header: m (up to 31) and gammas_off of EXPLICIT / CONST, q_off and q_cap of every kind but FOLD_POW
    are ignored, not checked -- garbage there is accepted and changes neither the scalars nor the sum."""
    for c in CASES["tails"] + CASES["overlap"]:
        junk = []
        for k in c.checks:
            if k.kind <= M.CONST:
                k = k._replace(m=31, gammas_off=0xFFFFFFF0)
            if k.kind != M.FOLD_POW:
                k = k._replace(q_off=0xFFFFFFFF, q_cap=0x12345678)
            junk.append(k)
        assert M.validate(junk, len(c.pool), c.n_crs, c.n_inst, c.n_extra)
        inst, _, pool, xp, xs = call_args(c, base_pts, oracle)
        a = gpu.dacc_run(resident(c), inst, M.pack_checks(c.checks), pool, xp, xs)
        b = gpu.dacc_run(resident(c), inst, M.pack_checks(junk), pool, xp, xs)
        assert (a[0] == b[0]).all() and (a[1] == b[1]).all(), c.name


CHILD = r"""
import sys
sys.path[:0] = [%(pkg)r, %(oracle)r, %(tests)r]
import numpy as np
import bls12381_ref as oracle
import curdlemsm as cm
import dacc_model as M
cm.init(0)
base = cm.Rand(2024).get_g1_affines(257)
for c in M.family("routes"):
    crs, inst, loose = M.case_points(c, base)
    out, sc = cm.dacc_run(cm.DBases(crs), inst, M.pack_checks(c.checks), M.pack_fr(c.pool, oracle), loose,
                          M.pack_fr(c.extra_scalars, oracle))
    assert M.unpack_fr(sc, oracle) == M.slots(c.checks, c.pool, c.n_crs, c.n_inst), c.name
    print("ran", M.path(c.n_total, len(c.pool), len(c.checks)), len(c.pool))
print("all four routes ran")
"""


@pytest.mark.timeout(400)
def test_kernel_trace_names_all_four_builds(gpu):
    """A fresh child process under the profiler's kernel trace (no counters, one run) executes the four `routes`
    cases: the trace must name k_dacc_front and both instantiations of k_dacc_scalars.  The staged and the
    unstaged k_dacc_front are one symbol; only the LDS size of the dispatch (the kernel trace's LDS_Block_Size
    column) could tell them apart: the unstaged launch carries the conversion's static 32 KiB stage alone, the
    staged one the pool and the checks on top of it.  Whether the column counts LDS asked for at launch is read
    off the trace itself: k_dacc_scalars<true> has no static LDS and is launched with lds_bytes(pool, checks) of
    dynamic LDS, so a row of it below that size shows a column that holds the code object's static size only.
    Then (as with a profiler without the column) the two k_dacc_front forms cannot be told apart by the trace:
    the three names that can are asserted and the fact is printed.  Otherwise both sizes of k_dacc_front must be
    there.  (Measured on an MI355X with ROCm 7.2's rocprofv3: 32768 for every k_dacc_front dispatch.)
    Which form ran is asserted from the library's own counters in test_kernels_match_the_model_bit_for_bit."""
    prof = shutil.which("rocprofv3") or (os.path.exists("/opt/rocm/bin/rocprofv3") and "/opt/rocm/bin/rocprofv3")
    if not prof:
        pytest.fail("rocprofv3 is not on this machine's path: the kernel trace cannot be taken")
    code = CHILD % {"pkg": os.path.join(ROOT, "go-curdleproofs_amd"), "oracle": os.path.join(ROOT, "oracle", "py"),
                    "tests": os.path.join(ROOT, "tests")}
    rows = []
    with tempfile.TemporaryDirectory() as d:
        p = subprocess.run(["timeout", "-k", "10", "300", prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d,
                            "-o", "dacc", "--", sys.executable, "-c", code], capture_output=True, text=True, timeout=360)
        assert p.returncode == 0 and "all four routes ran" in p.stdout, (p.returncode, p.stdout[-1500:], p.stderr[-3000:])
        for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            with open(path, errors="replace", newline="") as f:
                rows += list(csv.DictReader(f))
    assert rows, "the profiler wrote no kernel trace"
    names = {r.get("Kernel_Name", "") for r in rows}
    front = [r for r in rows if "k_dacc_front" in r.get("Kernel_Name", "")]
    assert front, sorted(names)
    assert any("k_dacc_scalars<true>" in n or "k_dacc_scalarsILb1EE" in n for n in names), sorted(names)
    assert any("k_dacc_scalars<false>" in n or "k_dacc_scalarsILb0EE" in n for n in names), sorted(names)
    lds_col = [k for k in rows[0] if k and k.startswith("LDS_Block_Size")]
    print("kernel trace columns:", list(rows[0]))
    if not lds_col:
        print("no LDS_Block_Size column in this profiler's kernel trace: the staged and unstaged k_dacc_front are not told apart")
        return
    lds = sorted({int(r[lds_col[0]]) for r in front})
    for r in rows:                                   # what the column holds, dispatch by dispatch, before it is judged
        if "dacc" in r["Kernel_Name"] or "k_hist" in r["Kernel_Name"]:
            print(r["Kernel_Name"][:48], "LDS", r[lds_col[0]], "grid", r.get("Grid_Size_X"))
    print("LDS of the k_dacc_front dispatches:", lds)
    split = max(int(r[lds_col[0]]) for r in rows if "k_dacc_scalars<true>" in r["Kernel_Name"] or "k_dacc_scalarsILb1EE" in r["Kernel_Name"])
    split_case = [c for c in CASES["routes"] if M.path(c.n_total, len(c.pool), len(c.checks)) == "split_lds"][0]
    if split < M.lds_bytes(len(split_case.pool), len(split_case.checks), M.SPLIT_BUDGET):
        print(f"LDS_Block_Size of k_dacc_scalars<true> is {split}: this profiler's column leaves out the LDS asked for at launch; "
              "the staged and unstaged k_dacc_front are not told apart")
        return
    staged_pool = min(len(c.pool) for c in CASES["routes"])        # the fused case whose pool still stages
    assert len(lds) >= 2 and lds[-1] - lds[0] >= staged_pool * 32, lds


def test_the_verifiers_map_is_read_by_the_same_helper(gpu, oracle):
    """The direct file and the verifier's file (test_device_accumulator.py) share as_map from the model module:
    the verifier's device accumulator against its host mirror at two sizes, read through it."""
    from test_protocol_gpu import setup
    import test_device_accumulator as tda
    assert tda.as_map is as_map
    for n in (16, 64):
        crs, Rs, Ss, Ts, Us, Mp, perm, k, rs_m = setup(gpu, n)
        proof = gpu.Proof(gpu.prove(crs, Rs, Ss, Ts, Us, Mp, perm, k, rs_m, gpu.Rand(42)))
        pm, sm, ok_m = gpu.verify_export_accumulator(crs, proof, Rs, Ss, Ts, Us, Mp, gpu.Rand(43), device=False)
        pd, sd, ok_d = gpu.verify_export_accumulator(crs, proof, Rs, Ss, Ts, Us, Mp, gpu.Rand(43), device=True)
        assert ok_m and ok_d and as_map(oracle, pm, sm) == as_map(oracle, pd, sd)
