"""The membership check for G1 points that arrive in memory (curdle_g1_check_batch, check_kernels.hip) through
EVERY build of its kernel, and the checked verifier entry points that use it.

tests/golden/affine_check_points.npz (generator beside it) holds 555 points in gnark's in-memory layout whose
answers follow from the definitions alone: every point of the decoder's edge fixture (small-order points, T + Q,
composite orders, cofactor-cleared points, ...), points of OTHER curves y^2 = x^3 + b' -- which every point kernel
would process without a trace, the group law never using b --, mixed-up coordinates, words that are no field
element, and infinity.  No point is skipped.

Builds, forced with the library's own knob (QUAD_MAX_LANES):
  quad   defaults                        k_g1_check_affine<true,true>    (up to 32,768 points)
  lane   QUAD_MAX_LANES=0                k_g1_check_affine<false,true>
  nosub  subgroup_check = False          k_g1_check_affine<false,false>
test_kernel_trace_names_all_three_builds proves with a kernel trace that these run the kernels named."""
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile
import threading

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(ROOT, "tests", "golden", "affine_check_points.npz")
DECODER_FIXTURE = os.path.join(ROOT, "tests", "golden", "decode_edge_records.npz")
BUILD_NAMES = ("quad", "lane", "nosub")
SMALL_SIZES = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257)          # quad, wave and block tails
LAST_KINDS = ("torsion", "other_curve", "infinity", "g1")     # what sits in the last, partly filled quad / block
TEXT = {2: "not a field element", 3: "not on the curve", 4: "not in the prime-order subgroup"}


class Points:
    def __init__(self):
        z = np.load(FIXTURE)
        self.pts = z["points"]
        self.st_sub = z["status_subgroup"]
        self.st_nosub = z["status_no_subgroup"]
        self.family = [f.decode() for f in z["family"]]
        self.n = len(self.pts)
        first = lambda pred: next(i for i in range(self.n) if pred(i))
        self.first = {"torsion": first(lambda i: self.family[i] == "from_decoder" and self.st_sub[i] == 4),
                      "other_curve": first(lambda i: self.family[i] == "other_curve"),
                      "infinity": first(lambda i: self.st_sub[i] == 1),
                      "g1": first(lambda i: self.family[i] == "from_decoder" and self.st_sub[i] == 0),
                      "range": first(lambda i: self.family[i] == "range")}

    def tiled(self, n, last_kind):
        """Indices of n points, the fixture repeated and rotated so that point n - 1 is of `last_kind`."""
        return (np.arange(n) + (self.first[last_kind] - (n - 1))) % self.n


@pytest.fixture(scope="module")
def fx():
    return Points()


def run_build(gpu, build, pts, device=False):
    import torch
    sub = build != "nosub"
    if device:
        d = torch.from_numpy(np.ascontiguousarray(pts).view(np.int64)).to("cuda:0")
        call = lambda: gpu.g1_check_batch_device(d.data_ptr(), len(pts), sub)
    else:
        call = lambda: gpu.g1_check_batch(pts, sub)
    if build == "lane":
        with gpu.knobs(QUAD_MAX_LANES=0):
            return call()
    return call()


def check_build(gpu, fx, build, idx, device=False):
    want = fx.st_nosub[idx] if build == "nosub" else fx.st_sub[idx]
    got = run_build(gpu, build, fx.pts[idx], device)
    bad = np.nonzero(got != want)[0]
    print("build %s%s n=%d: %d of %d statuses differ from the fixture" % (build, " (device)" if device else "", len(idx), len(bad), len(idx)))
    assert got.shape == want.shape and len(bad) == 0, \
        (build, len(idx), [(int(i), fx.family[idx[i]], "want %d got %d" % (want[i], got[i])) for i in bad[:12]], len(bad))


def test_fixture_is_whole(fx):
    from collections import Counter
    count = Counter(fx.family)
    assert count["from_decoder"] >= 360 and count["other_curve"] == 128 and count["mixed"] >= 32 and count["range"] >= 18
    assert set(fx.st_sub.tolist()) == {0, 1, 2, 3, 4} and set(fx.st_nosub.tolist()) == {0, 1, 2, 3}


@pytest.mark.parametrize("build", BUILD_NAMES)
def test_every_point_through_every_build(gpu, fx, build):
    check_build(gpu, fx, build, np.arange(fx.n))


@pytest.mark.parametrize("build", ["quad", "nosub"])
def test_every_point_from_a_resident_array(gpu, fx, build):
    check_build(gpu, fx, build, np.arange(fx.n), device=True)


def test_a_resident_array_on_the_callers_stream(gpu, fx):
    import torch
    d = torch.from_numpy(fx.pts.view(np.int64)).to("cuda:0")
    s = torch.cuda.Stream()
    got = gpu.g1_check_batch_device(d.data_ptr(), fx.n, True, stream=s.cuda_stream)
    assert (got == fx.st_sub).all()


@pytest.mark.parametrize("n", SMALL_SIZES)
def test_tails_of_quads_waves_and_blocks(gpu, fx, n):
    """Batch sizes that leave the last quad-of-lanes group, wave and block partly empty; which kind of point comes
    last rotates with the size and the build, so that every kind is last in every build."""
    for r, build in enumerate(BUILD_NAMES):
        kind = LAST_KINDS[(SMALL_SIZES.index(n) + r) % len(LAST_KINDS)]
        idx = fx.tiled(n, kind)
        assert idx[-1] == fx.first[kind]
        check_build(gpu, fx, build, idx)


def test_rotation_puts_every_kind_last_in_every_build():
    for r in range(len(BUILD_NAMES)):
        assert {LAST_KINDS[(i + r) % len(LAST_KINDS)] for i in range(len(SMALL_SIZES))} == set(LAST_KINDS)


@pytest.mark.parametrize("n", [32768, 32769])
def test_the_boundary_where_the_build_changes(gpu, fx, n):
    """32,768 points are the last launch on four lanes per point, 32,769 the first on one lane."""
    check_build(gpu, fx, "quad", fx.tiled(n, "torsion" if n == 32768 else "other_curve"))


def test_agreement_with_the_decoder(gpu):
    """Every record of the decoder's fixture that decodes to a point: the check of the decoded point says what the
    decoder said of the record, with and without the subgroup test."""
    z = np.load(DECODER_FIXTURE)
    blob = z["records"].tobytes()
    pts, st_nosub = gpu.g1_decompress_batch(blob, False)
    _, st_sub = gpu.g1_decompress_batch(blob, True)
    rows = np.nonzero(st_nosub == 0)[0]
    assert len(rows) >= 360 and (st_nosub == z["status_no_subgroup"]).all() and (st_sub == z["status_subgroup"]).all()
    assert (gpu.g1_check_batch(pts[rows], True) == st_sub[rows]).all()
    assert (gpu.g1_check_batch(pts[rows], False) == st_nosub[rows]).all()
    assert {int(s) for s in st_sub[rows]} == {0, 4}


# ---------------------------------------------------------------------------------------------------------------
# the checked verifier
# ---------------------------------------------------------------------------------------------------------------
class Case:
    """The committed proof of one ell with its instance, and the points to plant."""

    def __init__(self, gpu, oracle, fx, ell):
        from test_decode_edges_gpu import attack_records
        from test_proof_fixtures import instance
        v = np.load(os.path.join(ROOT, "tests", "golden", "proof_vectors.npz"))
        self.ell = ell
        self.proof = v[f"ell{ell}_proof"].tobytes()
        self.crs, self.Rs, self.Ss, self.Ts, self.Us, self.M = instance(gpu, ell, int(v[f"ell{ell}_seed"][0]))[:6]
        z = np.load(DECODER_FIXTURE)
        by_record = {z["records"][i].tobytes(): z["points"][i].tobytes() for i in range(len(z["records"]))}
        self.bad, self.bad_M = {}, {}
        for name, rec in attack_records(oracle).items():          # order 3, order 11, T + Q: each asserted there
            b = by_record[rec]
            pt = (int.from_bytes(b[:48], "big"), int.from_bytes(b[48:], "big"))
            self.bad[name] = (np.array(oracle.affine_to_mont_limbs(pt), dtype=np.uint64), 4)
            self.bad_M[name] = np.array(oracle.jac_to_mont_limbs(pt), dtype=np.uint64)
        self.bad["other curve"] = (fx.pts[fx.first["other_curve"] + 5], 3)
        self.bad["range"] = (fx.pts[fx.first["range"]], 2)
        assert fx.st_sub[fx.first["other_curve"] + 5] == 3 and fx.st_sub[fx.first["range"]] == 2

    def vectors(self):
        return {"Rs": self.Rs.copy(), "Ss": self.Ss.copy(), "Ts": self.Ts.copy(), "Us": self.Us.copy()}


@pytest.fixture(scope="module")
def cases(gpu, oracle, fx):
    return {ell: Case(gpu, oracle, fx, ell) for ell in (12, 60)}


def outcome(call):
    import curdlemsm as cm
    try:
        return ("accept bit", call())
    except cm.CurdleError as e:
        return ("error", e.code, e.msg)


def checked_fns(gpu, c, entry):
    """(checked, unchecked) over (Rs, Ss, Ts, Us, M, seed) for the byte or the decoded-proof entry points."""
    if entry == "bytes":
        return (lambda R, S, T, U, M, seed=5: gpu.verify_checked(c.crs, c.proof, R, S, T, U, M, gpu.Rand(seed)),
                lambda R, S, T, U, M, seed=5: gpu.verify(c.crs, c.proof, R, S, T, U, M, gpu.Rand(seed)))
    proof = gpu.Proof(c.proof)
    return (lambda R, S, T, U, M, seed=5: gpu.verify_proof_checked(c.crs, proof, R, S, T, U, M, gpu.Rand(seed)),
            lambda R, S, T, U, M, seed=5: gpu.verify_proof(c.crs, proof, R, S, T, U, M, gpu.Rand(seed)))


def expect_refusal(gpu, call, where, status):
    with pytest.raises(gpu.CurdleError) as e:
        call()
    assert e.value.code == gpu.EINVAL, e.value
    assert e.value.msg.startswith(where + ": ") and TEXT[status] in e.value.msg, (where, status, e.value.msg)


def run_checked_set(gpu, c, entry):
    checked, plain = checked_fns(gpu, c, entry)
    v = c.vectors()
    # honest, on both accumulators
    for device_acc in (True, False):
        gpu.verify_set_device_acc(device_acc)
        try:
            assert checked(v["Rs"], v["Ss"], v["Ts"], v["Us"], c.M) is True
        finally:
            gpu.verify_set_device_acc(True)
    # wrong but in G1: accept bit and error text are the unchecked call's
    assert outcome(lambda: checked(v["Ss"], v["Rs"], v["Ts"], v["Us"], c.M)) == \
        outcome(lambda: plain(v["Ss"], v["Rs"], v["Ts"], v["Us"], c.M)) == ("accept bit", False)
    # one point at a time, first and last index of every vector
    for name, (pt, status) in c.bad.items():
        for vec in ("Rs", "Ss", "Ts", "Us"):
            for i in (0, c.ell - 1):
                w = c.vectors()
                w[vec][i] = pt
                expect_refusal(gpu, lambda: checked(w["Rs"], w["Ss"], w["Ts"], w["Us"], c.M), "%s[%d]" % (vec, i), status)
    for name, M in c.bad_M.items():
        expect_refusal(gpu, lambda: checked(v["Rs"], v["Ss"], v["Ts"], v["Us"], M), "M", 4)
    # the lowest vector in the order R, S, T, U, M, then the lowest index, is the one reported
    w = c.vectors()
    w["Ts"][0], w["Ss"][3], w["Rs"][5], w["Rs"][c.ell - 1] = c.bad["order 3"][0], c.bad["range"][0], c.bad["other curve"][0], c.bad["T+Q"][0]
    expect_refusal(gpu, lambda: checked(w["Rs"], w["Ss"], w["Ts"], w["Us"], c.bad_M["order 11"]), "Rs[5]", 3)
    w = c.vectors()
    w["Us"][c.ell - 1] = c.bad["order 11"][0]
    expect_refusal(gpu, lambda: checked(w["Rs"], w["Ss"], w["Ts"], w["Us"], c.bad_M["order 3"]), "Us[%d]" % (c.ell - 1), 4)
    # an instance point at infinity is acceptable to the check: the verdict is the unchecked call's
    for vec in ("Rs", "Us"):
        w = c.vectors()
        w[vec][1] = 0
        got = outcome(lambda: checked(w["Rs"], w["Ss"], w["Ts"], w["Us"], c.M))
        assert got == outcome(lambda: plain(w["Rs"], w["Ss"], w["Ts"], w["Us"], c.M)), got
        assert got != ("accept bit", True)


@pytest.mark.parametrize("ell", [12, 60])
def test_verify_checked(gpu, cases, ell):
    run_checked_set(gpu, cases[ell], "bytes")


def test_verify_checked_reports_a_malformed_proof_as_verify_does(gpu, cases):
    c = cases[12]
    v = c.vectors()
    for proof in (c.proof[:-1], c.proof[:100], b""):
        args = (v["Rs"], v["Ss"], v["Ts"], v["Us"], c.M)
        want = outcome(lambda: gpu.verify(c.crs, proof, *args, gpu.Rand(5)))
        assert want[0] == "error"
        assert outcome(lambda: gpu.verify_checked(c.crs, proof, *args, gpu.Rand(5))) == want


def test_verify_proof_checked(gpu, cases):
    run_checked_set(gpu, cases[12], "decoded")


def planted(c, t, j):
    """Call j of the bad thread: which point goes where."""
    vec = ("Rs", "Ss", "Ts", "Us")[j % 4]
    name = list(c.bad)[(t + j) % len(c.bad)]
    i = (7 * j + t) % c.ell
    return vec, i, name


def test_eight_threads_of_checked_verifications(gpu, cases):
    """Eight threads x four checked verifications each (ell = 60, from bytes), thread 3's instances planted bad: exact
    results per call.  There are four decode contexts and a verification from bytes takes one for its proof's points
    besides the one its check takes, so with eight threads some checks may find every context busy and run to their end
    through an MSM slot first; how many did is printed from the library's own counters (curdle_stat_check_paths) and
    depends on the timing -- test_check_with_every_decode_context_taken below forces that path."""
    c = cases[60]
    before = gpu.stat_check_paths()
    results = [[None] * 4 for _ in range(8)]

    def worker(t):
        for j in range(4):
            w = c.vectors()
            if t == 3:
                vec, i, name = planted(c, t, j)
                w[vec][i] = c.bad[name][0]
            results[t][j] = outcome(lambda: gpu.verify_checked(c.crs, c.proof, w["Rs"], w["Ss"], w["Ts"], w["Us"], c.M,
                                                               gpu.Rand(100 * t + j)))

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    after = gpu.stat_check_paths()
    print("checks beside the verification: %d, run to the end first: %d" % (after["beside"] - before["beside"],
                                                                            after["first"] - before["first"]))
    assert (after["beside"] - before["beside"]) + (after["first"] - before["first"]) == 32
    for t in range(8):
        for j in range(4):
            if t != 3:
                assert results[t][j] == ("accept bit", True), (t, j, results[t][j])
                continue
            vec, i, name = planted(c, t, j)
            kind, code, msg = results[t][j]
            assert kind == "error" and code == gpu.EINVAL, results[t][j]
            assert msg.startswith("%s[%d]: " % (vec, i)) and TEXT[c.bad[name][1]] in msg, (vec, i, name, msg)


def test_check_with_every_decode_context_taken(gpu, cases):
    """All four decode contexts held by point decodings in flight: the check of a checked verification runs to its
    end through an MSM slot first (the counter says so), holds nothing while the verifier runs, and the results are
    the same."""
    c = cases[12]
    z = np.load(DECODER_FIXTURE)
    blob = z["records"][:8].tobytes()
    tickets = [gpu.g1_decompress_start(blob) for _ in range(4)]
    try:
        before = gpu.stat_check_paths()
        v = c.vectors()
        assert gpu.verify_checked(c.crs, c.proof, v["Rs"], v["Ss"], v["Ts"], v["Us"], c.M, gpu.Rand(5)) is True
        v["Ss"][c.ell - 1] = c.bad["T+Q"][0]
        expect_refusal(gpu, lambda: gpu.verify_checked(c.crs, c.proof, v["Rs"], v["Ss"], v["Ts"], v["Us"], c.M, gpu.Rand(5)),
                       "Ss[%d]" % (c.ell - 1), 4)
        after = gpu.stat_check_paths()
        assert (after["first"] - before["first"], after["beside"] - before["beside"]) == (2, 0)
    finally:
        for t in tickets:
            gpu.g1_decompress_finish(t, 8)
    before = gpu.stat_check_paths()
    v = c.vectors()
    assert gpu.verify_checked(c.crs, c.proof, v["Rs"], v["Ss"], v["Ts"], v["Us"], c.M, gpu.Rand(5)) is True
    after = gpu.stat_check_paths()
    assert (after["first"] - before["first"], after["beside"] - before["beside"]) == (0, 1)


CHILD = r"""
import sys
sys.path[:0] = [%(pkg)r, %(tests)r]
import numpy as np
import curdlemsm as cm
cm.init(0)
z = np.load(%(fixture)r)
pts = z["points"]
got = [cm.g1_check_batch(pts, True)]
with cm.knobs(QUAD_MAX_LANES=0):
    got.append(cm.g1_check_batch(pts, True))
assert all((g == z["status_subgroup"]).all() for g in got), [int((g != z["status_subgroup"]).sum()) for g in got]
assert (cm.g1_check_batch(pts, False) == z["status_no_subgroup"]).all()
print("the three builds ran")
"""

BUILDS = {"k_g1_check_affine<true,true>": r"k_g1_check_affine<true,\s*true>|k_g1_check_affineILb1ELb1EE",
          "k_g1_check_affine<false,true>": r"k_g1_check_affine<false,\s*true>|k_g1_check_affineILb0ELb1EE",
          "k_g1_check_affine<false,false>": r"k_g1_check_affine<false,\s*false>|k_g1_check_affineILb0ELb0EE"}


@pytest.mark.timeout(400)
def test_kernel_trace_names_all_three_builds(gpu):
    """A child process under the profiler's kernel trace (no counters) runs the three builds once on the fixture; its
    statistics must name every build of the kernel.  If the child fails the test fails; nothing is retried."""
    prof = shutil.which("rocprofv3") or (os.path.exists("/opt/rocm/bin/rocprofv3") and "/opt/rocm/bin/rocprofv3")
    if not prof:
        pytest.fail("rocprofv3 is not on this machine's path: the kernel trace cannot be taken")
    code = CHILD % {"pkg": os.path.join(ROOT, "go-curdleproofs_amd"), "tests": os.path.join(ROOT, "tests"), "fixture": FIXTURE}
    with tempfile.TemporaryDirectory() as d:
        p = subprocess.run(["timeout", "-k", "10", "300", prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d,
                            "-o", "check", "--", sys.executable, "-c", code], capture_output=True, text=True, timeout=360)
        assert p.returncode == 0 and "the three builds ran" in p.stdout, (p.returncode, p.stdout[-1500:], p.stderr[-3000:])
        text = ""
        for path in glob.glob(os.path.join(d, "**", "*.csv"), recursive=True):
            with open(path, errors="replace") as f:
                text += f.read()
    assert text, "the profiler wrote no csv"
    named = {b: bool(re.search(pat, text)) for b, pat in BUILDS.items()}
    print(named)
    assert all(named.values()), named
