"""curdle_crs_from_points / _from_bytes on the GPU, at ell = 4, 12, 60 and 124: validated round trips (points and bytes,
and the golden fixture the pure-Python oracle wrote), an imported handle against the generated one through Prove, Verify,
the decoded-proof verifier, the batch verifier, the Whisk pair and the constant-time prover handle, a CRS no seed produces
(oracle points s_i G, H / Gt / Gu under random Z), every fault with its field, index and reason, the order faults are
reported in, the check-path counter, and two imports beside an MSM on three threads.  The last test prints the wall time
of one validated from_points and one from_bytes at ell = 124 (median of 7 after 2 warm-ups); it asserts nothing about it.

The fault points come from the fixtures the point-check tests use: tests/golden/affine_check_points.npz (off the curve, a
coordinate >= p, torsion points) and tests/golden/decode_edge_records.npz (the same as 48-byte records)."""
import hashlib
import importlib.util
import os
import threading
import time

import numpy as np
import pytest

from conftest import ROOT
from test_prove_ct_gpu import instance

pytestmark = pytest.mark.gpu

ELLS = (4, 12, 60, 124)
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIELDS = ("Gs", "Hs", "H", "Gt", "Gu", "Gsum", "Hsum")
OK, INFINITY, BAD_ENCODING, NOT_ON_CURVE, NOT_IN_SUBGROUP = range(5)
TEXT = {INFINITY: "the point at infinity is no generator", NOT_ON_CURVE: "not on the curve",
        NOT_IN_SUBGROUP: "not in the prime-order subgroup"}


def same_points(a, b):
    return all((np.asarray(a[k]) == np.asarray(b[k])).all() for k in FIELDS)


def copy_points(p):
    return {k: np.array(p[k], dtype=np.uint64, copy=True) for k in FIELDS}


def name_of(field, index):
    return "%s[%d]" % (FIELDS[field], index) if field <= 1 else FIELDS[field]


def expect_fault(cm, call, field, index, reason, text=None):
    with pytest.raises(cm.CrsFault) as e:
        call()
    f = e.value
    assert (f.code, f.field, f.index, f.reason) == (cm.EINVAL, field, index, reason), (f.field, f.index, f.reason, f.msg)
    assert f.msg.startswith(name_of(field, index) + ": "), f.msg
    if text is None:
        text = TEXT.get(reason)
    if text:
        assert text in f.msg, f.msg


@pytest.fixture(scope="module")
def generated(gpu):
    """Per ell: a generated handle, its exported points and its wire bytes.  Never modified."""
    out = {}
    for ell in ELLS:
        crs = gpu.CRS(ell, gpu.Rand(700 + ell))
        out[ell] = (crs, crs.points(), crs.to_bytes())
    return out


@pytest.fixture(scope="module")
def bad(oracle):
    """Affine fault points (twelve words) and fault records (48 bytes), from the point-check fixtures."""
    z = np.load(os.path.join(GOLDEN, "affine_check_points.npz"))
    fam, st = z["family"], z["status_subgroup"]
    pick = lambda f, s: z["points"][np.nonzero((fam == f) & (st == s))[0][0]].copy()
    pts = {NOT_ON_CURVE: pick(b"mixed", NOT_ON_CURVE), BAD_ENCODING: pick(b"range", BAD_ENCODING),
           NOT_IN_SUBGROUP: pick(b"from_decoder", NOT_IN_SUBGROUP), INFINITY: np.zeros(12, dtype=np.uint64)}
    d = np.load(os.path.join(GOLDEN, "decode_edge_records.npz"))
    rec = lambda s: d["records"][np.nonzero(d["status_subgroup"] == s)[0][0]].tobytes()
    recs = {NOT_ON_CURVE: rec(NOT_ON_CURVE), NOT_IN_SUBGROUP: rec(NOT_IN_SUBGROUP), INFINITY: oracle.compress(oracle.INF)}
    one = np.array(oracle.jac_to_mont_limbs(oracle.G1)[12:], dtype=np.uint64)
    jac = {s: np.concatenate([p, one]) for s, p in pts.items() if s != INFINITY}
    jac[INFINITY] = np.concatenate([pts[NOT_ON_CURVE], np.zeros(6, dtype=np.uint64)])   # Z = 0: X and Y are not looked at
    return pts, jac, recs


def draw(tag, mod):
    return int.from_bytes(hashlib.shake_256(("crs-import-gpu/" + tag).encode()).digest(64), "big") % mod


def under_z(oracle, pt, z):
    """The Jacobian words (X Z^2, Y Z^3, Z) of an affine oracle point."""
    c = (pt[0] * z * z % oracle.P, pt[1] * z * z * z % oracle.P, z)
    return np.array(sum((oracle.fp_to_mont_limbs(v) for v in c), []), dtype=np.uint64)


@pytest.fixture(scope="module")
def unseeded(oracle, coracle):
    """Per ell: a CRS of oracle points s_i G for scalars no common.Rand draws, H / Gt / Gu under random Z, the sums as
    (sum of s_i) G -- and the same with Z = 1, which is what a handle exports."""
    out = {}
    for ell in ELLS:
        s = [draw("%d/%d" % (ell, i), oracle.R - 1) + 1 for i in range(ell + 7)]
        assert len(set(s)) == len(s)
        aff = np.stack([coracle.scalar_mul_gen(v) for v in s])
        ints = [oracle.affine_from_mont_limbs([int(w) for w in aff[ell + 4 + j]]) for j in range(3)]
        given = {"Gs": aff[:ell], "Hs": aff[ell:ell + 4],
                 "Gsum": coracle.scalar_mul_gen(sum(s[:ell]) % oracle.R), "Hsum": coracle.scalar_mul_gen(sum(s[ell:ell + 4]) % oracle.R)}
        stored = dict(given)
        for j, k in enumerate(("H", "Gt", "Gu")):
            given[k] = under_z(oracle, ints[j], draw("%d/z%d" % (ell, j), oracle.P - 1) + 1)
            stored[k] = np.array(oracle.jac_to_mont_limbs(ints[j]), dtype=np.uint64)
        out[ell] = (given, stored)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# round trips
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ell", ELLS)
def test_validated_round_trips(gpu, generated, ell):
    crs, pts, wire = generated[ell]
    assert len(wire) == 48 * (ell + 9)
    by_points = gpu.CRS.from_points(**pts)
    assert by_points.ell == ell and same_points(by_points.points(), pts) and by_points.to_bytes() == wire
    by_bytes = gpu.CRS.from_bytes(wire)
    assert by_bytes.ell == ell and same_points(by_bytes.points(), pts) and by_bytes.to_bytes() == wire


def test_the_golden_fixture_decodes_to_the_oracle_s_points(gpu, oracle):
    spec = importlib.util.spec_from_file_location("gen_crs_fixture", os.path.join(GOLDEN, "gen_crs_fixture.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    Gs, Hs, H, Gt, Gu, Gsum, Hsum = gen.crs_points()
    with open(os.path.join(GOLDEN, "crs_ell4.bin"), "rb") as f:
        wire = f.read()
    crs = gpu.CRS.from_bytes(wire)
    got = crs.points()
    assert crs.ell == 4 and crs.to_bytes() == wire
    assert got["Gs"].tolist() == [oracle.affine_to_mont_limbs(p) for p in Gs]
    assert got["Hs"].tolist() == [oracle.affine_to_mont_limbs(p) for p in Hs]
    for k, p in (("H", H), ("Gt", Gt), ("Gu", Gu)):
        assert got[k].tolist() == oracle.jac_to_mont_limbs(p)
    assert got["Gsum"].tolist() == oracle.affine_to_mont_limbs(Gsum) and got["Hsum"].tolist() == oracle.affine_to_mont_limbs(Hsum)


# ---------------------------------------------------------------------------------------------------------------------
# an imported handle is a generated one
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ell", ELLS)
def test_an_imported_handle_proves_and_verifies_as_the_generated_one(gpu, ell):
    crs, Rs, Ss, Ts, Us, M, perm, k, rs_m = instance(gpu, ell, "random")
    imp = gpu.CRS.from_points(**crs.points())
    assert imp.to_bytes() == crs.to_bytes()
    r0, r1 = gpu.Rand(2000 + ell), gpu.Rand(2000 + ell)
    proof = gpu.prove(crs, Rs, Ss, Ts, Us, M, perm, k, rs_m, r0)
    assert gpu.prove(imp, Rs, Ss, Ts, Us, M, perm, k, rs_m, r1) == proof
    assert (r0.get_frs(3) == r1.get_frs(3)).all()
    # crossed: each handle accepts the proof (the other one made the same bytes), from bytes and decoded
    decoded = gpu.Proof(proof)
    for h in (imp, crs):
        assert gpu.verify(h, proof, Rs, Ss, Ts, Us, M, gpu.Rand(43)) is True
        assert gpu.verify_proof(h, decoded, Rs, Ss, Ts, Us, M, gpu.Rand(44)) is True
    if ell in (4, 12):
        prover = gpu.ProverCt(imp)
        try:
            assert prover.prove(Rs, Ss, Ts, Us, M, perm, k, rs_m, gpu.Rand(2000 + ell)) == proof
        finally:
            prover.free()
    if ell == gpu.WHISK_ELL:
        # a batch of three: the good proof, a damaged one, the good one again
        damaged = bytearray(proof)
        damaged[-1] ^= 1
        cols = ([proof, bytes(damaged), proof], [Rs] * 3, [Ss] * 3, [Ts] * 3, [Us] * 3, [M] * 3)
        assert gpu.verify_batch(imp, *cols, gpu.Rand(9), nthreads=3) == gpu.verify_batch(crs, *cols, gpu.Rand(9), nthreads=3) \
            == [True, False, True]
        # the Whisk pair, crossed
        r = gpu.Rand(31)
        trk, _ = gpu.whisk_compute_trackers_batch(r.get_frs(ell), r.get_frs(ell), commitments=False)
        pre = [trk[i].tobytes() for i in range(ell)]
        ra, rb = gpu.Rand(61), gpu.Rand(61)
        post, shuffle_proof = gpu.whisk_generate_shuffle_proof(imp, pre, ra)
        assert (post, shuffle_proof) == gpu.whisk_generate_shuffle_proof(crs, pre, rb)
        assert (ra.get_frs(2) == rb.get_frs(2)).all()
        assert gpu.whisk_is_valid_shuffle_proof(crs, pre, post, shuffle_proof, gpu.Rand(43)) is True
        assert gpu.whisk_is_valid_shuffle_proof(imp, pre, post, shuffle_proof, gpu.Rand(43)) is True


def outcome(cm, call):
    try:
        return ("accept bit", call())
    except cm.CurdleError as e:
        return ("error", e.code, e.msg)


@pytest.mark.parametrize("ell", ELLS)
def test_a_crs_no_seed_produces(gpu, generated, unseeded, ell):
    given, stored = unseeded[ell]
    crs = gpu.CRS.from_points(**given)
    assert same_points(crs.points(), stored)                    # H, Gt, Gu stored with Z = 1
    assert same_points(gpu.CRS.from_bytes(crs.to_bytes()).points(), stored)
    rand = gpu.Rand(3000 + ell)
    perm = np.asarray(rand.generate_permutation(ell), dtype=np.uint32)
    k, Rs, Ss = rand.get_fr(), rand.get_g1_affines(ell), rand.get_g1_affines(ell)
    Ts, Us, M, rs_m = gpu.shuffle_permute_commit(crs, Rs, Ss, perm, k, rand)
    proof = gpu.prove(crs, Rs, Ss, Ts, Us, M, perm, k, rs_m, gpu.Rand(5))
    assert gpu.verify(crs, proof, Rs, Ss, Ts, Us, M, gpu.Rand(43)) is True
    other = generated[ell][0]
    assert gpu.verify(other, proof, Rs, Ss, Ts, Us, M, gpu.Rand(43)) is False      # another CRS: ok = 0, no error
    # a flipped byte rejects, or errors, exactly as it does for a proof made and checked on a generated handle: the
    # compressed-form flag of the first point (no encoding: an error), the lowest bit of the last scalar (a reject)
    g_crs, g_Rs, g_Ss, g_Ts, g_Us, g_M, g_perm, g_k, g_rs_m = instance(gpu, ell, "random")
    g_proof = gpu.prove(g_crs, g_Rs, g_Ss, g_Ts, g_Us, g_M, g_perm, g_k, g_rs_m, gpu.Rand(5))
    assert len(g_proof) == len(proof)
    seen = []
    for at, bit in ((0, 0x80), (len(proof) - 1, 1)):
        mine, theirs = bytearray(proof), bytearray(g_proof)
        mine[at] ^= bit
        theirs[at] ^= bit
        a = outcome(gpu, lambda: gpu.verify(crs, bytes(mine), Rs, Ss, Ts, Us, M, gpu.Rand(43)))
        b = outcome(gpu, lambda: gpu.verify(g_crs, bytes(theirs), g_Rs, g_Ss, g_Ts, g_Us, g_M, gpu.Rand(43)))
        assert a == b, (at, a, b)
        seen.append(a[0])
    assert seen == ["error", "accept bit"]


# ---------------------------------------------------------------------------------------------------------------------
# faults
# ---------------------------------------------------------------------------------------------------------------------
def places(ell):
    """(field, index) of every place a point fault is planted."""
    return [(0, 0), (0, ell - 1), (1, 0), (1, 3), (2, 0), (3, 0), (4, 0), (5, 0), (6, 0)]


def plant(pts, field, index, value):
    k = FIELDS[field]
    if field <= 1:
        pts[k][index] = value
    else:
        pts[k] = np.array(value, dtype=np.uint64)


@pytest.mark.parametrize("ell", ELLS)
def test_every_point_fault_from_points(gpu, generated, bad, ell):
    affine, jac, _ = bad
    for field, index in places(ell):
        for reason in (NOT_ON_CURVE, BAD_ENCODING, NOT_IN_SUBGROUP, INFINITY):
            if reason == INFINITY and field >= 5:
                continue                                        # a sum at infinity is a matter of the sums: below
            pts = copy_points(generated[ell][1])
            plant(pts, field, index, (jac if 2 <= field <= 4 else affine)[reason])
            text = "not a field element" if reason == BAD_ENCODING else None
            expect_fault(gpu, lambda: gpu.CRS.from_points(**pts), field, index, reason, text)


@pytest.mark.parametrize("ell", ELLS)
def test_every_point_fault_from_bytes(gpu, generated, bad, ell):
    _, _, recs = bad
    wire = generated[ell][2]
    encodings = dict(recs)
    encodings["infinity flag with stray low bits"] = bytes([0xC0]) + bytes(46) + b"\x01"
    encodings["infinity flag with the sign flag"] = bytes([0xE0]) + bytes(47)
    encodings["uncompressed form"] = bytes([wire[0] & 0x7F]) + wire[1:48]
    encodings["uncompressed infinity"] = bytes([0x40]) + bytes(47)
    encodings["x >= p"] = bytes([0x9F]) + b"\xff" * 47
    for at, (field, index) in zip([0, ell - 1, ell, ell + 3, ell + 4, ell + 5, ell + 6, ell + 7, ell + 8], places(ell)):
        for what, rec in encodings.items():
            reason = what if isinstance(what, int) else BAD_ENCODING
            data = wire[:48 * at] + rec + wire[48 * (at + 1):]
            if reason == INFINITY and field >= 5:
                expect_fault(gpu, lambda: gpu.CRS.from_bytes(data), field, 0, gpu.CRS_SUM_MISMATCH)
                continue
            text = "not a valid compressed encoding" if reason == BAD_ENCODING else None
            expect_fault(gpu, lambda: gpu.CRS.from_bytes(data), field, index, reason, text)


@pytest.mark.parametrize("ell", ELLS)
def test_duplicates(gpu, generated, oracle, ell):
    base = generated[ell][1]
    dup = gpu.CRS_DUPLICATE
    pts = copy_points(base)
    pts["Gs"][ell - 1] = pts["Gs"][0]
    expect_fault(gpu, lambda: gpu.CRS.from_points(**pts), 0, ell - 1, dup, "equal to Gs[0]")
    pts = copy_points(base)
    pts["Hs"][2] = pts["Gs"][1]
    expect_fault(gpu, lambda: gpu.CRS.from_points(**pts), 1, 2, dup, "equal to Gs[1]")
    pts = copy_points(base)
    pts["Gt"] = pts["H"].copy()
    expect_fault(gpu, lambda: gpu.CRS.from_points(**pts), 3, 0, dup, "equal to H")
    pts = copy_points(base)
    H = oracle.jac_from_mont_limbs([int(v) for v in base["H"]])
    pts["Gu"] = under_z(oracle, H, draw("dup/z", oracle.P - 1) + 1)
    assert not (pts["Gu"] == pts["H"]).all()
    expect_fault(gpu, lambda: gpu.CRS.from_points(**pts), 4, 0, dup, "equal to H")
    # the same relations in bytes
    wire = generated[ell][2]
    data = wire[:48 * (ell - 1)] + wire[:48] + wire[48 * ell:]
    expect_fault(gpu, lambda: gpu.CRS.from_bytes(data), 0, ell - 1, dup, "equal to Gs[0]")
    data = wire[:48 * (ell + 5)] + wire[48 * (ell + 4):48 * (ell + 5)] + wire[48 * (ell + 6):]
    expect_fault(gpu, lambda: gpu.CRS.from_bytes(data), 3, 0, dup, "equal to H")


@pytest.mark.parametrize("ell", ELLS)
def test_sums(gpu, generated, oracle, ell):
    base = generated[ell][1]
    mismatch = gpu.CRS_SUM_MISMATCH
    gsum = oracle.affine_from_mont_limbs([int(v) for v in base["Gsum"]])
    pts = copy_points(base)
    pts["Gsum"] = np.array(oracle.affine_to_mont_limbs(oracle.add(gsum, oracle.G1)), dtype=np.uint64)     # off by G
    expect_fault(gpu, lambda: gpu.CRS.from_points(**pts), 5, 0, mismatch, "not the sum of Gs")
    pts = copy_points(base)
    pts["Gsum"], pts["Hsum"] = pts["Hsum"], pts["Gsum"]
    expect_fault(gpu, lambda: gpu.CRS.from_points(**pts), 5, 0, mismatch, "not the sum of Gs")
    pts = copy_points(base)
    pts["Hsum"] = pts["Gsum"].copy()
    expect_fault(gpu, lambda: gpu.CRS.from_points(**pts), 6, 0, mismatch, "not the sum of Hs")
    # a Gsum at infinity is accepted exactly when the Gs sum to infinity: Gs = {P, Q, ..., -(P + Q + ...)}
    pts = copy_points(base)
    pts["Gsum"] = np.zeros(12, dtype=np.uint64)
    expect_fault(gpu, lambda: gpu.CRS.from_points(**pts), 5, 0, mismatch)
    last = oracle.affine_from_mont_limbs([int(v) for v in base["Gs"][ell - 1]])
    cancel = oracle.neg(oracle.add(gsum, oracle.neg(last)))                  # minus the sum of the others
    pts["Gs"][ell - 1] = np.array(oracle.affine_to_mont_limbs(cancel), dtype=np.uint64)
    crs = gpu.CRS.from_points(**pts)
    assert same_points(crs.points(), pts) and crs.to_bytes()[48 * (ell + 7):48 * (ell + 8)] == oracle.compress(oracle.INF)
    assert gpu.CRS.from_bytes(crs.to_bytes()).to_bytes() == crs.to_bytes()
    pts["Gsum"] = base["Gsum"].copy()                                        # ... and then nothing else is
    expect_fault(gpu, lambda: gpu.CRS.from_points(**pts), 5, 0, mismatch)


@pytest.mark.parametrize("ell", ELLS)
def test_the_first_fault_in_wire_order_and_points_before_duplicates_before_sums(gpu, generated, bad, ell):
    affine, jac, recs = bad
    base, wire = generated[ell][1], generated[ell][2]
    pts = copy_points(base)                                     # two point faults: the earlier one in wire order
    pts["Hs"][0] = affine[NOT_ON_CURVE]
    pts["Gs"][ell - 1] = affine[NOT_IN_SUBGROUP]
    expect_fault(gpu, lambda: gpu.CRS.from_points(**pts), 0, ell - 1, NOT_IN_SUBGROUP)
    pts = copy_points(base)                                     # a Jacobian field lies BEFORE the sums, after Hs
    pts["Gsum"] = affine[BAD_ENCODING]
    pts["Gt"] = jac[NOT_ON_CURVE]
    expect_fault(gpu, lambda: gpu.CRS.from_points(**pts), 3, 0, NOT_ON_CURVE)
    pts["Hs"][3] = affine[NOT_IN_SUBGROUP]
    expect_fault(gpu, lambda: gpu.CRS.from_points(**pts), 1, 3, NOT_IN_SUBGROUP)
    pts = copy_points(base)                                     # a point fault late in wire order beats an early duplicate
    pts["Gs"][1] = pts["Gs"][0]
    pts["Hsum"] = affine[NOT_IN_SUBGROUP]
    expect_fault(gpu, lambda: gpu.CRS.from_points(**pts), 6, 0, NOT_IN_SUBGROUP)
    pts["Hsum"] = base["Hsum"].copy()                           # the duplicate (which also breaks Gsum) beats the sum
    expect_fault(gpu, lambda: gpu.CRS.from_points(**pts), 0, 1, gpu.CRS_DUPLICATE, "equal to Gs[0]")
    pts = copy_points(base)                                     # two duplicates: the earlier LATER point
    pts["Gu"] = pts["Gt"].copy()
    pts["Hs"][1] = pts["Gs"][ell - 1]
    expect_fault(gpu, lambda: gpu.CRS.from_points(**pts), 1, 1, gpu.CRS_DUPLICATE, "equal to Gs[%d]" % (ell - 1))
    # bytes: the same order
    data = wire[:48 * (ell + 8)] + recs[NOT_IN_SUBGROUP]
    data = data[:48] + data[:48] + data[96:]
    expect_fault(gpu, lambda: gpu.CRS.from_bytes(data), 6, 0, NOT_IN_SUBGROUP)
    data = wire[:48] + wire[:48] + wire[96:]
    expect_fault(gpu, lambda: gpu.CRS.from_bytes(data), 0, 1, gpu.CRS_DUPLICATE)


# ---------------------------------------------------------------------------------------------------------------------
# routes, threads, wall time
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ell", ELLS)
def test_the_validated_import_checks_on_the_device_and_the_trusted_one_does_not(gpu, generated, ell):
    pts = generated[ell][1]
    s0 = gpu.stat_check_paths()
    trusted = gpu.CRS.from_points(**pts, flags=gpu.CRS_TRUSTED)
    s1 = gpu.stat_check_paths()
    validated = gpu.CRS.from_points(**pts)
    s2 = gpu.stat_check_paths()
    assert s1 == s0                                             # TRUSTED: no counter moves
    assert s2["first"] - s1["first"] == 2 and s2["beside"] == s1["beside"]      # one affine check, one Jacobian check
    assert trusted.to_bytes() == validated.to_bytes() == generated[ell][2]


def test_two_imports_beside_an_msm_on_three_threads(gpu, generated, coracle, oracle):
    ell = 124
    _, pts, wire = generated[ell]
    n = 4096
    kq = oracle.Rand(1).get_frs(2)
    mpts = coracle.points_walk(kq[0], kq[1], n)
    sc = np.random.default_rng(7).integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    sc[:, 3] &= np.uint64((1 << 62) - 1)
    want = coracle.msm_pippenger(mpts, sc, threads=4)
    results, errors = {}, []

    def run(name, fn):
        try:
            results[name] = [fn() for _ in range(4)]
        except Exception as e:                                  # noqa: BLE001 -- reported below, on the main thread
            errors.append((name, repr(e)))

    threads = [threading.Thread(target=run, args=("points", lambda: gpu.CRS.from_points(**pts).to_bytes())),
               threading.Thread(target=run, args=("bytes", lambda: gpu.CRS.from_bytes(wire).to_bytes())),
               threading.Thread(target=run, args=("msm", lambda: gpu.msm_g1(mpts, sc)))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert results["points"] == [wire] * 4 and results["bytes"] == [wire] * 4
    assert all((r == want).all() for r in results["msm"])


def test_wall_time_of_one_validated_import_at_124(gpu, generated):
    """Prints the figure DESIGN.md quotes; no timing gate."""
    _, pts, wire = generated[124]

    def median_ms(fn):
        for _ in range(2):
            fn()
        took = []
        for _ in range(7):
            t0 = time.perf_counter()
            fn()
            took.append((time.perf_counter() - t0) * 1e3)
        return sorted(took)[3]

    a = median_ms(lambda: gpu.CRS.from_points(**pts))
    b = median_ms(lambda: gpu.CRS.from_bytes(wire))
    c = median_ms(lambda: gpu.CRS.from_points(**pts, flags=gpu.CRS_TRUSTED))
    print("CRS import at ell = 124, median of 7 after 2 warm-ups: validated from_points %.3f ms, from_bytes %.3f ms, "
          "TRUSTED from_points %.3f ms" % (a, b, c))
