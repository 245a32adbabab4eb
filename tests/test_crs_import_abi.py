"""curdle_crs_from_points / _from_bytes / _export_points / _to_bytes without a GPU: the four symbols and the two structs in
the header and in the binding, every refusal that comes before device work (in the header's order, *out NULL, the fault
left as it was), the TRUSTED import -- which needs no device -- round-tripped against a generated handle, a Jacobian H
with Z != 1 stored with Z = 1, the wire form against tests/golden/crs_ell4.bin (bytes the pure-Python oracle wrote), and
CURDLE_ENODEV, with no fallback, from the validated forms on a machine without a device."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest

from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = os.path.join(GOLDEN, "crs_ell4.bin")
HEADER = os.path.join(ROOT, "include", "curdle_msm.h")
SENTINEL = (0x5a5a, 0x1234567, 0x7e7e)


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("gen_crs_fixture", os.path.join(GOLDEN, "gen_crs_fixture.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def fixture_points(gen):
    return gen.crs_points()


def limbs_of(oracle, pts):
    Gs, Hs, H, Gt, Gu, Gsum, Hsum = pts
    aff = lambda ps: np.array([oracle.affine_to_mont_limbs(p) for p in ps], dtype=np.uint64)
    jac = lambda p: np.array(oracle.jac_to_mont_limbs(p), dtype=np.uint64)
    return {"Gs": aff(Gs), "Hs": aff(Hs), "H": jac(H), "Gt": jac(Gt), "Gu": jac(Gu), "Gsum": aff([Gsum])[0], "Hsum": aff([Hsum])[0]}


def same_points(a, b):
    return all((a[k] == b[k]).all() for k in ("Gs", "Hs", "H", "Gt", "Gu", "Gsum", "Hsum"))


def raw(cm):
    lib = C.CDLL(cm.LIB_PATH)
    lib.curdle_crs_from_points.argtypes = [C.POINTER(cm.CrsPoints), C.c_uint, C.POINTER(C.c_void_p), C.POINTER(cm.CrsFaultRecord)]
    lib.curdle_crs_from_bytes.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(cm.CrsFaultRecord)]
    lib.curdle_crs_export_points.argtypes = [C.c_void_p] * 8
    lib.curdle_crs_to_bytes.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.curdle_crs_free.argtypes = [C.c_void_p]
    for f in (lib.curdle_crs_from_points, lib.curdle_crs_from_bytes, lib.curdle_crs_export_points, lib.curdle_crs_to_bytes):
        f.restype = C.c_int
    lib.curdle_crs_free.restype = None
    return lib


def test_the_fixture_regenerates(gen):
    with open(FIXTURE, "rb") as f:
        committed = f.read()
    assert len(committed) == 624 == 48 * (gen.ELL + 9)
    assert gen.wire_bytes() == committed


def test_symbols_structs_and_prototypes(cm):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    flat = re.sub(r"\s+", " ", text)
    for proto in (
        "int curdle_crs_from_points(const curdle_crs_points* in, unsigned flags, curdle_crs** out, curdle_crs_fault* fault);",
        "int curdle_crs_from_bytes(const uint8_t* in, size_t len, curdle_crs** out, curdle_crs_fault* fault);",
        "int curdle_crs_export_points(const curdle_crs* crs, uint64_t* Gs, uint64_t* Hs, uint64_t H[18], uint64_t Gt[18], "
        "uint64_t Gu[18], uint64_t Gsum[12], uint64_t Hsum[12]);",
        "int curdle_crs_to_bytes(const curdle_crs* crs, uint8_t* out, size_t cap, size_t* len);",
        "typedef struct { const uint64_t* Gs; size_t ell; const uint64_t* Hs; const uint64_t* H; const uint64_t* Gt; "
        "const uint64_t* Gu; const uint64_t* Gsum; const uint64_t* Hsum; } curdle_crs_points;",
        "typedef struct { int field; size_t index; int reason; } curdle_crs_fault;",
    ):
        assert proto in flat, proto
    defines = dict(re.findall(r"#define (CURDLE_CRS_[A-Z_]+) (.+)", text))
    want = {"CURDLE_CRS_N_BLINDERS": "4", "CURDLE_CRS_MAX_ELL": "((size_t)1 << 20)", "CURDLE_CRS_TRUSTED": "1u", "CURDLE_CRS_GS": "0",
            "CURDLE_CRS_HS": "1", "CURDLE_CRS_H": "2", "CURDLE_CRS_GT": "3", "CURDLE_CRS_GU": "4", "CURDLE_CRS_GSUM": "5",
            "CURDLE_CRS_HSUM": "6", "CURDLE_CRS_DUPLICATE": "16", "CURDLE_CRS_SUM_MISMATCH": "17"}
    assert {k: v.strip() for k, v in defines.items()} == want
    # the header says whose the wire form is
    assert "THE REFERENCE DEFINES NO CRS SERIALISATION" in open(HEADER).read()
    lib = C.CDLL(cm.LIB_PATH)
    for name in ("curdle_crs_from_points", "curdle_crs_from_bytes", "curdle_crs_export_points", "curdle_crs_to_bytes"):
        assert hasattr(lib, name) and name in cm.SYMBOLS
    # the binding's mirrors of the two structs and of the constants
    assert [f[0] for f in cm.CrsPoints._fields_] == ["Gs", "ell", "Hs", "H", "Gt", "Gu", "Gsum", "Hsum"]
    assert C.sizeof(cm.CrsPoints) == 64 and cm.CrsPoints.ell.offset == 8
    assert [f[0] for f in cm.CrsFaultRecord._fields_] == ["field", "index", "reason"]
    assert C.sizeof(cm.CrsFaultRecord) == 24 and cm.CrsFaultRecord.index.offset == 8 and cm.CrsFaultRecord.reason.offset == 16
    assert (cm.CRS_N_BLINDERS, cm.CRS_MAX_ELL, cm.CRS_TRUSTED, cm.CRS_DUPLICATE, cm.CRS_SUM_MISMATCH) == (4, 1 << 20, 1, 16, 17)
    assert (cm.CRS_GS, cm.CRS_HS, cm.CRS_H, cm.CRS_GT, cm.CRS_GU, cm.CRS_GSUM, cm.CRS_HSUM) == tuple(range(7))
    assert issubclass(cm.CrsFault, cm.CurdleError)
    e = cm.CrsFault(cm.EINVAL, "Gs[17]: not in the prime-order subgroup", cm.CRS_GS, 17, 4)
    assert (e.code, e.field, e.index, e.reason) == (cm.EINVAL, 0, 17, 4) and "Gs[17]" in str(e)


def test_refusals_before_any_device_work(cm, oracle, fixture_points):
    """Null argument, then an undefined flag bit, then ell; for bytes null, then the length.  CURDLE_EINVAL, *out NULL, the
    fault untouched -- on any machine, since nothing here reaches a device."""
    lib = raw(cm)
    L = limbs_of(oracle, fixture_points)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    fields = ("Gs", "Hs", "H", "Gt", "Gu", "Gsum", "Hsum")

    def points(ell=4, **nulls):
        return cm.CrsPoints(*[(None if k in nulls else ptr(L[k])) if k != "ell" else ell
                              for k in ("Gs", "ell", "Hs", "H", "Gt", "Gu", "Gsum", "Hsum")])

    def refused(call, text):
        out, fault = C.c_void_p(0xdead0), cm.CrsFaultRecord(*SENTINEL)
        assert call(C.byref(out), C.byref(fault)) == cm.EINVAL
        assert out.value is None
        assert (fault.field, fault.index, fault.reason) == SENTINEL
        assert text in cm.last_error(), cm.last_error()

    for flags in (0, cm.CRS_TRUSTED, 2, 0x80000000):         # a null argument comes first, whatever the flags and ell
        refused(lambda o, f: lib.curdle_crs_from_points(None, flags, o, f), "null argument")
        for k in fields:
            refused(lambda o, f: lib.curdle_crs_from_points(C.byref(points(ell=0, **{k: True})), flags, o, f), "null argument")
        fault = cm.CrsFaultRecord(*SENTINEL)
        assert lib.curdle_crs_from_points(C.byref(points()), flags, None, C.byref(fault)) == cm.EINVAL
        assert "null argument" in cm.last_error() and (fault.field, fault.index, fault.reason) == SENTINEL
    for flags in (2, 3, 0x80000000, 0x80000001):             # then the flags, before ell is looked at
        for ell in (4, 0, cm.CRS_MAX_ELL + 1):
            refused(lambda o, f: lib.curdle_crs_from_points(C.byref(points(ell=ell)), flags, o, f), "unknown flag bits")
    for flags in (0, cm.CRS_TRUSTED):                        # then ell
        for ell in (0, cm.CRS_MAX_ELL + 1, 1 << 40):
            refused(lambda o, f: lib.curdle_crs_from_points(C.byref(points(ell=ell)), flags, o, f), "ell must be")

    ell = 4
    buf = np.zeros(48 * (ell + 9) + 1, dtype=np.uint8)
    refused(lambda o, f: lib.curdle_crs_from_bytes(None, 48 * (ell + 9), o, f), "null argument")
    fault = cm.CrsFaultRecord(*SENTINEL)
    assert lib.curdle_crs_from_bytes(ptr(buf), 48 * (ell + 9), None, C.byref(fault)) == cm.EINVAL
    assert (fault.field, fault.index, fault.reason) == SENTINEL
    # lengths: nothing, no Gs at all, one byte short or long, one point more than CURDLE_CRS_MAX_ELL allows (never read)
    for n in (0, 48 * 9, 48 * (ell + 9) - 1, 48 * (ell + 9) + 1, 48 * ((1 << 20) + 10)):
        refused(lambda o, f: lib.curdle_crs_from_bytes(ptr(buf), n, o, f), "is not 48 (ell + 9)")

    # export and to_bytes: null arguments
    crs = cm.CRS(4, cm.Rand(1))
    bufs = [np.zeros(48, dtype=np.uint64) for _ in range(7)]
    for i in range(8):
        args = [crs._h] + [ptr(b) for b in bufs]
        args[i] = None
        assert lib.curdle_crs_export_points(*args) == cm.EINVAL and "null argument" in cm.last_error()
    n = C.c_size_t(77)
    out = np.zeros(624, dtype=np.uint8)
    assert lib.curdle_crs_to_bytes(None, ptr(out), 624, C.byref(n)) == cm.EINVAL and n.value == 77
    assert lib.curdle_crs_to_bytes(crs._h, ptr(out), 624, None) == cm.EINVAL
    assert lib.curdle_crs_to_bytes(crs._h, None, 624, C.byref(n)) == cm.EINVAL and n.value == 624


@pytest.mark.parametrize("ell", [4, 124])
def test_trusted_round_trip_of_a_generated_crs(cm, ell):
    crs = cm.CRS(ell, cm.Rand(40 + ell))
    pts = crs.points()
    assert pts["Gs"].shape == (ell, 12) and pts["Gs"].any() and pts["Hsum"].any()
    again = cm.CRS.from_points(**pts, flags=cm.CRS_TRUSTED)
    assert again.ell == ell
    assert same_points(again.points(), pts)
    data = crs.to_bytes()
    assert len(data) == 48 * (ell + 9) and again.to_bytes() == data


def test_a_jacobian_point_with_any_z_is_stored_with_z_one(cm, oracle, fixture_points):
    L = limbs_of(oracle, fixture_points)
    H = fixture_points[2]
    one = [int(v) for v in oracle.jac_to_mont_limbs(H)[12:]]
    for j, z in enumerate((2, 0x1234567, oracle.P - 1)):
        scaled = (H[0] * z * z % oracle.P, H[1] * z * z * z % oracle.P, z)     # (X Z^2, Y Z^3, Z)
        given = dict(L)
        key = ("H", "Gt", "Gu")[j]
        given[key] = np.array(sum((oracle.fp_to_mont_limbs(c) for c in scaled), []), dtype=np.uint64)
        assert oracle.jac_from_mont_limbs([int(v) for v in given[key]]) == H
        got = cm.CRS.from_points(**given, flags=cm.CRS_TRUSTED).points()[key]
        assert [int(v) for v in got[12:]] == one
        assert [int(v) for v in got] == oracle.jac_to_mont_limbs(H)


def test_to_bytes_with_a_short_buffer_reports_the_needed_length(cm):
    lib = raw(cm)
    crs = cm.CRS(12, cm.Rand(3))
    need = 48 * (12 + 9)
    full = crs.to_bytes()
    for cap in (0, 1, need - 1):
        out = np.full(need, 0xee, dtype=np.uint8)
        n = C.c_size_t(0)
        assert lib.curdle_crs_to_bytes(crs._h, out.ctypes.data_as(C.c_void_p), cap, C.byref(n)) == cm.EINVAL
        assert n.value == need and (out == 0xee).all() and "too small" in cm.last_error()
    out = np.full(need + 5, 0xee, dtype=np.uint8)
    n = C.c_size_t(0)
    assert lib.curdle_crs_to_bytes(crs._h, out.ctypes.data_as(C.c_void_p), need + 5, C.byref(n)) == cm.OK
    assert n.value == need and bytes(out[:need]) == full and (out[need:] == 0xee).all()


def test_wire_form_of_the_oracle_points_is_the_fixture(cm, oracle, fixture_points):
    with open(FIXTURE, "rb") as f:
        committed = f.read()
    L = limbs_of(oracle, fixture_points)
    crs = cm.CRS.from_points(**L, flags=cm.CRS_TRUSTED)
    assert crs.ell == 4 and crs.to_bytes() == committed
    assert same_points(crs.points(), L)


def test_trusted_import_takes_an_inconsistent_gsum_as_given(cm, oracle, fixture_points):
    L = limbs_of(oracle, fixture_points)
    wrong = dict(L)
    wrong["Gsum"] = np.array(oracle.affine_to_mont_limbs(oracle.add(fixture_points[5], oracle.G1)), dtype=np.uint64)
    crs = cm.CRS.from_points(**wrong, flags=cm.CRS_TRUSTED)
    assert (crs.points()["Gsum"] == wrong["Gsum"]).all() and not (wrong["Gsum"] == L["Gsum"]).all()
    assert crs.to_bytes()[48 * 11:48 * 12] == oracle.compress(oracle.add(fixture_points[5], oracle.G1))
    # ... and infinity, (0, 0), as either sum
    wrong["Gsum"] = np.zeros(12, dtype=np.uint64)
    crs = cm.CRS.from_points(**wrong, flags=cm.CRS_TRUSTED)
    assert not crs.points()["Gsum"].any() and crs.to_bytes()[48 * 11:48 * 12] == oracle.compress(oracle.INF)


def test_the_c_example_compiles_as_c99_and_round_trips(cm, tmp_path):
    """examples/crs_from_c.c, built the way the other examples are: generate, export, import TRUSTED, the same bytes.  No
    device is needed for any of it."""
    import subprocess
    exe = str(tmp_path / "crs_from_c")
    pkg = os.path.join(ROOT, "go-curdleproofs_amd")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "crs_from_c.c"), "-L" + pkg, "-lcurdlemsm",
                           "-Wl,-rpath," + pkg, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    want = cm.CRS(8, cm.Rand(7)).to_bytes()
    assert r.stdout.strip() == "crs ell=8 bytes=%d first=%s same=1" % (len(want), want[:4].hex())


def test_validated_imports_need_a_device(cm, oracle, fixture_points):
    """No host fallback: without a device both validated forms answer CURDLE_ENODEV and hand out nothing."""
    if cm.device_available():
        pytest.skip("a device is visible")
    lib = raw(cm)
    L = limbs_of(oracle, fixture_points)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    pts = cm.CrsPoints(ptr(L["Gs"]), 4, ptr(L["Hs"]), ptr(L["H"]), ptr(L["Gt"]), ptr(L["Gu"]), ptr(L["Gsum"]), ptr(L["Hsum"]))
    out, fault = C.c_void_p(0xdead0), cm.CrsFaultRecord(*SENTINEL)
    assert lib.curdle_crs_from_points(C.byref(pts), 0, C.byref(out), C.byref(fault)) == cm.ENODEV
    assert out.value is None
    data = np.fromfile(FIXTURE, dtype=np.uint8)
    out = C.c_void_p(0xdead0)
    assert lib.curdle_crs_from_bytes(ptr(data), data.size, C.byref(out), C.byref(fault)) == cm.ENODEV
    assert out.value is None
    with pytest.raises(cm.CurdleError) as e:
        cm.CRS.from_bytes(data.tobytes())
    assert e.value.code == cm.ENODEV and not isinstance(e.value, cm.CrsFault)
    with pytest.raises(cm.CurdleError) as e:
        cm.CRS.from_points(**L)
    assert e.value.code == cm.ENODEV
