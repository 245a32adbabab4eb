"""The rule of the Jacobian membership check (curdle_g1_check_jac_batch) stated with big integers and oracle/py's
group law (tests/jac_check_cases.py) against what its cases were built to be, and the C-ABI surface of the check and of
the checked batch verifier as far as it shows without a device: symbols, prototypes, argument refusals, the empty call,
the loud failure where no GPU is visible."""
import ctypes as C
import os
import re
from collections import Counter

import numpy as np
import pytest

import jac_check_cases as jc
from conftest import ROOT

NEW = ("curdle_g1_check_jac_batch", "curdle_g1_check_jac_batch_device", "curdle_verify_batch_checked", "curdle_stat_batch_checked")


@pytest.fixture(scope="module")
def cs():
    return jc.cases()


@pytest.fixture(scope="module")
def model(cs):
    return (np.array([jc.model_status(w.tolist(), True) for w in cs.points], dtype=np.uint8),
            np.array([jc.model_status(w.tolist(), False) for w in cs.points], dtype=np.uint8))


def test_scaled_points_keep_the_status_of_the_affine_point(cs, model):
    """(x Z^2, y Z^3, Z) for Z = 1, p - 1 and random: the rule gives what the fixture says of (x, y), with and without
    the subgroup test; points of other curves stay off the curve under every Z."""
    rows = np.nonzero(cs.affine_row >= 0)[0]
    assert len(rows) == 3 * len(cs.fixture["points"]) == 3 * 555
    assert Counter(cs.kind[i] for i in rows) == {"scaled_one": 555, "scaled_minus_one": 555, "scaled_random": 555}
    assert (model[0][rows] == cs.fixture["status_subgroup"][cs.affine_row[rows]]).all()
    assert (model[1][rows] == cs.fixture["status_no_subgroup"][cs.affine_row[rows]]).all()
    fam = cs.fixture["family"][cs.affine_row[rows]]
    assert (model[0][rows][fam == b"other_curve"] == jc.NOT_ON_CURVE).all() and (fam == b"other_curve").sum() == 3 * 128


def test_z_zero_decides_first(cs, model):
    rows = [i for i in range(cs.n) if cs.kind[i] == "z_zero"]
    assert len(rows) >= 5
    assert any(jc.raw(cs.points[i][:6]) >= jc.o.P and jc.raw(cs.points[i][6:12]) >= jc.o.P for i in rows)
    assert all(model[0][i] == model[1][i] == jc.INFINITY for i in rows)


def test_every_coordinate_out_of_range(cs, model):
    for c in "XYZ":
        rows = [i for i in range(cs.n) if cs.kind[i] == "range_" + c]
        vals = {jc.raw(cs.points[i][6 * "XYZ".index(c):6 * "XYZ".index(c) + 6]) for i in rows}
        assert vals == {jc.o.P, jc.o.P + 1, jc.TOP}
        assert all(model[0][i] == model[1][i] == jc.BAD_ENCODING for i in rows)


def test_wrong_scaling_is_off_the_curve(cs, model):
    rows = [i for i in range(cs.n) if cs.kind[i] == "wrong_scaling"]
    assert len(rows) == 4 and all(model[0][i] == model[1][i] == jc.NOT_ON_CURVE for i in rows)


def test_the_model_agrees_with_what_every_case_was_built_to_be(cs, model):
    assert (model[0] == cs.want_sub).all() and (model[1] == cs.want_nosub).all()


def test_every_status_occurs(cs, model):
    assert set(model[0].tolist()) == {0, 1, 2, 3, 4} and set(model[1].tolist()) == {0, 1, 2, 3}
    for kind, i in cs.first.items():
        assert cs.tiled(7, kind)[-1] == i
    assert [int(model[0][cs.first[k]]) for k in ("torsion", "other_curve", "infinity", "g1", "range")] == [4, 3, 1, 0, 2]


def test_normalised_points_are_the_fixture_points(cs):
    """The affine form of every scaled case is the fixture point it came from: what the GPU test compares the affine
    kernel on."""
    rows, aff = cs.normalised()
    src = cs.affine_row[rows]
    keep = src >= 0
    assert keep.sum() >= 3 * 500
    assert (aff[keep] == cs.fixture["points"][src[keep]]).all()


# ---------------------------------------------------------------------------------------------------------------
# the surface
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib(cm):
    lib = C.CDLL(cm.LIB_PATH)
    vp = C.c_void_p
    lib.curdle_g1_check_jac_batch.argtypes = [vp, C.c_size_t, C.c_int, vp]
    lib.curdle_g1_check_jac_batch_device.argtypes = [vp, C.c_size_t, C.c_int, vp, vp]
    lib.curdle_verify_batch_checked.argtypes = [vp, C.c_size_t, vp, vp, vp, vp, vp, vp, C.c_size_t, vp, vp, C.c_int, vp, vp]
    lib.curdle_stat_batch_checked.argtypes = [vp]
    return lib


def test_the_new_symbols_are_exported_and_bound(cm, lib):
    for name in NEW:
        assert hasattr(lib, name) and name in cm.SYMBOLS, name
    for name in ("g1_check_jac_batch", "g1_check_jac_batch_device", "verify_batch_checked", "stat_batch_checked"):
        assert callable(getattr(cm, name)), name


def prototype(header, name):
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, header)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_prototypes_match_the_header(cm):
    with open(os.path.join(ROOT, "include", "curdle_msm.h")) as f:
        header = f.read()
    assert prototype(header, "curdle_g1_check_jac_batch") == \
        ["const uint64_t* jac_points", "size_t n", "int subgroup_check", "uint8_t* status"]
    assert prototype(header, "curdle_g1_check_jac_batch_device") == \
        ["const void* d_jac_points", "size_t n", "int subgroup_check", "uint8_t* status", "void* stream"]
    plain, checked = prototype(header, "curdle_verify_batch"), prototype(header, "curdle_verify_batch_checked")
    assert checked == plain + ["curdle_point_fault* faults"] and plain[-1] == "int* oks"
    assert prototype(header, "curdle_stat_batch_checked") == ["unsigned long long out[3]"]
    m = re.search(r"typedef struct \{([^}]*)\} curdle_point_fault;", header)
    fields = re.findall(r"(uint\d+_t)\s+(\w+);", m.group(1))
    assert fields == [("uint8_t", "code"), ("uint8_t", "vector"), ("uint16_t", "pad"), ("uint32_t", "index")]
    assert cm.POINT_FAULT.itemsize == 8 and [cm.POINT_FAULT.fields[n][1] for n in ("code", "vector", "pad", "index")] == [0, 1, 2, 4]
    # the sentences this replaces are gone
    assert "is checked by its caller" not in header
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        assert "has no checked form" not in f.read()


def test_empty_check_is_ok_without_a_device(cm, lib):
    st = cm.g1_check_jac_batch(np.zeros((0, 18), np.uint64))
    assert st.shape == (0,) and st.dtype == np.uint8
    assert cm.g1_check_jac_batch(np.zeros((0, 18), np.uint64), subgroup_check=False).shape == (0,)
    assert cm.g1_check_jac_batch_device(0, 0).shape == (0,)
    assert lib.curdle_g1_check_jac_batch(None, 0, 1, None) == cm.OK
    assert lib.curdle_g1_check_jac_batch_device(None, 0, 1, None, None) == cm.OK


def test_null_pointers_and_oversized_batches_are_einval(cm, lib):
    pts = np.zeros((2, 18), np.uint64)
    st = np.zeros(2, np.uint8)
    p, s = pts.ctypes.data_as(C.c_void_p), st.ctypes.data_as(C.c_void_p)
    for sub in (0, 1):
        assert lib.curdle_g1_check_jac_batch(None, 2, sub, s) == cm.EINVAL and "null argument" in cm.last_error()
        assert lib.curdle_g1_check_jac_batch(p, 2, sub, None) == cm.EINVAL
        assert lib.curdle_g1_check_jac_batch_device(None, 2, sub, s, None) == cm.EINVAL
        assert lib.curdle_g1_check_jac_batch_device(p, 2, sub, None, None) == cm.EINVAL
        # refused on the count alone, before anything is read: the two points stand in for 2^27 + 1
        assert lib.curdle_g1_check_jac_batch(p, (1 << 27) + 1, sub, s) == cm.EINVAL and "2^27" in cm.last_error()
        assert lib.curdle_g1_check_jac_batch_device(p, (1 << 27) + 1, sub, s, None) == cm.EINVAL and "2^27" in cm.last_error()


def test_an_empty_checked_batch_is_ok_without_a_device(cm):
    rand = cm.Rand(3)
    crs = cm.CRS(4, rand)                                        # host only
    assert cm.verify_batch_checked(crs, [], [], [], [], [], [], rand) == ([], [])
    out = cm.stat_batch_checked()
    assert set(out) == {"batches", "rejected", "chunks"}


def test_checked_batch_refuses_null_arguments_and_leaves_no_verdict(cm, lib):
    rand = cm.Rand(3)
    crs = cm.CRS(4, rand)
    oks = (C.c_int * 2)(7, 7)
    faults = np.zeros(2, dtype=cm.POINT_FAULT)
    a = np.zeros((4, 12), np.uint64).ctypes.data_as(C.c_void_p)
    f = faults.ctypes.data_as(C.c_void_p)
    assert lib.curdle_verify_batch_checked(None, 2, a, a, a, a, a, a, 4, a, rand._h, 2, oks, f) == cm.EINVAL
    assert "null argument" in cm.last_error()
    assert list(oks) == [0, 0] and faults["code"].tolist() == [0xff, 0xff]
    assert lib.curdle_verify_batch_checked(crs._h, 2, a, a, a, a, a, a, 4, a, rand._h, 2, None, f) == cm.EINVAL
    assert lib.curdle_verify_batch_checked(crs._h, 2, a, a, a, None, a, a, 4, a, rand._h, 2, oks, None) == cm.EINVAL
    oks[0] = 5
    assert lib.curdle_verify_batch_checked(crs._h, 2, a, a, a, a, a, a, 5, a, rand._h, 2, oks, f) == cm.EINVAL
    assert "ell does not match the CRS" in cm.last_error() and list(oks) == [0, 0]
    assert lib.curdle_stat_batch_checked(None) == cm.EINVAL


def test_no_device_means_loud_failure_not_fallback(cm, oracle):
    if cm.device_available():
        pytest.skip("a device is visible")
    pts = np.array([oracle.jac_to_mont_limbs(oracle.G1)], dtype=np.uint64)
    for sub in (True, False):
        with pytest.raises(cm.CurdleError) as e:
            cm.g1_check_jac_batch(pts, sub)
        assert e.value.code == cm.ENODEV
    with pytest.raises(cm.CurdleError) as e:
        cm.g1_check_jac_batch_device(pts.ctypes.data, 1)
    assert e.value.code == cm.ENODEV
    # the checked batch starts with the check: no device, no verdict
    rand = cm.Rand(3)
    crs = cm.CRS(4, rand)
    inst = np.repeat(np.array([oracle.affine_to_mont_limbs(oracle.G1)], dtype=np.uint64), 4, axis=0)
    with pytest.raises(cm.CurdleError) as e:
        cm.verify_batch_checked(crs, [b"\x00" * 64] * 2, [inst] * 2, [inst] * 2, [inst] * 2, [inst] * 2, [pts[0]] * 2, rand)
    assert e.value.code == cm.ENODEV
