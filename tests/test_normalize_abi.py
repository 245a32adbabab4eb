"""The batched G1 normalisation and the resident scalar-multiplication batch at the C ABI, without a GPU:
curdle_g1_normalize_batch / _device, curdle_g1_scalar_mul_batch_device and curdle_stat_normalize exist as
include/curdle_msm.h declares them, an empty call needs no device, and everything malformed is refused before any
device work (the refused calls below pass pointers that must never be read: they name no memory)."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("curdle_g1_normalize_batch", "curdle_g1_normalize_batch_device", "curdle_g1_scalar_mul_batch_device",
         "curdle_stat_normalize")
vp = C.c_void_p
FAKE = 0x7000_0000_1000          # a multiple of 16 that names no memory: a refused call never reads it


def _f(cm, name, *argtypes):
    f = getattr(cm._lib, name)
    f.restype = C.c_int
    f.argtypes = list(argtypes)
    return f


def _fns(cm):
    return (_f(cm, "curdle_g1_normalize_batch", vp, C.c_int, C.c_size_t, vp),
            _f(cm, "curdle_g1_normalize_batch_device", vp, C.c_int, C.c_size_t, vp, vp),
            _f(cm, "curdle_g1_scalar_mul_batch_device", vp, vp, C.c_size_t, vp, C.c_size_t, vp, vp))


def test_symbols_and_prototypes(cm):
    header = open(os.path.join(ROOT, "include", "curdle_msm.h")).read()
    flat = re.sub(r"\s+", " ", header)
    for name in NAMES:
        assert hasattr(cm._lib, name) and name in cm.SYMBOLS, name
    for proto in (
            "#define CURDLE_G1_FORM_JAC 0",
            "#define CURDLE_G1_FORM_XYZZ 1",
            "int curdle_g1_normalize_batch(const uint64_t* points, int form, size_t n, uint64_t* out_affine);",
            "int curdle_g1_normalize_batch_device(const void* d_points, int form, size_t n, void* d_out_affine, void* stream);",
            "int curdle_g1_scalar_mul_batch_device(const void* d_points, const void* d_scalars, size_t n_scalars, "
            "const void* d_addends, size_t n, void* d_out_affine, void* stream);",
            "int curdle_stat_normalize(unsigned long long out[2]);"):
        assert proto in flat, proto
    for name in ("g1_normalize_batch", "g1_normalize_batch_device", "g1_scalar_mul_batch_device", "stat_normalize"):
        assert callable(getattr(cm, name)), name
    assert (cm.G1_FORM_JAC, cm.G1_FORM_XYZZ) == (0, 1)
    assert "BatchJacobianToAffineG1" in header


def test_empty_calls_need_no_device_and_write_nothing(cm):
    host, dev, mul = _fns(cm)
    before = cm.stat_normalize()
    pts = np.full(24, 7, dtype=np.uint64)
    out = np.full(12, 77, dtype=np.uint64)
    for form in (0, 1):
        assert host(pts.ctypes.data, form, 0, out.ctypes.data) == cm.OK
        assert host(None, form, 0, None) == cm.OK
        assert dev(FAKE, form, 0, FAKE, None) == cm.OK
        assert dev(None, form, 0, None, None) == cm.OK
    assert mul(FAKE, FAKE, 1, FAKE, 0, FAKE, None) == cm.OK
    assert mul(None, None, 0, None, 0, None, None) == cm.OK
    assert (out == 77).all()
    assert cm.g1_normalize_batch(np.zeros((0, 18), dtype=np.uint64)).shape == (0, 12)
    assert cm.g1_normalize_batch(np.zeros((0, 24), dtype=np.uint64)).shape == (0, 12)
    cm.g1_normalize_batch_device(0, cm.G1_FORM_XYZZ, 0, 0)
    cm.g1_scalar_mul_batch_device(0, 0, 0, 0, 0, 0)
    assert cm.stat_normalize() == before


def test_refusals_happen_before_device_work(cm):
    host, dev, mul = _fns(cm)
    before = cm.stat_normalize()
    pts = np.zeros(48, dtype=np.uint64)
    out = np.full(24, 77, dtype=np.uint64)
    # a null pointer
    assert host(None, 0, 2, out.ctypes.data) == cm.EINVAL and "null argument" in cm.last_error()
    assert host(pts.ctypes.data, 1, 2, None) == cm.EINVAL
    assert dev(None, 0, 2, FAKE, None) == cm.EINVAL
    assert dev(FAKE, 1, 2, None, None) == cm.EINVAL
    assert mul(None, FAKE, 2, None, 2, FAKE, None) == cm.EINVAL
    assert mul(FAKE, None, 2, None, 2, FAKE, None) == cm.EINVAL
    assert mul(FAKE, FAKE, 2, None, 2, None, None) == cm.EINVAL and "null argument" in cm.last_error()
    # an unknown form
    for form in (-1, 2, 7):
        assert host(pts.ctypes.data, form, 2, out.ctypes.data) == cm.EINVAL and "form" in cm.last_error()
        assert dev(FAKE, form, 2, FAKE, None) == cm.EINVAL and "form" in cm.last_error()
    # refused by the count alone: nothing behind the pointers is read
    big = (1 << 24) + 1
    assert host(pts.ctypes.data, 0, big, out.ctypes.data) == cm.EINVAL and "2^24" in cm.last_error()
    assert dev(FAKE, 1, big, FAKE, None) == cm.EINVAL and "2^24" in cm.last_error()
    assert mul(FAKE, FAKE, 1, None, big, FAKE, None) == cm.EINVAL and "2^24" in cm.last_error()
    # a device pointer that is not a multiple of 16
    for off in (1, 4, 8):
        assert dev(FAKE + off, 0, 2, FAKE, None) == cm.EINVAL and "multiples of 16" in cm.last_error()
        assert dev(FAKE, 1, 2, FAKE + off, None) == cm.EINVAL
        for hole in range(4):
            a = [FAKE + (off if j == hole else 0) for j in range(4)]
            assert mul(a[0], a[1], 2, a[2], 2, a[3], None) == cm.EINVAL and "multiples of 16" in cm.last_error()
    # n_scalars neither n nor 1
    for ns in (0, 2, 4):
        assert mul(FAKE, FAKE, ns, None, 3, FAKE, None) == cm.EINVAL and "n_scalars" in cm.last_error()
    assert (out == 77).all()
    assert cm.stat_normalize() == before


def test_stat_normalize_refuses_null(cm):
    f = _f(cm, "curdle_stat_normalize", vp)
    assert f(None) == cm.EINVAL
    assert set(cm.stat_normalize()) == {"points", "groups"}
