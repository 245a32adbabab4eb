"""The C-ABI surface of the membership check for points in memory (curdle_g1_check_batch, its device form and
the checked verifier entry points), as far as it can be seen without a device: argument validation, the empty
call, and the loud failure where no GPU is visible -- there is no CPU fallback."""
import ctypes as C

import numpy as np
import pytest

NEW = ("curdle_g1_check_batch", "curdle_g1_check_batch_device", "curdle_verify_checked", "curdle_verify_proof_checked",
       "curdle_stat_check_paths")


@pytest.fixture(scope="module")
def lib(cm):
    lib = C.CDLL(cm.LIB_PATH)
    vp = C.c_void_p
    lib.curdle_g1_check_batch.argtypes = [vp, C.c_size_t, C.c_int, vp]
    lib.curdle_g1_check_batch_device.argtypes = [vp, C.c_size_t, C.c_int, vp, vp]
    lib.curdle_verify_checked.argtypes = [vp, vp, C.c_size_t, vp, vp, vp, vp, C.c_size_t, vp, vp, vp]
    lib.curdle_verify_proof_checked.argtypes = [vp, vp, vp, vp, vp, vp, C.c_size_t, vp, vp, vp]
    return lib


def test_the_new_symbols_are_exported_and_bound(cm, lib):
    for name in NEW:
        assert hasattr(lib, name) and name in cm.SYMBOLS, name
    for name in ("g1_check_batch", "g1_check_batch_device", "verify_checked", "verify_proof_checked"):
        assert callable(getattr(cm, name)), name


def test_empty_check_is_ok_without_a_device(cm, lib):
    st = cm.g1_check_batch(np.zeros((0, 12), np.uint64))
    assert st.shape == (0,) and st.dtype == np.uint8
    assert cm.g1_check_batch(np.zeros((0, 12), np.uint64), subgroup_check=False).shape == (0,)
    assert cm.g1_check_batch_device(0, 0).shape == (0,)
    # n = 0 reads and writes nothing: null pointers are fine
    assert lib.curdle_g1_check_batch(None, 0, 1, None) == cm.OK
    assert lib.curdle_g1_check_batch_device(None, 0, 1, None, None) == cm.OK


def test_null_pointers_and_oversized_batches_are_einval(cm, lib):
    pts = np.zeros((2, 12), np.uint64)
    st = np.zeros(2, np.uint8)
    p, s = pts.ctypes.data_as(C.c_void_p), st.ctypes.data_as(C.c_void_p)
    for sub in (0, 1):
        assert lib.curdle_g1_check_batch(None, 2, sub, s) == cm.EINVAL and "null argument" in cm.last_error()
        assert lib.curdle_g1_check_batch(p, 2, sub, None) == cm.EINVAL
        assert lib.curdle_g1_check_batch_device(None, 2, sub, s, None) == cm.EINVAL
        assert lib.curdle_g1_check_batch_device(p, 2, sub, None, None) == cm.EINVAL
        # refused on the count alone, before anything is read: the two points stand in for 2^27 + 1
        assert lib.curdle_g1_check_batch(p, (1 << 27) + 1, sub, s) == cm.EINVAL and "2^27" in cm.last_error()
        assert lib.curdle_g1_check_batch_device(p, (1 << 27) + 1, sub, s, None) == cm.EINVAL and "2^27" in cm.last_error()


def test_checked_verifier_refuses_null_arguments(cm, lib):
    ok = C.c_int(7)
    a = np.zeros((1, 12), np.uint64).ctypes.data_as(C.c_void_p)
    assert lib.curdle_verify_checked(None, a, 1, a, a, a, a, 1, a, a, C.byref(ok)) == cm.EINVAL
    assert "null argument" in cm.last_error()
    assert lib.curdle_verify_proof_checked(None, a, a, a, a, a, 1, a, a, C.byref(ok)) == cm.EINVAL
    assert lib.curdle_verify_checked(a, a, 1, a, a, a, a, 1, a, a, None) == cm.EINVAL


def test_checked_verifier_refuses_an_ell_that_is_not_the_crs(cm, lib):
    rand = cm.Rand(3)
    crs = cm.CRS(4, rand)                                        # host only
    z = np.zeros((5, 12), np.uint64)
    with pytest.raises(cm.CurdleError) as e:
        cm.verify_checked(_with_ell(crs, 5), b"\x00" * 8, z, z, z, z, np.zeros(18, np.uint64), rand)
    assert e.value.code == cm.EINVAL and "ell does not match the CRS" in e.value.msg


class _with_ell:
    """A CRS handle presented with another ell: what a caller with arrays of the wrong length passes."""

    def __init__(self, crs, ell):
        self._h, self.ell, self._keep = crs._h, ell, crs


def test_no_device_means_loud_failure_not_fallback(cm, oracle):
    if cm.device_available():
        pytest.skip("a device is visible")
    pts = np.array([oracle.affine_to_mont_limbs(oracle.G1)], dtype=np.uint64)
    for sub in (True, False):
        with pytest.raises(cm.CurdleError) as e:
            cm.g1_check_batch(pts, sub)
        assert e.value.code == cm.ENODEV
    with pytest.raises(cm.CurdleError) as e:
        cm.g1_check_batch_device(pts.ctypes.data, 1)
    assert e.value.code == cm.ENODEV
    # the checked verifier starts with the check: no device, no verdict -- not even for an instance a host could judge
    rand = cm.Rand(3)
    crs = cm.CRS(4, rand)
    inst = np.repeat(pts, 4, axis=0)
    M = np.array(oracle.jac_to_mont_limbs(oracle.G1), dtype=np.uint64)
    with pytest.raises(cm.CurdleError) as e:
        cm.verify_checked(crs, b"\x00" * 64, inst, inst, inst, inst, M, rand)
    assert e.value.code == cm.ENODEV
