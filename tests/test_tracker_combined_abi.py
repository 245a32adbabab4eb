"""The combined tracker batch at the C ABI, without a GPU: the four entry points and the kernel timer of the
benchmark exist as include/curdle_msm.h declares them, the empty calls need no device and write nothing, and everything malformed is refused before any device
work -- null pointers, the seed among them, and more than one pass for the diagnostic that reads the scalars back."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("curdle_whisk_is_valid_tracker_proof_batch_combined", "curdle_whisk_is_valid_tracker_proof_batch_combined_device",
         "curdle_stat_tracker_combined", "curdle_whisk_tracker_combined_scalars", "curdle_tracker_combined_last_kernel_ms")
PASS = 1 << 16


def _fn(cm, name, *argtypes):
    f = getattr(cm._lib, name)
    f.restype = C.c_int
    f.argtypes = list(argtypes)
    return f


def _host(cm):
    return _fn(cm, NAMES[0], C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p)


def _dev(cm):
    return _fn(cm, NAMES[1], C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p)


def _scalars(cm):
    return _fn(cm, NAMES[3], C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p)


def _args(k):
    return (np.zeros(96 * k, np.uint8), np.zeros(48 * k, np.uint8), np.zeros(128 * k, np.uint8), np.zeros(32, np.uint8))


def test_symbols_and_prototypes(cm):
    header = open(os.path.join(ROOT, "include", "curdle_msm.h")).read()
    flat = re.sub(r"\s+", " ", header)
    for name in NAMES:
        assert hasattr(cm._lib, name) and name in cm.SYMBOLS, name
    assert ("int curdle_whisk_is_valid_tracker_proof_batch_combined(const uint8_t* trackers, const uint8_t* k_commitments, "
            "const uint8_t* proofs, size_t k, const uint8_t seed[32], int* results);") in flat
    assert ("int curdle_whisk_is_valid_tracker_proof_batch_combined_device(const void* d_trackers, "
            "const void* d_k_commitments, const void* d_proofs, size_t k, const uint8_t seed[32], int* results, "
            "void* stream);") in flat
    assert "int curdle_stat_tracker_combined(unsigned long long out[4]);" in flat
    assert ("int curdle_whisk_tracker_combined_scalars(const uint8_t* trackers, const uint8_t* k_commitments, "
            "const uint8_t* proofs, size_t k, const uint8_t seed[32], uint64_t* scalars_out, uint64_t g_out[4]);") in flat
    assert "int curdle_tracker_combined_last_kernel_ms(double* out);" in flat
    # what the header owes its reader: the seed's contract, the bound and the cost of a bad batch
    for phrase in ("unpredictable", "FRESH", "2^-128", "degree 1", "PLUS the chains"):
        assert phrase in header, phrase


def test_empty_calls_need_no_device_and_write_nothing(cm):
    host, dev, sc = _host(cm), _dev(cm), _scalars(cm)
    t, kc, p, seed = _args(1)
    res = np.full(4, 77, dtype=np.int32)
    out = np.full(20, 77, dtype=np.uint64)
    assert host(t.ctypes.data, kc.ctypes.data, p.ctypes.data, 0, seed.ctypes.data, res.ctypes.data) == cm.OK
    assert host(None, None, None, 0, None, None) == cm.OK
    assert dev(t.ctypes.data, kc.ctypes.data, p.ctypes.data, 0, seed.ctypes.data, res.ctypes.data, None) == cm.OK
    assert dev(None, None, None, 0, None, None, None) == cm.OK
    assert sc(None, None, None, 0, None, None, None) == cm.OK
    assert sc(t.ctypes.data, kc.ctypes.data, p.ctypes.data, 0, seed.ctypes.data, out.ctypes.data, None) == cm.OK
    assert (res == 77).all() and (out == 77).all()
    assert len(cm.whisk_is_valid_tracker_proof_batch_combined([], [], [], bytes(32))) == 0
    assert len(cm.whisk_is_valid_tracker_proof_batch_combined_device(0, 0, 0, 0, bytes(32))) == 0
    scalars, g = cm.whisk_tracker_combined_scalars([], [], [], bytes(32))
    assert scalars.shape == (0, 5, 4) and not g.any()


def test_null_pointers_are_einval_before_device_work(cm):
    host, dev, sc = _host(cm), _dev(cm), _scalars(cm)
    t, kc, p, seed = _args(2)
    res = np.full(2, 77, dtype=np.int32)
    ptrs = (t.ctypes.data, kc.ctypes.data, p.ctypes.data, 2, seed.ctypes.data)
    for hole in (0, 1, 2, 4):                                            # the three arrays and the seed
        a = [None if j == hole else v for j, v in enumerate(ptrs)]
        res[:] = 77
        assert host(*a, res.ctypes.data) == cm.EINVAL
        assert (res == cm.EINVAL).all()
        res[:] = 77
        assert dev(*a, res.ctypes.data, None) == cm.EINVAL
        assert (res == cm.EINVAL).all()
        out, g = np.zeros(40, np.uint64), np.zeros(4, np.uint64)
        assert sc(*a, out.ctypes.data, g.ctypes.data) == cm.EINVAL
    assert host(*ptrs, None) == cm.EINVAL
    assert dev(*ptrs, None, None) == cm.EINVAL
    out, g = np.zeros(40, np.uint64), np.zeros(4, np.uint64)
    assert sc(*ptrs, None, g.ctypes.data) == cm.EINVAL
    assert sc(*ptrs, out.ctypes.data, None) == cm.EINVAL


def test_scalars_of_more_than_one_pass_are_refused(cm):
    sc = _scalars(cm)
    k = PASS + 1
    t, kc, p, seed = _args(k)
    out, g = np.zeros(20 * k, np.uint64), np.zeros(4, np.uint64)
    assert sc(t.ctypes.data, kc.ctypes.data, p.ctypes.data, k, seed.ctypes.data, out.ctypes.data, g.ctypes.data) == cm.EINVAL
    assert not out.any()
    buf = C.create_string_buffer(256)
    cm._lib.curdle_last_error(buf, 256)
    assert b"one pass" in buf.value


def test_stat_refuses_null_and_names_its_counters(cm):
    f = _fn(cm, NAMES[2], C.c_void_p)
    assert f(None) == cm.EINVAL
    assert list(cm.stat_tracker_combined()) == ["settled", "fell_back", "accepted", "excluded"]
    assert _fn(cm, NAMES[4], C.c_void_p)(None) == cm.EINVAL
    assert cm.tracker_combined_last_kernel_ms() >= 0


def test_python_wrappers_check_the_seed(cm):
    import pytest
    with pytest.raises(ValueError):
        cm.whisk_is_valid_tracker_proof_batch_combined([], [], [], bytes(31))
    with pytest.raises(ValueError):
        cm.whisk_is_valid_tracker_proof_batch_combined_device(0, 0, 0, 0, bytes(33))
