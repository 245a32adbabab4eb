"""The flagged ownership search at the C ABI, without a GPU: curdle_whisk_find_own_trackers_ex / _device_ex and
curdle_stat_tracker_own_ct exist as include/curdle_msm.h declares them, an empty call needs no device, an unknown flag
bit is refused before anything else is looked at (and fills `owned` in the host form), whatever the calls without flags
refuse is refused the same way with the flag (the refused _device calls pass pointers that name no memory), and without
a device the flagged calls fail with CURDLE_ENODEV: no host fallback."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from test_normalize_abi import FAKE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("curdle_whisk_find_own_trackers_ex", "curdle_whisk_find_own_trackers_device_ex", "curdle_stat_tracker_own_ct")
vp = C.c_void_p
CT = 1
FLAGS = (0, CT)
BAD_FLAGS = (2, 3, 4, 0x80, 1 << 31, 0xFFFFFFFE, 0xFFFFFFFF)


def _f(cm, name, *argtypes):
    f = getattr(cm._lib, name)
    f.restype = C.c_int
    f.argtypes = list(argtypes)
    return f


def _fns(cm):
    return (_f(cm, "curdle_whisk_find_own_trackers_ex", vp, C.c_size_t, vp, C.c_size_t, vp, C.c_uint),
            _f(cm, "curdle_whisk_find_own_trackers_device_ex", vp, C.c_size_t, vp, C.c_size_t, vp, vp, C.c_uint))


def _stats(cm):
    return cm.stat_tracker_own_ct(), cm.stat_tracker_own(), cm.stat_g1_mul_ct(), cm.stat_normalize()


def test_symbols_and_prototypes(cm):
    header = open(os.path.join(ROOT, "include", "curdle_msm.h")).read()
    flat = re.sub(r"\s+", " ", header)
    for name in NAMES:
        assert hasattr(cm._lib, name) and name in cm.SYMBOLS, name
    for proto in (
            "#define CURDLE_TRACKER_OWN_CONSTANT_TIME 1u",
            "int curdle_whisk_find_own_trackers_ex(const uint8_t* trackers, size_t n, const uint64_t* ks, size_t m, "
            "uint8_t* owned, unsigned flags);",
            "int curdle_whisk_find_own_trackers_device_ex(const void* d_trackers, size_t n, const void* d_ks, size_t m, "
            "void* d_owned, void* stream, unsigned flags);",
            "int curdle_stat_tracker_own_ct(unsigned long long out[3]);"):
        assert proto in flat, proto
    assert cm.TRACKER_OWN_CONSTANT_TIME == CT
    assert set(cm.stat_tracker_own_ct()) == {"pairs", "launches", "bad"}
    for name in ("whisk_find_own_trackers", "whisk_find_own_trackers_device"):
        par = inspect.signature(getattr(cm, name)).parameters
        assert "flags" in par and par["flags"].default is None, name
    # what the flag promises, what is public and what stays outside is in the header; the default path's warning is
    # where it was and points at the flag
    for text in ("k_tracker_own_ct", "BRANCHES ON KEY BITS", "WHAT IS PUBLIC", "curdle_whisk_is_own_tracker, whose",
                 "NOT a default", "CURDLE_TRACKER_OWN_PAIRS lanes"):
        assert text in flat, text
    assert flat.count("WHAT THE FLAG PROMISES") >= 3 and flat.count("power draw and clock behaviour") >= 3
    csrc = os.path.join(ROOT, "go-curdleproofs_amd", "csrc")
    make = open(os.path.join(ROOT, "go-curdleproofs_amd", "Makefile")).read()
    assert "csrc/tracker_own_ct_kernels.hip" in make and "build/tracker_own_ct_kernels.o" in make
    # ONE constant-time mixed addition for variable bases in the tree: the shared header's
    walk = open(os.path.join(csrc, "g1_walk_ct.h")).read()
    assert "void madd_bit(" in walk and "k = r - 1" in walk
    for unit in ("g1_mul_ct_kernels.hip", "tracker_own_ct_kernels.hip"):
        text = open(os.path.join(csrc, unit)).read()
        assert '#include "g1_walk_ct.h"' in text and "void madd_bit(" not in text, unit


def test_empty_calls_need_no_device_and_write_nothing(cm):
    host, dev = _fns(cm)
    before = _stats(cm)
    trk = np.full(96, 7, dtype=np.uint8)
    ks = np.full(4, 7, dtype=np.uint64)
    out = np.full(8, 77, dtype=np.uint8)
    for flags in FLAGS:
        for n, m in ((0, 0), (0, 1), (1, 0), (0, 5), (5, 0)):
            assert host(trk.ctypes.data, n, ks.ctypes.data, m, out.ctypes.data, flags) == cm.OK
            assert host(None, n, None, m, None, flags) == cm.OK
            assert dev(FAKE, n, FAKE, m, FAKE, None, flags) == cm.OK
            assert dev(FAKE + 1, n, FAKE + 4, m, FAKE + 3, None, flags) == cm.OK
            assert dev(None, n, None, m, None, None, flags) == cm.OK
        assert cm.whisk_find_own_trackers([], np.zeros((3, 4), dtype=np.uint64), flags=flags).shape == (3, 0)
        assert cm.whisk_find_own_trackers([bytes(96)], np.zeros((0, 4), dtype=np.uint64), flags=flags).shape == (0, 1)
        cm.whisk_find_own_trackers_device(0, 0, 0, 0, 0, flags=flags)
    assert (out == 77).all()
    assert _stats(cm) == before


def test_an_unknown_flag_bit_is_refused_first(cm):
    """Before the counts and the pointers are looked at, with n = 0 or m = 0 and with null pointers too; the host form
    fills `owned` with 255, as on every negative return."""
    host, dev = _fns(cm)
    before = _stats(cm)
    for flags in BAD_FLAGS:
        for n, m in ((0, 0), (0, 3), (2, 2), ((1 << 20) + 1, 1), (1, 65536)):
            assert dev(FAKE + 1, n, FAKE + 8, m, FAKE, None, flags) == cm.EINVAL and "flag" in cm.last_error(), (flags, n, m)
            assert dev(None, n, None, m, None, None, flags) == cm.EINVAL and "flag" in cm.last_error(), (flags, n, m)
            assert host(None, n, None, m, None, flags) == cm.EINVAL and "flag" in cm.last_error(), (flags, n, m)
            assert host(FAKE, n, FAKE, m, None, flags) == cm.EINVAL and "flag" in cm.last_error(), (flags, n, m)
        # null trackers and the counts would be refused next: the flag is named, and owned reads as no verdict
        for n, m in ((2, 3), (3, 1)):
            out = np.full(n * m + 2, 77, dtype=np.uint8)
            assert host(None, n, FAKE, m, out.ctypes.data, flags) == cm.EINVAL and "flag" in cm.last_error()
            assert (out[:n * m] == cm.TRACKER_UNKNOWN).all() and (out[n * m:] == 77).all()
        out = np.full(4, 77, dtype=np.uint8)
        assert host(FAKE, 0, FAKE, 5, out.ctypes.data, flags) == cm.EINVAL and (out == 77).all()   # m n = 0 bytes
    with pytest.raises(cm.CurdleError) as e:
        cm.whisk_find_own_trackers([bytes(96)] * 2, np.zeros((3, 4), dtype=np.uint64), flags=2)
    assert e.value.code == cm.EINVAL and "flag" in e.value.msg
    with pytest.raises(cm.CurdleError) as e:
        cm.whisk_find_own_trackers_device(FAKE, 2, FAKE, 2, FAKE, flags=6)
    assert e.value.code == cm.EINVAL and "flag" in e.value.msg
    assert _stats(cm) == before


@pytest.mark.parametrize("flags", FLAGS)
def test_refusals_happen_before_device_work(cm, flags):
    """Every refusal of the calls without flags, with flags = 0 (which IS that call) and with the flag alike."""
    host, dev = _fns(cm)
    before = _stats(cm)
    trk = np.zeros(2 * 96, dtype=np.uint8)
    ks = np.zeros(2 * 4, dtype=np.uint64)
    out = np.full(4, 77, dtype=np.uint8)
    # a null pointer
    assert host(None, 2, ks.ctypes.data, 2, out.ctypes.data, flags) == cm.EINVAL and "null argument" in cm.last_error()
    assert (out == cm.TRACKER_UNKNOWN).all()             # a refused call never reads as a verdict
    assert host(trk.ctypes.data, 2, None, 2, out.ctypes.data, flags) == cm.EINVAL and "null argument" in cm.last_error()
    assert host(trk.ctypes.data, 2, ks.ctypes.data, 2, None, flags) == cm.EINVAL and "null argument" in cm.last_error()
    for hole in range(3):
        a = [None if j == hole else FAKE for j in range(3)]
        assert dev(a[0], 2, a[1], 2, a[2], None, flags) == cm.EINVAL and "null argument" in cm.last_error()
    # refused by the counts alone: nothing behind the input pointers is read
    assert 24929 * 673 == (1 << 24) + 1
    for n, m, what in (((1 << 20) + 1, 1, "2^20"), (1, 65536, "65,535"), (24929, 673, "2^24")):
        assert dev(FAKE, n, FAKE, m, FAKE, None, flags) == cm.EINVAL and what in cm.last_error(), (n, m)
        big = np.zeros(m * n, dtype=np.uint8)
        assert host(FAKE, n, FAKE, m, big.ctypes.data, flags) == cm.EINVAL and what in cm.last_error(), (n, m)
        assert (big == cm.TRACKER_UNKNOWN).all()
    # exactly 2^24 pairs are within the limit: such a call gets past the counts (to the alignment check, still before the device)
    assert dev(FAKE + 8, 1 << 12, FAKE, 1 << 12, FAKE, None, flags) == cm.EINVAL and "multiples of 16" in cm.last_error()
    # a device pointer that is not a multiple of 16; d_owned may have any alignment, so it is the other two that decide
    for off in (1, 4, 8):
        assert dev(FAKE + off, 2, FAKE, 2, FAKE, None, flags) == cm.EINVAL and "multiples of 16" in cm.last_error()
        assert dev(FAKE, 2, FAKE + off, 2, FAKE, None, flags) == cm.EINVAL and "multiples of 16" in cm.last_error()
        assert dev(FAKE + off, 2, FAKE + off, 2, FAKE + off, None, flags) == cm.EINVAL and "multiples of 16" in cm.last_error()
    assert _f(cm, "curdle_stat_tracker_own_ct", vp)(None) == cm.EINVAL
    assert _stats(cm) == before


def test_no_device_no_fallback(cm):
    """Without a device the flagged calls fail with CURDLE_ENODEV, fill `owned` and count nothing (with one, the GPU
    tests speak)."""
    if cm.device_available():
        return
    host, _ = _fns(cm)
    before = _stats(cm)
    ks = np.zeros((3, 4), dtype=np.uint64)
    for flags in FLAGS:
        for call in (lambda: cm.whisk_find_own_trackers([bytes(96)] * 2, ks, flags=flags),
                     lambda: cm.whisk_find_own_trackers_device(FAKE, 2, FAKE, 3, FAKE, flags=flags)):
            with pytest.raises(cm.CurdleError) as e:
                call()
            assert e.value.code == cm.ENODEV
        trk = np.zeros(2 * 96, dtype=np.uint8)
        out = np.full(6, 77, dtype=np.uint8)
        assert host(trk.ctypes.data, 2, ks.ctypes.data, 3, out.ctypes.data, flags) == cm.ENODEV
        assert (out == cm.TRACKER_UNKNOWN).all()
    assert _stats(cm) == before
