"""The flagged fixed-base entry points at the C ABI, without a GPU: curdle_g1_fixed_base_mul_batch_ex / _device_ex,
curdle_whisk_compute_trackers_batch_ex and curdle_stat_fbase_ct exist as include/curdle_msm.h declares them, an empty
call needs no device, everything malformed -- an unknown flag bit first of all -- is refused before any device work
(the refused calls pass pointers that name no memory), with CURDLE_FBASE_CONSTANT_TIME and with flags = 0 alike, and
without a device the flagged calls fail with CURDLE_ENODEV: no host fallback."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_normalize_abi import FAKE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("curdle_g1_fixed_base_mul_batch_ex", "curdle_g1_fixed_base_mul_batch_device_ex",
         "curdle_whisk_compute_trackers_batch_ex", "curdle_stat_fbase_ct")
vp = C.c_void_p
CT = 1
FLAGS = (0, CT)


def _f(cm, name, *argtypes):
    f = getattr(cm._lib, name)
    f.restype = C.c_int
    f.argtypes = list(argtypes)
    return f


def _fns(cm):
    return (_f(cm, "curdle_g1_fixed_base_mul_batch_ex", vp, vp, vp, C.c_size_t, C.c_int, C.c_uint, vp),
            _f(cm, "curdle_g1_fixed_base_mul_batch_device_ex", vp, vp, vp, C.c_size_t, C.c_int, C.c_uint, vp, vp),
            _f(cm, "curdle_whisk_compute_trackers_batch_ex", vp, vp, C.c_size_t, C.c_uint, vp, vp))


def _stats(cm):
    return cm.stat_fbase(), cm.stat_fbase_ct()


def test_symbols_and_prototypes(cm):
    header = open(os.path.join(ROOT, "include", "curdle_msm.h")).read()
    flat = re.sub(r"\s+", " ", header)
    for name in NAMES:
        assert hasattr(cm._lib, name) and name in cm.SYMBOLS, name
    for proto in (
            "#define CURDLE_FBASE_CONSTANT_TIME 1u",
            "int curdle_g1_fixed_base_mul_batch_ex(const curdle_fbase* base, const uint64_t* scalars, const uint64_t* multipliers, "
            "size_t n, int out_form, unsigned flags, void* out);",
            "int curdle_g1_fixed_base_mul_batch_device_ex(const curdle_fbase* base, const void* d_scalars, const void* d_multipliers, "
            "size_t n, int out_form, unsigned flags, void* d_out, void* stream);",
            "int curdle_whisk_compute_trackers_batch_ex(const uint64_t* ks, const uint64_t* rs, size_t n, unsigned flags, "
            "uint8_t* trackers_out, uint8_t* k_commitments_out);",
            "int curdle_stat_fbase_ct(unsigned long long out[2]);"):
        assert proto in flat, proto
    # the binding: the flag's value, the counters, flags= on the three wrappers
    assert cm.FBASE_CONSTANT_TIME == CT
    assert set(cm.stat_fbase_ct()) == {"scalars", "launches"}
    import inspect
    for name in ("g1_fixed_base_mul_batch", "g1_fixed_base_mul_batch_device", "whisk_compute_trackers_batch"):
        assert "flags" in inspect.signature(getattr(cm, name)).parameters, name
    # what the flag promises and what it does not is in the header; the default path's warning is where it was
    for text in ("instruction stream", "address stream", "only copies", "public output", "power draw and clock behaviour"):
        assert text in flat, text
    assert "READS TABLE ENTRIES AT ADDRESSES CHOSEN BY SCALAR DIGITS" in flat
    for src in ("fbase_kernels.hip", "fbase_api.hip"):
        text = re.sub(r"\s*\n//\s*", " ", open(os.path.join(ROOT, "go-curdleproofs_amd", "csrc", src)).read())
        assert "READS TABLE ENTRIES AT ADDRESSES CHOSEN BY SCALAR DIGITS" in text, src
    assert os.path.exists(os.path.join(ROOT, "go-curdleproofs_amd", "csrc", "fbase_ct_kernels.hip"))
    assert "csrc/fbase_ct_kernels.hip" in open(os.path.join(ROOT, "go-curdleproofs_amd", "Makefile")).read()


def test_empty_calls_need_no_device_and_write_nothing(cm):
    host, dev, batch = _fns(cm)
    before = _stats(cm)
    sc = np.full(4, 7, dtype=np.uint64)
    out = np.full(96, 77, dtype=np.uint8)
    for flags in FLAGS:
        for form in (cm.G1_OUT_AFFINE, cm.G1_OUT_COMPRESSED, 99):
            assert host(None, sc.ctypes.data, sc.ctypes.data, 0, form, flags, out.ctypes.data) == cm.OK
            assert host(None, None, None, 0, form, flags, None) == cm.OK
            assert host(FAKE, FAKE, FAKE, 0, form, flags, FAKE) == cm.OK
            assert dev(None, FAKE, FAKE, 0, form, flags, FAKE, None) == cm.OK
            assert dev(FAKE, FAKE + 1, FAKE + 4, 0, form, flags, FAKE + 3, None) == cm.OK
            assert dev(None, None, None, 0, form, flags, None, None) == cm.OK
        assert batch(sc.ctypes.data, sc.ctypes.data, 0, flags, out.ctypes.data, out.ctypes.data) == cm.OK
        assert batch(None, None, 0, flags, None, None) == cm.OK
        assert batch(FAKE, FAKE, 0, flags, FAKE, FAKE) == cm.OK
        assert cm.g1_fixed_base_mul_batch(np.zeros((0, 4), dtype=np.uint64), flags=flags).shape == (0, 12)
        assert cm.g1_fixed_base_mul_batch(np.zeros((0, 4), dtype=np.uint64), out_form=cm.G1_OUT_COMPRESSED, flags=flags).shape == (0, 48)
        cm.g1_fixed_base_mul_batch_device(0, 0, 0, 0, flags=flags)
        t, c = cm.whisk_compute_trackers_batch(np.zeros((0, 4), dtype=np.uint64), flags=flags)
        assert t.shape == (0, 96) and c.shape == (0, 48)
    assert (out == 77).all()
    assert _stats(cm) == before


def test_an_unknown_flag_bit_is_refused_first(cm):
    """Before the count, the pointers and the output form are looked at, with n = 0 too, and without touching the
    tracker batch's outputs."""
    host, dev, batch = _fns(cm)
    before = _stats(cm)
    sc = np.zeros(8, dtype=np.uint64)
    out = np.full(192, 77, dtype=np.uint8)
    for flags in (2, 3, 4, 0x80, 1 << 31, 0xFFFFFFFE, 0xFFFFFFFF):
        for n in (0, 2, (1 << 24) + 1):
            assert host(None, FAKE, FAKE, n, 0, flags, FAKE) == cm.EINVAL and "flag" in cm.last_error(), (flags, n)
            assert dev(None, FAKE + 1, FAKE, n, 99, flags, FAKE, None) == cm.EINVAL and "flag" in cm.last_error(), (flags, n)
            assert batch(FAKE, FAKE, n, flags, FAKE, FAKE) == cm.EINVAL and "flag" in cm.last_error(), (flags, n)
        assert host(None, None, None, 2, 0, flags, None) == cm.EINVAL and "flag" in cm.last_error()
        assert batch(sc.ctypes.data, None, 2, flags, out.ctypes.data, out.ctypes.data + 96) == cm.EINVAL
        assert "flag" in cm.last_error() and (out == 77).all()
    with pytest.raises(cm.CurdleError) as e:
        cm.g1_fixed_base_mul_batch(np.zeros((3, 4), dtype=np.uint64), flags=2)
    assert e.value.code == cm.EINVAL and "flag" in e.value.msg
    assert _stats(cm) == before


@pytest.mark.parametrize("flags", FLAGS)
def test_refusals_happen_before_device_work(cm, flags):
    host, dev, batch = _fns(cm)
    before = _stats(cm)
    sc = np.zeros(8, dtype=np.uint64)
    out = np.full(192, 77, dtype=np.uint8)
    # a null pointer with n > 0; a null multiplier array is no error
    assert host(None, None, sc.ctypes.data, 2, 0, flags, out.ctypes.data) == cm.EINVAL and "null argument" in cm.last_error()
    assert host(None, sc.ctypes.data, sc.ctypes.data, 2, 0, flags, None) == cm.EINVAL and "null argument" in cm.last_error()
    assert dev(None, None, FAKE, 2, 0, flags, FAKE, None) == cm.EINVAL and "null argument" in cm.last_error()
    assert dev(None, FAKE, FAKE, 2, 1, flags, None, None) == cm.EINVAL and "null argument" in cm.last_error()
    # an unknown output form
    for form in (-1, 2, 99):
        assert host(None, sc.ctypes.data, None, 2, form, flags, out.ctypes.data) == cm.EINVAL and "output form" in cm.last_error()
        assert dev(None, FAKE, None, 2, form, flags, FAKE, None) == cm.EINVAL and "output form" in cm.last_error()
    # the counts: nothing behind the pointers is read
    for form in (0, 1):
        assert host(None, FAKE, FAKE, (1 << 24) + 1, form, flags, FAKE) == cm.EINVAL and "2^24" in cm.last_error()
        assert dev(None, FAKE, FAKE, (1 << 24) + 1, form, flags, FAKE, None) == cm.EINVAL and "2^24" in cm.last_error()
    # exactly 2^24 is within the limit: such a call gets past the count (to the alignment check, still before the device)
    assert dev(None, FAKE + 8, None, 1 << 24, 0, flags, FAKE, None) == cm.EINVAL and "multiples of 16" in cm.last_error()
    # resident pointers off a multiple of 16; a compressed d_out may have any alignment, an affine one may not
    for off in (1, 4, 8):
        for form in (0, 1):
            assert dev(None, FAKE + off, None, 2, form, flags, FAKE, None) == cm.EINVAL and "multiples of 16" in cm.last_error()
            assert dev(None, FAKE, FAKE + off, 2, form, flags, FAKE, None) == cm.EINVAL and "multiples of 16" in cm.last_error()
        assert dev(None, FAKE, None, 2, 0, flags, FAKE + off, None) == cm.EINVAL and "multiples of 16" in cm.last_error()
    assert (out == 77).all()
    # the tracker batch: a count beyond 2^22 touches nothing; a null argument zeroes what it was given
    assert batch(FAKE, FAKE, (1 << 22) + 1, flags, FAKE, FAKE) == cm.EINVAL and "2^22" in cm.last_error()
    trk = np.full(2 * 96, 77, dtype=np.uint8)
    com = np.full(2 * 48, 77, dtype=np.uint8)
    assert batch(None, sc.ctypes.data, 2, flags, trk.ctypes.data, com.ctypes.data) == cm.EINVAL and "null argument" in cm.last_error()
    assert not trk.any() and not com.any()           # the outputs of a refused tracker batch are zero
    com[:] = 77
    assert batch(sc.ctypes.data, None, 2, flags, None, com.ctypes.data) == cm.EINVAL and "null argument" in cm.last_error()
    assert not com.any()
    assert _f(cm, "curdle_stat_fbase_ct", vp)(None) == cm.EINVAL
    assert _stats(cm) == before


def test_no_device_no_fallback(cm):
    """Without a device the flagged calls fail with CURDLE_ENODEV and count nothing (with one, the GPU tests speak)."""
    if cm.device_available():
        return
    before = _stats(cm)
    for flags in FLAGS:
        for call in (lambda: cm.g1_fixed_base_mul_batch(np.zeros((3, 4), dtype=np.uint64), flags=flags),
                     lambda: cm.g1_fixed_base_mul_batch(np.zeros((3, 4), dtype=np.uint64), out_form=cm.G1_OUT_COMPRESSED, flags=flags),
                     lambda: cm.g1_fixed_base_mul_batch_device(FAKE, 0, 3, FAKE, flags=flags),
                     lambda: cm.whisk_compute_trackers_batch(np.zeros((3, 4), dtype=np.uint64), flags=flags)):
            with pytest.raises(cm.CurdleError) as e:
                call()
            assert e.value.code == cm.ENODEV
    assert _stats(cm) == before
