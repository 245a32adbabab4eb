"""The batched field inversion and the division-step finish at the C ABI, without a GPU: curdle_fp_invert_batch /
_device and curdle_stat_fp_invert exist as include/curdle_msm.h declares them and the binding has them with the two
flags; the promise sentences are in the header; knob CT_FINISH_DIVSTEPS is known to curdle_plan_override; every refusal
arrives in the stated order before any device work (the refused calls pass pointers that name no memory); n = 0 needs no
device and without one the calls fail with CURDLE_ENODEV: no host fallback; the two units are in the Makefile; the
finish kernels are where they were, beside their _ds twins, over ONE sum_tail and ONE write_result."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_normalize_abi import FAKE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "go-curdleproofs_amd", "csrc")
NAMES = ("curdle_fp_invert_batch", "curdle_fp_invert_batch_device", "curdle_stat_fp_invert")
vp = C.c_void_p
FERMAT, RAW = 1, 2
FLAGS = (0, FERMAT, RAW, FERMAT | RAW)
BAD_FLAGS = (4, 5, 8, 0x80, 1 << 31, 0xFFFFFFFC, 0xFFFFFFFF)


def _f(cm, name, *argtypes):
    f = getattr(cm._lib, name)
    f.restype = C.c_int
    f.argtypes = list(argtypes)
    return f


def _fns(cm):
    return (_f(cm, "curdle_fp_invert_batch", vp, C.c_size_t, vp, C.c_uint),
            _f(cm, "curdle_fp_invert_batch_device", vp, C.c_size_t, vp, C.c_uint, vp))


def test_symbols_prototypes_and_the_promise(cm):
    header = open(os.path.join(ROOT, "include", "curdle_msm.h")).read()
    flat = re.sub(r"\s+", " ", header)
    for name in NAMES:
        assert hasattr(cm._lib, name) and name in cm.SYMBOLS, name
    for proto in ("#define CURDLE_FP_INVERT_FERMAT 1u", "#define CURDLE_FP_INVERT_RAW28 2u",
                  "int curdle_fp_invert_batch(const uint64_t* in, size_t n, uint64_t* out, unsigned flags);",
                  "int curdle_fp_invert_batch_device(const void* d_in, size_t n, void* d_out, unsigned flags, void* stream);",
                  "int curdle_stat_fp_invert(unsigned long long out[4]);"):
        assert proto in flat, proto
    assert (cm.FP_INVERT_FERMAT, cm.FP_INVERT_RAW28) == (FERMAT, RAW)
    assert set(cm.stat_fp_invert()) == {"calls", "elements", "finish_divsteps", "finish_fermat"}
    for name in ("fp_invert_batch", "fp_invert_batch_device"):
        assert callable(getattr(cm, name)), name
    text = re.sub(r"\s+", " ", re.sub(r"\n \*", "\n", header))               # the comment's leading stars go
    section = text[text.index("Batched inversion in Fp"):text.index("int curdle_stat_fp_invert(")]
    for text in ("k_fp_invert", "csrc/invert_ds.h", "csrc/invert28.h", "1,110 steps", "0 gives 0", "out may be in",
                 "WHAT THE FLAG PROMISES", "WHAT IT DOES NOT PROMISE", "OUTSIDE THE PROMISE", "power draw and clock behaviour",
                 "instruction stream", "address stream", "THIS VERDICT IS THE ONLY THING ABOUT THE ELEMENTS THE CALL REVEALS",
                 "an unknown flag bit, a null pointer with n > 0, n > 2^24, and", "CURDLE_ENODEV", "CT_FINISH_DIVSTEPS",
                 "k_msm_ct_finish_ds", "NOT a measurement"):
        assert text in section, text


def test_the_knob_is_known(cm):
    with cm.knobs(CT_FINISH_DIVSTEPS=1):
        pass
    cm.plan_override("CURDLE_CT_FINISH_DIVSTEPS", 0)
    cm.plan_override("CT_FINISH_DIVSTEPS", None)
    with pytest.raises(cm.CurdleError):
        cm.plan_override("CT_FINISH_DIVSTEPS_", 1)
    assert "CT_FINISH_DIVSTEPS," in open(os.path.join(ROOT, "go-curdleproofs_amd", "host", "knobs.h")).read()
    assert '"CT_FINISH_DIVSTEPS"' in open(os.path.join(ROOT, "go-curdleproofs_amd", "host", "knobs.cpp")).read()


def test_refusals_in_their_order_before_any_device_work(cm):
    host, dev = _fns(cm)
    before = cm.stat_fp_invert()
    big = (1 << 24) + 1
    out = np.full(14, 77, dtype=np.uint64)
    # 1. an unknown flag bit: before the pointers, the count and the alignment are looked at, with n = 0 too
    for flags in BAD_FLAGS:
        for n in (0, 2, big):
            for a, b in ((None, None), (FAKE, FAKE), (FAKE + 1, FAKE + 8)):
                assert host(a, n, b, flags) == cm.EINVAL and "flag" in cm.last_error(), (flags, n)
                assert dev(a, n, b, flags, None) == cm.EINVAL and "flag" in cm.last_error(), (flags, n)
    for flags in FLAGS:
        # 2. a null pointer with n > 0: before the count and the alignment
        for n in (1, big):
            for a, b in ((None, out.ctypes.data), (out.ctypes.data, None), (None, None)):
                assert host(a, n, b, flags) == cm.EINVAL and "null argument" in cm.last_error(), (flags, n)
            for a, b in ((None, FAKE + 1), (FAKE + 1, None), (None, None)):
                assert dev(a, n, b, flags, None) == cm.EINVAL and "null argument" in cm.last_error(), (flags, n)
        # 3. n > 2^24: before the alignment; nothing behind the pointers is read
        assert host(FAKE, big, FAKE, flags) == cm.EINVAL and "2^24" in cm.last_error()
        assert dev(FAKE + 4, big, FAKE + 8, flags, None) == cm.EINVAL and "2^24" in cm.last_error()
        # 4. misalignment (the resident form); exactly 2^24 gets past the count
        for a, b in ((FAKE + 8, FAKE), (FAKE, FAKE + 4), (FAKE + 1, FAKE + 1)):
            for n in (1, 1 << 24):
                assert dev(a, n, b, flags, None) == cm.EINVAL and "multiples of 16" in cm.last_error(), (flags, n)
        # 5. n = 0: CURDLE_OK without a device, nothing written
        assert host(None, 0, None, flags) == cm.OK
        assert host(FAKE, 0, out.ctypes.data, flags) == cm.OK
        assert dev(None, 0, None, flags, None) == cm.OK
        assert dev(FAKE, 0, FAKE + 16, flags, None) == cm.OK
        assert cm.fp_invert_batch(np.zeros((0, 7 if flags & RAW else 6), dtype=np.uint64), flags=flags).shape[0] == 0
        cm.fp_invert_batch_device(0, 0, 0, flags=flags)
    assert (out == 77).all()
    assert _f(cm, "curdle_stat_fp_invert", vp)(None) == cm.EINVAL
    with pytest.raises(cm.CurdleError) as e:
        cm.fp_invert_batch(np.zeros((3, 6), dtype=np.uint64), flags=4)
    assert e.value.code == cm.EINVAL and "flag" in e.value.msg
    with pytest.raises(ValueError):
        cm.fp_invert_batch(np.zeros((3, 6), dtype=np.uint64), flags=RAW)      # the raw form's items are 7 words
    assert cm.stat_fp_invert() == before


def test_no_device_no_fallback(cm):
    """Without a device the calls fail with CURDLE_ENODEV and count nothing (with one, the GPU tests speak)."""
    if cm.device_available():
        return
    before = cm.stat_fp_invert()
    for flags in FLAGS:
        rows = np.zeros((3, 7 if flags & RAW else 6), dtype=np.uint64)
        for call in (lambda: cm.fp_invert_batch(rows, flags=flags), lambda: cm.fp_invert_batch_device(FAKE, 3, FAKE, flags=flags)):
            with pytest.raises(cm.CurdleError) as e:
                call()
            assert e.value.code == cm.ENODEV
    assert cm.stat_fp_invert() == before


def test_the_units_and_the_shared_bodies():
    make = open(os.path.join(ROOT, "go-curdleproofs_amd", "Makefile")).read()
    for unit in ("fp_invert_kernels", "fp_invert_api"):
        assert os.path.exists(os.path.join(CSRC, unit + ".hip")), unit
        assert "csrc/%s.hip" % unit in make and "build/%s.o" % unit in make, unit
    kernels = open(os.path.join(CSRC, "msm_ct_kernels.hip")).read()
    for k in ("k_msm_ct_finish(", "k_msm_ct_finish_seg(", "k_msm_ct_finish_ds(", "k_msm_ct_finish_seg_ds("):
        assert " " + k in kernels, k
    # one body each: the functions are defined once, and the _ds kernels are instantiations, not copies
    assert len(re.findall(r"void sum_tail\(", kernels)) == 1
    assert len(re.findall(r"void write_result\(", kernels)) == 1
    assert len(re.findall(r"void finish_block\(", kernels)) == 1 and len(re.findall(r"void finish_seg_block\(", kernels)) == 1
    assert kernels.count("affine_words_ct<") == 1 and kernels.count("sum_tail(term") == 2  # its two users
    assert "CT_FINISH_DIVSTEPS" in kernels and "k_msm_ct_finish_ds," in kernels and "k_msm_ct_finish_seg_ds," in kernels
    exit_h = open(os.path.join(CSRC, "g1_exit_ct.h")).read()
    assert "template <class Inv = InvertFermat>" in exit_h and "struct InvertDivsteps" in exit_h
    ds = open(os.path.join(CSRC, "invert_ds.h")).read()
    assert "asm" not in ds.replace("assembly", "") and "kBatches = 37" in ds
    # the exits that stay on the Fermat chain name no inversion: they take the default
    for unit in ("g1_mul_ct_kernels.hip", "fbase_ct_kernels.hip", "tracker_own_ct_kernels.hip", "selftest_ct_kernels.hip"):
        text = open(os.path.join(CSRC, unit)).read()
        assert "InvertDivsteps" not in text and "invert_ds" not in text, unit
