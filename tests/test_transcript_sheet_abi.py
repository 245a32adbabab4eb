"""The sheet kernel's surface at the C ABI, without a GPU: curdle_stat_transcript_paths and curdle_keccak_permute_batch
exist as include/curdle_msm.h declares them, the binding has them, knob TRANSCRIPT_SHEET is known, and every call the
header says is refused is refused before any device work (the refused calls pass pointers that name no memory)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_normalize_abi import FAKE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp = C.c_void_p


def _permute(cm):
    f = cm._lib.curdle_keccak_permute_batch
    f.restype = C.c_int
    f.argtypes = [vp, C.c_size_t, C.c_uint, C.c_uint, vp, C.POINTER(C.c_double)]
    return f


def test_symbols_and_prototypes(cm):
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "curdle_msm.h")).read())
    for name in ("curdle_stat_transcript_paths", "curdle_keccak_permute_batch"):
        assert hasattr(cm._lib, name) and name in cm.SYMBOLS, name
    for proto in (
            "int curdle_stat_transcript_paths(unsigned long long out[2]);",
            "int curdle_keccak_permute_batch(const uint64_t* states_in, size_t n, unsigned form, unsigned reps, "
            "uint64_t* states_out, double* kernel_ms);",
            "#define CURDLE_KECCAK_PERMUTE_MAX_REPS 4096",
            "#define CURDLE_KECCAK_PERMUTE_MAX_STATES 65536",
            "int curdle_stat_transcript(unsigned long long out[2]);"):
        assert proto in flat, proto
    assert "TRANSCRIPT_SHEET" in flat                 # the header's paragraph on the two kernels and the knob
    for name in ("stat_transcript_paths", "keccak_permute_batch"):
        assert callable(getattr(cm, name)), name
    assert (cm.KECCAK_LANE, cm.KECCAK_SHEET) == (0, 1)
    assert (cm.KECCAK_PERMUTE_MAX_REPS, cm.KECCAK_PERMUTE_MAX_STATES) == (4096, 65536)
    assert set(cm.stat_transcript_paths()) == {"lane", "sheet"}


def test_the_knob_is_known(cm):
    override = cm._lib.curdle_plan_override
    for name in (b"TRANSCRIPT_SHEET", b"CURDLE_TRANSCRIPT_SHEET"):
        for v in (0, 1, -1):
            assert override(name, v) == cm.OK, (name, v)
    assert override(b"TRANSCRIPT_SHEETS", 1) == cm.EINVAL
    with cm.knobs(TRANSCRIPT_SHEET=1):
        pass


def test_refusals_happen_before_device_work(cm):
    permute = _permute(cm)
    before = cm.stat_transcript_paths()
    ms = C.c_double(-1.0)
    # a null array
    assert permute(None, 3, 0, 1, FAKE, None) == cm.EINVAL and "null argument" in cm.last_error()
    assert permute(FAKE, 3, 1, 1, None, C.byref(ms)) == cm.EINVAL and "null argument" in cm.last_error()
    # the form
    for form in (2, 3, 0xFFFFFFFF):
        assert permute(FAKE, 3, form, 1, FAKE, None) == cm.EINVAL and "form" in cm.last_error()
    # the repetitions
    for reps in (0, 4097, 0xFFFFFFFF):
        for form in (0, 1):
            assert permute(FAKE, 3, form, reps, FAKE, None) == cm.EINVAL and "reps" in cm.last_error()
    # the count
    for form in (0, 1):
        assert permute(FAKE, 65537, form, 1, FAKE, None) == cm.EINVAL and "CURDLE_KECCAK_PERMUTE_MAX_STATES" in cm.last_error()
    assert ms.value == -1.0
    # n = 0 is fine, needs no device and reads nothing
    for form in (0, 1):
        assert permute(FAKE, 0, form, 1, FAKE, None) == cm.OK
        assert permute(FAKE, 0, form, 4096, FAKE, C.byref(ms)) == cm.OK
    assert cm.keccak_permute_batch(np.zeros((0, 25), dtype=np.uint64), cm.KECCAK_SHEET).shape == (0, 25)
    with pytest.raises(ValueError):
        cm.keccak_permute_batch(np.zeros((2, 24), dtype=np.uint64), cm.KECCAK_SHEET)
    # the counters
    paths = cm._lib.curdle_stat_transcript_paths
    paths.restype = C.c_int
    paths.argtypes = [vp]
    assert paths(None) == cm.EINVAL
    assert cm.stat_transcript_paths() == before


def test_without_a_device_the_permutation_is_enodev(cm):
    if cm.device_available():
        return                                        # tests/test_keccak_sheet_gpu.py runs it
    states = np.zeros((2, 25), dtype=np.uint64)
    for form in (cm.KECCAK_LANE, cm.KECCAK_SHEET):
        with pytest.raises(cm.CurdleError) as e:
            cm.keccak_permute_batch(states, form)
        assert e.value.code == cm.ENODEV
