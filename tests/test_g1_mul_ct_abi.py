"""The flagged scalar-multiplication and tracker-proof entry points at the C ABI, without a GPU:
curdle_g1_scalar_mul_batch_ex / _device_ex, curdle_stat_g1_mul_ct and the two
curdle_whisk_generate_tracker_proof_batch*_ex exist as include/curdle_msm.h declares them, knob G1_MUL_CT_PASS is
known, an empty call needs no device, everything malformed -- an unknown flag bit first of all, addends under the
flag -- is refused before any device work (the refused calls pass pointers that name no memory), whatever the calls
without flags refuse is refused the same way with the flag, and without a device the flagged calls fail with
CURDLE_ENODEV: no host fallback."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from test_normalize_abi import FAKE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("curdle_g1_scalar_mul_batch_ex", "curdle_g1_scalar_mul_batch_device_ex", "curdle_stat_g1_mul_ct",
         "curdle_whisk_generate_tracker_proof_batch_blinders_ex", "curdle_whisk_generate_tracker_proof_batch_ex")
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
    return (_f(cm, "curdle_g1_scalar_mul_batch_ex", vp, vp, C.c_size_t, vp, C.c_size_t, C.c_uint, vp),
            _f(cm, "curdle_g1_scalar_mul_batch_device_ex", vp, vp, C.c_size_t, vp, C.c_size_t, C.c_uint, vp, vp),
            _f(cm, "curdle_whisk_generate_tracker_proof_batch_blinders_ex", vp, vp, vp, C.c_size_t, C.c_uint, vp, vp),
            _f(cm, "curdle_whisk_generate_tracker_proof_batch_ex", vp, vp, vp, C.c_size_t, C.c_uint, vp, vp))


def _stats(cm):
    return cm.stat_g1_mul_ct(), cm.stat_normalize(), cm.stat_fbase_ct(), cm.stat_fbase(), cm.stat_tracker_prove()


def test_symbols_and_prototypes(cm):
    header = open(os.path.join(ROOT, "include", "curdle_msm.h")).read()
    flat = re.sub(r"\s+", " ", header)
    for name in NAMES:
        assert hasattr(cm._lib, name) and name in cm.SYMBOLS, name
    for proto in (
            "#define CURDLE_G1_MUL_CONSTANT_TIME 1u",
            "int curdle_g1_scalar_mul_batch_ex(const uint64_t* points, const uint64_t* scalars, size_t n_scalars, "
            "const uint64_t* addends, size_t n, unsigned flags, uint64_t* out_affine);",
            "int curdle_g1_scalar_mul_batch_device_ex(const void* d_points, const void* d_scalars, size_t n_scalars, "
            "const void* d_addends, size_t n, unsigned flags, void* d_out_affine, void* stream);",
            "int curdle_stat_g1_mul_ct(unsigned long long out[2]);",
            "#define CURDLE_TRACKER_PROVE_CONSTANT_TIME 1u",
            "int curdle_whisk_generate_tracker_proof_batch_blinders_ex(const uint8_t* trackers, const uint64_t* ks, "
            "const uint64_t* blinders, size_t k, unsigned flags, uint8_t* proofs_out, int* results);",
            "int curdle_whisk_generate_tracker_proof_batch_ex(const uint8_t* trackers, const uint64_t* ks, curdle_rand* rand, "
            "size_t k, unsigned flags, uint8_t* proofs_out, int* results);"):
        assert proto in flat, proto
    # the binding: the flags' values, the counters, flags= on the wrappers
    assert cm.G1_MUL_CONSTANT_TIME == CT and cm.TRACKER_PROVE_CONSTANT_TIME == CT
    assert set(cm.stat_g1_mul_ct()) == {"scalars", "launches"}
    for name in ("g1_scalar_mul_batch", "g1_scalar_mul_batch_device", "whisk_generate_tracker_proof_batch"):
        assert "flags" in inspect.signature(getattr(cm, name)).parameters, name
    # what the flags promise, what they do not and what stays outside is in the header; the default paths' warnings
    # are where they were and point at the flags
    for text in ("k_g1_mul_ct", "k_tracker_response", "WHAT THE FLAG PROMISES", "WHAT IT DOES NOT PROMISE", "OUTSIDE THE PROMISE",
                 "power draw and clock behaviour", "BRANCHES ON SCALAR BITS", "NOT constant time in the scalars",
                 "CURDLE_G1_MUL_CT_PASS", "addends must be NULL"):
        assert text in flat, text
    assert flat.count("instruction stream") >= 3 and flat.count("address stream") >= 3
    csrc = os.path.join(ROOT, "go-curdleproofs_amd", "csrc")
    assert os.path.exists(os.path.join(csrc, "g1_mul_ct_kernels.hip"))
    assert "csrc/g1_mul_ct_kernels.hip" in open(os.path.join(ROOT, "go-curdleproofs_amd", "Makefile")).read()
    assert "k = r - 1" in open(os.path.join(csrc, "g1_mul_ct_kernels.hip")).read()       # the exactness argument


def test_the_pass_knob_is_known(cm):
    with cm.knobs(G1_MUL_CT_PASS=256):
        pass
    cm.plan_override("CURDLE_G1_MUL_CT_PASS", 1 << 20)
    cm.plan_override("G1_MUL_CT_PASS", None)
    with pytest.raises(cm.CurdleError):
        cm.plan_override("G1_MUL_CT_PASS_", 1)


def test_empty_calls_need_no_device_and_write_nothing(cm):
    host, dev, prove_b, prove_r = _fns(cm)
    before = _stats(cm)
    out = np.full(128, 77, dtype=np.uint8)
    rand = cm.Rand(5)
    for flags in FLAGS:
        assert host(None, None, 0, None, 0, flags, None) == cm.OK
        assert host(FAKE, FAKE, 1, None, 0, flags, out.ctypes.data) == cm.OK
        assert host(FAKE, FAKE, 1, FAKE, 0, flags, FAKE) == cm.OK
        assert dev(None, None, 0, None, 0, flags, None, None) == cm.OK
        assert dev(FAKE, FAKE + 1, 1, FAKE + 4, 0, flags, FAKE + 3, None) == cm.OK
        assert prove_b(None, None, None, 0, flags, None, None) == cm.OK
        assert prove_b(FAKE, FAKE, FAKE, 0, flags, out.ctypes.data, out.ctypes.data) == cm.OK
        assert prove_r(None, None, None, 0, flags, None, None) == cm.OK
        assert prove_r(FAKE, FAKE, rand._h, 0, flags, out.ctypes.data, FAKE) == cm.OK
        assert cm.g1_scalar_mul_batch(np.zeros((0, 12), dtype=np.uint64), np.zeros((0, 4), dtype=np.uint64), flags=flags).shape == (0, 12)
        cm.g1_scalar_mul_batch_device(0, 0, 0, 0, 0, 0, flags=flags)
        p, r = cm.whisk_generate_tracker_proof_batch([], np.zeros((0, 4), dtype=np.uint64), blinders=np.zeros((0, 4), dtype=np.uint64),
                                                     flags=flags)
        assert p.shape == (0, 128) and r.shape == (0,)
    assert (out == 77).all()
    assert _stats(cm) == before


def test_an_unknown_flag_bit_is_refused_first(cm):
    """Before the counts and the pointers are looked at, with n = 0 and null pointers too, and without touching the
    provers' outputs."""
    host, dev, prove_b, prove_r = _fns(cm)
    before = _stats(cm)
    out = np.full(2 * 128, 77, dtype=np.uint8)
    res = np.full(2, 77, dtype=np.int32)
    sc = np.zeros(8, dtype=np.uint64)
    for flags in BAD_FLAGS:
        for n in (0, 2, (1 << 24) + 1):
            assert host(FAKE, FAKE, 7, FAKE, n, flags, FAKE) == cm.EINVAL and "flag" in cm.last_error(), (flags, n)
            assert dev(FAKE + 1, FAKE, 7, FAKE + 8, n, flags, FAKE, None) == cm.EINVAL and "flag" in cm.last_error(), (flags, n)
            assert prove_b(FAKE, FAKE, FAKE, n, flags, FAKE, FAKE) == cm.EINVAL and "flag" in cm.last_error(), (flags, n)
            assert prove_r(FAKE, FAKE, FAKE, n, flags, FAKE, FAKE) == cm.EINVAL and "flag" in cm.last_error(), (flags, n)
        for n in (0, 2):
            assert host(None, None, n, None, n, flags, None) == cm.EINVAL and "flag" in cm.last_error()
            assert dev(None, None, n, None, n, flags, None, None) == cm.EINVAL and "flag" in cm.last_error()
            assert prove_b(None, None, None, n, flags, None, None) == cm.EINVAL and "flag" in cm.last_error()
            assert prove_r(None, None, None, n, flags, None, None) == cm.EINVAL and "flag" in cm.last_error()
        # null trackers would be refused next and zero the outputs: the flag is refused first and they stay
        assert prove_b(None, sc.ctypes.data, sc.ctypes.data, 2, flags, out.ctypes.data, res.ctypes.data) == cm.EINVAL
        assert "flag" in cm.last_error() and (out == 77).all() and (res == 77).all()
        assert prove_r(None, sc.ctypes.data, None, 2, flags, out.ctypes.data, res.ctypes.data) == cm.EINVAL
        assert "flag" in cm.last_error() and (out == 77).all() and (res == 77).all()
    with pytest.raises(cm.CurdleError) as e:
        cm.g1_scalar_mul_batch(np.zeros((3, 12), dtype=np.uint64), np.zeros((3, 4), dtype=np.uint64), flags=2)
    assert e.value.code == cm.EINVAL and "flag" in e.value.msg
    assert _stats(cm) == before


def test_addends_are_refused_under_the_flag(cm):
    host, dev, _, _ = _fns(cm)
    before = _stats(cm)
    pts, sc = np.zeros(24, dtype=np.uint64), np.zeros(8, dtype=np.uint64)
    out = np.full(24, 77, dtype=np.uint64)
    assert host(pts.ctypes.data, sc.ctypes.data, 2, FAKE, 2, CT, out.ctypes.data) == cm.EINVAL and "addends" in cm.last_error()
    assert host(pts.ctypes.data, sc.ctypes.data, 1, FAKE, 2, CT, out.ctypes.data) == cm.EINVAL and "addends" in cm.last_error()
    assert dev(FAKE, FAKE, 2, FAKE, 2, CT, FAKE, None) == cm.EINVAL and "addends" in cm.last_error()
    assert dev(FAKE, FAKE, 1, FAKE, 1 << 24, CT, FAKE, None) == cm.EINVAL and "addends" in cm.last_error()
    with pytest.raises(cm.CurdleError) as e:
        cm.g1_scalar_mul_batch(pts.reshape(2, 12), sc.reshape(2, 4), addends=pts.reshape(2, 12), flags=CT)
    assert e.value.code == cm.EINVAL and "addends" in e.value.msg
    assert (out == 77).all()
    assert _stats(cm) == before


@pytest.mark.parametrize("flags", FLAGS)
def test_refusals_happen_before_device_work(cm, flags):
    """Every refusal of the calls without flags, with flags = 0 (which IS that call) and with the flag alike."""
    host, dev, prove_b, prove_r = _fns(cm)
    before = _stats(cm)
    pts, sc = np.zeros(24, dtype=np.uint64), np.zeros(8, dtype=np.uint64)
    out = np.full(24, 77, dtype=np.uint64)
    # a null pointer with n > 0; null addends are no error
    assert host(None, sc.ctypes.data, 2, None, 2, flags, out.ctypes.data) == cm.EINVAL and "null argument" in cm.last_error()
    assert host(pts.ctypes.data, None, 2, None, 2, flags, out.ctypes.data) == cm.EINVAL and "null argument" in cm.last_error()
    assert host(pts.ctypes.data, sc.ctypes.data, 2, None, 2, flags, None) == cm.EINVAL and "null argument" in cm.last_error()
    assert dev(None, FAKE, 2, None, 2, flags, FAKE, None) == cm.EINVAL and "null argument" in cm.last_error()
    assert dev(FAKE, None, 2, None, 2, flags, FAKE, None) == cm.EINVAL and "null argument" in cm.last_error()
    assert dev(FAKE, FAKE, 2, None, 2, flags, None, None) == cm.EINVAL and "null argument" in cm.last_error()
    # n_scalars neither n nor 1
    for ns in (0, 2, 4):
        assert host(FAKE, FAKE, ns, None, 3, flags, FAKE) == cm.EINVAL and "n_scalars" in cm.last_error()
        assert dev(FAKE, FAKE, ns, None, 3, flags, FAKE, None) == cm.EINVAL and "n_scalars" in cm.last_error()
    # the count: nothing behind the pointers is read
    big = (1 << 24) + 1
    for ns in (1, big):
        assert host(FAKE, FAKE, ns, None, big, flags, FAKE) == cm.EINVAL and "2^24" in cm.last_error()
        assert dev(FAKE, FAKE, ns, None, big, flags, FAKE, None) == cm.EINVAL and "2^24" in cm.last_error()
    # exactly 2^24 is within the limit: such a call gets past the count (to the alignment check, still before the device)
    assert dev(FAKE + 8, FAKE, 1, None, 1 << 24, flags, FAKE, None) == cm.EINVAL and "multiples of 16" in cm.last_error()
    # a device pointer that is not a multiple of 16, the addends' included
    for off in (1, 4, 8):
        for hole in range(4):
            a = [FAKE + (off if j == hole else 0) for j in range(4)]
            assert dev(a[0], a[1], 2, a[2], 2, flags, a[3], None) == cm.EINVAL and "multiples of 16" in cm.last_error()
    assert (out == 77).all()
    # the provers: a null argument zeroes what it was given and fills the results
    trk = np.zeros(2 * 96, dtype=np.uint8)
    rand = cm.Rand(9)
    for call in (lambda p, r: prove_b(None, sc.ctypes.data, sc.ctypes.data, 2, flags, p, r),
                 lambda p, r: prove_b(trk.ctypes.data, None, sc.ctypes.data, 2, flags, p, r),
                 lambda p, r: prove_b(trk.ctypes.data, sc.ctypes.data, None, 2, flags, p, r),
                 lambda p, r: prove_r(trk.ctypes.data, sc.ctypes.data, None, 2, flags, p, r),
                 lambda p, r: prove_r(None, sc.ctypes.data, rand._h, 2, flags, p, r)):
        proofs = np.full(2 * 128, 77, dtype=np.uint8)
        res = np.full(2, 77, dtype=np.int32)
        assert call(proofs.ctypes.data, res.ctypes.data) == cm.EINVAL and "null argument" in cm.last_error()
        assert not proofs.any() and (res == cm.EINVAL).all()
    assert prove_b(trk.ctypes.data, sc.ctypes.data, sc.ctypes.data, 2, flags, None, None) == cm.EINVAL
    assert _f(cm, "curdle_stat_g1_mul_ct", vp)(None) == cm.EINVAL
    assert _stats(cm) == before


def test_no_device_no_fallback(cm):
    """Without a device the flagged calls fail with CURDLE_ENODEV and count nothing (with one, the GPU tests speak)."""
    if cm.device_available():
        return
    before = _stats(cm)
    pts, sc = np.zeros((3, 12), dtype=np.uint64), np.zeros((3, 4), dtype=np.uint64)
    for flags in FLAGS:
        for call in (lambda: cm.g1_scalar_mul_batch(pts, sc, flags=flags),
                     lambda: cm.g1_scalar_mul_batch(pts, sc[0], flags=flags),
                     lambda: cm.g1_scalar_mul_batch_device(FAKE, FAKE, 3, 0, 3, FAKE, flags=flags),
                     lambda: cm.whisk_generate_tracker_proof_batch([bytes(96)] * 3, sc, blinders=sc, flags=flags),
                     lambda: cm.whisk_generate_tracker_proof_batch([bytes(96)] * 3, sc, rand=cm.Rand(1), flags=flags)):
            with pytest.raises(cm.CurdleError) as e:
                call()
            assert e.value.code == cm.ENODEV
    assert _stats(cm) == before
