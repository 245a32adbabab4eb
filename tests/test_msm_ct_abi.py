"""The constant-time MSM and the flagged shuffle step at the C ABI, without a GPU: curdle_msm_g1_ct / _device,
curdle_stat_msm_ct and curdle_shuffle_permute_commit_ex exist as include/curdle_msm.h declares them, the header says
what is promised and what is not, an empty call needs no device, everything malformed is refused before any device work
in the stated order (null, scalar_bits, n, alignment; the refused calls pass pointers that name no memory), an unknown
flag bit of the shuffle step is refused first of all with the outputs untouched, and without a device the calls fail
with CURDLE_ENODEV: no host fallback."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from test_normalize_abi import FAKE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("curdle_msm_g1_ct", "curdle_msm_g1_ct_device", "curdle_stat_msm_ct", "curdle_shuffle_permute_commit_ex",
         "curdle_g1_permute_ct_device")
vp = C.c_void_p
CT = 1
BAD_FLAGS = (2, 3, 4, 0x80, 1 << 31, 0xFFFFFFFE, 0xFFFFFFFF)
MAX = 65536


def _f(cm, name, *argtypes):
    f = getattr(cm._lib, name)
    f.restype = C.c_int
    f.argtypes = list(argtypes)
    return f


def _fns(cm):
    return (_f(cm, "curdle_msm_g1_ct", vp, vp, C.c_size_t, C.c_uint, vp),
            _f(cm, "curdle_msm_g1_ct_device", vp, vp, C.c_size_t, C.c_uint, vp, vp),
            _f(cm, "curdle_shuffle_permute_commit_ex", vp, vp, vp, C.c_size_t, vp, vp, vp, C.c_uint, vp, vp, vp, vp))


def _stats(cm):
    return cm.stat_msm_ct(), cm.stat_g1_mul_ct(), cm.stat_normalize()


def test_symbols_and_prototypes(cm):
    header = open(os.path.join(ROOT, "include", "curdle_msm.h")).read()
    flat = re.sub(r"\s+", " ", header)
    for name in NAMES:
        assert hasattr(cm._lib, name) and name in cm.SYMBOLS, name
    for proto in (
            "int curdle_msm_g1_ct(const uint64_t* points, const uint64_t* scalars, size_t n, unsigned scalar_bits, "
            "uint64_t out_jac[18]);",
            "int curdle_msm_g1_ct_device(const void* d_points, const void* d_scalars, size_t n, unsigned scalar_bits, "
            "uint64_t out_jac[18], void* stream);",
            "int curdle_stat_msm_ct(unsigned long long out[3]);",
            "#define CURDLE_SHUFFLE_CONSTANT_TIME 1u",
            "int curdle_g1_permute_ct_device(const void* d_in, const void* d_perm, size_t n, void* d_out, void* stream);",
            "int curdle_shuffle_permute_commit_ex(const curdle_crs* crs, const uint64_t* Rs, const uint64_t* Ss, size_t ell, "
            "const uint32_t* perm, const uint64_t k[4], curdle_rand* rand, unsigned flags, uint64_t* Ts_out, "
            "uint64_t* Us_out, uint64_t M_out[18], uint64_t rs_m_out[16]);"):
        assert proto in flat, proto
    # the binding
    assert cm.SHUFFLE_CONSTANT_TIME == CT
    assert set(cm.stat_msm_ct()) == {"pairs", "walks", "sums"}
    assert "flags" in inspect.signature(cm.shuffle_permute_commit).parameters
    assert "scalar_bits" in inspect.signature(cm.msm_g1_ct).parameters
    assert "scalar_bits" in inspect.signature(cm.msm_g1_ct_device).parameters
    # what is promised, what is not and what stays outside; the verdict is the only thing revealed
    for text in ("k_msm_ct_walk", "k_g1_sum_ct", "k_msm_ct_finish", "k_g1_permute_ct", "csrc/g1_add_ct.h",
                 "WHAT THE FLAG PROMISES", "WHAT IT DOES NOT PROMISE", "OUTSIDE THE PROMISE", "power draw and clock behaviour",
                 "THIS VERDICT IS THE ONLY THING ABOUT THE SCALARS THE CALL REVEALS", "NOT A DEFAULT", "not a default",
                 "never exists outside the device workspace", "ell <= 4,096", "n <= 65,536",
                 "a null argument, scalar_bits, n, and"):
        assert text in flat, text
    assert flat.count("instruction stream") >= 4 and flat.count("address stream") >= 4
    # the build lists the new units; one madd_bit, one equal_mod_p
    csrc = os.path.join(ROOT, "go-curdleproofs_amd", "csrc")
    make = open(os.path.join(ROOT, "go-curdleproofs_amd", "Makefile")).read()
    for unit in ("msm_ct_kernels", "msm_ct_api"):
        assert "csrc/%s.hip" % unit in make and "build/%s.o" % unit in make, unit
    kernels = open(os.path.join(csrc, "msm_ct_kernels.hip")).read()
    assert '#include "g1_walk_ct.h"' in kernels and '#include "g1_add_ct.h"' in kernels and "void madd_bit(" not in kernels
    for k in ("k_msm_ct_walk(", "k_g1_sum_ct(", "k_msm_ct_finish(", "k_g1_permute_ct("):
        assert k in kernels, k
    add = open(os.path.join(csrc, "g1_add_ct.h")).read()
    assert "void add_ct(X28& acc, const X28& b)" in add and "u32 equal_mod_p(" in add and "Bounds." in add
    own = open(os.path.join(csrc, "tracker_own_ct_kernels.hip")).read()
    assert '#include "g1_add_ct.h"' in own and "u32 equal_mod_p(" not in own


def test_empty_calls_need_no_device_and_return_infinity(cm, oracle):
    host, dev, _ = _fns(cm)
    before = _stats(cm)
    inf = np.array(oracle.jac_to_mont_limbs(oracle.INF), dtype=np.uint64)
    for bits in (1, 9, 255):
        for call in (lambda o: host(None, None, 0, bits, o), lambda o: host(FAKE, FAKE, 0, bits, o),
                     lambda o: dev(None, None, 0, bits, o, None), lambda o: dev(FAKE + 1, FAKE + 4, 0, bits, o, None)):
            out = np.full(20, 77, dtype=np.uint64)
            assert call(out.ctypes.data) == cm.OK
            assert (out[:18] == inf).all() and (out[18:] == 77).all()
        assert (cm.msm_g1_ct(np.zeros((0, 12), dtype=np.uint64), np.zeros((0, 4), dtype=np.uint64), bits) == inf).all()
        assert (cm.msm_g1_ct_device(0, 0, 0, bits) == inf).all()
    assert (cm.msm_g1_ct([], []) == cm.msm_g1([], [])).all()                # curdle_msm_g1's encoding
    assert _stats(cm) == before


def test_refusals_happen_before_device_work_in_order(cm):
    host, dev, _ = _fns(cm)
    before = _stats(cm)
    out = np.full(20, 77, dtype=np.uint64)
    o = out.ctypes.data
    err = cm.last_error
    # 1. null: the output always, the inputs when n > 0 -- before bad bits, a bad count and a bad alignment
    for bits in (0, 9, 256):
        for n in (0, 2, MAX + 1):
            assert host(FAKE, FAKE, n, bits, None) == cm.EINVAL and "null argument" in err()
            assert dev(FAKE + 1, FAKE, n, bits, None, None) == cm.EINVAL and "null argument" in err()
        for n in (2, MAX + 1):
            assert host(None, FAKE, n, bits, o) == cm.EINVAL and "null argument" in err()
            assert host(FAKE, None, n, bits, o) == cm.EINVAL and "null argument" in err()
            assert dev(None, FAKE + 1, n, bits, o, None) == cm.EINVAL and "null argument" in err()
            assert dev(FAKE + 1, None, n, bits, o, None) == cm.EINVAL and "null argument" in err()
    # 2. scalar_bits: 0 and beyond 255, also with n = 0, before the count and the alignment
    for bits in (0, 256, 257, 1 << 31, 0xFFFFFFFF):
        for n in (0, 2, MAX + 1):
            assert host(FAKE, FAKE, n, bits, o) == cm.EINVAL and "scalar_bits" in err(), (bits, n)
            assert dev(FAKE + 1, FAKE, n, bits, o, None) == cm.EINVAL and "scalar_bits" in err(), (bits, n)
    # 3. n: nothing behind the pointers is read
    for n in (MAX + 1, 1 << 24, 1 << 40):
        assert host(FAKE, FAKE, n, 255, o) == cm.EINVAL and "65,536" in err()
        assert dev(FAKE + 1, FAKE + 8, n, 1, o, None) == cm.EINVAL and "65,536" in err()
    # 4. exactly 65,536 is within the limit: such a call gets to the alignment check, still before the device
    for off in (1, 4, 8):
        assert dev(FAKE + off, FAKE, MAX, 255, o, None) == cm.EINVAL and "multiples of 16" in err()
        assert dev(FAKE, FAKE + off, 2, 9, o, None) == cm.EINVAL and "multiples of 16" in err()
    assert (out == 77).all()
    assert _f(cm, "curdle_stat_msm_ct", vp)(None) == cm.EINVAL
    # the gather alone: empty, null, the count, the alignment
    gather = _f(cm, "curdle_g1_permute_ct_device", vp, vp, C.c_size_t, vp, vp)
    assert gather(None, None, 0, None, None) == cm.OK
    assert gather(None, FAKE, 2, FAKE, None) == cm.EINVAL and "null argument" in err()
    assert gather(FAKE, None, 2, FAKE, None) == cm.EINVAL and "null argument" in err()
    assert gather(FAKE, FAKE, 2, None, None) == cm.EINVAL and "null argument" in err()
    assert gather(FAKE + 1, FAKE + 1, 4097, FAKE, None) == cm.EINVAL and "4,096" in err()
    for a in ((FAKE + 8, FAKE, FAKE), (FAKE, FAKE + 2, FAKE), (FAKE, FAKE, FAKE + 4)):
        assert gather(a[0], a[1], 4096, a[2], None) == cm.EINVAL and "multiples of 16" in err()
    with pytest.raises(cm.CurdleError) as e:
        cm.msm_g1_ct(np.zeros((3, 12), dtype=np.uint64), np.zeros((3, 4), dtype=np.uint64), 0)
    assert e.value.code == cm.EINVAL and "scalar_bits" in e.value.msg
    assert _stats(cm) == before


def test_an_unknown_flag_bit_of_the_shuffle_step_is_refused_first(cm):
    """Before the pointers and the count are looked at, with null pointers too, and the outputs stay as they were."""
    _, _, step = _fns(cm)
    before = _stats(cm)
    out = np.full(4 * 12 * 2 + 18 + 16, 77, dtype=np.uint64)
    ts, us, m, rs = (out[:48].ctypes.data, out[48:96].ctypes.data, out[96:114].ctypes.data, out[114:].ctypes.data)
    rand = cm.Rand(7)
    crs = cm.CRS(4, cm.Rand(8))
    nxt = cm.Rand(7).get_frs(1)
    for flags in BAD_FLAGS:
        assert step(None, None, None, 0, None, None, None, flags, None, None, None, None) == cm.EINVAL and "flag" in cm.last_error()
        assert step(FAKE, FAKE, FAKE, 4097, FAKE, FAKE, FAKE, flags, FAKE, FAKE, FAKE, FAKE) == cm.EINVAL and "flag" in cm.last_error()
        assert step(crs._h, FAKE, FAKE, 4, FAKE, FAKE, rand._h, flags, ts, us, m, rs) == cm.EINVAL and "flag" in cm.last_error()
    assert (out == 77).all()
    assert (rand.get_frs(1) == nxt).all()                                   # nothing was drawn
    with pytest.raises(cm.CurdleError) as e:
        z = np.zeros((4, 12), dtype=np.uint64)
        cm.shuffle_permute_commit(crs, z, z, np.arange(4), np.zeros(4, dtype=np.uint64), rand, flags=2)
    assert e.value.code == cm.EINVAL and "flag" in e.value.msg
    assert _stats(cm) == before


def test_the_flagged_shuffle_step_refuses_before_device_work(cm):
    """Null arguments, the cap of 4,096 (and ell = 0), an ell that is not the CRS's and an out-of-range permutation
    entry, in that order: all CURDLE_EINVAL, outputs untouched, nothing drawn from rand."""
    _, _, step = _fns(cm)
    before = _stats(cm)
    crs, rand = cm.CRS(4, cm.Rand(8)), cm.Rand(7)
    nxt = cm.Rand(7).get_frs(1)
    pts = np.zeros((4, 12), dtype=np.uint64)
    k = np.zeros(4, dtype=np.uint64)
    perm = np.arange(4, dtype=np.uint32)
    out = np.full(4 * 12 * 2 + 18 + 16, 77, dtype=np.uint64)
    ts, us, m, rs = (out[:48].ctypes.data, out[48:96].ctypes.data, out[96:114].ctypes.data, out[114:].ctypes.data)
    good = [crs._h, pts.ctypes.data, pts.ctypes.data, 4, perm.ctypes.data, k.ctypes.data, rand._h, CT, ts, us, m, rs]
    for hole in (0, 1, 2, 4, 5, 6, 8, 9, 10, 11):
        a = list(good)
        a[hole] = None
        assert step(*a) == cm.EINVAL and "null argument" in cm.last_error(), hole
    for ell, why in ((0, "4,096"), (4097, "4,096"), (1 << 40, "4,096"), (3, "does not match"), (5, "does not match")):
        a = list(good)
        a[3] = ell
        assert step(*a) == cm.EINVAL and why in cm.last_error(), ell
    a = list(good)
    a[3], a[7] = 4097, 0                                                    # the cap is the flag's: without it, the CRS check
    assert step(*a) == cm.EINVAL and "does not match" in cm.last_error()
    bad = perm.copy()
    bad[2] = 4
    a = list(good)
    a[4] = bad.ctypes.data
    assert step(*a) == cm.EINVAL and "out of range" in cm.last_error()
    assert (out == 77).all()
    assert (rand.get_frs(1) == nxt).all()
    assert _stats(cm) == before


def test_no_device_no_fallback(cm):
    """Without a device the calls fail with CURDLE_ENODEV and count nothing (with one, the GPU tests speak)."""
    if cm.device_available():
        return
    before = _stats(cm)
    pts, sc = np.zeros((3, 12), dtype=np.uint64), np.zeros((3, 4), dtype=np.uint64)
    crs, rand = cm.CRS(4, cm.Rand(8)), cm.Rand(7)
    z = np.zeros((4, 12), dtype=np.uint64)
    for call in (lambda: cm.msm_g1_ct(pts, sc), lambda: cm.msm_g1_ct(pts, sc, 9),
                 lambda: cm.msm_g1_ct_device(FAKE, FAKE, 3, 255),
                 lambda: cm.shuffle_permute_commit(crs, z, z, np.arange(4), np.zeros(4, dtype=np.uint64), rand,
                                                   flags=cm.SHUFFLE_CONSTANT_TIME)):
        with pytest.raises(cm.CurdleError) as e:
            call()
        assert e.value.code == cm.ENODEV
    assert _stats(cm) == before
