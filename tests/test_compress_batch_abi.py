"""The batched G1 compression and the batched tracker-proof generator at the C ABI, without a GPU:
curdle_g1_compress_batch / _device, curdle_whisk_generate_tracker_proof_batch / _blinders and curdle_stat_tracker_prove
exist as include/curdle_msm.h declares them, and refuse what is malformed before a device is needed."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("curdle_g1_compress_batch", "curdle_g1_compress_batch_device", "curdle_whisk_generate_tracker_proof_batch_blinders",
         "curdle_whisk_generate_tracker_proof_batch", "curdle_stat_tracker_prove")
vp = C.c_void_p


def _f(cm, name, *argtypes):
    f = getattr(cm._lib, name)
    f.restype = C.c_int
    f.argtypes = list(argtypes)
    return f


def _compress(cm):
    return (_f(cm, "curdle_g1_compress_batch", vp, C.c_size_t, vp),
            _f(cm, "curdle_g1_compress_batch_device", vp, C.c_size_t, vp, vp))


def _generate(cm):
    return (_f(cm, "curdle_whisk_generate_tracker_proof_batch_blinders", vp, vp, vp, C.c_size_t, vp, vp),
            _f(cm, "curdle_whisk_generate_tracker_proof_batch", vp, vp, vp, C.c_size_t, vp, vp))


def test_symbols_and_prototypes(cm):
    header = open(os.path.join(ROOT, "include", "curdle_msm.h")).read()
    flat = re.sub(r"\s+", " ", header)
    for name in NAMES:
        assert hasattr(cm._lib, name) and name in cm.SYMBOLS, name
    for proto in (
            "int curdle_g1_compress_batch(const uint64_t* jac_points, size_t n, uint8_t* out);",
            "int curdle_g1_compress_batch_device(const void* d_jac_points, size_t n, void* d_out, void* stream);",
            "int curdle_whisk_generate_tracker_proof_batch_blinders(const uint8_t* trackers, const uint64_t* ks, "
            "const uint64_t* blinders, size_t k, uint8_t* proofs_out, int* results);",
            "int curdle_whisk_generate_tracker_proof_batch(const uint8_t* trackers, const uint64_t* ks, curdle_rand* rand, "
            "size_t k, uint8_t* proofs_out, int* results);",
            "int curdle_stat_tracker_prove(unsigned long long out[2]);"):
        assert proto in flat, proto
    for name in ("g1_compress_batch", "g1_compress_batch_device", "whisk_generate_tracker_proof_batch", "stat_tracker_prove"):
        assert callable(getattr(cm, name)), name


def test_empty_calls_need_no_device_and_write_nothing(cm):
    host, dev = _compress(cm)
    pts = np.full(18, 7, dtype=np.uint64)
    out = np.full(48, 77, dtype=np.uint8)
    assert host(pts.ctypes.data, 0, out.ctypes.data) == cm.OK
    assert host(None, 0, None) == cm.OK
    assert dev(pts.ctypes.data, 0, out.ctypes.data, None) == cm.OK
    assert dev(None, 0, None, None) == cm.OK
    assert (out == 77).all()
    assert cm.g1_compress_batch(np.zeros((0, 18), dtype=np.uint64)).shape == (0, 48)
    cm.g1_compress_batch_device(0, 0, 0)

    blind, drawn = _generate(cm)
    t, ks = np.zeros(96, np.uint8), np.zeros(4, np.uint64)
    proofs, res = np.full(128, 77, np.uint8), np.full(1, 77, np.int32)
    rand = cm.Rand(5)
    assert blind(t.ctypes.data, ks.ctypes.data, ks.ctypes.data, 0, proofs.ctypes.data, res.ctypes.data) == cm.OK
    assert blind(None, None, None, 0, None, None) == cm.OK
    assert drawn(t.ctypes.data, ks.ctypes.data, rand._h, 0, proofs.ctypes.data, res.ctypes.data) == cm.OK
    assert drawn(None, None, None, 0, None, None) == cm.OK
    assert (proofs == 77).all() and (res == 77).all()
    # ... and nothing was drawn
    assert (rand.get_fr() == cm.Rand(5).get_fr()).all()
    p, r = cm.whisk_generate_tracker_proof_batch([], np.zeros((0, 4), np.uint64), blinders=np.zeros((0, 4), np.uint64))
    assert p.shape == (0, 128) and r.shape == (0,)
    p, r = cm.whisk_generate_tracker_proof_batch([], np.zeros((0, 4), np.uint64), rand=rand)
    assert p.shape == (0, 128) and r.shape == (0,)


def test_null_pointers_and_oversize_are_einval(cm):
    host, dev = _compress(cm)
    pts = np.zeros(36, dtype=np.uint64)
    out = np.full(96, 77, dtype=np.uint8)
    assert host(None, 2, out.ctypes.data) == cm.EINVAL and "null argument" in cm.last_error()
    assert host(pts.ctypes.data, 2, None) == cm.EINVAL
    assert dev(None, 2, out.ctypes.data, None) == cm.EINVAL
    assert dev(pts.ctypes.data, 2, None, None) == cm.EINVAL
    # refused by the count alone: nothing behind the pointers is read
    assert host(pts.ctypes.data, (1 << 27) + 1, out.ctypes.data) == cm.EINVAL and "2^27" in cm.last_error()
    assert dev(pts.ctypes.data, (1 << 27) + 1, out.ctypes.data, None) == cm.EINVAL and "2^27" in cm.last_error()
    assert (out == 77).all()

    blind, drawn = _generate(cm)
    t, ks, bs = np.zeros(192, np.uint8), np.zeros(8, np.uint64), np.zeros(8, np.uint64)
    proofs, res = np.zeros(256, np.uint8), np.full(2, 77, np.int32)
    rand = cm.Rand(5)
    good = [t.ctypes.data, ks.ctypes.data, bs.ctypes.data]
    for hole in range(3):
        a = [None if j == hole else v for j, v in enumerate(good)]
        res[:] = 77
        assert blind(*a, 2, proofs.ctypes.data, res.ctypes.data) == cm.EINVAL
        assert (res == cm.EINVAL).all()
        a = [None if j == hole else v for j, v in enumerate(good[:2] + [rand._h])]
        res[:] = 77
        assert drawn(*a, 2, proofs.ctypes.data, res.ctypes.data) == cm.EINVAL
        assert (res == cm.EINVAL).all()
    assert blind(*good, 2, None, res.ctypes.data) == cm.EINVAL
    assert blind(*good, 2, proofs.ctypes.data, None) == cm.EINVAL
    assert drawn(*good[:2], rand._h, 2, None, res.ctypes.data) == cm.EINVAL
    assert drawn(*good[:2], rand._h, 2, proofs.ctypes.data, None) == cm.EINVAL
    assert (rand.get_fr() == cm.Rand(5).get_fr()).all()


def test_stat_tracker_prove_refuses_null(cm):
    f = _f(cm, "curdle_stat_tracker_prove", vp)
    assert f(None) == cm.EINVAL
    assert set(cm.stat_tracker_prove()) == {"device", "host"}
