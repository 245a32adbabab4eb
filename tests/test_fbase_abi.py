"""The fixed-base multiplication and the bulk tracker computation at the C ABI, without a GPU: the symbols exist as
include/curdle_msm.h declares them, an empty call needs no device, everything malformed is refused before any device
work (the refused _device calls pass pointers that must never be read: they name no memory), and the two single Whisk
calls -- host code -- write what the big-integer model of tests/fbase_model.py expects and feed the reference's
TestWhiskTrackerProof flow."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fbase_model as fm
from test_normalize_abi import FAKE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("curdle_fbase_create", "curdle_fbase_free", "curdle_g1_fixed_base_mul_batch", "curdle_g1_fixed_base_mul_batch_device",
         "curdle_stat_fbase", "curdle_whisk_compute_tracker", "curdle_whisk_k_commitment", "curdle_whisk_compute_trackers_batch")
vp = C.c_void_p
INF48 = bytes([0xC0]) + bytes(47)


def _f(cm, name, *argtypes):
    f = getattr(cm._lib, name)
    f.restype = C.c_int
    f.argtypes = list(argtypes)
    return f


def _fns(cm):
    return (_f(cm, "curdle_g1_fixed_base_mul_batch", vp, vp, vp, C.c_size_t, C.c_int, vp),
            _f(cm, "curdle_g1_fixed_base_mul_batch_device", vp, vp, vp, C.c_size_t, C.c_int, vp, vp),
            _f(cm, "curdle_whisk_compute_trackers_batch", vp, vp, C.c_size_t, vp, vp))


def limbs(oracle, k):
    return np.array(oracle.fr_to_mont_limbs(k % oracle.R), dtype=np.uint64)


def test_symbols_and_prototypes(cm):
    header = open(os.path.join(ROOT, "include", "curdle_msm.h")).read()
    flat = re.sub(r"\s+", " ", header)
    for name in NAMES:
        assert hasattr(cm._lib, name) and name in cm.SYMBOLS, name
    for proto in (
            "typedef struct curdle_fbase curdle_fbase;",
            "#define CURDLE_G1_OUT_AFFINE 0",
            "#define CURDLE_G1_OUT_COMPRESSED 1",
            "int curdle_fbase_create(const uint64_t point_affine[12], curdle_fbase** out);",
            "void curdle_fbase_free(curdle_fbase* b);",
            "int curdle_g1_fixed_base_mul_batch(const curdle_fbase* base, const uint64_t* scalars, const uint64_t* multipliers, "
            "size_t n, int out_form, void* out);",
            "int curdle_g1_fixed_base_mul_batch_device(const curdle_fbase* base, const void* d_scalars, const void* d_multipliers, "
            "size_t n, int out_form, void* d_out, void* stream);",
            "int curdle_stat_fbase(unsigned long long out[3]);",
            "int curdle_whisk_compute_tracker(const uint64_t k[4], const uint64_t r[4], uint8_t tracker_out[CURDLE_WHISK_TRACKER_SIZE]);",
            "int curdle_whisk_k_commitment(const uint64_t k[4], uint8_t out[48]);",
            "int curdle_whisk_compute_trackers_batch(const uint64_t* ks, const uint64_t* rs, size_t n, uint8_t* trackers_out, "
            "uint8_t* k_commitments_out);"):
        assert proto in flat, proto
    for name in ("fbase_create", "FBase", "g1_fixed_base_mul_batch", "g1_fixed_base_mul_batch_device", "stat_fbase",
                 "whisk_compute_tracker", "whisk_k_commitment", "whisk_compute_trackers_batch"):
        assert callable(getattr(cm, name)), name
    assert (cm.G1_OUT_AFFINE, cm.G1_OUT_COMPRESSED) == (0, 1)
    assert "READS TABLE ENTRIES AT ADDRESSES CHOSEN BY SCALAR DIGITS" in flat
    for src in ("fbase_kernels.hip", "fbase_api.hip"):
        text = re.sub(r"\s*\n//\s*", " ", open(os.path.join(ROOT, "go-curdleproofs_amd", "csrc", src)).read())
        assert "READS TABLE ENTRIES AT ADDRESSES CHOSEN BY SCALAR DIGITS" in text, src
    with cm.knobs(FBASE_PASS=256):                   # the knob exists
        pass


def test_empty_calls_need_no_device_and_write_nothing(cm):
    host, dev, batch = _fns(cm)
    before = cm.stat_fbase()
    sc = np.full(4, 7, dtype=np.uint64)
    out = np.full(96, 77, dtype=np.uint8)
    for form in (cm.G1_OUT_AFFINE, cm.G1_OUT_COMPRESSED, 99):
        assert host(None, sc.ctypes.data, sc.ctypes.data, 0, form, out.ctypes.data) == cm.OK
        assert host(None, None, None, 0, form, None) == cm.OK
        assert host(FAKE, FAKE, FAKE, 0, form, FAKE) == cm.OK
        assert dev(None, FAKE, FAKE, 0, form, FAKE, None) == cm.OK
        assert dev(FAKE, FAKE + 1, FAKE + 4, 0, form, FAKE + 3, None) == cm.OK
        assert dev(None, None, None, 0, form, None, None) == cm.OK
    assert batch(sc.ctypes.data, sc.ctypes.data, 0, out.ctypes.data, out.ctypes.data) == cm.OK
    assert batch(None, None, 0, None, None) == cm.OK
    assert batch(FAKE, FAKE, 0, FAKE, FAKE) == cm.OK
    assert (out == 77).all()
    assert cm.g1_fixed_base_mul_batch(np.zeros((0, 4), dtype=np.uint64)).shape == (0, 12)
    assert cm.g1_fixed_base_mul_batch(np.zeros((0, 4), dtype=np.uint64), out_form=cm.G1_OUT_COMPRESSED).shape == (0, 48)
    cm.g1_fixed_base_mul_batch_device(0, 0, 0, 0)
    t, c = cm.whisk_compute_trackers_batch(np.zeros((0, 4), dtype=np.uint64))
    assert t.shape == (0, 96) and c.shape == (0, 48)
    cm._lib.curdle_fbase_free.restype = None
    cm._lib.curdle_fbase_free.argtypes = [vp]
    cm._lib.curdle_fbase_free(None)                  # a no-op
    assert cm.stat_fbase() == before


def test_refusals_happen_before_device_work(cm):
    host, dev, batch = _fns(cm)
    before = cm.stat_fbase()
    sc = np.zeros(8, dtype=np.uint64)
    out = np.full(192, 77, dtype=np.uint8)
    # a null pointer with n > 0; a null multiplier array is no error
    assert host(None, None, sc.ctypes.data, 2, 0, out.ctypes.data) == cm.EINVAL and "null argument" in cm.last_error()
    assert host(None, sc.ctypes.data, sc.ctypes.data, 2, 0, None) == cm.EINVAL and "null argument" in cm.last_error()
    assert dev(None, None, FAKE, 2, 0, FAKE, None) == cm.EINVAL and "null argument" in cm.last_error()
    assert dev(None, FAKE, FAKE, 2, 1, None, None) == cm.EINVAL and "null argument" in cm.last_error()
    # an unknown output form
    for form in (-1, 2, 99):
        assert host(None, sc.ctypes.data, None, 2, form, out.ctypes.data) == cm.EINVAL and "output form" in cm.last_error()
        assert dev(None, FAKE, None, 2, form, FAKE, None) == cm.EINVAL and "output form" in cm.last_error()
    # the counts: nothing behind the pointers is read
    for form in (0, 1):
        assert host(None, FAKE, FAKE, (1 << 24) + 1, form, FAKE) == cm.EINVAL and "2^24" in cm.last_error()
        assert dev(None, FAKE, FAKE, (1 << 24) + 1, form, FAKE, None) == cm.EINVAL and "2^24" in cm.last_error()
    # exactly 2^24 is within the limit: such a call gets past the count (to the alignment check, still before the device)
    assert dev(None, FAKE + 8, None, 1 << 24, 0, FAKE, None) == cm.EINVAL and "multiples of 16" in cm.last_error()
    # resident pointers off a multiple of 16; a compressed d_out may have any alignment, an affine one may not
    for off in (1, 4, 8):
        for form in (0, 1):
            assert dev(None, FAKE + off, None, 2, form, FAKE, None) == cm.EINVAL and "multiples of 16" in cm.last_error()
            assert dev(None, FAKE, FAKE + off, 2, form, FAKE, None) == cm.EINVAL and "multiples of 16" in cm.last_error()
        assert dev(None, FAKE, None, 2, 0, FAKE + off, None) == cm.EINVAL and "multiples of 16" in cm.last_error()
    assert (out == 77).all()
    # the tracker batch: a count beyond 2^22 touches nothing; a null argument zeroes what it was given
    assert batch(FAKE, FAKE, (1 << 22) + 1, FAKE, FAKE) == cm.EINVAL and "2^22" in cm.last_error()
    trk = np.full(2 * 96, 77, dtype=np.uint8)
    com = np.full(2 * 48, 77, dtype=np.uint8)
    assert batch(None, sc.ctypes.data, 2, trk.ctypes.data, com.ctypes.data) == cm.EINVAL and "null argument" in cm.last_error()
    assert not trk.any() and not com.any()           # the outputs of a refused tracker batch are zero
    com[:] = 77
    assert batch(sc.ctypes.data, None, 2, None, com.ctypes.data) == cm.EINVAL and "null argument" in cm.last_error()
    assert not com.any()
    assert _f(cm, "curdle_stat_fbase", vp)(None) == cm.EINVAL
    assert set(cm.stat_fbase()) == {"scalars", "launches", "tables"}
    assert cm.stat_fbase() == before


def test_fbase_create_refuses_bad_points_on_the_host(cm, oracle):
    """Infinity, a point off the curve and a curve point outside the subgroup (the torsion points of the subgroup tests'
    fixture) are refused with the reason named, before the device is asked for: this runs without one."""
    create = _f(cm, "curdle_fbase_create", vp, C.POINTER(vp))
    before = cm.stat_fbase()
    z = np.load(os.path.join(ROOT, "tests", "golden", "affine_check_points.npz"))
    pts, sub, nosub = z["points"], z["status_subgroup"], z["status_no_subgroup"]
    torsion = pts[(sub == 4) & (nosub == 0)]
    off = pts[nosub == 3]
    big = pts[nosub == 2]
    assert len(torsion) >= 20 and len(off) >= 10 and len(big) >= 1
    h = vp(5)
    g = np.array(oracle.affine_to_mont_limbs(oracle.G1), dtype=np.uint64)
    assert create(None, C.byref(h)) == cm.EINVAL and create(g.ctypes.data, None) == cm.EINVAL
    for what, rows in (("infinity", np.zeros((1, 12), dtype=np.uint64)), ("not on the curve", off[:10]),
                       ("not in the prime-order subgroup", torsion[:20]), ("not below p", big[:1])):
        for row in rows:
            p = np.ascontiguousarray(row, dtype=np.uint64)
            h = vp(5)
            assert create(p.ctypes.data, C.byref(h)) == cm.EINVAL and what in cm.last_error(), what
            assert h.value is None
            with pytest.raises(cm.CurdleError) as e:
                cm.FBase(p)
            assert e.value.code == cm.EINVAL and what in e.value.msg
    if not cm.device_available():                    # a good point gets as far as the device: no host fallback
        with pytest.raises(cm.CurdleError) as e:
            cm.FBase(g)
        assert e.value.code == cm.ENODEV
        for call in (lambda: cm.g1_fixed_base_mul_batch(np.zeros((3, 4), dtype=np.uint64)),
                     lambda: cm.whisk_compute_trackers_batch(np.zeros((3, 4), dtype=np.uint64))):
            with pytest.raises(cm.CurdleError) as e:
                call()
            assert e.value.code == cm.ENODEV
        assert cm.stat_fbase() == before


@pytest.fixture(scope="module")
def whisk_values(oracle):
    return fm.whisk_scalars(oracle)


def test_the_single_calls_against_the_model(cm, oracle, coracle, whisk_values):
    """k, r in {0, 1, 2, r - 1, r - 2, lambda, 2^128, a dozen random}, crossed, and k r = 1."""
    comm = {}
    for kname, k in whisk_values:
        kl = limbs(oracle, k)
        comm[k] = cm.whisk_k_commitment(kl)
        assert comm[k] == fm.expected(oracle, coracle, k)[1], kname
        for rname, r in whisk_values:
            got = cm.whisk_compute_tracker(kl, limbs(oracle, r))
            assert (got, comm[k]) == fm.tracker_bytes(oracle, coracle, k, r), (kname, rname)
    assert comm[0] == INF48 and cm.whisk_compute_tracker(limbs(oracle, 0), limbs(oracle, 5))[48:] == INF48
    assert cm.whisk_compute_tracker(limbs(oracle, 5), limbs(oracle, 0)) == INF48 + INF48
    k = whisk_values[-1][1]
    t = cm.whisk_compute_tracker(limbs(oracle, k), limbs(oracle, pow(k, -1, oracle.R)))      # k r = 1: krG is the generator
    assert t[48:] == oracle.compress(oracle.G1) and t == fm.tracker_bytes(oracle, coracle, k, pow(k, -1, oracle.R))[0]
    # the fork's initial tracker, computeTracker(k, fr.One()): (G, k G)
    assert cm.whisk_compute_tracker(limbs(oracle, k), limbs(oracle, 1)) == oracle.compress(oracle.G1) + comm[k]
    single = _f(cm, "curdle_whisk_compute_tracker", vp, vp, vp)
    kc = _f(cm, "curdle_whisk_k_commitment", vp, vp)
    a, out = limbs(oracle, 3), np.zeros(96, dtype=np.uint8)
    for hole in range(3):
        args = [None if j == hole else x.ctypes.data for j, x in enumerate((a, a, out))]
        assert single(*args) == cm.EINVAL and "null argument" in cm.last_error()
    assert kc(None, out.ctypes.data) == cm.EINVAL and kc(a.ctypes.data, None) == cm.EINVAL


def test_computed_trackers_are_owned_and_open(cm, oracle, whisk_values):
    """The computed tracker is its key's (curdle_whisk_is_own_tracker) and not the next key's, and a proof generated
    over it verifies with the computed commitment: the reference's TestWhiskTrackerProof through the new calls."""
    rand = cm.Rand(17)
    rs = [v for _, v in whisk_values if v][:6]
    for j, (kname, k) in enumerate(whisk_values):
        r = rs[j % len(rs)]
        kl = limbs(oracle, k)
        t = cm.whisk_compute_tracker(kl, limbs(oracle, r))
        assert cm.whisk_is_own_tracker(t, kl), kname
        assert not cm.whisk_is_own_tracker(t, limbs(oracle, k + 1)), kname
        proof = cm.whisk_generate_tracker_proof(t, kl, rand)
        assert cm.whisk_is_valid_tracker_proof(t, cm.whisk_k_commitment(kl), proof), kname
        assert not cm.whisk_is_valid_tracker_proof(t, cm.whisk_k_commitment(limbs(oracle, k + 1)), proof), kname
