"""The ownership search over Whisk trackers at the C ABI, without a GPU: curdle_whisk_is_own_tracker,
curdle_whisk_find_own_trackers / _device and curdle_stat_tracker_own exist as include/curdle_msm.h declares them, an
empty call needs no device, everything malformed is refused before any device work (the refused _device calls pass
pointers that must never be read: they name no memory), and the single call -- host code -- answers every case family
as the big-integer model of tests/tracker_own_model.py does."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import tracker_own_model as tom
from test_normalize_abi import FAKE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("curdle_whisk_is_own_tracker", "curdle_whisk_find_own_trackers", "curdle_whisk_find_own_trackers_device",
         "curdle_stat_tracker_own")
vp = C.c_void_p


def _f(cm, name, *argtypes):
    f = getattr(cm._lib, name)
    f.restype = C.c_int
    f.argtypes = list(argtypes)
    return f


def _fns(cm):
    return (_f(cm, "curdle_whisk_find_own_trackers", vp, C.c_size_t, vp, C.c_size_t, vp),
            _f(cm, "curdle_whisk_find_own_trackers_device", vp, C.c_size_t, vp, C.c_size_t, vp, vp))


def limbs(oracle, k):
    return np.array(oracle.fr_to_mont_limbs(k % oracle.R), dtype=np.uint64)


def test_symbols_and_prototypes(cm):
    header = open(os.path.join(ROOT, "include", "curdle_msm.h")).read()
    flat = re.sub(r"\s+", " ", header)
    for name in NAMES:
        assert hasattr(cm._lib, name) and name in cm.SYMBOLS, name
    for proto in (
            "#define CURDLE_TRACKER_NOT_OWNED 0",
            "#define CURDLE_TRACKER_OWNED 1",
            "#define CURDLE_TRACKER_BAD 2",
            "#define CURDLE_TRACKER_UNKNOWN 255",
            "int curdle_whisk_is_own_tracker(const uint8_t tracker[CURDLE_WHISK_TRACKER_SIZE], const uint64_t k[4], int* owned);",
            "int curdle_whisk_find_own_trackers(const uint8_t* trackers, size_t n, const uint64_t* ks, size_t m, uint8_t* owned);",
            "int curdle_whisk_find_own_trackers_device(const void* d_trackers, size_t n, const void* d_ks, size_t m, "
            "void* d_owned, void* stream);",
            "int curdle_stat_tracker_own(unsigned long long out[3]);"):
        assert proto in flat, proto
    for name in ("whisk_is_own_tracker", "whisk_find_own_trackers", "whisk_find_own_trackers_device", "stat_tracker_own"):
        assert callable(getattr(cm, name)), name
    assert (cm.TRACKER_NOT_OWNED, cm.TRACKER_OWNED, cm.TRACKER_BAD, cm.TRACKER_UNKNOWN) == (0, 1, 2, 255)
    assert (tom.NOT_OWNED, tom.OWNED, tom.BAD) == (0, 1, 2)
    assert "BRANCHES ON KEY BITS" in header


def test_empty_calls_need_no_device_and_write_nothing(cm):
    host, dev = _fns(cm)
    before = cm.stat_tracker_own()
    trk = np.full(96, 7, dtype=np.uint8)
    ks = np.full(4, 7, dtype=np.uint64)
    out = np.full(8, 77, dtype=np.uint8)
    for n, m in ((0, 0), (0, 1), (1, 0), (0, 5), (5, 0)):
        assert host(trk.ctypes.data, n, ks.ctypes.data, m, out.ctypes.data) == cm.OK
        assert host(None, n, None, m, None) == cm.OK
        assert dev(FAKE, n, FAKE, m, FAKE, None) == cm.OK
        assert dev(FAKE + 1, n, FAKE + 4, m, FAKE + 3, None) == cm.OK
        assert dev(None, n, None, m, None, None) == cm.OK
    assert (out == 77).all()
    assert cm.whisk_find_own_trackers([], np.zeros((3, 4), dtype=np.uint64)).shape == (3, 0)
    assert cm.whisk_find_own_trackers([bytes(96)], np.zeros((0, 4), dtype=np.uint64)).shape == (0, 1)
    cm.whisk_find_own_trackers_device(0, 0, 0, 0, 0)
    assert cm.stat_tracker_own() == before


def test_refusals_happen_before_device_work(cm):
    host, dev = _fns(cm)
    before = cm.stat_tracker_own()
    trk = np.zeros(2 * 96, dtype=np.uint8)
    ks = np.zeros(2 * 4, dtype=np.uint64)
    out = np.full(4, 77, dtype=np.uint8)
    # a null pointer
    assert host(None, 2, ks.ctypes.data, 2, out.ctypes.data) == cm.EINVAL and "null argument" in cm.last_error()
    assert (out == cm.TRACKER_UNKNOWN).all()             # a refused call never reads as a verdict
    assert host(trk.ctypes.data, 2, None, 2, out.ctypes.data) == cm.EINVAL
    assert host(trk.ctypes.data, 2, ks.ctypes.data, 2, None) == cm.EINVAL and "null argument" in cm.last_error()
    for hole in range(3):
        a = [None if j == hole else FAKE for j in range(3)]
        assert dev(a[0], 2, a[1], 2, a[2], None) == cm.EINVAL and "null argument" in cm.last_error()
    # refused by the counts alone: nothing behind the input pointers is read
    # 2^24 + 1 = 97 * 257 * 673: (24,929, 673) is inside both single limits and one pair beyond the product's
    assert 24929 * 673 == (1 << 24) + 1
    for n, m, what in (((1 << 20) + 1, 1, "2^20"), (1, 65536, "65,535"), (24929, 673, "2^24"), (1 << 20, 17, "2^24"),
                       ((1 << 12) + 1, 1 << 12, "2^24")):
        assert (m * n > (1 << 24) and n <= (1 << 20) and m <= 65535) == (what == "2^24")
        assert dev(FAKE, n, FAKE, m, FAKE, None) == cm.EINVAL and what in cm.last_error(), (n, m)
        big = np.zeros(m * n, dtype=np.uint8)
        assert host(FAKE, n, FAKE, m, big.ctypes.data) == cm.EINVAL and what in cm.last_error(), (n, m)
        assert (big == cm.TRACKER_UNKNOWN).all()
    # exactly 2^24 pairs are within the limit: such a call gets past the counts (to the alignment check, still before the device)
    assert dev(FAKE + 8, 1 << 12, FAKE, 1 << 12, FAKE, None) == cm.EINVAL and "multiples of 16" in cm.last_error()
    # a device pointer that is not a multiple of 16; d_owned may have any alignment, so it is the other two that decide
    for off in (1, 4, 8):
        assert dev(FAKE + off, 2, FAKE, 2, FAKE, None) == cm.EINVAL and "multiples of 16" in cm.last_error()
        assert dev(FAKE, 2, FAKE + off, 2, FAKE, None) == cm.EINVAL and "multiples of 16" in cm.last_error()
        assert dev(FAKE + off, 2, FAKE + off, 2, FAKE + off, None) == cm.EINVAL and "multiples of 16" in cm.last_error()
    assert cm.stat_tracker_own() == before


def test_the_single_call_and_stat_refuse_null(cm):
    single = _f(cm, "curdle_whisk_is_own_tracker", vp, vp, C.POINTER(C.c_int))
    trk = np.zeros(96, dtype=np.uint8)
    k = np.zeros(4, dtype=np.uint64)
    owned = C.c_int(5)
    assert single(None, k.ctypes.data, C.byref(owned)) == cm.EINVAL and "null argument" in cm.last_error()
    assert single(trk.ctypes.data, None, C.byref(owned)) == cm.EINVAL
    assert single(trk.ctypes.data, k.ctypes.data, None) == cm.EINVAL
    assert _f(cm, "curdle_stat_tracker_own", vp)(None) == cm.EINVAL
    assert set(cm.stat_tracker_own()) == {"pairs", "launches", "bad"}


@pytest.fixture(scope="module")
def families(oracle):
    return tom.case_families(oracle)


def test_the_case_families_hold_what_they_promise(oracle, families):
    keys, trackers = families
    names = [n for n, _ in keys]
    assert {"0", "1", "2", "r-1", "lambda", "lambda+1", "r-lambda", "k2=0", "k1=0", "random 0"} <= set(names)
    assert len(keys) >= 60 and len({k for _, k in keys}) == len(keys)
    assert sum(n.startswith("bad ") for n, _ in trackers) == 10
    assert 16 <= len(trackers) - 10 <= 28
    by = dict(trackers)
    kv = dict(keys)
    inf = oracle.compress(None)
    assert by["honest 0"][48:] == inf and by["honest 0"][:48] != inf
    assert by["honest 1"][:48] == by["honest 1"][48:]
    # every named key owns its honest tracker; infinity | infinity is everybody's, infinity | finite nobody's
    for name, k in keys[:9]:
        assert tom.verdict(oracle, by["honest " + name], k) == tom.OWNED, name
    assert tom.verdict(oracle, by["krG negated, lambda"], kv["lambda"]) == tom.NOT_OWNED
    assert tom.verdict(oracle, by["krG negated, lambda"], kv["r-lambda"]) == tom.OWNED
    assert all(tom.verdict(oracle, by["rG = krG = infinity"], k) == tom.OWNED for k in (0, 1, kv["random 1"]))
    assert all(tom.verdict(oracle, by["rG = infinity, krG finite"], k) == tom.NOT_OWNED for k in (0, 1, kv["random 1"]))
    assert [tom.verdict(oracle, by["krG = infinity"], k) for k in (0, 1, oracle.R - 1)] == [tom.OWNED, tom.NOT_OWNED, tom.NOT_OWNED]
    assert all(tom.verdict(oracle, by["another key 0"], k) == tom.NOT_OWNED for _, k in keys[:13])


def test_the_single_call_against_the_model_over_every_family(cm, oracle, families):
    keys, trackers = families
    want = tom.matrix(oracle, [t for _, t in trackers], [k for _, k in keys])
    seen = set()
    for j, (kname, k) in enumerate(keys):
        kl = limbs(oracle, k)
        for i, (tname, t) in enumerate(trackers):
            try:
                got = tom.OWNED if cm.whisk_is_own_tracker(t, kl) else tom.NOT_OWNED
            except cm.CurdleError as e:
                assert e.code == cm.EINVAL, (kname, tname)
                got = tom.BAD
            assert got == want[j][i], (kname, tname)
            assert (got == tom.BAD) == tname.startswith("bad "), (kname, tname)
            seen.add(got)
    assert seen == {tom.NOT_OWNED, tom.OWNED, tom.BAD}
