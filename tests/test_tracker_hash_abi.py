"""The tracker batch's choice of where its transcripts are hashed, at the C ABI and without a GPU:
curdle_whisk_is_valid_tracker_proof_batch_ex, _batch_device and curdle_stat_tracker exist as include/curdle_msm.h
declares them, refuse what is malformed before a device is needed, and the constant program the device path runs
(whisk.go:131-134) is pinned three ways on honest members: a plain model of Merlin, the library's host twin of the
transcript kernel, and the protocol's own equation c k = b - s, which involves neither."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import merlin_model as mm
from test_tracker_batch_gpu import honest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("curdle_whisk_is_valid_tracker_proof_batch_ex", "curdle_whisk_is_valid_tracker_proof_batch_device",
         "curdle_stat_tracker")
# the program of the device path: Transcript("whisk_opening_proof"), six encodings, one challenge
LABEL = b"whisk_opening_proof"
PROGRAM = [(mm.TR_APPEND, b"tracker_opening_proof", 6, 48), (mm.TR_CHALLENGES, b"tracker_opening_proof_challenge", 1, 0)]


def _ex(cm):
    f = cm._lib.curdle_whisk_is_valid_tracker_proof_batch_ex
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint, C.c_void_p]
    return f


def _dev(cm):
    f = cm._lib.curdle_whisk_is_valid_tracker_proof_batch_device
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    return f


def _args(k):
    return (np.zeros(96 * k, np.uint8), np.zeros(48 * k, np.uint8), np.zeros(128 * k, np.uint8))


def test_symbols_and_prototypes(cm):
    header = open(os.path.join(ROOT, "include", "curdle_msm.h")).read()
    flat = re.sub(r"\s+", " ", header)
    for name in NAMES:
        assert hasattr(cm._lib, name) and name in cm.SYMBOLS, name
    assert ("int curdle_whisk_is_valid_tracker_proof_batch_ex(const uint8_t* trackers, const uint8_t* k_commitments, "
            "const uint8_t* proofs, size_t k, unsigned flags, int* results);") in flat
    assert ("int curdle_whisk_is_valid_tracker_proof_batch_device(const void* d_trackers, const void* d_k_commitments, "
            "const void* d_proofs, size_t k, int* results, void* stream);") in flat
    assert "int curdle_stat_tracker(unsigned long long out[3]);" in flat
    for name, value in (("DEFAULT", 0), ("HOST", 1), ("DEVICE", 2)):
        assert re.search(r"#define CURDLE_TRACKER_HASH_%s %du\b" % (name, value), header)
        assert getattr(cm, "TRACKER_HASH_" + name) == value


def test_empty_batch_needs_no_device_and_writes_nothing(cm):
    ex, dev = _ex(cm), _dev(cm)
    res = np.full(4, 77, dtype=np.int32)
    t, kc, p = _args(1)
    for flags in (cm.TRACKER_HASH_DEFAULT, cm.TRACKER_HASH_HOST, cm.TRACKER_HASH_DEVICE):
        assert ex(t.ctypes.data, kc.ctypes.data, p.ctypes.data, 0, flags, res.ctypes.data) == cm.OK
        assert ex(None, None, None, 0, flags, None) == cm.OK
    assert dev(t.ctypes.data, kc.ctypes.data, p.ctypes.data, 0, res.ctypes.data, None) == cm.OK
    assert dev(None, None, None, 0, None, None) == cm.OK
    assert (res == 77).all()
    assert len(cm.whisk_is_valid_tracker_proof_batch([], [], [], flags=cm.TRACKER_HASH_DEVICE)) == 0
    assert len(cm.whisk_is_valid_tracker_proof_batch_device(0, 0, 0, 0)) == 0


def test_null_pointers_and_unknown_flags_are_einval(cm):
    ex, dev = _ex(cm), _dev(cm)
    t, kc, p = _args(2)
    res = np.full(2, 77, dtype=np.int32)
    ptrs = (t.ctypes.data, kc.ctypes.data, p.ctypes.data)
    for hole in range(3):
        a = [None if j == hole else v for j, v in enumerate(ptrs)]
        for flags in (cm.TRACKER_HASH_HOST, cm.TRACKER_HASH_DEVICE):
            res[:] = 77
            assert ex(*a, 2, flags, res.ctypes.data) == cm.EINVAL
            assert (res == cm.EINVAL).all()
        res[:] = 77
        assert dev(*a, 2, res.ctypes.data, None) == cm.EINVAL
        assert (res == cm.EINVAL).all()
    assert ex(*ptrs, 2, cm.TRACKER_HASH_DEVICE, None) == cm.EINVAL
    assert dev(*ptrs, 2, None, None) == cm.EINVAL
    for flags in (3, 4, 0x80000000, 0xffffffff):
        res[:] = 77
        assert ex(*ptrs, 2, flags, res.ctypes.data) == cm.EINVAL
        assert (res == cm.EINVAL).all()
        assert ex(None, None, None, 0, flags, None) == cm.EINVAL


def test_stat_tracker_refuses_null_and_counts_from_zero(cm):
    f = cm._lib.curdle_stat_tracker
    f.restype = C.c_int
    f.argtypes = [C.c_void_p]
    assert f(None) == cm.EINVAL
    assert set(cm.stat_tracker()) == {"device", "host", "handed_back"}


def test_knob_exists(cm):
    with cm.knobs(TRACKER_DEVICE_HASH=1):
        pass
    with cm.knobs(TRACKER_DEVICE_HASH=0):
        pass


def test_the_program_is_pinned_on_honest_members(cm, oracle):
    R = oracle.R
    rand = oracle.Rand(2024)
    gen = oracle.compress(oracle.G1)
    members, rows = [], []
    for j in range(3):
        k, r = rand.get_fr(), rand.get_fr()
        (tracker, kc, proof), b = honest(cm, oracle, k, r, 300 + j)
        members.append((k, b, proof))
        rows.append(kc + gen + tracker[48:] + tracker[:48] + proof[:96])   # kG | g1Gen | krG | rG | A | B
    data = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(3, 288)
    ch, _, status = cm.transcript_batch(PROGRAM, data, label=LABEL, host=True)
    assert not status.any()
    for j, (k, b, proof) in enumerate(members):
        challenges, tries, _, st, _ = mm.run_program(PROGRAM, rows[j], LABEL)
        assert st == 0 and len(challenges) == 1 and tries[0] >= 1
        assert ch[j, 0].tobytes() == challenges[0]                           # the model against the library's twin
        c, s = int.from_bytes(challenges[0], "big"), int.from_bytes(proof[96:], "big")
        assert c < R and s < R
        assert c * k % R == (b - s) % R                                      # whisk.go:163: s = b - c k
