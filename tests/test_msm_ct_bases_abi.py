"""The constant-time MSM over a resident base set at the C ABI, without a GPU: curdle_ct_bases_* and
curdle_msm_g1_ct_bases / _device / _batch / _batch_device exist as include/curdle_msm.h declares them and the binding
covers them, the header says what is promised and that the table is public, empty handles and empty calls need no
device, everything malformed is refused before any device work in the stated order with the outputs untouched (the
refused calls pass pointers that name no memory), without a device the calls fail with CURDLE_ENODEV, the two new units
are in the Makefile and the constant-time G1 layer still has one definition of each function."""
import ctypes as C
import glob
import inspect
import os
import re

import numpy as np
import pytest

from test_normalize_abi import FAKE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("curdle_ct_bases_create", "curdle_ct_bases_create_device", "curdle_ct_bases_free", "curdle_ct_bases_size",
         "curdle_ct_bases_chunk_bits", "curdle_ct_bases_export", "curdle_msm_g1_ct_bases", "curdle_msm_g1_ct_bases_device",
         "curdle_msm_g1_ct_bases_batch", "curdle_msm_g1_ct_bases_batch_device", "curdle_stat_msm_ct_bases")
vp = C.c_void_p
MAX, KMAX = 65536, 4096
CHUNKS = {8: 32, 16: 16, 32: 8, 64: 4}


def _f(cm, name, *argtypes, restype=C.c_int):
    f = getattr(cm._lib, name)
    f.restype = restype
    f.argtypes = list(argtypes)
    return f


def _fns(cm):
    return (_f(cm, "curdle_msm_g1_ct_bases", vp, vp, vp, C.c_size_t, C.c_uint, vp),
            _f(cm, "curdle_msm_g1_ct_bases_device", vp, vp, vp, C.c_size_t, C.c_uint, vp, vp),
            _f(cm, "curdle_msm_g1_ct_bases_batch", vp, vp, vp, vp, C.c_size_t, C.c_uint, vp),
            _f(cm, "curdle_msm_g1_ct_bases_batch_device", vp, vp, vp, vp, C.c_size_t, C.c_uint, vp, vp))


def _creators(cm):
    return (_f(cm, "curdle_ct_bases_create", vp, C.c_size_t, C.c_uint, vp),
            _f(cm, "curdle_ct_bases_create_device", vp, C.c_size_t, C.c_uint, vp, vp))


def _stats(cm):
    return cm.stat_msm_ct_bases(), cm.stat_msm_ct(), cm.stat_msm_ct_batch(), cm.stat_normalize()


def _offs(*v):
    return np.array(v, dtype=np.uint64)


def _empty(cm, chunk_bits=0):
    return cm.CtBases(np.zeros((0, 12), dtype=np.uint64), chunk_bits)


def test_symbols_and_prototypes(cm):
    header = open(os.path.join(ROOT, "include", "curdle_msm.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"\n \* ?", "\n", header))   # a comment's sentences run over its line starts
    for name in NAMES:
        assert hasattr(cm._lib, name) and name in cm.SYMBOLS, name
    for proto in (
            "typedef struct curdle_ct_bases curdle_ct_bases;",
            "int curdle_ct_bases_create(const uint64_t* points, size_t n, unsigned chunk_bits, curdle_ct_bases** out);",
            "int curdle_ct_bases_create_device(const void* d_points, size_t n, unsigned chunk_bits, curdle_ct_bases** out, "
            "void* stream);",
            "void curdle_ct_bases_free(curdle_ct_bases* b);",
            "size_t curdle_ct_bases_size(const curdle_ct_bases* b);",
            "unsigned curdle_ct_bases_chunk_bits(const curdle_ct_bases* b);",
            "int curdle_ct_bases_export(const curdle_ct_bases* b, unsigned chunk, uint64_t* rows_out /* n x 12 */);",
            "int curdle_msm_g1_ct_bases(const curdle_ct_bases* b, const uint32_t* rows, const uint64_t* scalars, size_t n, "
            "unsigned scalar_bits, uint64_t out_jac[18]);",
            "int curdle_msm_g1_ct_bases_device(const curdle_ct_bases* b, const uint32_t* rows, const void* d_scalars, size_t n, "
            "unsigned scalar_bits, uint64_t out_jac[18], void* stream);",
            "int curdle_msm_g1_ct_bases_batch(const curdle_ct_bases* b, const uint32_t* rows, const uint64_t* scalars, "
            "const size_t* offsets, size_t k, unsigned scalar_bits, uint64_t* out_jac);",
            "int curdle_msm_g1_ct_bases_batch_device(const curdle_ct_bases* b, const uint32_t* rows, const void* d_scalars, "
            "const size_t* offsets, size_t k, unsigned scalar_bits, uint64_t* out_jac, void* stream);",
            "int curdle_stat_msm_ct_bases(unsigned long long out[4]);"):
        assert proto in flat, proto
    # the binding: a wrapper class owns a handle
    assert set(cm.stat_msm_ct_bases()) == {"tables", "calls", "lanes", "msms"}
    for fn in (cm.CtBases.msm, cm.CtBases.msm_device, cm.CtBases.msm_batch, cm.CtBases.msm_batch_device):
        p = inspect.signature(fn).parameters
        assert p["scalar_bits"].default == 255 and p["rows"].default is None
    assert inspect.signature(cm.CtBases.__init__).parameters["chunk_bits"].default == 0
    for m in ("free", "export", "__del__"):
        assert hasattr(cm.CtBases, m)
    # the contract, the promise and what is public
    for text in ("k = sum_j 2^(c j) d_j", "row j holds 2^(chunk_bits j) P_i at table[j n + i]", "row 0 is the input",
                 "infinity stays the all-zero record in every row", "chunk_bits is 8, 16, 32 or 64; 0 is the library's choice, 16",
                 "Limit: n C <= 65,536", "gives an empty handle without a device",
                 "a null argument, chunk_bits, n C, and (the _device form) a device pointer that is not a multiple of 16",
                 "without a device the call returns CURDLE_ENODEV", "a free during a call is deferred to that call's end",
                 "THE TABLE IS PUBLIC: nothing of it is wiped", "chunk >= C is CURDLE_EINVAL",
                 "rows is always a HOST array of n PUBLIC indices", "indices may repeat",
                 "The library stages rows itself: it is public and is not wiped","Cb = ceil(scalar_bits / chunk_bits) chunks are walked",
                 "the top chunk takes scalar_bits - chunk_bits (Cb - 1) steps", "EVERY word of out_jac stays untouched",
                 "n Cb <= 65,536 terms per call (one pass), k <= 4,096",
                 "scalar_bits, k, offsets that decrease, the term total, a row index out of range, and (the _device forms) a "
                 "device pointer that is not a multiple of 16",
                 "One MSM slot is held for the call.", "one block of 144 k + 4 bytes",
                 "WHAT THE FLAG PROMISES, WHAT IT DOES NOT PROMISE and what is OUTSIDE THE PROMISE are curdle_msm_g1_ct's, word for word.",
                 "The instruction stream and the address stream also depend on rows, on chunk_bits and on which table points are "
                 "infinity, all of which are public.",
                 "nothing in the library routes to these calls yet", "k_ct_bases_shift", "k_msm_ct_walk_rows",
                 "do not move curdle_stat_msm_ct"):
        assert text in flat, text
    # the two units are built, and hold the two kernels
    csrc = os.path.join(ROOT, "go-curdleproofs_amd", "csrc")
    make = open(os.path.join(ROOT, "go-curdleproofs_amd", "Makefile")).read()
    for unit in ("msm_ct_bases_kernels", "msm_ct_bases_api"):
        assert make.count("csrc/%s.hip" % unit) == 1 and make.count("build/%s.o" % unit) == 1, unit
    kernels = open(os.path.join(csrc, "msm_ct_bases_kernels.hip")).read()
    for k in ("k_ct_bases_shift(", "k_msm_ct_walk_rows(", "msm_ct_lane(", "load_fr_lane(", "d28::dbl(acc)",
              '#include "g1_walk_ct.h"', '#include "msm_ct_lane.h"'):
        assert k in kernels, k
    # the lane behind the addresses is the one k_msm_ct_walk runs: the walk and the ONE atomic OR are there, once
    lane = open(os.path.join(csrc, "msm_ct_lane.h")).read()
    assert "walk_ct(acc, k, x2, y2, steps)" in lane and "store_words_masked<14>(" in lane
    both = kernels + lane
    assert "asm" not in both and "__shared__" not in both and both.count("atomicOr(") == 1
    assert "atomicOr(" not in open(os.path.join(csrc, "msm_ct_kernels.hip")).read()
    api = open(os.path.join(csrc, "msm_ct_bases_api.hip")).read()
    for k in ("seg_walk_sum_fetch(", "launch_g1_normalize(", "kNormalizeXyzz", "ResidentCopy", "SlotHold", "WipeList"):
        assert k in api, k
    # ONE segmented call body: over all the C ABI units the segmented sum is launched from exactly one place
    apis = "".join(open(p).read() for p in glob.glob(os.path.join(csrc, "*_api.hip")))
    assert apis.count("launch_msm_ct_sum_seg(") == 1
    # one definition of each function of the constant-time G1 layer in the tree, and one place for each refusal text the
    # two MSM families share
    homes = {"void add_ct(": "g1_add_ct.h", "void madd_bit(": "g1_walk_ct.h", "u32 walk_ct(": "g1_walk_ct.h",
             "void affine_words_ct(": "g1_exit_ct.h", "void load_fr_lane(": "g1_walk_ct.h", "u32 finite_mask(": "g1_add_ct.h",
             "u32 next_bit_msb(": "g1_walk_ct.h", "void msm_ct_lane(": "msm_ct_lane.h",
             "offsets decrease at": "msm_ct_api.hip", "is not in 1...255": "msm_ct_api.hip",
             "a scalar is not below 2^scalar_bits": "msm_ct_api.hip"}
    defs = {d: [] for d in homes}
    for path in glob.glob(os.path.join(csrc, "*")):
        text = open(path, errors="replace").read()
        for d in defs:
            defs[d] += [os.path.basename(path)] * text.count(d)
    assert defs == {d: [home] for d, home in homes.items()}


def test_empty_handles_and_empty_calls_need_no_device(cm, oracle):
    single, dev, batch, bdev = _fns(cm)
    export = _f(cm, "curdle_ct_bases_export", vp, C.c_uint, vp)
    before = _stats(cm)
    inf = np.array(oracle.jac_to_mont_limbs(oracle.INF), dtype=np.uint64)
    for c, rows in CHUNKS.items():
        e = _empty(cm, c)
        assert (e.n, e.chunk_bits, e.chunks) == (0, c, rows)
        assert e.export(0).shape == (0, 12) and e.export(rows - 1).shape == (0, 12)
        assert export(e._h, 0, None) == cm.OK                     # nothing to write: a null destination is fine
        assert export(e._h, rows, FAKE) == cm.EINVAL and "chunk" in cm.last_error()
        assert export(None, 0, FAKE) == cm.EINVAL and "null argument" in cm.last_error()
        e.free()
        e.free()
    e = _empty(cm)
    assert e.chunk_bits == 16                                      # the library's choice
    # the empty handle by the resident creator too: a null and a misaligned pointer are not looked at for n = 0 ... the
    # alignment is checked only when there is something to read
    h = vp()
    assert _creators(cm)[1](None, 0, 32, C.byref(h), None) == cm.OK and h.value
    assert _f(cm, "curdle_ct_bases_chunk_bits", vp, restype=C.c_uint)(h) == 32
    assert _f(cm, "curdle_ct_bases_size", vp, restype=C.c_size_t)(h) == 0
    _f(cm, "curdle_ct_bases_free", vp, restype=None)(h)
    _f(cm, "curdle_ct_bases_free", vp, restype=None)(None)
    assert _f(cm, "curdle_ct_bases_size", vp, restype=C.c_size_t)(None) == 0
    out = np.full(3 * 18 + 2, 77, dtype=np.uint64)
    o = out[1:].ctypes.data
    # n = 0: the infinity encoding; rows and the scalars may be null or name no memory
    for bits in (1, 9, 255):
        for call in (lambda: single(e._h, None, None, 0, bits, o), lambda: single(e._h, FAKE, FAKE, 0, bits, o),
                     lambda: dev(e._h, None, None, 0, bits, o, None), lambda: dev(e._h, FAKE, FAKE + 1, 0, bits, o, None)):
            out[:] = 77
            assert call() == cm.OK
            assert (out[1:19] == inf).all() and out[0] == 77 and (out[19:] == 77).all()
    # k = 0: CURDLE_OK, nothing written, a null out_jac is fine
    out[:] = 77
    one = _offs(5)
    assert batch(e._h, None, None, one.ctypes.data, 0, 255, None) == cm.OK
    assert bdev(e._h, FAKE, FAKE + 1, one.ctypes.data, 0, 9, o, None) == cm.OK
    assert (out == 77).all()
    # all MSMs empty: the infinity encoding k times, no device
    for offs in (_offs(0, 0, 0, 0), _offs(9, 9, 9, 9)):
        for call in (lambda: batch(e._h, None, FAKE, offs.ctypes.data, 3, 255, o),
                     lambda: bdev(e._h, FAKE, FAKE, offs.ctypes.data, 3, 9, o, None)):
            out[:] = 77
            assert call() == cm.OK
            assert (out[1:55].reshape(3, 18) == inf).all() and out[0] == 77 and out[55] == 77
    z4 = np.zeros((0, 4), dtype=np.uint64)
    assert (e.msm(z4) == inf).all() and (e.msm(z4) == cm.msm_g1_ct(np.zeros((0, 12), dtype=np.uint64), z4)).all()
    assert e.msm_batch(z4, [0]).shape == (0, 18) and (e.msm_batch(z4, [0, 0, 0]) == inf).all()
    assert _stats(cm) == before


def test_the_creators_refuse_before_device_work_in_order(cm):
    create, create_dev = _creators(cm)
    before = _stats(cm)
    err = cm.last_error
    h = vp(12345)

    def refused(rc, what):
        assert rc == cm.EINVAL and what in err(), (rc, err())
        assert h.value is None                                    # *out is null after every refusal behind the null check
        h.value = 12345

    # 1. a null argument, before chunk_bits and n C
    for c in (0, 7, 16):
        for n in (0, 1, MAX + 1):
            assert create(FAKE, n, c, None) == cm.EINVAL and "null argument" in err()
            assert create_dev(FAKE + 8, n, c, None, None) == cm.EINVAL and "null argument" in err()
        refused(create(None, 1, c, C.byref(h)), "null argument")
        refused(create_dev(None, MAX + 1, c, C.byref(h), None), "null argument")
    # 2. chunk_bits, before n C and the alignment
    for c in (1, 7, 9, 15, 17, 24, 48, 63, 65, 128, 1 << 31):
        for n in (0, 1, MAX + 1):
            refused(create(FAKE, n, c, C.byref(h)), "chunk_bits")
            refused(create_dev(FAKE + 8, n, c, C.byref(h), None), "chunk_bits")
    # 3. n C <= 65,536, before the alignment
    for c, rows in list(CHUNKS.items()) + [(0, 16)]:
        for n in (MAX // rows + 1, MAX + 1, 1 << 62):
            refused(create(FAKE, n, c, C.byref(h)), "65,536")
            refused(create_dev(FAKE + 8, n, c, C.byref(h), None), "65,536")
    # 4. the resident form: alignment, at the largest n the limit allows
    for c, rows in CHUNKS.items():
        for off in (1, 4, 8):
            refused(create_dev(FAKE + off, MAX // rows, c, C.byref(h), None), "multiples of 16")
    with pytest.raises(cm.CurdleError) as e:
        cm.CtBases(np.zeros((3, 12), dtype=np.uint64), 12)
    assert e.value.code == cm.EINVAL and "chunk_bits" in e.value.msg
    assert _f(cm, "curdle_stat_msm_ct_bases", vp)(None) == cm.EINVAL
    assert _stats(cm) == before


def test_the_msm_refuses_before_device_work_in_order(cm):
    """On an EMPTY handle, which needs no device: every index is out of range for it, so the row check is the last
    refusal such a call can reach; the alignment behind it is reached by the batch whose MSMs are all empty (and, over a
    real handle, in the GPU tests)."""
    single, dev, batch, bdev = _fns(cm)
    before = _stats(cm)
    err = cm.last_error
    out = np.full(40, 77, dtype=np.uint64)
    o = out.ctypes.data
    e16, e64 = _empty(cm, 16), _empty(cm, 64)
    b = e16._h
    good, down, big = _offs(0, 2, 3), _offs(0, 3, 2), _offs(0, 2, MAX + 1)
    many = np.zeros(KMAX + 2, dtype=np.uint64)
    g, d, bg, m = good.ctypes.data, down.ctypes.data, big.ctypes.data, many.ctypes.data
    row0 = np.zeros(4, dtype=np.uint32)
    # 1. a null argument: the handle, the output, the scalars when n > 0; rows may be null
    for bits in (0, 9, 256):
        for n in (1, MAX + 1):
            for a in ([None, FAKE, FAKE, n, bits, o], [b, FAKE, None, n, bits, o], [b, None, FAKE, n, bits, None]):
                assert single(*a) == cm.EINVAL and "null argument" in err(), a
                assert dev(*a, None) == cm.EINVAL and "null argument" in err(), a
        assert single(None, None, None, 0, bits, o) == cm.EINVAL and "null argument" in err()
        # the batch: the handle and offsets always; out_jac and the scalars when k > 0
        for k in (0, 2, KMAX + 1):
            for a in ([b, FAKE, FAKE + 1, None, k, bits, o], [None, FAKE, FAKE + 1, g, k, bits, o]):
                assert batch(*a) == cm.EINVAL and "null argument" in err(), a
                assert bdev(*a, None) == cm.EINVAL and "null argument" in err(), a
        for k, offs in ((2, d), (2, bg), (KMAX + 1, m)):
            for a in ([b, FAKE, None, offs, k, bits, o], [b, None, FAKE + 1, offs, k, bits, None]):
                assert batch(*a) == cm.EINVAL and "null argument" in err(), a
                assert bdev(*a, None) == cm.EINVAL and "null argument" in err(), a
    # 2. scalar_bits: before k, the offsets, the term total, the rows and the alignment
    for bits in (0, 256, 257, 1 << 31, 0xFFFFFFFF):
        for n in (0, 1, MAX + 1):
            assert single(b, FAKE, FAKE, n, bits, o) == cm.EINVAL and "scalar_bits" in err()
            assert dev(b, FAKE, FAKE + 1, n, bits, o, None) == cm.EINVAL and "scalar_bits" in err()
        for k, offs in ((0, g), (2, d), (2, bg), (KMAX + 1, m)):
            assert batch(b, FAKE, FAKE, offs, k, bits, o) == cm.EINVAL and "scalar_bits" in err()
            assert bdev(b, FAKE, FAKE + 1, offs, k, bits, o, None) == cm.EINVAL and "scalar_bits" in err()
    # 3. k: nothing behind offsets is read
    for k, offs in ((KMAX + 1, m), (1 << 40, FAKE)):
        assert batch(b, FAKE, FAKE, offs, k, 255, o) == cm.EINVAL and "4,096" in err()
        assert bdev(b, FAKE, FAKE + 1, offs, k, 1, o, None) == cm.EINVAL and "4,096" in err()
    # 4. offsets that decrease: before the term total (they end beyond it)
    down_big = _offs(0, MAX + 9, MAX + 8)
    for offs in (d, down_big.ctypes.data):
        assert batch(b, FAKE, FAKE, offs, 2, 255, o) == cm.EINVAL and "decrease" in err()
        assert bdev(b, FAKE, FAKE + 1, offs, 2, 9, o, None) == cm.EINVAL and "decrease" in err()
    # 5. the term total n Cb: before the rows (which name no memory) and the alignment
    for h, c in ((e16._h, 16), (e64._h, 64)):
        for bits in (1, c, c + 1, 2 * c, 255):
            cb = (bits + c - 1) // c
            n = MAX // cb + 1
            assert single(h, FAKE, FAKE, n, bits, o) == cm.EINVAL and "65,536" in err(), (c, bits)
            assert dev(h, FAKE, FAKE + 1, n, bits, o, None) == cm.EINVAL and "65,536" in err(), (c, bits)
            offs = _offs(3, 5, n + 3)
            assert batch(h, FAKE, FAKE, offs.ctypes.data, 2, bits, o) == cm.EINVAL and "65,536" in err(), (c, bits)
            assert bdev(h, FAKE, FAKE + 1, offs.ctypes.data, 2, bits, o, None) == cm.EINVAL and "65,536" in err(), (c, bits)
    # 6. a row index out of range (any index is, for an empty set), and rows = null beyond the set: before the alignment
    for bits in (9, 255):
        assert single(b, row0.ctypes.data, FAKE, 1, bits, o) == cm.EINVAL and "not below" in err()
        assert dev(b, row0.ctypes.data, FAKE + 1, 4, bits, o, None) == cm.EINVAL and "not below" in err()
        assert single(b, None, FAKE, 1, bits, o) == cm.EINVAL and "rows is null" in err()
        assert dev(b, None, FAKE + 1, MAX // 16, bits, o, None) == cm.EINVAL and "rows is null" in err()
        assert batch(b, row0.ctypes.data, FAKE, g, 2, bits, o) == cm.EINVAL and "not below" in err()
        assert bdev(b, None, FAKE + 1, g, 2, bits, o, None) == cm.EINVAL and "rows is null" in err()
    # 7. the alignment, reached by a batch of empty MSMs
    for off in (1, 4, 8):
        assert bdev(b, None, FAKE + off, _offs(2, 2, 2).ctypes.data, 2, 255, o, None) == cm.EINVAL and "multiples of 16" in err()
    assert (out == 77).all()
    with pytest.raises(cm.CurdleError) as e:
        e16.msm(np.zeros((3, 4), dtype=np.uint64), scalar_bits=0)
    assert e.value.code == cm.EINVAL and "scalar_bits" in e.value.msg
    with pytest.raises(cm.CurdleError) as e:
        e16.msm_batch(np.zeros((3, 4), dtype=np.uint64), [0, 3, 2])
    assert e.value.code == cm.EINVAL and "decrease" in e.value.msg
    assert _stats(cm) == before


def test_no_device_no_fallback(cm):
    """Without a device a handle over points cannot be made: CURDLE_ENODEV, *out null, nothing counted (with one, the
    GPU tests speak)."""
    if cm.device_available():
        return
    before = _stats(cm)
    create, create_dev = _creators(cm)
    pts = np.zeros((3, 12), dtype=np.uint64)
    for c in (0, 8, 64):
        h = vp(12345)
        assert create(pts.ctypes.data, 3, c, C.byref(h)) == cm.ENODEV and h.value is None
        h = vp(12345)
        assert create_dev(FAKE, 3, c, C.byref(h), None) == cm.ENODEV and h.value is None
        with pytest.raises(cm.CurdleError) as e:
            cm.CtBases(pts, c)
        assert e.value.code == cm.ENODEV
    assert _stats(cm) == before
