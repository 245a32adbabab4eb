"""The batched constant-time MSM and the flagged Prove at the C ABI, without a GPU: curdle_msm_g1_ct_batch / _device,
curdle_msm_g1_ct_multi, curdle_stat_msm_ct_batch, curdle_prove_ex and curdle_stat_alg_msm exist as include/curdle_msm.h
declares them, the header says what the flag promises and that the host-side operations of Prove are outside, empty
calls need no device, everything malformed is refused before any device work in the stated order (the refused calls
pass pointers that name no memory), an unknown flag bit of curdle_prove_ex is refused first of all with the outputs
untouched, the fold-bases knob refuses the flagged call, and without a device the four flagged paths fail with
CURDLE_ENODEV: no host fallback."""
import ctypes as C
import glob
import inspect
import os
import re

import numpy as np
import pytest

from test_normalize_abi import FAKE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("curdle_msm_g1_ct_batch", "curdle_msm_g1_ct_batch_device", "curdle_msm_g1_ct_multi", "curdle_stat_msm_ct_batch",
         "curdle_prove_ex", "curdle_stat_alg_msm")
vp = C.c_void_p
CT = 1
BAD_FLAGS = (2, 3, 4, 0x80, 1 << 31, 0xFFFFFFFE, 0xFFFFFFFF)
MAX, KMAX = 65536, 4096


def _f(cm, name, *argtypes):
    f = getattr(cm._lib, name)
    f.restype = C.c_int
    f.argtypes = list(argtypes)
    return f


def _fns(cm):
    return (_f(cm, "curdle_msm_g1_ct_batch", vp, vp, vp, C.c_size_t, C.c_uint, vp),
            _f(cm, "curdle_msm_g1_ct_batch_device", vp, vp, vp, C.c_size_t, C.c_uint, vp, vp),
            _f(cm, "curdle_msm_g1_ct_multi", vp, C.c_size_t, vp, C.c_size_t, C.c_uint, vp),
            _f(cm, "curdle_prove_ex", vp, vp, vp, vp, vp, C.c_size_t, vp, vp, vp, vp, vp, C.c_uint, vp, C.c_size_t, vp))


def _stats(cm):
    return cm.stat_msm_ct(), cm.stat_msm_ct_batch(), cm.stat_alg_msm(), cm.stat_g1_mul_ct(), cm.stat_normalize()


def _offs(*v):
    return np.array(v, dtype=np.uint64)


def test_symbols_and_prototypes(cm):
    header = open(os.path.join(ROOT, "include", "curdle_msm.h")).read()
    flat = re.sub(r"\s+", " ", header)
    for name in NAMES:
        assert hasattr(cm._lib, name) and name in cm.SYMBOLS, name
    for proto in (
            "int curdle_msm_g1_ct_batch(const uint64_t* points, const uint64_t* scalars, const size_t* offsets, size_t k, "
            "unsigned scalar_bits, uint64_t* out_jac);",
            "int curdle_msm_g1_ct_batch_device(const void* d_points, const void* d_scalars, const size_t* offsets, size_t k, "
            "unsigned scalar_bits, uint64_t* out_jac, void* stream);",
            "int curdle_msm_g1_ct_multi(const uint64_t* const* points_sets, size_t k, const uint64_t* scalars, size_t n, "
            "unsigned scalar_bits, uint64_t* out_jac);",
            "int curdle_stat_msm_ct_batch(unsigned long long out[3]);",
            "#define CURDLE_PROVE_MSM_CONSTANT_TIME 1u",
            "int curdle_prove_ex(const curdle_crs* crs, const uint64_t* Rs, const uint64_t* Ss, const uint64_t* Ts, "
            "const uint64_t* Us, size_t ell, const uint64_t M[18], const uint32_t* perm, const uint64_t k[4], "
            "const uint64_t rs_m[16], curdle_rand* rand, unsigned flags, uint8_t* proof_out, size_t cap, size_t* proof_len);",
            "int curdle_stat_alg_msm(unsigned long long out[4]);"):
        assert proto in flat, proto
    # the binding
    assert cm.PROVE_MSM_CONSTANT_TIME == CT
    assert set(cm.stat_msm_ct_batch()) == {"calls", "msms", "levels"}
    assert set(cm.stat_alg_msm()) == {"bucket_calls", "bucket_pairs", "ct_calls", "ct_pairs"}
    assert inspect.signature(cm.prove).parameters["flags"].default is None
    for fn in (cm.msm_g1_ct_batch, cm.msm_g1_ct_batch_device, cm.msm_g1_ct_multi):
        assert inspect.signature(fn).parameters["scalar_bits"].default == 255
    # the promise, in the form of the existing ones, with the sentence that the host-side operations are outside
    for text in ("k_g1_sum_ct_seg", "k_msm_ct_finish_seg", "WHAT THE FLAG PROMISES: the DEVICE WORK OF PROVE'S MSMs, and only that",
                 "WHAT IT DOES NOT PROMISE: power draw and clock behaviour, as above; and NOTHING ABOUT THE HOST.",
                 "OUTSIDE THE PROMISE: the host-side operations of Prove on the same secrets are outside",
                 "Point::Mul calls on r_k, k, r_t and r_u", "GroupCommitment::New", "the Fr vector arithmetic",
                 "the generation of the blinders", "alg::ScalarMulBatch", "They are the next follow-up.",
                 "flags = 0 IS curdle_prove.", "CURDLE_PROVER_FOLD_BASES=1", "k <= 4,096", "k n <= 65,536",
                 "EVERY word of out_jac stays untouched", "one block of 144 k bytes and the status word",
                 "a null argument (offsets always; out_jac, the points and the scalars when k > 0), scalar_bits, k, offsets that",
                 "decrease, the total, and (the _device form) device pointers that are not multiples of 16",
                 "curdle_prove_ex, each under its flag"):
        assert text in flat, text
    assert flat.count("WHAT THE FLAG PROMISES") >= 4 and flat.count("OUTSIDE THE PROMISE") >= 4
    # the new kernels live in the unit the build already lists; add_ct and madd_bit are defined nowhere new
    csrc = os.path.join(ROOT, "go-curdleproofs_amd", "csrc")
    make = open(os.path.join(ROOT, "go-curdleproofs_amd", "Makefile")).read()
    kernels = open(os.path.join(csrc, "msm_ct_kernels.hip")).read()
    for k in ("k_msm_ct_walk(", "k_g1_sum_ct_seg(", "k_msm_ct_finish_seg("):
        assert k in kernels, k
    for path in glob.glob(os.path.join(csrc, "*.hip")):
        unit = os.path.basename(path)[:-4]
        assert "csrc/%s.hip" % unit in make and "build/%s.o" % unit in make, unit
    # the whole constant-time G1 layer has one definition each: the walk, the exit and the small helpers too
    # ("void affine_words_ct(": the bare name with its parenthesis is also what a call looks like)
    homes = {"void add_ct(": "g1_add_ct.h", "void madd_bit(": "g1_walk_ct.h", "u32 equal_mod_p(": "g1_add_ct.h",
             "void to_gnark_ct(": "g1_exit_ct.h", "void affine_words_ct(": "g1_exit_ct.h", "u32 walk_ct(": "g1_walk_ct.h",
             "void select3(": "g1_walk_ct.h", "void load_fr_lane(": "g1_walk_ct.h", "u32 finite_mask(": "g1_add_ct.h",
             "void madd_select(": "fbase_walk_ct.h", "void msm_ct_lane(": "msm_ct_lane.h",
             # the refusal texts the two MSM families share are written once, in the unit that defines msm_ct_call.h
             "offsets decrease at": "msm_ct_api.hip", "is not in 1...255": "msm_ct_api.hip",
             "a scalar is not below 2^scalar_bits": "msm_ct_api.hip"}
    defs = {d: [] for d in homes}
    gone = {"to_gnark_msm_ct": [], "load_fr_ct": []}
    for path in glob.glob(os.path.join(csrc, "*")):
        text = open(path, errors="replace").read()
        for d in defs:
            defs[d] += [os.path.basename(path)] * text.count(d)
        for d in gone:
            gone[d] += [os.path.basename(path)] * text.count(d)
    assert defs == {d: [home] for d, home in homes.items()}
    assert gone == {"to_gnark_msm_ct": [], "load_fr_ct": []}
    # the host layer names the primitive weakly
    alg = re.sub(r"\s+", " ", open(os.path.join(ROOT, "go-curdleproofs_amd", "host", "algebra.cpp")).read())
    for name in ("curdle_msm_g1_ct", "curdle_msm_g1_ct_batch", "curdle_msm_g1_ct_multi"):
        assert re.search(r'extern "C" int %s\([^;]*\) __attribute__\(\(weak\)\);' % name, alg), name


def test_empty_calls_need_no_device(cm, oracle):
    batch, dev, multi, _ = _fns(cm)
    before = _stats(cm)
    inf = np.array(oracle.jac_to_mont_limbs(oracle.INF), dtype=np.uint64)
    out = np.full(3 * 18 + 2, 77, dtype=np.uint64)
    o = out[1:].ctypes.data
    one = _offs(5)
    # k = 0: CURDLE_OK, nothing written, null arrays and a null out_jac are fine
    for bits in (1, 9, 255):
        assert batch(None, None, one.ctypes.data, 0, bits, None) == cm.OK
        assert batch(FAKE, FAKE, one.ctypes.data, 0, bits, o) == cm.OK
        assert dev(None, None, one.ctypes.data, 0, bits, None, None) == cm.OK
        assert dev(FAKE + 1, FAKE + 1, one.ctypes.data, 0, bits, o, None) == cm.OK
        assert multi(None, 0, None, 0, bits, None) == cm.OK and multi(None, 0, FAKE, 5, bits, o) == cm.OK
    assert (out == 77).all()
    # all MSMs empty: the infinity encoding k times, nothing else written, no device
    for offs in (_offs(0, 0, 0, 0), _offs(9, 9, 9, 9)):
        for call in (lambda: batch(FAKE, FAKE, offs.ctypes.data, 3, 255, o), lambda: dev(FAKE, FAKE, offs.ctypes.data, 3, 9, o, None)):
            out[:] = 77
            assert call() == cm.OK
            assert (out[1:55].reshape(3, 18) == inf).all() and out[0] == 77 and out[55] == 77
    out[:] = 77
    sets = (vp * 3)(FAKE, FAKE, None)
    assert multi(C.cast(sets, vp), 3, None, 0, 1, o) == cm.OK
    assert (out[1:55].reshape(3, 18) == inf).all() and out[0] == 77 and out[55] == 77
    z12, z4 = np.zeros((0, 12), dtype=np.uint64), np.zeros((0, 4), dtype=np.uint64)
    assert cm.msm_g1_ct_batch(z12, z4, [0]).shape == (0, 18)
    assert (cm.msm_g1_ct_batch(z12, z4, [0, 0, 0]) == inf).all()
    assert (cm.msm_g1_ct_batch(z12, z4, [0, 0, 0]) == cm.msm_g1_batch(z12, z4, [0, 0, 0])).all()   # curdle_msm_g1_batch's encoding
    assert (cm.msm_g1_ct_multi([z12, z12], z4) == inf).all()
    assert _stats(cm) == before


def test_refusals_happen_before_device_work_in_order(cm):
    batch, dev, multi, _ = _fns(cm)
    before = _stats(cm)
    out = np.full(40, 77, dtype=np.uint64)
    o = out.ctypes.data
    err = cm.last_error
    good, down, big = _offs(0, 2, 3), _offs(0, 3, 2), _offs(0, 2, MAX + 1)
    many = np.zeros(KMAX + 2, dtype=np.uint64)
    g, d, b, m = good.ctypes.data, down.ctypes.data, big.ctypes.data, many.ctypes.data
    # 1. null: offsets always; the output, the points and the scalars when k > 0 -- before everything else
    for bits in (0, 9, 256):
        for k in (0, 2, KMAX + 1):
            assert batch(FAKE, FAKE, None, k, bits, o) == cm.EINVAL and "null argument" in err()
            assert dev(FAKE + 1, FAKE, None, k, bits, o, None) == cm.EINVAL and "null argument" in err()
        for k, offs in ((2, d), (2, b), (KMAX + 1, m)):
            for hole in (0, 1, 5):
                a = [FAKE + 1, FAKE + 1, offs, k, bits, o]
                a[hole] = None
                assert batch(*a) == cm.EINVAL and "null argument" in err(), (bits, k, hole)
                assert dev(*a, None) == cm.EINVAL and "null argument" in err(), (bits, k, hole)
    # 2. scalar_bits: also with k = 0, before k, the offsets, the total and the alignment
    for bits in (0, 256, 257, 1 << 31, 0xFFFFFFFF):
        for k, offs in ((0, g), (2, d), (2, b), (KMAX + 1, m)):
            assert batch(FAKE, FAKE, offs, k, bits, o) == cm.EINVAL and "scalar_bits" in err(), (bits, k)
            assert dev(FAKE + 1, FAKE, offs, k, bits, o, None) == cm.EINVAL and "scalar_bits" in err(), (bits, k)
    # 3. k: nothing behind offsets is read (`many` has k + 1 entries for 4,097 only; 2^40 names no memory)
    for k, offs in ((KMAX + 1, m), (1 << 40, FAKE)):
        assert batch(FAKE, FAKE, offs, k, 255, o) == cm.EINVAL and "4,096" in err()
        assert dev(FAKE + 1, FAKE + 8, offs, k, 1, o, None) == cm.EINVAL and "4,096" in err()
    # 4. offsets that decrease: before the total (the decreasing offsets end beyond it) and the alignment
    down_big = _offs(0, MAX + 9, MAX + 8)
    for offs in (d, down_big.ctypes.data):
        assert batch(FAKE, FAKE, offs, 2, 255, o) == cm.EINVAL and "decrease" in err()
        assert dev(FAKE + 1, FAKE + 8, offs, 2, 9, o, None) == cm.EINVAL and "decrease" in err()
    # 5. the total: 65,537 pairs, before the alignment
    assert batch(FAKE, FAKE, b, 2, 255, o) == cm.EINVAL and "65,536" in err()
    assert dev(FAKE + 1, FAKE + 8, b, 2, 255, o, None) == cm.EINVAL and "65,536" in err()
    # 6. exactly 4,096 MSMs and 65,536 pairs are within the limits: such a call gets to the alignment check
    full = (np.arange(KMAX + 1, dtype=np.uint64) * np.uint64(16))
    assert int(full[-1]) == MAX
    for off in (1, 4, 8):
        assert dev(FAKE + off, FAKE, full.ctypes.data, KMAX, 255, o, None) == cm.EINVAL and "multiples of 16" in err()
        assert dev(FAKE, FAKE + off, g, 2, 9, o, None) == cm.EINVAL and "multiples of 16" in err()
    # _multi: null, scalar_bits, k, k n, a null base set
    sets = (vp * 3)(FAKE, None, FAKE)
    s = C.cast(sets, vp)
    for bits in (0, 255):
        assert multi(None, 3, FAKE, 2, bits, o) == cm.EINVAL and "null argument" in err()
        assert multi(s, 3, None, 2, bits, o) == cm.EINVAL and "null argument" in err()
        assert multi(s, KMAX + 1, FAKE, MAX, bits, None) == cm.EINVAL and "null argument" in err()
    for k, n in ((0, 0), (3, 2), (KMAX + 1, MAX)):
        assert multi(s, k, FAKE, n, 0, o) == cm.EINVAL and "scalar_bits" in err()
        assert multi(s, k, FAKE, n, 256, o) == cm.EINVAL and "scalar_bits" in err()
    assert multi(FAKE, KMAX + 1, FAKE, MAX, 255, o) == cm.EINVAL and "4,096" in err()
    for k, n in ((3, MAX // 3 + 1), (2, MAX // 2 + 1), (1, MAX + 1), (3, 1 << 62), (KMAX, 17)):
        assert multi(s if k == 3 else FAKE, k, FAKE, n, 255, o) == cm.EINVAL and "65,536" in err(), (k, n)
    assert multi(s, 3, FAKE, 2, 255, o) == cm.EINVAL and "base set 1" in err()
    assert (out == 77).all()
    assert _f(cm, "curdle_stat_msm_ct_batch", vp)(None) == cm.EINVAL and _f(cm, "curdle_stat_alg_msm", vp)(None) == cm.EINVAL
    with pytest.raises(cm.CurdleError) as e:
        cm.msm_g1_ct_batch(np.zeros((3, 12), dtype=np.uint64), np.zeros((3, 4), dtype=np.uint64), [0, 2, 3], 0)
    assert e.value.code == cm.EINVAL and "scalar_bits" in e.value.msg
    with pytest.raises(cm.CurdleError) as e:
        cm.msm_g1_ct_batch(np.zeros((3, 12), dtype=np.uint64), np.zeros((3, 4), dtype=np.uint64), [0, 3, 2])
    assert e.value.code == cm.EINVAL and "decrease" in e.value.msg
    assert _stats(cm) == before


def _prove_args(cm, ell=4):
    crs, rand = cm.CRS(ell, cm.Rand(8)), cm.Rand(7)
    pts = np.zeros((ell, 12), dtype=np.uint64)
    M, k, rs_m = np.zeros(18, dtype=np.uint64), np.zeros(4, dtype=np.uint64), np.zeros(16, dtype=np.uint64)
    perm = np.arange(ell, dtype=np.uint32)
    keep = (crs, rand, pts, M, k, rs_m, perm)
    return keep, [crs._h, pts.ctypes.data, pts.ctypes.data, pts.ctypes.data, pts.ctypes.data, ell, M.ctypes.data,
                  perm.ctypes.data, k.ctypes.data, rs_m.ctypes.data, rand._h]


def test_an_unknown_flag_bit_of_prove_is_refused_first(cm):
    """Before the pointers and the count are looked at, with null pointers too; proof_out and *proof_len stay as they
    were and nothing is drawn from rand."""
    prove = _fns(cm)[3]
    before = _stats(cm)
    keep, args = _prove_args(cm)
    rand = keep[1]
    nxt = cm.Rand(7).get_frs(1)
    buf = np.full(4096, 77, dtype=np.uint8)
    n = C.c_size_t(12345)
    for flags in BAD_FLAGS:
        assert prove(*([None] * 5), 0, *([None] * 5), flags, None, 0, None) == cm.EINVAL and "flag" in cm.last_error()
        assert prove(*([FAKE] * 5), 4097, *([FAKE] * 5), flags, FAKE, 1 << 20, FAKE) == cm.EINVAL and "flag" in cm.last_error()
        assert prove(*args, flags, buf.ctypes.data, len(buf), C.addressof(n)) == cm.EINVAL and "flag" in cm.last_error()
    assert (buf == 77).all() and n.value == 12345
    assert (rand.get_frs(1) == nxt).all()
    with pytest.raises(cm.CurdleError) as e:
        crs, _, pts, M, k, rs_m, perm = keep
        cm.prove(crs, pts, pts, pts, pts, M, perm, k, rs_m, rand, flags=2)
    assert e.value.code == cm.EINVAL and "flag" in e.value.msg
    assert _stats(cm) == before


def test_the_flagged_prove_refuses_before_any_msm(cm):
    """Null arguments, an ell that is not the CRS's and the fold-bases knob: CURDLE_EINVAL, outputs untouched, nothing
    drawn from rand, nothing counted."""
    prove = _fns(cm)[3]
    before = _stats(cm)
    keep, args = _prove_args(cm)
    rand = keep[1]
    nxt = cm.Rand(7).get_frs(1)
    buf = np.full(4096, 77, dtype=np.uint8)
    n = C.c_size_t(12345)
    tail = [CT, buf.ctypes.data, len(buf), C.addressof(n)]
    for hole in (0, 1, 2, 3, 4, 6, 7, 8, 9, 10):
        a = list(args)
        a[hole] = None
        assert prove(*a, *tail) == cm.EINVAL and "null argument" in cm.last_error(), hole
    assert prove(*args, CT, buf.ctypes.data, len(buf), None) == cm.EINVAL and "null argument" in cm.last_error()
    for ell in (0, 3, 5):
        a = list(args)
        a[5] = ell
        assert prove(*a, *tail) == cm.EINVAL and "does not match" in cm.last_error(), ell
    with cm.knobs(PROVER_FOLD_BASES=1):
        assert prove(*args, *tail) == cm.EINVAL and "PROVER_FOLD_BASES" in cm.last_error()
    assert (buf == 77).all() and n.value == 12345
    assert (rand.get_frs(1) == nxt).all()
    assert _stats(cm) == before


def test_no_device_no_fallback(cm):
    """Without a device the four flagged paths fail with CURDLE_ENODEV and count nothing (with one, the GPU tests speak)."""
    if cm.device_available():
        return
    before = _stats(cm)
    pts, sc = np.zeros((3, 12), dtype=np.uint64), np.zeros((3, 4), dtype=np.uint64)
    (crs, rand, z, M, k, rs_m, perm), _ = _prove_args(cm)
    for call in (lambda: cm.msm_g1_ct_batch(pts, sc, [0, 2, 3]), lambda: cm.msm_g1_ct_batch(pts, sc, [0, 0, 3], 9),
                 lambda: cm.msm_g1_ct_batch_device(FAKE, FAKE, [0, 2, 3], 255),
                 lambda: cm.msm_g1_ct_multi([pts, pts], sc),
                 lambda: cm.prove(crs, z, z, z, z, M, perm, k, rs_m, rand, flags=cm.PROVE_MSM_CONSTANT_TIME)):
        with pytest.raises(cm.CurdleError) as e:
            call()
        assert e.value.code == cm.ENODEV
    assert _stats(cm) == before
