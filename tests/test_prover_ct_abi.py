"""curdle_msm_g1_ct_bases_sets_batch / _device, curdle_prover_ct_* and curdle_stat_alg_msm_resident at the C ABI, without a
GPU: the symbols exist as include/curdle_msm.h declares them and the binding covers them, the header says what is
promised, every refusal comes before any device work in the stated order with the outputs untouched (the refused calls
pass pointers that name no memory; empty handles need no device), the prover's refusals leave rand where it was, without
a device the creators fail with CURDLE_ENODEV, the knob PROVE_RESIDENT_TERMS is known, the host layer names the device
calls weakly, and the constant-time G1 layer still has one definition of each function and ONE rows walk kernel."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

from test_normalize_abi import FAKE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("curdle_msm_g1_ct_bases_sets_batch", "curdle_msm_g1_ct_bases_sets_batch_device", "curdle_prover_ct_create",
         "curdle_prover_ct_free", "curdle_prover_ct_prove", "curdle_prover_ct_whisk_shuffle_proof", "curdle_stat_alg_msm_resident")
vp = C.c_void_p
MAX, KMAX = 65536, 4096


def _f(cm, name, *argtypes, restype=C.c_int):
    f = getattr(cm._lib, name)
    f.restype = restype
    f.argtypes = list(argtypes)
    return f


def _fns(cm):
    return (_f(cm, "curdle_msm_g1_ct_bases_sets_batch", vp, C.c_size_t, vp, vp, vp, C.c_size_t, C.c_uint, vp),
            _f(cm, "curdle_msm_g1_ct_bases_sets_batch_device", vp, C.c_size_t, vp, vp, vp, C.c_size_t, C.c_uint, vp, vp))


def _stats(cm):
    return cm.stat_msm_ct_bases(), cm.stat_msm_ct(), cm.stat_msm_ct_batch(), cm.stat_alg_msm(), cm.stat_alg_msm_resident()


def _offs(*v):
    return np.array(v, dtype=np.uint64)


def _empty(cm, chunk_bits=0):
    return cm.CtBases(np.zeros((0, 12), dtype=np.uint64), chunk_bits)


def _arr(*handles):
    return (vp * max(1, len(handles)))(*[h._h if hasattr(h, "_h") else h for h in handles])


def test_symbols_prototypes_and_promises(cm):
    header = open(os.path.join(ROOT, "include", "curdle_msm.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"\n \* ?", "\n", header))
    for name in NAMES:
        assert hasattr(cm._lib, name) and name in cm.SYMBOLS, name
    for proto in (
            "#define CURDLE_CT_BASES_MAX_SETS 4",
            "int curdle_msm_g1_ct_bases_sets_batch(const curdle_ct_bases* const* sets, size_t n_sets, const uint32_t* rows, "
            "const uint64_t* scalars, const size_t* offsets, size_t k, unsigned scalar_bits, uint64_t* out_jac);",
            "int curdle_msm_g1_ct_bases_sets_batch_device(const curdle_ct_bases* const* sets, size_t n_sets, const uint32_t* rows, "
            "const void* d_scalars, const size_t* offsets, size_t k, unsigned scalar_bits, uint64_t* out_jac, void* stream);",
            "typedef struct curdle_prover_ct curdle_prover_ct;",
            "int curdle_prover_ct_create(const curdle_crs* crs, unsigned chunk_bits, curdle_prover_ct** out);",
            "void curdle_prover_ct_free(curdle_prover_ct* p);",
            "int curdle_prover_ct_prove(curdle_prover_ct* p, const uint64_t* Rs, const uint64_t* Ss, const uint64_t* Ts, "
            "const uint64_t* Us, size_t ell, const uint64_t M[18], const uint32_t* perm, const uint64_t k[4], "
            "const uint64_t rs_m[16], curdle_rand* rand, uint8_t* proof_out, size_t cap, size_t* proof_len);",
            "int curdle_prover_ct_whisk_shuffle_proof(curdle_prover_ct* p, const uint8_t* pre_trackers, size_t n, curdle_rand* rand, "
            "uint8_t* post_trackers_out, uint8_t* proof_out);",
            "int curdle_stat_alg_msm_resident(unsigned long long out[4]);"):
        assert proto in flat, proto
    assert cm.CT_BASES_MAX_SETS == 4
    assert set(cm.stat_alg_msm_resident()) == {"resident_calls", "resident_pairs", "fallback_calls", "fallback_pairs"}
    for m in ("free", "prove", "whisk_shuffle_proof", "__del__"):
        assert hasattr(cm.ProverCt, m)
    for text in ("set s covers [B_s, B_s + n_s) with B_0 = 0 and B_(s+1) = B_s + n_s", "an empty set covers nothing",
                 "rows may not be null when the call has pairs",
                 "what curdle_msm_g1_ct_bases_batch returns for the same rows, scalars and offsets over ONE handle created from "
                 "the concatenated points at the same chunk_bits",
                 "WHAT THE FLAG PROMISES, WHAT IT DOES NOT PROMISE and what is OUTSIDE THE PROMISE are curdle_msm_g1_ct's, word for word.",
                 "Addresses, branch conditions and loop counts stay functions of public values only: rows, the sets' sizes, the "
                 "chunk index, chunk_bits and scalar_bits.",
                 "a lane finds its set by at most three compares",
                 "n_sets = 0 or above 4, sets whose chunk_bits differ, then the single-handle batch's order",
                 "a free during the call is deferred, for each of them",
                 "These are new entry points, not new flag bits",
                 "builds ONE table over Gs | Hs | H | Gt | Gu | one all-zero record of the CRS",
                 "THE CRS MUST OUTLIVE THE HANDLE",
                 "a CRS too large for one table ((ell + 8) C > 65,536",
                 "the contract is curdle_prove_ct's, word for word",
                 "The route depends on shapes and public points only.",
                 "the call runs exactly as curdle_prove_ct",
                 "The handle may be used by several threads at once",
                 "nothing about a scalar reaches it",
                 "the same group element, the same canonical result",
                 "PROVE_RESIDENT_TERMS"):
        assert text in flat, text
    # the knob, through the one hook that changes it
    for name in ("PROVE_RESIDENT_TERMS", "CURDLE_PROVE_RESIDENT_TERMS"):
        cm.plan_override(name, 2048)
        cm.plan_override(name, None)
    assert "PROVE_RESIDENT_TERMS," in open(os.path.join(ROOT, "go-curdleproofs_amd", "host", "knobs.h")).read()


def test_the_source_keeps_one_of_each(cm):
    csrc = os.path.join(ROOT, "go-curdleproofs_amd", "csrc")
    host = os.path.join(ROOT, "go-curdleproofs_amd", "host")
    make = open(os.path.join(ROOT, "go-curdleproofs_amd", "Makefile")).read()
    for path in glob.glob(os.path.join(csrc, "*.hip")):
        unit = os.path.basename(path)[:-4]
        assert make.count("csrc/%s.hip" % unit) == 1 and make.count("build/%s.o" % unit) >= 1, unit
    # one definition of each function of the constant-time G1 layer, ONE rows walk kernel and ONE rows_call
    homes = {"void add_ct(": "g1_add_ct.h", "void madd_bit(": "g1_walk_ct.h", "u32 walk_ct(": "g1_walk_ct.h",
             "void msm_ct_lane(": "msm_ct_lane.h", "k_msm_ct_walk_rows(const": "msm_ct_bases_kernels.hip",
             "int rows_call(": "msm_ct_bases_api.hip", "hipLaunchKernelGGL(k_msm_ct_walk_rows": "msm_ct_bases_kernels.hip"}
    defs = {d: [] for d in homes}
    for path in glob.glob(os.path.join(csrc, "*")):
        text = open(path, errors="replace").read()
        for d in defs:
            defs[d] += [os.path.basename(path)] * text.count(d)
    assert defs == {d: [home] for d, home in homes.items()}
    kernels = open(os.path.join(csrc, "msm_ct_bases_kernels.hip")).read()
    assert kernels.count("__global__") == 2 and "CtRowSets sets" in kernels and kernels.count("msm_ct_lane(") == 1
    api = open(os.path.join(csrc, "msm_ct_bases_api.hip")).read()
    assert api.count("launch_msm_ct_walk_rows(") == 1 and api.count("rows_call(") == 3     # the definition, the single call, the batch
    # the host layer names the device calls weakly
    alg = re.sub(r"\s+", " ", open(os.path.join(host, "algebra.cpp")).read())
    for name in ("curdle_ct_bases_create", "curdle_ct_bases_free", "curdle_msm_g1_ct_bases_sets_batch"):
        assert re.search(r'extern "C" (int|void) %s\([^;]*\) __attribute__\(\(weak\)\);' % name, alg), name
    assert "bool ResidentBasesScope::Available() { return curdle_ct_bases_create && curdle_ct_bases_free && curdle_msm_g1_ct_bases_sets_batch; }" in alg


def test_the_sets_call_refuses_before_device_work_in_order(cm):
    """On EMPTY handles, which need no device: every index is out of range for them, so the row check is the last refusal
    such a call can reach."""
    batch, bdev = _fns(cm)
    before = _stats(cm)
    err = cm.last_error
    out = np.full(40, 77, dtype=np.uint64)
    o = out.ctypes.data
    e16, f16, e64 = _empty(cm, 16), _empty(cm), _empty(cm, 64)
    one, two, five = _arr(e16), _arr(e16, f16), _arr(e16, f16, e16, f16, e16)
    good, down = _offs(0, 2, 3), _offs(0, 3, 2)
    many = np.zeros(KMAX + 2, dtype=np.uint64)
    g, d, m = good.ctypes.data, down.ctypes.data, many.ctypes.data
    row0 = np.zeros(4, dtype=np.uint32)
    r0 = row0.ctypes.data

    def both(sets, n_sets, rows, scalars, offs, k, bits, outp, what):
        for rc in (batch(sets, n_sets, rows, scalars, offs, k, bits, outp), bdev(sets, n_sets, rows, scalars, offs, k, bits, outp, None)):
            assert rc == cm.EINVAL and what in err(), (rc, err(), what)

    # 1. a null argument -- sets, a set, offsets; out_jac and the scalars when k > 0; rows when the call has pairs --
    #    before the set count (5, 0), the chunk widths, scalar_bits and k
    for sets, n_sets in ((one, 0), (one, 1), (five, 5)):
        for bits in (0, 255, 256):
            both(None, n_sets, r0, FAKE, g, 2, bits, o, "null argument")
            both(sets, n_sets, r0, FAKE, None, 2, bits, o, "null argument")
            both(sets, n_sets, r0, None, g, 2, bits, o, "null argument")
            both(sets, n_sets, r0, FAKE, g, 2, bits, None, "null argument")
            both(sets, n_sets, None, FAKE, g, 2, bits, o, "null argument")
    both(_arr(e16, None), 2, r0, FAKE, g, 2, 255, o, "null argument")
    both(_arr(None, e16, e64), 3, r0, FAKE, g, 2, 0, o, "null argument")
    both(_arr(e16, e64, f16, None, e16), 5, r0, FAKE, g, 2, 0, o, "null argument")       # the fourth of five: still the null
    # 2. the set count, before the chunk widths and everything of the single-handle batch
    for bits in (0, 255):
        both(five, 5, r0, FAKE, g, 2, bits, o, "n_sets")
        both(one, 0, r0, FAKE, g, 2, bits, o, "n_sets")
        both(_arr(e16, e64, e16, e64, e16), 1 << 40, r0, FAKE, d, KMAX + 1, bits, o, "n_sets")
    # 3. differing chunk widths, before scalar_bits, k and the offsets
    for bits in (0, 255):
        both(_arr(e16, e64), 2, r0, FAKE, d, 2, bits, o, "chunk_bits differ")
        both(_arr(e16, f16, e16, e64), 4, r0, FAKE, m, KMAX + 1, bits, o, "chunk_bits differ")
    # 4. then the single-handle batch's order: scalar_bits, k, offsets that decrease, the term total, the rows
    for bits in (0, 256, 1 << 31):
        both(two, 2, r0, FAKE, m, KMAX + 1, bits, o, "scalar_bits")
        both(two, 2, r0, FAKE, d, 2, bits, o, "scalar_bits")
    both(two, 2, r0, FAKE, m, KMAX + 1, 255, o, "4,096")
    both(two, 2, FAKE, FAKE, d, 2, 255, o, "decrease")
    for sets, c in ((two, 16), (_arr(e64, e64), 64)):
        for bits in (1, c + 1, 255):
            n = MAX // ((bits + c - 1) // c) + 1
            both(sets, 2, FAKE, FAKE, _offs(3, 5, n + 3).ctypes.data, 2, bits, o, "65,536")
    # a row equal to the total size (0 for empty sets): the last refusal
    both(two, 2, r0, FAKE, g, 2, 255, o, "not below")
    both(_arr(e16, f16, e16, f16), 4, r0, FAKE, g, 2, 9, o, "not below")
    # the alignment, reached by a batch of empty MSMs, where rows may be null
    for off in (1, 4, 8):
        assert bdev(two, 2, None, FAKE + off, _offs(2, 2, 2).ctypes.data, 2, 255, o, None) == cm.EINVAL and "multiples of 16" in err()
    assert (out == 77).all()
    # what needs no device: k = 0 writes nothing, empty MSMs give the infinity encoding
    assert batch(two, 2, None, None, g, 0, 255, None) == cm.OK
    assert batch(two, 2, None, FAKE, _offs(9, 9, 9).ctypes.data, 2, 255, o) == cm.OK
    inf = cm.msm_g1_ct_bases_sets_batch([e16, f16], None, np.zeros((0, 4), dtype=np.uint64), [0, 0])
    assert (out[:36].reshape(2, 18) == inf[0]).all() and (out[36:] == 77).all()
    with pytest.raises(cm.CurdleError) as e:
        cm.msm_g1_ct_bases_sets_batch([e16, e64], np.zeros(3, dtype=np.uint32), np.zeros((3, 4), dtype=np.uint64), [0, 3])
    assert e.value.code == cm.EINVAL and "chunk_bits differ" in e.value.msg
    assert _f(cm, "curdle_stat_alg_msm_resident", vp)(None) == cm.EINVAL
    assert _stats(cm) == before


def test_the_prover_refuses_with_outputs_untouched_and_rand_not_advanced(cm):
    create = _f(cm, "curdle_prover_ct_create", vp, C.c_uint, vp)
    prove = _f(cm, "curdle_prover_ct_prove", vp, vp, vp, vp, vp, C.c_size_t, vp, vp, vp, vp, vp, vp, C.c_size_t, vp)
    whisk = _f(cm, "curdle_prover_ct_whisk_shuffle_proof", vp, vp, C.c_size_t, vp, vp, vp)
    _f(cm, "curdle_prover_ct_free", vp, restype=None)(None)
    err = cm.last_error
    before = _stats(cm)
    crs = cm.CRS(4, cm.Rand(3))
    h = vp(12345)
    # create: a null argument, then chunk_bits, each with *out null
    assert create(None, 7, C.byref(h)) == cm.EINVAL and "null argument" in err() and h.value is None
    assert create(crs._h, 7, None) == cm.EINVAL and "null argument" in err()
    for c in (1, 7, 9, 24, 65, 128):
        h.value = 12345
        assert create(crs._h, c, C.byref(h)) == cm.EINVAL and "chunk_bits" in err() and h.value is None
    with pytest.raises(cm.CurdleError) as e:
        cm.ProverCt(crs, 12)
    assert e.value.code == cm.EINVAL and "chunk_bits" in e.value.msg
    # prove and the Whisk form on a null handle: the null argument, nothing written, nothing drawn
    rand, same = cm.Rand(9), cm.Rand(9)
    out = np.full(64, 0x5A, dtype=np.uint8)
    n = C.c_size_t(77)
    assert prove(None, FAKE, FAKE, FAKE, FAKE, 4, FAKE, FAKE, FAKE, FAKE, rand._h, out.ctypes.data, 64, C.byref(n)) == cm.EINVAL
    assert "null argument" in err()
    assert whisk(None, FAKE, 124, rand._h, out.ctypes.data, out.ctypes.data) == cm.EINVAL and "null argument" in err()
    assert n.value == 77 and (out == 0x5A).all()
    assert (rand.get_frs(2) == same.get_frs(2)).all()
    assert _stats(cm) == before


def test_no_device_no_fallback(cm):
    """Without a device a handle cannot be made: CURDLE_ENODEV, *out null, nothing counted (with one, the GPU tests
    speak).  A CRS too large for one table is refused before the device is looked for."""
    create = _f(cm, "curdle_prover_ct_create", vp, C.c_uint, vp)
    crs = cm.CRS(12, cm.Rand(3))
    before = _stats(cm)
    # (ell + 8) C > 65,536: ell = 2,044 at chunk_bits 8 is 2,052 x 32 records
    big = cm.CRS(2044, cm.Rand(5))
    h = vp(12345)
    assert create(big._h, 8, C.byref(h)) == cm.EINVAL and "too large for one table" in cm.last_error() and h.value is None
    if not cm.device_available():
        for c in (0, 8, 16, 32, 64):
            h = vp(12345)
            assert create(crs._h, c, C.byref(h)) == cm.ENODEV and h.value is None
            with pytest.raises(cm.CurdleError) as e:
                cm.ProverCt(crs, c)
            assert e.value.code == cm.ENODEV
        h = vp(12345)
        assert create(big._h, 16, C.byref(h)) == cm.ENODEV and h.value is None           # this one fits: 2,052 x 16
    assert _stats(cm) == before
