"""The constant-time prover's entry points at the C ABI, without a GPU: curdle_fr_permute_ct / _device,
curdle_stat_fr_permute_ct, curdle_prove_ct, curdle_whisk_generate_shuffle_proof_ct and curdle_stat_host_point_mul exist as
include/curdle_msm.h declares them, the header states the promise in the three-part form and keeps every sentence of
curdle_prove_ex's, an empty gather needs no device, everything malformed is refused before any device work in the stated
order (the refused calls pass pointers that name no memory) with the outputs untouched and rand not advanced, and
without a device the three device-backed calls fail with CURDLE_ENODEV: no host fallback."""
import ctypes as C
import inspect
import os
import re
import threading

import numpy as np
import pytest

from test_normalize_abi import FAKE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("curdle_fr_permute_ct", "curdle_fr_permute_ct_device", "curdle_stat_fr_permute_ct", "curdle_prove_ct",
         "curdle_whisk_generate_shuffle_proof_ct", "curdle_stat_host_point_mul")
vp = C.c_void_p
NMAX = 4096


def _f(cm, name, *argtypes):
    f = getattr(cm._lib, name)
    f.restype = C.c_int
    f.argtypes = list(argtypes)
    return f


def _fns(cm):
    return (_f(cm, "curdle_fr_permute_ct", vp, vp, C.c_size_t, vp),
            _f(cm, "curdle_fr_permute_ct_device", vp, vp, C.c_size_t, vp, vp),
            _f(cm, "curdle_prove_ct", vp, vp, vp, vp, vp, C.c_size_t, vp, vp, vp, vp, vp, vp, C.c_size_t, vp),
            _f(cm, "curdle_whisk_generate_shuffle_proof_ct", vp, vp, C.c_size_t, vp, vp, vp))


def _stats(cm):
    return (cm.stat_fr_permute_ct(), cm.stat_msm_ct(), cm.stat_msm_ct_batch(), cm.stat_alg_msm(), cm.stat_g1_mul_ct(),
            cm.stat_host_point_mul())


def test_symbols_prototypes_and_promises(cm):
    header = open(os.path.join(ROOT, "include", "curdle_msm.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"\n \*(?=\s)", " ", header))   # a comment's lines joined, without their " * "
    for name in NAMES:
        assert hasattr(cm._lib, name) and name in cm.SYMBOLS, name
    for proto in (
            "int curdle_fr_permute_ct(const uint64_t* in, const uint32_t* perm, size_t n, uint64_t* out);",
            "int curdle_fr_permute_ct_device(const void* d_in, const void* d_perm, size_t n, void* d_out, void* stream);",
            "int curdle_stat_fr_permute_ct(unsigned long long out[2]);",
            "int curdle_prove_ct(const curdle_crs* crs, const uint64_t* Rs, const uint64_t* Ss, const uint64_t* Ts, "
            "const uint64_t* Us, size_t ell, const uint64_t M[18], const uint32_t* perm, const uint64_t k[4], "
            "const uint64_t rs_m[16], curdle_rand* rand, uint8_t* proof_out, size_t cap, size_t* proof_len);",
            "int curdle_whisk_generate_shuffle_proof_ct(const curdle_crs* crs, const uint8_t* pre_trackers, size_t n, "
            "curdle_rand* rand, uint8_t* post_trackers_out, uint8_t* proof_out);",
            "int curdle_stat_host_point_mul(unsigned long long* out);"):
        assert proto in flat, proto
    # the binding
    assert set(cm.stat_fr_permute_ct()) == {"records", "launches"}
    assert isinstance(cm.stat_host_point_mul(), int)
    assert list(inspect.signature(cm.prove_ct).parameters) == list(inspect.signature(cm.prove).parameters)[:-1]
    assert (list(inspect.signature(cm.whisk_generate_shuffle_proof_ct).parameters)
            == list(inspect.signature(cm.whisk_generate_shuffle_proof).parameters))
    # the promise of the two calls and of the gather, in the form of the existing ones
    for text in ("k_fr_permute_ct", "alg::SecretOpsScope", "these entry points ARE the constant-time form",
                 "on the host, no branch, loop count or memory address in Prove is made of the witness, the blinders or the "
                 "permutation, except those listed as outside",
                 "what the host compiler made of the mask arithmetic",
                 "OUTSIDE THE PROMISE: rand's own code (GeneratePermutation is a Fisher-Yates that indexes by what it draws)",
                 "the range check of perm", "`if (den.IsZero()) throw` and the constraint self-check",
                 "reveal only that generation failed", "ordinary std::vector copies of the witness, which are not wiped",
                 "the proof itself", "Neither call is a default",
                 "no address, branch, loop count or exec mask of the kernel is made of perm",
                 "a null argument, n, and (the _device form) d_in / d_out that are not multiples of 16 or that overlap",
                 "an entry at or above n gives a zero record", "n <= 4,096",
                 "a null argument (proof_out may be null, as for curdle_prove), ell against the CRS, ell > 4,096, "
                 "CURDLE_PROVER_FOLD_BASES=1", "CURDLE_ENODEV, no fallback",
                 "A curdle_prove makes 14, a curdle_prove_ct 2", "profiles/r29_prove_ct.json"):
        assert text in flat, text
    assert flat.count("WHAT THE FLAG PROMISES") >= 6 and flat.count("OUTSIDE THE PROMISE") >= 6
    # curdle_prove_ex's pinned sentences are where they were
    for text in ("WHAT THE FLAG PROMISES: the DEVICE WORK OF PROVE'S MSMs, and only that",
                 "WHAT IT DOES NOT PROMISE: power draw and clock behaviour, as above; and NOTHING ABOUT THE HOST.",
                 "OUTSIDE THE PROMISE: the host-side operations of Prove on the same secrets are outside",
                 "Point::Mul calls on r_k, k, r_t and r_u", "They are the next follow-up.", "flags = 0 IS curdle_prove.",
                 "curdle_prove_ex, each under its flag"):
        assert text in flat, text
    # one gather body, two kernels, in the unit the build already lists
    kernels = open(os.path.join(ROOT, "go-curdleproofs_amd", "csrc", "msm_ct_kernels.hip")).read()
    assert "k_fr_permute_ct(" in kernels and "k_g1_permute_ct(" in kernels
    assert kernels.count("void gather_ct(") == 1 and "gather_ct<6>(" in kernels and "gather_ct<2>(" in kernels
    assert "asm(" not in kernels and "asm volatile" not in kernels
    # the host layer names the device-backed entry points weakly
    alg = re.sub(r"\s+", " ", open(os.path.join(ROOT, "go-curdleproofs_amd", "host", "algebra.cpp")).read())
    api = re.sub(r"\s+", " ", open(os.path.join(ROOT, "go-curdleproofs_amd", "host", "proto_api.cpp")).read())
    assert re.search(r'extern "C" int curdle_fr_permute_ct\([^;]*\) __attribute__\(\(weak\)\);', alg)
    for name in ("curdle_shuffle_permute_commit_ex", "curdle_device_available"):
        assert re.search(r'extern "C" int %s\([^;]*\) __attribute__\(\(weak\)\);' % name, api), name


def test_an_empty_gather_needs_no_device(cm):
    host, dev, _, _ = _fns(cm)
    before = _stats(cm)
    out = np.full(8, 77, dtype=np.uint64)
    assert host(None, None, 0, None) == cm.OK and host(FAKE, FAKE, 0, out.ctypes.data) == cm.OK
    assert dev(None, None, 0, None, None) == cm.OK and dev(FAKE + 1, FAKE + 1, 0, FAKE + 1, None) == cm.OK
    assert (out == 77).all()
    assert cm.fr_permute_ct(np.zeros((0, 4), dtype=np.uint64), np.zeros(0, dtype=np.uint32)).shape == (0, 4)
    assert _stats(cm) == before


def test_the_gather_refuses_before_device_work_in_order(cm):
    host, dev, _, _ = _fns(cm)
    before = _stats(cm)
    err = cm.last_error
    out = np.full(8, 77, dtype=np.uint64)
    o = out.ctypes.data
    # 1. a null argument: before n and before the alignment
    for n in (1, NMAX + 1, 1 << 40):
        for hole in (0, 1, 3):
            a = [FAKE + 1, FAKE + 1, n, FAKE + 1]
            a[hole] = None
            assert host(*a) == cm.EINVAL and "null argument" in err(), (n, hole)
            assert dev(*a, None) == cm.EINVAL and "null argument" in err(), (n, hole)
    # 2. n: before the alignment and the overlap; nothing behind the pointers is read
    for n in (NMAX + 1, 1 << 40):
        assert host(FAKE, FAKE, n, o) == cm.EINVAL and "4,096" in err()
        assert dev(FAKE + 1, FAKE + 1, n, FAKE + 1, None) == cm.EINVAL and "4,096" in err()
    # 3. the _device form: records not multiples of 16, records that overlap, a permutation that is no multiple of 4
    far = FAKE + (1 << 20)
    for d_in, d_perm, d_out in ((FAKE + 8, FAKE, far), (FAKE, FAKE, far + 4), (FAKE, FAKE + 2, far), (FAKE, FAKE + 1, far)):
        assert dev(d_in, d_perm, NMAX, d_out, None) == cm.EINVAL and "multiples of 16" in err()
    for n, d_in, d_out in ((1, FAKE, FAKE), (2, FAKE, FAKE + 32), (2, FAKE + 32, FAKE), (NMAX, FAKE, FAKE + 32 * NMAX - 16),
                           (NMAX, FAKE + 32 * NMAX - 16, FAKE)):
        assert dev(d_in, far, n, d_out, None) == cm.EINVAL and "overlap" in err(), (n, d_in, d_out)
    assert (out == 77).all()
    assert _f(cm, "curdle_stat_fr_permute_ct", vp)(None) == cm.EINVAL
    assert _f(cm, "curdle_stat_host_point_mul", vp)(None) == cm.EINVAL
    with pytest.raises(cm.CurdleError) as e:
        cm.fr_permute_ct(np.zeros((NMAX + 1, 4), dtype=np.uint64), np.zeros(NMAX + 1, dtype=np.uint32))
    assert e.value.code == cm.EINVAL and "4,096" in e.value.msg
    assert _stats(cm) == before


def _prove_args(cm, ell=4):
    crs, rand = cm.CRS(ell, cm.Rand(8)), cm.Rand(7)
    pts = np.zeros((ell, 12), dtype=np.uint64)
    M, k, rs_m = np.zeros(18, dtype=np.uint64), np.zeros(4, dtype=np.uint64), np.zeros(16, dtype=np.uint64)
    perm = np.arange(ell, dtype=np.uint32)
    keep = (crs, rand, pts, M, k, rs_m, perm)
    return keep, [crs._h, pts.ctypes.data, pts.ctypes.data, pts.ctypes.data, pts.ctypes.data, ell, M.ctypes.data,
                  perm.ctypes.data, k.ctypes.data, rs_m.ctypes.data, rand._h]


def test_prove_ct_refuses_in_order_before_any_draw(cm):
    """A null argument, ell against the CRS (0, 3 and 5 against 4), ell above 4,096, the fold-bases knob: CURDLE_EINVAL in
    that order, proof_out and *proof_len untouched, nothing drawn from rand, nothing counted."""
    prove = _fns(cm)[2]
    before = _stats(cm)
    keep, args = _prove_args(cm)
    rand = keep[1]
    nxt = cm.Rand(7).get_frs(1)
    buf = np.full(4096, 77, dtype=np.uint8)
    n = C.c_size_t(12345)
    tail = [buf.ctypes.data, len(buf), C.addressof(n)]
    err = cm.last_error
    # 1. null: before ell is looked at (every ell here would be refused next)
    for ell in (4, 3, NMAX + 1):
        for hole in (0, 1, 2, 3, 4, 6, 7, 8, 9, 10):
            a = list(args)
            a[5] = ell
            a[hole] = None
            assert prove(*a, *tail) == cm.EINVAL and "null argument" in err(), (ell, hole)
        a = list(args)
        a[5] = ell
        assert prove(*a, buf.ctypes.data, len(buf), None) == cm.EINVAL and "null argument" in err()
    # the pointers behind a refused call are never read
    assert prove(args[0], *([FAKE] * 4), 5, *([FAKE] * 4), args[10], FAKE, 1 << 20, C.addressof(n)) == cm.EINVAL
    assert "does not match" in err()
    # 2. ell against the CRS -- also where ell is above the cap: the CRS comes first
    for ell in (0, 3, 5, NMAX + 1):
        a = list(args)
        a[5] = ell
        assert prove(*a, *tail) == cm.EINVAL and "does not match" in err(), ell
    # 4. the fold-bases knob, with curdle_prove_ex's message; before the backend is asked for (this machine may have no device)
    with cm.knobs(PROVER_FOLD_BASES=1):
        assert prove(*args, *tail) == cm.EINVAL and "PROVER_FOLD_BASES" in err()
        msg = err()
        ex = _f(cm, "curdle_prove_ex", vp, vp, vp, vp, vp, C.c_size_t, vp, vp, vp, vp, vp, C.c_uint, vp, C.c_size_t, vp)
        assert ex(*args, cm.PROVE_MSM_CONSTANT_TIME, *tail) == cm.EINVAL and err() == msg
        with pytest.raises(cm.CurdleError) as e:
            crs, _, pts, M, k, rs_m, perm = keep
            cm.prove_ct(crs, pts, pts, pts, pts, M, perm, k, rs_m, rand)
        assert e.value.code == cm.EINVAL and "PROVER_FOLD_BASES" in e.value.msg
    assert (buf == 77).all() and n.value == 12345
    assert (rand.get_frs(1) == nxt).all()
    assert _stats(cm) == before


def test_prove_ct_refuses_ell_above_4096(cm):
    """3. ell = 4,097 against a CRS of 4,097: refused for its size, before the knob and the backend, with nothing drawn.
    (CRS generation is host work: about a second.)"""
    prove = _fns(cm)[2]
    ell = NMAX + 1
    crs, rand = cm.CRS(ell, cm.Rand(8)), cm.Rand(7)
    nxt = cm.Rand(7).get_frs(1)
    M, k, rs_m = np.zeros(18, dtype=np.uint64), np.zeros(4, dtype=np.uint64), np.zeros(16, dtype=np.uint64)
    buf = np.full(64, 77, dtype=np.uint8)
    n = C.c_size_t(12345)
    before = _stats(cm)
    call = lambda: prove(crs._h, *([FAKE] * 4), ell, M.ctypes.data, FAKE, k.ctypes.data, rs_m.ctypes.data, rand._h,
                         buf.ctypes.data, len(buf), C.addressof(n))
    assert call() == cm.EINVAL and "4,096" in cm.last_error()
    with cm.knobs(PROVER_FOLD_BASES=1):
        assert call() == cm.EINVAL and "4,096" in cm.last_error()
    assert (buf == 77).all() and n.value == 12345 and (rand.get_frs(1) == nxt).all()
    assert _stats(cm) == before


def test_whisk_ct_refuses_null_arguments(cm):
    whisk = _fns(cm)[3]
    keep, args = _prove_args(cm)
    rand = keep[1]
    nxt = cm.Rand(7).get_frs(1)
    for hole in (0, 1, 3, 4, 5):
        a = [args[0], FAKE, cm.WHISK_ELL, rand._h, FAKE, FAKE]
        a[hole] = None
        assert whisk(*a) == cm.EINVAL and "null argument" in cm.last_error(), hole
    assert (rand.get_frs(1) == nxt).all()


def test_host_point_mul_counts_the_calling_thread(cm):
    """An unflagged, non-folding Prove at ell = 4 makes 14 calls of alg::Point::Mul: three in each of the four
    GroupCommitment::New of the same-scalar argument's A, B and of T, U (X.Mul(s), crsG.Mul(r), crsH.Mul(r)), Hcrs.Mul(beta)
    in the inner-product argument and M.Mul(alpha) in the same-permutation argument.  Another thread sees none of them.
    curdle_prove needs a device for its MSMs: without one there is nothing to count."""
    if not cm.device_available():
        return
    ell = 4
    rand = cm.Rand(ell)
    crs = cm.CRS(ell, rand)
    perm = np.arange(ell, dtype=np.uint32)[::-1].copy()
    k, Rs, Ss = rand.get_fr(), rand.get_g1_affines(ell), rand.get_g1_affines(ell)
    Ts, Us, M, rs_m = cm.shuffle_permute_commit(crs, Rs, Ss, perm, k, rand)
    seen = []
    th = threading.Thread(target=lambda: seen.append(cm.stat_host_point_mul()))
    th.start()
    th.join()
    before = cm.stat_host_point_mul()
    cm.prove(crs, Rs, Ss, Ts, Us, M, perm, k, rs_m, cm.Rand(1))
    assert cm.stat_host_point_mul() - before == 14
    th = threading.Thread(target=lambda: seen.append(cm.stat_host_point_mul()))
    th.start()
    th.join()
    assert seen[1] - seen[0] == 0


def test_no_device_no_fallback(cm):
    """Without a device the three device-backed calls fail with CURDLE_ENODEV, count nothing and draw nothing (with one,
    the GPU tests speak)."""
    if cm.device_available():
        return
    before = _stats(cm)
    (crs, rand, z, M, k, rs_m, perm), _ = _prove_args(cm)
    nxt = cm.Rand(7).get_frs(1)
    recs = np.arange(12, dtype=np.uint64).reshape(3, 4)
    pre = [bytes(96)] * cm.WHISK_ELL
    for call in (lambda: cm.fr_permute_ct(recs, [2, 0, 1]), lambda: cm.fr_permute_ct_device(FAKE, FAKE, 3, FAKE + 4096),
                 lambda: cm.prove_ct(crs, z, z, z, z, M, perm, k, rs_m, rand),
                 lambda: cm.whisk_generate_shuffle_proof_ct(crs, pre, rand)):
        with pytest.raises(cm.CurdleError) as e:
            call()
        assert e.value.code == cm.ENODEV
    assert (rand.get_frs(1) == nxt).all()
    assert _stats(cm) == before
