"""Batch proving at the C ABI, without a GPU: curdle_prove_batch, curdle_whisk_generate_shuffle_proof_batch,
curdle_stat_prove_batch and the batched oblivious gather (curdle_fr_permute_ct_batch / _batch_device,
curdle_g1_permute_ct_batch_device) exist as include/curdle_msm.h declares them and the header carries the promise; k = 0
and n = 0 need no device; every refusal happens before any thread starts or any device work, in the stated order, with
the outputs untouched and rand not advanced; without a device the flagged calls fail with CURDLE_ENODEV; the two knobs
are known; and the gather kernels still share one body."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_normalize_abi import FAKE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("curdle_prove_batch", "curdle_whisk_generate_shuffle_proof_batch", "curdle_stat_prove_batch",
         "curdle_fr_permute_ct_batch", "curdle_fr_permute_ct_batch_device", "curdle_g1_permute_ct_batch_device")
vp = C.c_void_p
CT = 1
ELL = 4


def _f(cm, name, *argtypes):
    f = getattr(cm._lib, name)
    f.restype = C.c_int
    f.argtypes = list(argtypes)
    return f


def test_symbols_prototypes_and_the_promise(cm):
    header = open(os.path.join(ROOT, "include", "curdle_msm.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"\n \* ", " ", header))         # comment blocks as running text
    for name in NAMES:
        assert hasattr(cm._lib, name) and name in cm.SYMBOLS, name
    for proto in (
            "#define CURDLE_PROVE_BATCH_CONSTANT_TIME 1u",
            "int curdle_prove_batch(const curdle_crs* crs, size_t k, size_t ell, const uint64_t* const* Rs, const uint64_t* const* Ss, "
            "const uint64_t* const* Ts, const uint64_t* const* Us, const uint64_t* Ms /* k x 18 */, const uint32_t* const* perms, "
            "const uint64_t* ks /* k x 4 */, const uint64_t* rs_ms /* k x 16 */, curdle_rand* const* rands, unsigned flags, "
            "uint8_t* proofs_out, size_t stride, size_t* proof_lens, int* status);",
            "int curdle_whisk_generate_shuffle_proof_batch(const curdle_crs* crs, size_t k, const uint8_t* const* pre_trackers, size_t n, "
            "curdle_rand* const* rands, unsigned flags, uint8_t* post_trackers_out, uint8_t* proofs_out, int* status);",
            "int curdle_stat_prove_batch(unsigned long long out[4]);",
            "int curdle_fr_permute_ct_batch(const uint64_t* in, const uint32_t* perm, size_t n, size_t k, uint64_t* out);",
            "int curdle_fr_permute_ct_batch_device(const void* d_in, const void* d_perm, size_t n, size_t k, void* d_out, void* stream);",
            "int curdle_g1_permute_ct_batch_device(const void* d_in, const void* d_perm, size_t n, size_t k, void* d_out, void* stream);"):
        assert proto in flat, proto
    for text in ("bit for bit, those of the single call on member i's arguments",
                 "per member what curdle_prove_ct promises",
                 "the coalesced staging",
                 "is wiped like the single calls' staging",
                 "the member threads are the library's own",
                 "it is not a default",
                 "an undefined flag bit, a null argument",
                 "k = 0 is CURDLE_OK without a device",
                 "never another member's"):
        assert text in flat, text
    assert cm.PROVE_BATCH_CONSTANT_TIME == CT
    assert set(cm.stat_prove_batch()) == {"calls", "members", "groups", "device_calls"}
    for name in ("prove_batch", "whisk_generate_shuffle_proof_batch", "fr_permute_ct_batch", "fr_permute_ct_batch_device",
                 "g1_permute_ct_batch_device"):
        assert callable(getattr(cm, name)), name


def test_the_two_knobs_are_known(cm):
    for name in ("PROVE_BATCH_GROUP", "CURDLE_PROVE_BATCH_PAIRS"):
        cm.plan_override(name, 2)
        cm.plan_override(name, None)
    with pytest.raises(cm.CurdleError):
        cm.plan_override("PROVE_BATCH_NOTHING", 2)
    knobs_h = open(os.path.join(ROOT, "go-curdleproofs_amd", "host", "knobs.h")).read()
    assert "PROVE_BATCH_GROUP," in knobs_h and "PROVE_BATCH_PAIRS," in knobs_h


def test_one_body_for_the_gather_kernels():
    src = open(os.path.join(ROOT, "go-curdleproofs_amd", "csrc", "msm_ct_kernels.hip")).read()
    assert len(re.findall(r"void gather_ct\(", src)) == 1
    assert len(re.findall(r"template <int RecordBytes>\s*__global__ void __launch_bounds__\(kPermuteSegBlock\)\s*k_permute_ct_seg\(", src)) == 1
    # the three kernels call it and none walks the records on its own
    for kernel in ("k_g1_permute_ct", "k_fr_permute_ct", "k_permute_ct_seg"):
        body = src[src.index(kernel + "("):]
        body = body[:body.index("\n}\n")]
        assert "gather_ct<" in body and "for (" not in body, kernel
    assert "k_permute_ct_seg<32>" in src and "k_permute_ct_seg<96>" in src


def test_the_gather_s_empty_calls_and_refusals_need_no_device(cm):
    host = _f(cm, "curdle_fr_permute_ct_batch", vp, vp, C.c_size_t, C.c_size_t, vp)
    fr = _f(cm, "curdle_fr_permute_ct_batch_device", vp, vp, C.c_size_t, C.c_size_t, vp, vp)
    g1 = _f(cm, "curdle_g1_permute_ct_batch_device", vp, vp, C.c_size_t, C.c_size_t, vp, vp)
    before = cm.stat_fr_permute_ct()
    out = np.full(64, 77, dtype=np.uint8)
    for n, k in ((0, 0), (0, 9), (9, 0), (0, 5000), (5000, 0)):   # nothing to do: no pointer is looked at, no size either
        assert host(None, None, n, k, None) == cm.OK
        assert host(FAKE, FAKE, n, k, out.ctypes.data) == cm.OK
        for dev in (fr, g1):
            assert dev(None, None, n, k, None, None) == cm.OK
            assert dev(FAKE + 1, FAKE + 2, n, k, FAKE + 3, None) == cm.OK
    err = lambda: cm.last_error()
    for call in (lambda *a: host(*a), lambda *a: fr(*a, None), lambda *a: g1(*a, None)):
        # a null argument first, then n, then k, then k n
        assert call(None, FAKE, 4097, 4097, FAKE) == cm.EINVAL and "null argument" in err()
        assert call(FAKE, None, 2, 2, FAKE) == cm.EINVAL and "null argument" in err()
        assert call(FAKE, FAKE, 2, 2, None) == cm.EINVAL and "null argument" in err()
        assert call(FAKE, FAKE, 4097, 4097, FAKE) == cm.EINVAL and "4,096 records" in err()
        assert call(FAKE, FAKE, 2, 4097, FAKE) == cm.EINVAL and "4,096 members" in err()
        assert call(FAKE, FAKE, 4096, 257, FAKE) == cm.EINVAL and "2^20" in err()
    for dev in (fr, g1):                                          # then the pointers of the resident forms
        assert dev(FAKE + 8, FAKE, 4096, 257, FAKE, None) == cm.EINVAL and "2^20" in err()
        assert dev(FAKE + 8, FAKE, 2, 2, FAKE + 4096, None) == cm.EINVAL and "multiples of 16" in err()
        assert dev(FAKE, FAKE, 2, 2, FAKE + 4096 + 4, None) == cm.EINVAL and "multiples of 16" in err()
        assert dev(FAKE, FAKE + 2, 2, 2, FAKE + 4096, None) == cm.EINVAL and "multiple of 4" in err()
        assert dev(FAKE, FAKE, 2, 2, FAKE + 32, None) == cm.EINVAL and "overlap" in err()
    assert (out == 77).all()
    assert cm.stat_fr_permute_ct() == before
    assert cm.fr_permute_ct_batch(np.zeros((0, 4), dtype=np.uint64), np.zeros(0, dtype=np.uint32), 0, 3).shape == (0, 4)


class Batch:
    """Raw arguments of curdle_prove_batch for k members at ELL whose arrays hold 0x4D bytes: a refused call reads none."""

    def __init__(self, cm, k=2, ell=ELL):
        self.k = k
        self.arrs = [[np.full((ell, 12), 0x4D4D4D4D4D4D4D4D, dtype=np.uint64) for _ in range(k)] for _ in range(4)]
        self.perms = [np.arange(ell, dtype=np.uint32) for _ in range(k)]
        self.Ms = np.full((k, 18), 0x4D, dtype=np.uint64)
        self.ks = np.full((k, 4), 0x4D, dtype=np.uint64)
        self.rs_ms = np.full((k, 16), 0x4D, dtype=np.uint64)
        self.rands = [cm.Rand(50 + i) for i in range(k)]
        self.out = np.full(k * 4096, 0x5A, dtype=np.uint8)
        self.lens = (C.c_size_t * k)(*([777] * k))
        self.status = (C.c_int * k)(*([777] * k))
        self.f = _f(cm, "curdle_prove_batch", vp, C.c_size_t, C.c_size_t, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_uint, vp,
                    C.c_size_t, vp, vp)

    def args(self, crs, ell=ELL, flags=0):
        tab = lambda xs: (C.c_void_p * self.k)(*[x.ctypes.data for x in xs])
        rands = (C.c_void_p * self.k)(*[r._h if isinstance(r._h, int) else r._h.value for r in self.rands])
        self.keep = [tab(a) for a in self.arrs] + [tab(self.perms), rands]
        p = lambda a: C.cast(a, vp).value
        return [crs._h, self.k, ell, p(self.keep[0]), p(self.keep[1]), p(self.keep[2]), p(self.keep[3]), self.Ms.ctypes.data,
                p(self.keep[4]), self.ks.ctypes.data, self.rs_ms.ctypes.data, p(self.keep[5]), flags, self.out.ctypes.data, 4096,
                C.cast(self.lens, vp).value, C.cast(self.status, vp).value]

    def untouched(self, cm):
        assert (self.out == 0x5A).all() and list(self.lens) == [777] * self.k and list(self.status) == [777] * self.k
        for i, r in enumerate(self.rands):                       # not advanced: the next draw is a fresh generator's first
            assert (r.get_frs(1) == cm.Rand(50 + i).get_frs(1)).all()
        self.rands = [cm.Rand(50 + i) for i in range(self.k)]


@pytest.fixture(scope="module")
def crs(cm):
    return cm.CRS(ELL, cm.Rand(3))


def test_prove_batch_refusals_in_order(cm, crs):
    b = Batch(cm)
    before = cm.stat_prove_batch()
    err = lambda: cm.last_error()
    for flags in (0, CT):
        # an undefined flag bit before everything, null arguments included
        a = b.args(crs, flags=flags | 2)
        a[0] = None
        assert b.f(*a) == cm.EINVAL and "unknown flag bits 0x2" in err()
        # then a null argument: each top-level pointer, then a member's (ell is wrong here too: the null comes first)
        for hole in (0, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 16):
            a = b.args(crs, ell=ELL + 1, flags=flags)
            a[hole] = None
            assert b.f(*a) == cm.EINVAL and "null argument" in err(), hole
        a = b.args(crs, ell=ELL + 1, flags=flags)
        b.keep[2][1] = None
        assert b.f(*a) == cm.EINVAL and "null argument in batch member" in err()
        a = b.args(crs, ell=ELL + 1, flags=flags)
        b.keep[5][0] = None
        assert b.f(*a) == cm.EINVAL and "null argument in batch member" in err()
        a = b.args(crs, ell=ELL + 1, flags=flags)
        b.keep[5][1] = b.keep[5][0]
        assert b.f(*a) == cm.EINVAL and "share one rand" in err()
        # then ell against the CRS
        assert b.f(*b.args(crs, ell=ELL + 1, flags=flags)) == cm.EINVAL and "does not match the CRS" in err()
        b.untouched(cm)
    # under the flag curdle_prove_ct's own refusals, in its order: PROVER_FOLD_BASES before the backend
    with cm.knobs(PROVER_FOLD_BASES=1):
        assert b.f(*b.args(crs, flags=CT)) == cm.EINVAL and "PROVER_FOLD_BASES" in err()
    b.untouched(cm)
    assert cm.stat_prove_batch() == before


def test_ell_4097_is_refused_under_the_flag_before_the_backend_is_asked(cm):
    big = cm.CRS(4097, cm.Rand(3))
    b = Batch(cm, k=1, ell=4097)
    before = cm.stat_prove_batch()
    assert b.f(*b.args(big, ell=4097, flags=CT)) == cm.EINVAL and "4,096" in cm.last_error()
    b.untouched(cm)
    assert cm.stat_prove_batch() == before


def test_k_0_needs_no_device(cm, crs):
    before = cm.stat_prove_batch()
    f = Batch(cm).f
    for flags in (0, CT):
        assert f(crs._h, 0, ELL, None, None, None, None, None, None, None, None, None, flags, None, 0, None, None) == cm.OK
        assert cm.prove_batch(crs, [], flags) == ([], [])
        assert cm.whisk_generate_shuffle_proof_batch(crs, [], [], flags) == ([], [], [])
    assert f(None, 0, ELL, None, None, None, None, None, None, None, None, None, 0, None, 0, None, None) == cm.EINVAL
    assert cm.stat_prove_batch() == before


def test_whisk_batch_refusals(cm, crs):
    f = _f(cm, "curdle_whisk_generate_shuffle_proof_batch", vp, C.c_size_t, vp, C.c_size_t, vp, C.c_uint, vp, vp, vp)
    pre = np.full(96 * 124, 0x4D, dtype=np.uint8)
    rand = cm.Rand(9)
    h = rand._h if isinstance(rand._h, int) else rand._h.value
    tab, rands = (C.c_void_p * 1)(pre.ctypes.data), (C.c_void_p * 1)(h)
    out = np.full(96 * 124 + 4576, 0x5A, dtype=np.uint8)
    status = (C.c_int * 1)(777)
    p = lambda a: C.cast(a, vp).value
    args = [crs._h, 1, p(tab), 124, p(rands), 0, out.ctypes.data, out.ctypes.data + 96 * 124, p(status)]
    bad = list(args)
    bad[5], bad[0] = 2, None
    assert f(*bad) == cm.EINVAL and "unknown flag bits" in cm.last_error()
    for hole in (0, 2, 4, 6, 7, 8):
        bad = list(args)
        bad[hole] = None
        assert f(*bad) == cm.EINVAL and "null argument" in cm.last_error(), hole
    assert (out == 0x5A).all() and status[0] == 777
    assert (rand.get_frs(1) == cm.Rand(9).get_frs(1)).all()


def test_no_device_no_fallback(cm, crs):
    """Without a device the flagged calls fail with CURDLE_ENODEV, write nothing and draw nothing (with one, the GPU tests
    speak)."""
    if cm.device_available():
        return
    b = Batch(cm)
    before = cm.stat_prove_batch()
    assert b.f(*b.args(crs, flags=CT)) == cm.ENODEV
    b.untouched(cm)
    rand = cm.Rand(9)
    with pytest.raises(cm.CurdleError) as e:
        cm.whisk_generate_shuffle_proof_batch(crs, [[bytes(96)] * 124], [rand], CT)
    assert e.value.code == cm.ENODEV
    assert (rand.get_frs(1) == cm.Rand(9).get_frs(1)).all()
    assert cm.stat_prove_batch() == before
