"""The batched constant-time MSM on the GPU (csrc/msm_ct_kernels.hip: one k_msm_ct_walk over all pairs, k_g1_sum_ct_seg,
k_msm_ct_finish_seg): curdle_msm_g1_ct_batch / _device and curdle_msm_g1_ct_multi bit for bit against curdle_msm_g1_ct
per MSM, against curdle_msm_g1_batch (curdle_msm_g1_multi) on the same input AND against the point of the big-integer
model (tests/msm_ct_batch_model.py, whose expected words come from the C oracle, not from the library).  The cases are
the model's; every array starts LEAD pairs into its buffer (offsets[0] = 7), so that no offset is a multiple of 64."""
import ctypes as C
import threading

import numpy as np
import pytest

import msm_ct_batch_model as bm
import msm_ct_model as mm

pytestmark = pytest.mark.gpu
GUARD = 0x5A


class Env:
    def __init__(self, gpu, oracle, coracle):
        self.gpu, self.o, self.co = gpu, oracle, coracle
        self.inf = np.array(oracle.jac_to_mont_limbs(oracle.INF), dtype=np.uint64)

    def stats(self):
        return self.gpu.stat_msm_ct(), self.gpu.stat_msm_ct_batch(), self.gpu.stat_g1_mul_ct(), self.gpu.stat_normalize()

    def moved(self, before, pairs, k, nonempty, levels):
        """The counters of ONE completed batched call."""
        after = self.stats()
        ct = {n: after[0][n] - before[0][n] for n in after[0]}
        bt = {n: after[1][n] - before[1][n] for n in after[1]}
        assert ct == {"pairs": pairs, "walks": 1, "sums": nonempty}, ct
        assert bt == {"calls": 1, "msms": k, "levels": levels}, bt
        assert after[2:] == before[2:]

    def resident(self, pts, sc, offs, bits, stream=None):
        """The resident call on arrays that sit at record offsets between guard bytes; the caller's arrays and the
        guards are as they were afterwards."""
        import torch
        lead, tail = 96 * 3, 32 * 5                                        # multiples of 16
        raw = np.full(lead + pts.nbytes + 64 + sc.nbytes + tail, GUARD, dtype=np.uint8)
        p0, s0 = lead, lead + pts.nbytes + 64
        raw[p0:p0 + pts.nbytes] = pts.view(np.uint8).reshape(-1)
        raw[s0:s0 + sc.nbytes] = sc.view(np.uint8).reshape(-1)
        d = torch.from_numpy(raw).to("cuda:0")
        assert d.data_ptr() % 16 == 0
        torch.cuda.synchronize()
        try:
            return self.gpu.msm_g1_ct_batch_device(d.data_ptr() + p0, d.data_ptr() + s0, offs, bits, stream=stream or 0)
        finally:
            assert (d.cpu().numpy() == raw).all()

    def singles(self, pts, sc, offs, bits):
        """curdle_msm_g1_ct per MSM."""
        return np.array([self.gpu.msm_g1_ct(pts[int(offs[j]):int(offs[j + 1])], sc[int(offs[j]):int(offs[j + 1])], bits)
                         for j in range(len(offs) - 1)], dtype=np.uint64).reshape(-1, 18)

    def check(self, name, segs, bits, forms=("host", "device"), singles=True):
        """One case through the named entry forms: the model's point per MSM, curdle_msm_g1_batch's words,
        curdle_msm_g1_ct's per MSM, the counters."""
        pts, sc, offs = bm.arrays(self.o, self.co, segs)
        want = bm.expected(self.o, self.co, segs, bits)
        counts = [len(s) for s in segs]
        assert (self.gpu.msm_g1_batch(pts, sc, offs) == want).all(), name   # the bucket MSM on the same input
        if singles:
            assert (self.singles(pts, sc, offs, bits) == want).all(), name
        for form in forms:
            before = self.stats()
            got = self.gpu.msm_g1_ct_batch(pts, sc, offs, bits) if form == "host" else self.resident(pts, sc, offs, bits)
            assert (got == want).all(), (name, form)
            self.moved(before, sum(counts), len(counts), sum(1 for c in counts if c), bm.level_launches(counts))


@pytest.fixture(scope="module")
def env(gpu, oracle, coracle):
    return Env(gpu, oracle, coracle)


def test_one_msm_is_the_single_call(env):
    for name, segs, bits in bm.k1_cases(env.o):
        env.check(name, segs, bits)


def test_mixed_segments_with_empty_msms_first_in_the_middle_and_last(env):
    name, segs, bits = bm.mixed_case(env.o)
    assert [len(s) for s in segs] == list(bm.MIXED_COUNTS)
    env.check(name, segs, bits)
    got = env.gpu.msm_g1_ct_batch(*bm.arrays(env.o, env.co, segs), bits)
    assert all((got[j] == env.inf).all() for j in (0, 5, 9))


def test_the_boundaries_between_segments(env):
    for name, segs, bits in bm.boundary_cases(env.o):
        env.check(name, segs, bits)


def test_the_level_path(env):
    """[513, 3, 1025, 0, 512] takes exactly 2 level launches, [512, 512] none: read from curdle_stat_msm_ct_batch."""
    (name, segs, bits), (name0, segs0, bits0) = bm.level_cases(env.o)
    before = env.gpu.stat_msm_ct_batch()["levels"]
    env.check(name, segs, bits, forms=("device",), singles=False)
    assert env.gpu.stat_msm_ct_batch()["levels"] - before == 2
    env.check(name, segs, bits, forms=("host",))
    before = env.gpu.stat_msm_ct_batch()["levels"]
    env.check(name0, segs0, bits0)
    assert env.gpu.stat_msm_ct_batch()["levels"] == before


def test_proves_round_shape(env):
    name, segs, bits = bm.round_case(env.o)
    env.check(name, segs, bits)


def test_the_limits(env):
    """4,096 MSMs of 16 pairs (65,536 pairs) once, against curdle_msm_g1_batch and the C oracle; 4,097 MSMs and 65,537
    pairs refused."""
    gpu = env.gpu
    k, n = bm.MAX_MSMS, bm.MAX_PAIRS
    a, q = env.o.Rand(28).get_frs(2)
    pts = env.co.points_walk(a, q, n)
    sc = np.random.default_rng(28).integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    sc[:, 3] &= np.uint64((1 << 62) - 1)                                    # Montgomery words of canonical scalars: < r
    offs = np.arange(k + 1, dtype=np.uint64) * np.uint64(16)
    before = env.stats()
    got = gpu.msm_g1_ct_batch(pts, sc, offs)
    env.moved(before, n, k, k, 0)
    assert (got == gpu.msm_g1_batch(pts, sc, offs)).all()
    for j in (0, 1, 2047, 4095):
        assert (got[j] == env.co.msm_pippenger(pts[16 * j:16 * j + 16], sc[16 * j:16 * j + 16], threads=4)).all(), j
        assert (got[j] == gpu.msm_g1_ct(pts[16 * j:16 * j + 16], sc[16 * j:16 * j + 16])).all(), j
    after = env.stats()
    with pytest.raises(gpu.CurdleError) as e:
        gpu.msm_g1_ct_batch(pts, sc, np.arange(k + 2, dtype=np.uint64))
    assert e.value.code == gpu.EINVAL and "4,096" in e.value.msg
    with pytest.raises(gpu.CurdleError) as e:
        gpu.msm_g1_ct_batch(pts, sc, [0, 1, n + 1])
    assert e.value.code == gpu.EINVAL and "65,536" in e.value.msg
    assert env.stats() == after


def test_scalar_bits_with_the_scalars_at_the_top(env):
    for name, segs, bits in bm.bits_cases(env.o):
        env.check(name, segs, bits)


def test_one_scalar_of_two_to_the_bits_in_the_last_msm_fails_the_whole_call(env):
    """CURDLE_EINVAL, the guard words around ALL k results intact, nothing counted; the same call with that scalar one
    lower passes afterwards (the status word is cleared by every call)."""
    gpu = env.gpu
    for name, segs, bits in bm.violation_cases(env.o):
        pts, sc, offs = bm.arrays(env.o, env.co, segs)
        k = len(segs)
        before = env.stats()
        out = np.full(18 * k + 4, 77, dtype=np.uint64)
        rc = gpu._lib.curdle_msm_g1_ct_batch(C.c_void_p(pts.ctypes.data), C.c_void_p(sc.ctypes.data), C.c_void_p(offs.ctypes.data),
                                             C.c_size_t(k), C.c_uint(bits), C.c_void_p(out[2:].ctypes.data))
        assert rc == gpu.EINVAL and "scalar_bits" in gpu.last_error(), name
        assert (out == 77).all(), name
        with pytest.raises(gpu.CurdleError) as e:
            env.resident(pts, sc, offs, bits)
        assert e.value.code == gpu.EINVAL and "scalar_bits" in e.value.msg, name
        assert env.stats() == before, name
        lower = [[(kk - 1 if mm.violates(kk, bits) else kk, g) for kk, g in s] for s in segs]
        env.check(name + ", one lower", lower, bits)


def test_the_device_form_on_a_callers_stream_and_on_the_librarys(env):
    import torch
    name, segs, bits = bm.mixed_case(env.o)
    pts, sc, offs = bm.arrays(env.o, env.co, segs)
    want = bm.expected(env.o, env.co, segs, bits)
    s = torch.cuda.Stream()
    # the inputs are written on the caller's stream immediately before the call
    src = torch.from_numpy(np.concatenate([pts.reshape(-1), sc.reshape(-1)]).view(np.int64)).pin_memory()
    with torch.cuda.stream(s):
        d_in = torch.zeros_like(src, device="cuda:0")
        d_in.copy_(src, non_blocking=True)
        got = env.gpu.msm_g1_ct_batch_device(d_in.data_ptr(), d_in.data_ptr() + pts.nbytes, offs, bits, stream=s.cuda_stream)
        back = d_in.cpu().numpy()
    assert (got == want).all() and (back == src.numpy()).all()
    torch.cuda.synchronize()
    assert (env.resident(pts, sc, offs, bits, stream=s.cuda_stream) == want).all()
    assert (env.resident(pts, sc, offs, bits) == want).all()


@pytest.mark.parametrize("k,n", bm.MULTI_SHAPES)
def test_one_scalar_vector_against_k_base_sets(env, k, n):
    """Against curdle_msm_g1_multi, the batch form with replicated scalars and the model."""
    gpu = env.gpu
    name, gsets, ks, bits = [c for c in bm.multi_cases(env.o) if len(c[1]) == k and len(c[2]) == n][0]
    segs = bm.multi_as_batch(gsets, ks)
    pts, sc, offs = bm.arrays(env.o, env.co, segs, lead=0)
    sets = [pts[int(offs[j]):int(offs[j + 1])] for j in range(k)]
    want = bm.expected(env.o, env.co, segs, bits)
    before = env.stats()
    got = gpu.msm_g1_ct_multi(sets, sc[:n], bits)
    env.moved(before, k * n, k, k, 0)
    assert (got == want).all(), name
    assert (gpu.msm_g1_multi(sets, sc[:n]) == want).all(), name
    assert (gpu.msm_g1_ct_batch(pts, sc, offs, bits) == want).all(), name


def test_one_thread_beside_a_bucket_msm(env):
    name, segs, bits = bm.round_case(env.o)
    pts, sc, offs = bm.arrays(env.o, env.co, segs)
    want = bm.expected(env.o, env.co, segs, bits)
    a, q = env.o.Rand(1).get_frs(2)
    bases = env.co.points_walk(a, q, 4096)
    t = np.random.default_rng(4096).integers(0, 1 << 62, size=(4096, 4), dtype=np.uint64)
    exp = env.co.msm_pippenger(bases, t, threads=4)
    errors = []

    def worker():
        try:
            for _ in range(3):
                assert (env.gpu.msm_g1_ct_batch(pts, sc, offs, bits) == want).all()
                assert (env.resident(pts, sc, offs, bits) == want).all()
        except BaseException as e:  # noqa: BLE001 - reported by the main thread
            errors.append(e)

    th = threading.Thread(target=worker)
    th.start()
    msms = [env.gpu.msm_g1(bases, t) for _ in range(3)]
    th.join()
    assert not errors, errors
    for got in msms:
        assert (got == exp).all()


def test_the_counters(env):
    """Both constant-time counters move as the header says: pairs walked, ONE walk, the MSMs that are not empty; one
    batched call, its MSMs, its level launches.  A refused call and a call that needs no device count nothing."""
    gpu = env.gpu
    name, segs, bits = bm.mixed_case(env.o)
    pts, sc, offs = bm.arrays(env.o, env.co, segs)
    before = env.stats()
    gpu.msm_g1_ct_batch(pts, sc, offs, bits)
    env.moved(before, 267, 10, 7, 0)
    before = env.stats()
    gpu.msm_g1_ct_batch(pts, sc, [7, 7, 7])
    gpu.msm_g1_ct_batch(pts, sc, [7])
    with pytest.raises(gpu.CurdleError):
        gpu.msm_g1_ct_batch(pts, sc, [7, 9, 8])
    assert env.stats() == before
    # the single call counts in its own counter only
    gpu.msm_g1_ct(pts[:5], sc[:5])
    after = env.stats()
    assert after[1] == before[1] and after[0]["sums"] - before[0]["sums"] == 1
