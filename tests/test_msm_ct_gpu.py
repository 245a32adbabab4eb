"""The constant-time MSM on the GPU (csrc/msm_ct_kernels.hip): curdle_msm_g1_ct / _device bit for bit against
curdle_msm_g1 on the same inputs AND against the point of the big-integer model (tests/msm_ct_model.py, whose expected
words come from the C oracle, not from the library).  The cases are the model's: the arms of add_ct in isolation at
n = 2, sizes either side of a wave, a block and the one-block tail of the sum (512) with random terms, all terms
equal (doublings at the balanced levels), P / -P alternating (whole subtrees at infinity) and zeros, 1, r - 1 and
infinity bases at the edges; every scalar_bits with the scalars at the top of the range and a scalar of exactly
2^bits refused; 65,536 pairs once and 65,537 refused; beside an ordinary MSM; the counters."""
import threading

import numpy as np
import pytest

import msm_ct_model as mm

pytestmark = pytest.mark.gpu


class Env:
    def __init__(self, gpu, oracle, coracle):
        self.gpu, self.o, self.co = gpu, oracle, coracle

    def stats(self):
        return self.gpu.stat_msm_ct(), self.gpu.stat_g1_mul_ct(), self.gpu.stat_normalize()

    def resident(self, pts, sc, bits, stream=None):
        """The resident call; the caller's arrays are as they were afterwards."""
        import torch
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1)).to("cuda:0")
        d_pts, d_sc = dev(pts), dev(sc)
        torch.cuda.synchronize()
        try:
            return self.gpu.msm_g1_ct_device(d_pts.data_ptr(), d_sc.data_ptr(), len(pts), bits, stream=stream or 0)
        finally:
            assert (d_pts.cpu().numpy().view(np.uint64).reshape(pts.shape) == pts).all()
            assert (d_sc.cpu().numpy().view(np.uint64).reshape(sc.shape) == sc).all()

    def check(self, name, pairs, bits, forms=("host", "device")):
        """One case through the named entry forms: the model's point, curdle_msm_g1's words, the counters."""
        pts, sc, want, _ = mm.build(self.o, self.co, pairs, bits)
        assert (self.gpu.msm_g1(pts, sc) == want).all(), name              # the default MSM on the same input
        for form in forms:
            before = self.stats()
            got = self.gpu.msm_g1_ct(pts, sc, bits) if form == "host" else self.resident(pts, sc, bits)
            after = self.stats()
            assert (got == want).all(), (name, form)
            d = {k: after[0][k] - before[0][k] for k in after[0]}
            assert d == {"pairs": len(pairs), "walks": 1, "sums": 1} and after[1:] == before[1:], (name, form)


@pytest.fixture(scope="module")
def env(gpu, oracle, coracle):
    return Env(gpu, oracle, coracle)


def test_the_arms_in_isolation(env):
    for name, pairs, bits in mm.arm_cases(env.o):
        env.check(name, pairs, bits)


@pytest.mark.parametrize("n", mm.SIZES)
def test_sizes(env, n):
    """Random, all equal, P / -P alternating and the edges family, through both entry forms."""
    for name, pairs, bits in mm.size_cases(env.o, n):
        env.check(name, pairs, bits)


def test_scalar_bits_with_the_scalars_at_the_top(env):
    for name, pairs, bits in mm.bits_cases(env.o):
        env.check(name, pairs, bits)
    # a smaller bound than the call needs is the same sum: 9-bit scalars walked at 9, 64 and 255 steps
    pairs = [(k & 511, g) for k, g in mm.size_cases(env.o, 65)[0][1]]
    for bits in (9, 64, 255):
        env.check("9-bit scalars at %d steps" % bits, pairs, bits, forms=("device",))


def test_a_scalar_of_exactly_two_to_the_bits_is_refused(env):
    """CURDLE_EINVAL, the guard words around out_jac intact, nothing counted; the same call with that scalar one lower
    passes afterwards (the status word is cleared by every call)."""
    cm = env.gpu
    import ctypes as C
    for name, pairs, bits in mm.violation_cases(env.o):
        pts, sc = mm.arrays(env.o, env.co, pairs)
        before = env.stats()
        out = np.full(22, 77, dtype=np.uint64)
        rc = cm._lib.curdle_msm_g1_ct(C.c_void_p(pts.ctypes.data), C.c_void_p(sc.ctypes.data), C.c_size_t(len(pairs)),
                                      C.c_uint(bits), C.c_void_p(out[2:].ctypes.data))
        assert rc == cm.EINVAL and "scalar_bits" in cm.last_error(), name
        assert (out == 77).all(), name
        with pytest.raises(cm.CurdleError) as e:
            env.resident(pts, sc, bits)
        assert e.value.code == cm.EINVAL and "scalar_bits" in e.value.msg, name
        assert env.stats() == before, name
    name, pairs, bits = mm.violation_cases(env.o)[-1]
    env.check(name + ", one lower", [(k - 1 if mm.violates(k, bits) else k, g) for k, g in pairs], bits)


def test_a_callers_stream(env):
    """The inputs are written on the caller's stream immediately before the call."""
    import torch
    name, pairs, bits = mm.size_cases(env.o, 257)[3]
    pts, sc, want, _ = mm.build(env.o, env.co, pairs, bits)
    src = torch.from_numpy(np.concatenate([pts.reshape(-1), sc.reshape(-1)]).view(np.int64)).pin_memory()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_in = torch.zeros_like(src, device="cuda:0")
        d_in.copy_(src, non_blocking=True)
        got = env.gpu.msm_g1_ct_device(d_in.data_ptr(), d_in.data_ptr() + 96 * len(pairs), len(pairs), bits, stream=s.cuda_stream)
        back = d_in.cpu().numpy()
    assert (got == want).all() and (back == src.numpy()).all()
    torch.cuda.synchronize()
    assert (env.resident(pts, sc, bits, stream=s.cuda_stream) == want).all()


def test_65536_pairs_once_and_65537_refused(env):
    """256 full blocks, seven sum launches and the tail; against curdle_msm_g1 and the C oracle."""
    n = mm.MAX_PAIRS
    k, q = env.o.Rand(26).get_frs(2)
    pts = env.co.points_walk(k, q, n)
    sc = np.random.default_rng(26).integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    sc[:, 3] &= np.uint64((1 << 62) - 1)                                    # Montgomery words of canonical scalars: < r
    want = env.co.msm_pippenger(pts, sc, threads=8)
    before = env.stats()
    got = env.resident(pts, sc, 255)
    after = env.stats()
    assert (got == want).all() and (env.gpu.msm_g1(pts, sc) == want).all()
    assert after[0]["pairs"] - before[0]["pairs"] == n and after[0]["sums"] - before[0]["sums"] == 1
    with pytest.raises(env.gpu.CurdleError) as e:
        env.gpu.msm_g1_ct(np.zeros((n + 1, 12), dtype=np.uint64), np.zeros((n + 1, 4), dtype=np.uint64))
    assert e.value.code == env.gpu.EINVAL and "65,536" in e.value.msg
    assert env.stats() == after


def test_one_thread_beside_an_ordinary_msm(env):
    name, pairs, bits = mm.size_cases(env.o, 513)[0]
    pts, sc, want, _ = mm.build(env.o, env.co, pairs, bits)
    k, q = env.o.Rand(1).get_frs(2)
    bases = env.co.points_walk(k, q, 4096)
    t = np.random.default_rng(4096).integers(0, 1 << 62, size=(4096, 4), dtype=np.uint64)
    exp = env.co.msm_pippenger(bases, t, threads=4)
    errors = []

    def worker():
        try:
            for _ in range(3):
                assert (env.gpu.msm_g1_ct(pts, sc, bits) == want).all()
                assert (env.resident(pts, sc, bits) == want).all()
        except BaseException as e:  # noqa: BLE001 - reported by the main thread
            errors.append(e)

    th = threading.Thread(target=worker)
    th.start()
    msms = [env.gpu.msm_g1(bases, t) for _ in range(3)]
    th.join()
    assert not errors, errors
    for got in msms:
        assert (got == exp).all()
