"""curdle_g1_fixed_base_mul_batch / _device on the GPU (fbase_kernels.hip) against the big-integer model of
tests/fbase_model.py, bit for bit: both output forms, host and resident entry, the generator's table and a second base
(7 G through curdle_fbase_create).  The kernel takes one lane per scalar in blocks of 256 and walks 32 unsigned 8-bit
digits, so the scalars are the model's digit families (every window as the first addition, runs of zero digits, every
digit 0xff, the top byte of r - 1) and the sizes straddle a wave, a block and a pass (FBASE_PASS = 256)."""
import threading

import numpy as np
import pytest

import fbase_model as fm

pytestmark = pytest.mark.gpu

AFF, COMP = 0, 1


class Env:
    def __init__(self, gpu, oracle, coracle):
        self.gpu, self.o, self.co = gpu, oracle, coracle
        self.other = gpu.FBase(coracle.scalar_mul_gen(fm.OTHER_BASE))
        self.bases = ((None, None), (self.other, fm.OTHER_BASE))

    def want(self, ks, ms=None, base_int=None):
        prod = [fm.product(k, None if ms is None else ms[i]) for i, k in enumerate(ks)]
        return fm.expected_arrays(self.o, self.co, prod, base_int)

    def resident(self, sc, mu, form, base=None, stream=None, off=0):
        """The resident call; compressed output at byte offset `off` between guard bytes.  Returns the output rows."""
        import torch
        n, rec = len(sc), (48 if form == COMP else 96)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1)).to("cuda:0")
        d_sc, d_mu = dev(sc), (dev(mu) if mu is not None else None)
        d_out = torch.full((n * rec + 32,), 0x5A, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        self.gpu.g1_fixed_base_mul_batch_device(d_sc.data_ptr(), d_mu.data_ptr() if mu is not None else 0, n,
                                                d_out.data_ptr() + 16 + off, base=base, out_form=form, stream=stream)
        out = d_out.cpu().numpy()
        assert (out[:16 + off] == 0x5A).all() and (out[16 + off + n * rec:] == 0x5A).all()     # nothing outside the rows
        assert (d_sc.cpu().numpy().view(np.uint64).reshape(-1, 4) == sc).all()                 # the caller's scalars are as they were
        body = out[16 + off: 16 + off + n * rec].copy()
        return body.reshape(n, 48) if form == COMP else body.view(np.uint64).reshape(n, 12)

    def every_way(self, ks, ms=None, bases=None, names=None):
        """Host and resident entry, both forms, over `bases`."""
        sc = fm.to_limbs(self.o, ks)
        mu = fm.to_limbs(self.o, ms) if ms is not None else None
        for base, base_int in (bases or self.bases):
            aff, comp = self.want(ks, ms, base_int)
            for form, want in ((AFF, aff), (COMP, comp)):
                same(self.gpu.g1_fixed_base_mul_batch(sc, mu, base=base, out_form=form), want, names)
                same(self.resident(sc, mu, form, base), want, names)
        return aff, comp


def same(got, want, names=None):
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} rows differ, first at {bad[0]}" + (f" ({names[bad[0]]})" if names else "")


@pytest.fixture(scope="module")
def env(gpu, oracle, coracle):
    e = Env(gpu, oracle, coracle)
    yield e
    e.other.free()


@pytest.fixture(scope="module")
def families(oracle):
    return fm.digit_families(oracle)


@pytest.mark.parametrize("family", ["small_and_top", "single_digits", "all_ff", "zero_runs", "low_zero", "randoms"])
def test_digit_families(env, families, family):
    cases = families[family]
    assert 8 <= len(cases) < 1000
    aff, comp = env.every_way([k for _, k in cases], names=[n for n, _ in cases])
    if family == "small_and_top":
        assert not aff[0].any() and bytes(comp[0]) == bytes([0xC0]) + bytes(47)          # 0 * P
        assert bytes(comp[1]) == env.o.compress(env.o.scalar_mul(fm.OTHER_BASE, env.o.G1))


def test_multiplier_form(env):
    cases = fm.multiplier_cases(env.o)
    ks, ms = [s for _, s, _ in cases], [m for _, _, m in cases]
    aff, _ = env.every_way(ks, ms, names=[n for n, _, _ in cases])
    by = {n: j for j, (n, _, _) in enumerate(cases)}
    assert not aff[by["m=0"]].any() and not aff[by["s=0"]].any() and aff[by["m=1"]].any()
    # a null multiplier array against an array of ones: identical output
    sc, ones = fm.to_limbs(env.o, ks), fm.to_limbs(env.o, [1] * len(ks))
    for form in (AFF, COMP):
        a = env.gpu.g1_fixed_base_mul_batch(sc, None, out_form=form)
        b = env.gpu.g1_fixed_base_mul_batch(sc, ones, out_form=form)
        assert (a == b).all()
        assert (env.resident(sc, None, form) == env.resident(sc, ones, form)).all() and (a == env.resident(sc, ones, form)).all()


HOLES = {"none": lambda n: set(), "first": lambda n: {0}, "last": lambda n: {n - 1},
         "a run of 64": lambda n: set(range(n // 2, min(n, n // 2 + 64))), "everywhere": lambda n: set(range(n))}


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_sizes_with_infinity_results(env, families, n):
    """The edges of a wave and of a block; scalar 0 (an infinity result) first, last, in a run of 64 and everywhere."""
    pool = [k for _, k in families["randoms"]]
    for where, holes in HOLES.items():
        at = holes(n)
        ks = [0 if i in at else pool[(i * 7 + n) % len(pool)] for i in range(n)]
        bases = env.bases if where in ("none", "a run of 64") else env.bases[:1]
        aff, _ = env.every_way(ks, bases=bases)
        assert int((~aff.any(axis=1)).sum()) == len(at), where


@pytest.mark.parametrize("n", [256, 257, 513])
def test_the_pass_boundary(env, families, n):
    """FBASE_PASS = 256: ceil(n / 256) launches per call, and the rows on both sides of the boundary are exact."""
    pool = [k for _, k in families["randoms"]]
    ks = [pool[(3 * i + n) % len(pool)] for i in range(n)]
    ms = [pool[(5 * i + 1) % len(pool)] for i in range(n)]
    ks[255], ms[0] = 0, 0
    passes = (n + 255) // 256
    with env.gpu.knobs(FBASE_PASS=256):
        for m in (None, ms):
            a = env.gpu.stat_fbase()
            env.every_way(ks, m, bases=env.bases[:1])
            b = env.gpu.stat_fbase()
            assert b["launches"] - a["launches"] == 4 * passes and b["scalars"] - a["scalars"] == 4 * n
            assert b["tables"] == a["tables"]
    with env.gpu.knobs(FBASE_PASS=300):                  # rounded down to 256
        a = env.gpu.stat_fbase()
        env.gpu.g1_fixed_base_mul_batch(fm.to_limbs(env.o, ks))
        assert env.gpu.stat_fbase()["launches"] - a["launches"] == passes
    a = env.gpu.stat_fbase()
    env.gpu.g1_fixed_base_mul_batch(fm.to_limbs(env.o, ks))
    assert env.gpu.stat_fbase()["launches"] - a["launches"] == 1


@pytest.mark.parametrize("off", [0, 1, 3])
def test_resident_on_a_callers_stream_and_at_byte_offsets(env, families, off):
    """The scalars are written on the caller's stream immediately before the call; the compressed output starts `off`
    bytes into its array; then the same on the library's own stream."""
    import torch
    ks = [k for _, k in families["low_zero"]] + [k for _, k in families["randoms"]][:268]
    ms = list(reversed(ks))
    sc, mu = fm.to_limbs(env.o, ks), fm.to_limbs(env.o, ms)
    n = len(ks)
    aff, comp = env.want(ks, ms)
    src = torch.from_numpy(np.concatenate([sc, mu]).view(np.int64).reshape(-1)).pin_memory()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_in = torch.zeros_like(src, device="cuda:0")
        d_c = torch.full((n * 48 + 32,), 0x5A, dtype=torch.uint8, device="cuda:0")
        d_a = torch.zeros(n * 12, dtype=torch.int64, device="cuda:0")
        d_in.copy_(src, non_blocking=True)
        env.gpu.g1_fixed_base_mul_batch_device(d_in.data_ptr(), d_in.data_ptr() + 32 * n, n, d_c.data_ptr() + 16 + off,
                                               out_form=COMP, stream=s.cuda_stream)
        env.gpu.g1_fixed_base_mul_batch_device(d_in.data_ptr(), d_in.data_ptr() + 32 * n, n, d_a.data_ptr(),
                                               out_form=AFF, stream=s.cuda_stream)
        out = d_c.cpu().numpy()
        got_a = d_a.cpu().numpy().view(np.uint64).reshape(n, 12)
    same(out[16 + off: 16 + off + 48 * n].reshape(n, 48), comp)
    assert (out[:16 + off] == 0x5A).all() and (out[16 + off + 48 * n:] == 0x5A).all()
    same(got_a, aff)
    torch.cuda.synchronize()
    same(env.resident(sc, mu, COMP, off=off), comp)      # the library's own stream
    same(env.resident(sc, mu, COMP, env.other, off=off), env.want(ks, ms, fm.OTHER_BASE)[1])


@pytest.fixture(scope="module")
def three_hundred(env, families):
    ks = ([k for _, k in families["randoms"]] + [k for _, k in families["single_digits"]] + [0, 1, fm.R - 1])[:300]
    ks[17] = 0
    return ks, fm.to_limbs(env.o, ks), env.want(ks)[0]


def test_resident_results_are_msm_bases(env, three_hundred):
    """The 300 affine results go straight, still resident, to curdle_msm_g1_device as bases on the caller's stream."""
    import torch
    ks, sc, want = three_hundred
    n = len(ks)
    rng = np.random.default_rng(17)
    t = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    t[:, 3] &= np.uint64((1 << 62) - 1)                                                # < r
    exp = env.co.msm_pippenger(want, t, threads=4)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_sc = torch.from_numpy(sc.view(np.int64)).to("cuda:0")
        d_t = torch.from_numpy(t.view(np.int64)).to("cuda:0")
        d_out = torch.zeros(n * 12, dtype=torch.int64, device="cuda:0")
        env.gpu.g1_fixed_base_mul_batch_device(d_sc.data_ptr(), 0, n, d_out.data_ptr(), stream=s.cuda_stream)
        got = env.gpu.msm_g1_device(d_out.data_ptr(), d_t.data_ptr(), n, stream=s.cuda_stream)
    assert (got == exp).all()
    same(d_out.cpu().numpy().view(np.uint64).reshape(n, 12), want)


def test_the_glv_chain_over_the_replicated_base_gives_identical_records(env, three_hundred):
    """The parent's only way to the same points: curdle_g1_scalar_mul_batch_device over the base replicated n times."""
    import torch
    ks, sc, want = three_hundred
    n = len(ks)
    for base, base_int in env.bases:
        pts = np.tile(np.array(env.co.scalar_mul_gen(base_int or 1), dtype=np.uint64), (n, 1))
        d_p = torch.from_numpy(pts.view(np.int64)).to("cuda:0")
        d_sc = torch.from_numpy(sc.view(np.int64)).to("cuda:0")
        d_chain = torch.zeros(n * 12, dtype=torch.int64, device="cuda:0")
        d_fb = torch.zeros(n * 12, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        env.gpu.g1_scalar_mul_batch_device(d_p.data_ptr(), d_sc.data_ptr(), n, 0, n, d_chain.data_ptr())
        env.gpu.g1_fixed_base_mul_batch_device(d_sc.data_ptr(), 0, n, d_fb.data_ptr(), base=base)
        assert torch.equal(d_chain, d_fb)
        if base is None:
            same(d_fb.cpu().numpy().view(np.uint64).reshape(n, 12), want)


def test_two_threads_beside_an_msm(env, three_hundred):
    ks, sc, want = three_hundred
    want_c = env.want(ks)[1]
    want_o = env.want(ks, None, fm.OTHER_BASE)[0]
    k, q = env.o.Rand(1).get_frs(2)
    pts = env.co.points_walk(k, q, 4096)
    rng = np.random.default_rng(4096)
    t = rng.integers(0, 1 << 64, size=(4096, 4), dtype=np.uint64)
    t[:, 3] &= np.uint64((1 << 62) - 1)
    exp = env.co.msm_pippenger(pts, t, threads=4)
    errors = []

    def worker(which):
        try:
            for r in range(4):
                if (which + r) % 2:
                    same(env.gpu.g1_fixed_base_mul_batch(sc, out_form=COMP), want_c)
                    same(env.resident(sc, None, AFF, env.other), want_o)
                else:
                    same(env.gpu.g1_fixed_base_mul_batch(sc, base=env.other), want_o)
                    same(env.resident(sc, None, COMP), want_c)
        except BaseException as e:  # noqa: BLE001 - reported by the main thread
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(w,)) for w in range(2)]
    for th in threads:
        th.start()
    msms = [env.gpu.msm_g1(pts, t) for _ in range(3)]
    for th in threads:
        th.join()
    assert not errors, errors
    for got in msms:
        assert (got == exp).all()


def test_two_handles_alive_at_once(env, three_hundred):
    """A second handle (11 G) beside the first and the generator's: each call multiplies by its own base; a freed handle
    leaves the others as they were, and every handle built one table."""
    ks, sc, _ = three_hundred
    ks, sc = ks[:65], sc[:65]
    a = env.gpu.stat_fbase()
    eleven = env.gpu.FBase(env.co.scalar_mul_gen(11))
    assert env.gpu.stat_fbase()["tables"] - a["tables"] == 1
    for _ in range(2):
        same(env.gpu.g1_fixed_base_mul_batch(sc, base=eleven), env.want(ks, None, 11)[0])
        same(env.gpu.g1_fixed_base_mul_batch(sc, base=env.other), env.want(ks, None, fm.OTHER_BASE)[0])
        same(env.gpu.g1_fixed_base_mul_batch(sc), env.want(ks)[0])
    eleven.free()
    with pytest.raises(ValueError):
        env.gpu.g1_fixed_base_mul_batch(sc, base=eleven)          # never the generator's table by accident
    same(env.gpu.g1_fixed_base_mul_batch(sc, base=env.other, out_form=COMP), env.want(ks, None, fm.OTHER_BASE)[1])
    assert env.gpu.stat_fbase()["tables"] - a["tables"] == 1


def test_the_generators_table_is_built_once_under_a_race_and_handles_survive_a_shutdown(env, three_hundred):
    """After curdle_shutdown the context's copies are gone: two threads race for the generator's table in their first
    calls and ONE is built; the handle of 7 G, made before the shutdown, re-makes its copy on its next use."""
    ks, sc, want = three_hundred
    env.gpu.shutdown()
    env.gpu.init(0)
    a = env.gpu.stat_fbase()
    errors, gate = [], threading.Barrier(2)

    def worker():
        try:
            gate.wait()
            same(env.gpu.g1_fixed_base_mul_batch(sc), want)
        except BaseException as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=worker) for _ in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    b = env.gpu.stat_fbase()
    assert b["tables"] - a["tables"] == 1 and b["launches"] - a["launches"] == 2
    same(env.gpu.g1_fixed_base_mul_batch(sc, base=env.other), env.want(ks, None, fm.OTHER_BASE)[0])
    assert env.gpu.stat_fbase()["tables"] - a["tables"] == 2
    same(env.gpu.g1_fixed_base_mul_batch(sc), want)
    assert env.gpu.stat_fbase()["tables"] - a["tables"] == 2
