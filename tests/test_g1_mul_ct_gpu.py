"""CURDLE_G1_MUL_CONSTANT_TIME on the GPU (k_g1_mul_ct, csrc/g1_mul_ct_kernels.hip): the flagged entry points against
the big-integer model of tests/g1_mul_ct_model.py, bit for bit -- the expected records come from the C oracle, not from
the library -- and, second, against the untouched default chain on the same inputs.  The kernel takes one lane per
(point, scalar) pair in blocks of 256 and walks 255 bits with a doubling and an always-performed addition, so the
scalars are the model's families (every single bit as the first addition, every run of ones, r - 1 with its discarded
P + (-P), the GLV eigenvalue) over the generator, random points, P beside -P and infinity, and the sizes straddle a
wave, a block and a pass (G1_MUL_CT_PASS = 256).  The counters prove which kernel ran."""
import threading

import numpy as np
import pytest

import g1_mul_ct_model as gm

pytestmark = pytest.mark.gpu

CT = 1
FAMILIES = ["special", "single_bits", "all_ones", "randoms", "low_zero", "high_zero"]


def same(got, want, names=None):
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} rows differ, first at {bad[0]}" + (f" ({names[bad[0]]})" if names else "")


class Env:
    def __init__(self, gpu, oracle, coracle):
        self.gpu, self.o, self.co = gpu, oracle, coracle

    def stats(self):
        return self.gpu.stat_g1_mul_ct(), self.gpu.stat_normalize()

    def arrays(self, pairs):
        return gm.arrays(self.o, self.co, pairs)

    def resident(self, pts, sc, flags=CT, stream=None, off=0, in_place=False):
        """The resident call: the records start `off` records into their array, between guard bytes.  sc (n, 4) or one
        shared (4,).  Returns the output rows; the caller's scalars (and points, unless in place) are as they were."""
        import torch
        n = len(pts)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1)).to("cuda:0")
        d_pts, d_sc = dev(pts), dev(sc)
        d_out = torch.full((96 * (n + off) + 32,), 0x5A, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        ns = 1 if sc.ndim == 1 else n
        out_ptr = d_pts.data_ptr() if in_place else d_out.data_ptr() + 16 + 96 * off
        self.gpu.g1_scalar_mul_batch_device(d_pts.data_ptr(), d_sc.data_ptr(), ns, 0, n, out_ptr, stream=stream, flags=flags)
        assert (d_sc.cpu().numpy().view(np.uint64).reshape(sc.shape) == sc).all()
        if in_place:
            assert (d_out.cpu().numpy() == 0x5A).all()
            return d_pts.cpu().numpy().view(np.uint64).reshape(n, 12)
        assert (d_pts.cpu().numpy().view(np.uint64).reshape(n, 12) == pts).all()
        out = d_out.cpu().numpy()
        lo, hi = 16 + 96 * off, 16 + 96 * (off + n)
        assert (out[:lo] == 0x5A).all() and (out[hi:] == 0x5A).all()         # nothing outside the rows
        return out[lo:hi].copy().view(np.uint64).reshape(n, 12)


@pytest.fixture(scope="module")
def env(gpu, oracle, coracle):
    return Env(gpu, oracle, coracle)


@pytest.fixture(scope="module")
def families(oracle):
    return gm.scalar_families(oracle)


@pytest.fixture(scope="module")
def pool(env, families):
    """300 (scalar, point) pairs over every family, with their arrays: what the size, stream and thread tests cut from."""
    ks = [k for _, k in families["randoms"]] + [k for _, k in families["special"]] * 3 + \
         [k for _, k in families["single_bits"]][::6] + [k for _, k in families["low_zero"]][:27]
    pairs = gm.pairs_for(env.o, ks[:300])
    assert len(pairs) == 300
    return pairs, env.arrays(pairs)


@pytest.mark.parametrize("family", FAMILIES)
def test_scalar_families(env, families, family):
    cases = families[family]
    names = [n for n, _ in cases]
    pairs = gm.pairs_for(env.o, [k for _, k in cases])
    if family == "special":                      # every special scalar on every point, infinity included
        pool = [g for _, g in gm.subgroup_multiples(env.o)] + [None]
        pairs = [(k, g) for _, k in cases for g in pool]
        names = [n for n, _ in cases for _ in pool]
    pts, sc, want = env.arrays(pairs)
    a, nz = env.stats()
    got = env.resident(pts, sc)
    a2, nz2 = env.stats()
    same(got, want, names)
    assert (a2["scalars"] - a["scalars"], a2["launches"] - a["launches"]) == (len(pairs), 1) and nz2 == nz
    same(env.resident(pts, sc, flags=0), got, names)                         # the default chain: the same records
    a3, nz3 = env.stats()
    assert a3 == a2 and nz3["points"] - nz2["points"] == len(pairs)         # flags = 0 is the old kernel


def test_r_minus_1_discards_p_plus_minus_p_on_real_points(env):
    """k = r - 1 on every point: the last step's discarded sum is exactly P + (-P) (the model says so), the result -P."""
    o = env.o
    assert gm.walk(gm.R - 1)[2] == [(254, "P+(-P)")]
    mult = [g for _, g in gm.subgroup_multiples(o)]
    pts, sc, want = env.arrays([(gm.R - 1, g) for g in mult])
    got = env.resident(pts, sc)
    same(got, want)
    for row, g in zip(got, mult):
        assert o.affine_from_mont_limbs([int(v) for v in row]) == o.neg(o.scalar_mul(g, o.G1))


def test_the_shared_scalar_form_at_each_special_scalar(env, families):
    mult = [g for _, g in gm.subgroup_multiples(env.o)] + [None]
    gs = [mult[i % len(mult)] for i in range(70)]                            # more than a wave
    for name, k in families["special"] + families["randoms"][:2]:
        pts, _, want = env.arrays([(k, g) for g in gs])
        one = gm.to_limbs(env.o, [k])[0]
        a, nz = env.stats()
        same(env.resident(pts, one), want, [name] * len(gs))
        assert env.gpu.stat_g1_mul_ct()["scalars"] - a["scalars"] == len(gs) and env.gpu.stat_normalize() == nz
        same(env.gpu.g1_scalar_mul_batch(pts, one, flags=CT), want)
        same(env.resident(pts, one, flags=0), want)


def test_points_whose_x_has_the_top_bits_of_p(env):
    """Curve points with x just below p.  They are outside the subgroup (order a multiple of r), where the GLV chain of
    the default path does not multiply, so the reference here is the model's walk on the points alone."""
    o = env.o
    tops = gm.top_x_points(o)
    ks = [1, 2, 3, gm.R - 1, gm.R - 2, gm.LAMBDA] + gm.fm._rand(o, 2405, 6)
    pairs = [(k, p) for k in ks for p in tops]
    pts = np.array([o.affine_to_mont_limbs(p) for _, p in pairs], dtype=np.uint64)
    want = []
    for k, p in pairs:
        q, _ = gm.walk_points(o, k, p)                                       # asserts the walk is exact on this point
        want.append(o.affine_to_mont_limbs(q))
    same(env.resident(pts, gm.to_limbs(o, [k for k, _ in pairs])), np.array(want, dtype=np.uint64))


HOLES = {"none": lambda n: set(), "first": lambda n: {0}, "last": lambda n: {n - 1}, "first and last": lambda n: {0, n - 1}}


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_sizes_with_infinity_and_zero_at_the_edges(env, pool, n):
    """The edges of a wave and of a block; k = 0 and an infinity point (both store zeros through the mask) at the first
    and at the last index."""
    base, _ = pool
    for where, holes in HOLES.items():
        at = holes(n)
        for hole in ("k=0", "P=inf"):
            if not at and hole == "P=inf":
                continue
            pairs = [base[(7 * i + n) % len(base)] for i in range(n)]
            pairs = [(k or 5, g or 1) for k, g in pairs]                    # no holes but the ones placed here
            for i in at:
                pairs[i] = (0, pairs[i][1]) if hole == "k=0" else (pairs[i][0], None)
            pts, sc, want = env.arrays(pairs)
            assert int((~want.any(axis=1)).sum()) == len(at)
            got = env.resident(pts, sc)
            same(got, want)
            if where == "first and last":
                same(env.gpu.g1_scalar_mul_batch(pts, sc, flags=CT), want)   # the host form
                same(env.resident(pts, sc, flags=0), got)


@pytest.mark.parametrize("n", [256, 257, 513])
def test_the_pass_boundary_and_the_counters(env, pool, n):
    """G1_MUL_CT_PASS = 256: both sides of the boundary are exact; a flagged call moves curdle_stat_g1_mul_ct by n and
    ceil(n / 256) and curdle_stat_normalize not at all -- and the converse for flags = 0 and the calls without flags:
    a flag that is accepted and quietly routed to the old kernel fails here."""
    base, _ = pool
    pairs = [base[(3 * i + n) % len(base)] for i in range(n)]
    pairs[255] = (0, pairs[255][1])
    pts, sc, want = env.arrays(pairs)
    passes = (n + 255) // 256
    one = sc[1]
    want_one = env.arrays([(pairs[1][0], g) for _, g in pairs])[2]
    with env.gpu.knobs(G1_MUL_CT_PASS=256):
        for scalars, exp in ((sc, want), (one, want_one)):
            for call in (lambda f: env.gpu.g1_scalar_mul_batch(pts, scalars, flags=f),
                         lambda f: env.resident(pts, scalars, flags=f),
                         lambda f: env.resident(pts, scalars, flags=f, in_place=True)):
                a, nz = env.stats()
                same(call(CT), exp)
                a2, nz2 = env.stats()
                assert (a2["scalars"] - a["scalars"], a2["launches"] - a["launches"]) == (n, passes) and nz2 == nz
                for flags in (0, None):
                    same(call(flags), exp)
                    assert env.gpu.stat_g1_mul_ct() == a2
    a, _ = env.stats()
    env.gpu.g1_scalar_mul_batch(pts, sc, flags=CT)                           # the default pass size: one launch
    assert env.gpu.stat_g1_mul_ct()["launches"] - a["launches"] == 1


@pytest.mark.parametrize("off", [1, 3])
def test_a_callers_stream_and_the_librarys_at_record_offsets(env, pool, off):
    """The inputs are written on the caller's stream immediately before the call; the records start `off` records into
    their array between guard bytes; then the same on the library's stream, and in place over the points."""
    import torch
    pairs, (pts, sc, want) = pool
    n = len(pairs)
    src = torch.from_numpy(np.concatenate([pts.reshape(-1), sc.reshape(-1)]).view(np.int64)).pin_memory()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_in = torch.zeros_like(src, device="cuda:0")
        d_out = torch.full((96 * (n + off) + 32,), 0x5A, dtype=torch.uint8, device="cuda:0")
        d_in.copy_(src, non_blocking=True)
        env.gpu.g1_scalar_mul_batch_device(d_in.data_ptr(), d_in.data_ptr() + 96 * n, n, 0, n, d_out.data_ptr() + 16 + 96 * off,
                                           stream=s.cuda_stream, flags=CT)
        out = d_out.cpu().numpy()
        back = d_in.cpu().numpy()
    lo, hi = 16 + 96 * off, 16 + 96 * (off + n)
    same(out[lo:hi].copy().view(np.uint64).reshape(n, 12), want)
    assert (out[:lo] == 0x5A).all() and (out[hi:] == 0x5A).all()
    assert (back == src.numpy()).all()                                       # points and scalars unchanged
    torch.cuda.synchronize()
    same(env.resident(pts, sc, off=off), want)                               # the library's own stream
    same(env.resident(pts, sc, stream=s.cuda_stream, off=off, in_place=True), want)
    same(env.resident(pts, sc, in_place=True), want)


def test_the_results_are_bases_of_an_msm(env, pool):
    """Records written by the flagged call go straight to curdle_msm_g1_device as bases."""
    import torch
    pairs, (pts, sc, want) = pool
    n = len(pairs)
    d_pts = torch.from_numpy(pts.view(np.int64).reshape(-1)).to("cuda:0")
    d_sc = torch.from_numpy(sc.view(np.int64).reshape(-1)).to("cuda:0")
    env.gpu.g1_scalar_mul_batch_device(d_pts.data_ptr(), d_sc.data_ptr(), n, 0, n, d_pts.data_ptr(), flags=CT)
    t = np.random.default_rng(24).integers(0, 1 << 62, size=(n, 4), dtype=np.uint64)
    d_t = torch.from_numpy(t.view(np.int64).reshape(-1)).to("cuda:0")
    got = env.gpu.msm_g1_device(d_pts.data_ptr(), d_t.data_ptr(), n)
    assert (got == env.co.msm_pippenger(want, t, threads=4)).all()


def test_65537_pairs(env, pool):
    """The one large case: 257 blocks, the last with a single lane; the pool tiled, a sample against the model, the
    whole against the default chain."""
    pairs, (pts, sc, want) = pool
    n = 65537
    idx = (np.arange(n) * 7 + 3) % len(pairs)
    big_p, big_s = pts[idx], sc[idx]
    a, nz = env.stats()
    got = env.resident(big_p, big_s)
    a2, nz2 = env.stats()
    assert (a2["scalars"] - a["scalars"], a2["launches"] - a["launches"]) == (n, 1) and nz2 == nz
    same(got, want[idx])
    same(env.resident(big_p, big_s, flags=0), got)


def test_two_threads_beside_an_msm(env, pool):
    pairs, (pts, sc, want) = pool
    k, q = env.o.Rand(1).get_frs(2)
    bases = env.co.points_walk(k, q, 4096)
    t = np.random.default_rng(4096).integers(0, 1 << 62, size=(4096, 4), dtype=np.uint64)
    exp = env.co.msm_pippenger(bases, t, threads=4)
    errors = []

    def worker(j):
        try:
            for _ in range(3):
                same(env.gpu.g1_scalar_mul_batch(pts, sc, flags=CT), want)
                same(env.resident(pts, sc, in_place=bool(j)), want)
        except BaseException as e:  # noqa: BLE001 - reported by the main thread
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(j,)) for j in range(2)]
    [th.start() for th in threads]
    msms = [env.gpu.msm_g1(bases, t) for _ in range(3)]
    [th.join() for th in threads]
    assert not errors, errors
    for got in msms:
        assert (got == exp).all()
