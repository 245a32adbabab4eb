"""curdle_g1_normalize_batch / _device and curdle_g1_scalar_mul_batch_device on the GPU (normalize_kernels.hip): every
record equals oracle.affine_to_mont_limbs of the point its input stands for, bit for bit.  The kernel shares ONE
inversion over a wave of 64 lanes with one point each (blocks of 256) up to 65,536 points and eight each beyond (knob
NORMALIZE_LANE_POINTS forces either), so the sizes straddle a wave, a block and the eight-point group of 512, every
case runs under both builds, and one batch crosses the threshold itself."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000]
JAC, XYZZ = 0, 1
LANE_POINTS = [None, 8]          # the library's rule (one point per lane at these sizes) and the wide build


def sqrt_or_none(oracle, x):
    P = oracle.P
    rhs = (x * x * x + 4) % P
    y = pow(rhs, (P + 1) // 4, P)
    return y if y * y % P == rhs else None


@pytest.fixture(scope="module")
def pool(gpu, oracle):
    """Distinct affine points, built as tests/test_compress_batch_gpu.py builds its pool: multiples of G, P beside -P,
    and curve points whose x has the top bits of p."""
    rand = oracle.Rand(4242)
    pts = []
    for _ in range(12):
        p = oracle.scalar_mul(rand.get_fr(), oracle.G1)
        pts += [p, oracle.neg(p)]
    x = oracle.P - 1
    while len(pts) < 30:
        y = sqrt_or_none(oracle, x)
        if y is not None:
            pts += [(x, y), (x, oracle.P - y)]
        x -= 1
    assert sum(1 for p in pts if p[0] >> 376 == oracle.P >> 376) >= 6           # x with the top byte of p
    return pts


def raw_limbs(v):
    return [(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(6)]


def record(oracle, form, pt, den, rng):
    """One input record for the affine point `pt` (None: infinity, with non-zero X and Y).  den: 'one', 'random',
    'unrelated' (XYZZ: ZZ and ZZZ random and not z^2, z^3), or a way to spell a zero denominator: 'zero', 'p' (limbs
    that spell p itself), 'zzz0' (XYZZ: ZZ != 0, ZZZ = 0), 'zz0' (XYZZ: ZZ = 0, ZZZ != 0)."""
    P, m = oracle.P, oracle.fp_to_mont_limbs
    rnd = lambda: int.from_bytes(rng.bytes(47), "big") + 2
    x, y = pt if pt is not None else (5, 7)
    if form == JAC:
        z = {"one": 1, "zero": 0, "p": 0}.get(den) if den != "random" else rnd()
        assert (pt is None) == (z == 0)
        if z:
            x, y = x * z * z % P, y * z * z * z % P
        return m(x) + m(y) + (raw_limbs(P) if den == "p" else m(z))
    if den == "random":
        z = rnd()
        zz, zzz = z * z % P, z * z * z % P
    else:
        zz, zzz = {"one": (1, 1), "unrelated": (rnd(), rnd()), "zero": (0, 0), "p": (0, rnd()), "zzz0": (rnd(), 0),
                   "zz0": (0, rnd())}[den]
    assert (pt is None) == (zz * zzz % P == 0)
    if pt is not None:
        x, y = x * zz % P, y * zzz % P
    return m(x) + m(y) + (raw_limbs(P) if den == "p" else m(zz)) + m(zzz)


def batch(oracle, pool, n, form, seed, inf_at=None, inf_den="zero", dens=("one", "random", "zero")):
    """n records over the pool with the denominators of `dens` in turn (a zero one makes the point infinity); the
    indices of inf_at are infinity spelled as inf_den.  Returns the limbs and the expected affine records."""
    rng = np.random.default_rng(seed)
    aff = [oracle.affine_to_mont_limbs(p) for p in pool]
    limbs, want = [], []
    for i in range(n):
        j = i % len(pool) if n > 1 else seed % len(pool)
        den = dens[(i // len(pool) + i) % len(dens)]
        if inf_at is not None:
            den = inf_den if i in inf_at else den
        if den in ("zero", "p", "zzz0", "zz0"):
            limbs.append(record(oracle, form, None, den, rng))
            want.append([0] * 12)
        else:
            limbs.append(record(oracle, form, pool[j], den, rng))
            want.append(aff[j])
    return np.array(limbs, dtype=np.uint64), np.array(want, dtype=np.uint64)


def same(got, want):
    assert got.shape == want.shape and got.dtype == np.uint64
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} records differ, first at {bad[0]}: {got[bad[0]].tolist()}"


def on_device(gpu, limbs, form, stream=None):
    import torch
    n = limbs.shape[0]
    d_in = torch.from_numpy(limbs.view(np.int64)).to("cuda:0")
    d_out = torch.zeros(n * 12, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    gpu.g1_normalize_batch_device(d_in.data_ptr(), form, n, d_out.data_ptr(), stream=stream)
    return d_out.cpu().numpy().view(np.uint64).reshape(n, 12)


def every_way(gpu, limbs, want, form):
    """Host and device entry under both builds."""
    for lp in LANE_POINTS:
        with gpu.knobs(NORMALIZE_LANE_POINTS=lp):
            same(gpu.g1_normalize_batch(limbs, form), want)
            same(on_device(gpu, limbs, form), want)


@pytest.mark.parametrize("n", SIZES)
def test_sizes(gpu, oracle, pool, n):
    """Z is 1, random or 0 in turn; both forms, host and device entry, both builds; and the host's normalisation
    (curdle_host_batch_to_affine, reached through g1_scalar_mul_batch with the scalar 1) agrees on the same points."""
    for form in (JAC, XYZZ):
        limbs, want = batch(oracle, pool, n, form, 100 * n + form)
        assert limbs.shape == (n, 18 if form == JAC else 24)
        every_way(gpu, limbs, want, form)
    assert n < 3 or (not want[2].any() and want[0].any())                       # infinities among finite points
    same(gpu.g1_scalar_mul_batch(want, np.array(oracle.fr_to_mont_limbs(1), dtype=np.uint64)), want)


HOLES = {
    "first": {0}, "last": {299}, "a whole wave": set(range(64, 128)), "a whole block": set(range(0, 256)),
    "all but one": set(range(300)) - {137}, "everything": set(range(300)),
}


@pytest.mark.parametrize("where", sorted(HOLES))
@pytest.mark.parametrize("form,inf_den", [(JAC, "zero"), (JAC, "p"), (XYZZ, "zero"), (XYZZ, "zzz0"), (XYZZ, "zz0"), (XYZZ, "p")])
def test_a_zero_denominator_touches_no_neighbour(gpu, oracle, pool, where, form, inf_den):
    """Infinity (with non-zero X and Y) at the start, at the end, over a whole wave, over a whole block, everywhere but
    one index, everywhere -- spelled as zero words, as the limbs of p, and in XYZZ with only one of ZZ, ZZZ zero: every
    other index equals the oracle."""
    inf_at = HOLES[where]
    limbs, want = batch(oracle, pool, 300, form, 7 + len(inf_at), inf_at, inf_den, dens=("one", "random"))
    some = min(inf_at)
    assert limbs[some, :6].any() and limbs[some, 6:12].any()                    # X and Y are not zero there ...
    assert inf_den == "zero" or limbs[some, 12:].any()                          # ... nor, but for 'zero', are the denominator's words
    assert int((~want.any(axis=1)).sum()) == len(inf_at)                        # and nothing else is infinity
    if where == "all but one":
        assert want[137].any()
    every_way(gpu, limbs, want, form)


def test_xyzz_with_unrelated_zz_and_zzz(gpu, oracle, pool):
    limbs, want = batch(oracle, pool, 300, XYZZ, 31, dens=("unrelated",))
    P = oracle.P
    zz, zzz = oracle.fp_from_mont_limbs(limbs[5, 12:18]), oracle.fp_from_mont_limbs(limbs[5, 18:24])
    assert pow(zz, 3, P) != zzz * zzz % P                                       # not (z^2, z^3) for any z
    every_way(gpu, limbs, want, XYZZ)


@pytest.mark.parametrize("form", [JAC, XYZZ])
@pytest.mark.parametrize("off", [1, 3])
def test_resident_points_on_a_callers_stream_at_record_offsets(gpu, oracle, pool, form, off):
    """The points are written on the caller's stream immediately before the call; both pointers are offset by `off`
    records into their arrays, and nothing is written outside the n x 96 bytes."""
    import torch
    n, rec = 300, (144 if form == JAC else 192)
    limbs, want = batch(oracle, pool, n, form, 21 + off)
    raw = np.zeros((n + 4) * rec, dtype=np.uint8)
    raw[off * rec: (off + n) * rec] = limbs.view(np.uint8).reshape(-1)
    src = torch.from_numpy(raw).pin_memory()
    for lp in LANE_POINTS:
        with gpu.knobs(NORMALIZE_LANE_POINTS=lp):
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                d_in = torch.zeros_like(src, device="cuda:0")
                d_out = torch.full(((n + 4) * 96,), 0x5A, dtype=torch.uint8, device="cuda:0")
                d_in.copy_(src, non_blocking=True)
                gpu.g1_normalize_batch_device(d_in.data_ptr() + off * rec, form, n, d_out.data_ptr() + off * 96,
                                              stream=s.cuda_stream)
                out = d_out.cpu().numpy()
            same(out[off * 96: (off + n) * 96].view(np.uint64).reshape(n, 12), want)
            assert (out[: off * 96] == 0x5A).all() and (out[(off + n) * 96:] == 0x5A).all()
            # ... and on the library's own stream
            torch.cuda.synchronize()
            d_out.fill_(0x5A)
            torch.cuda.synchronize()
            gpu.g1_normalize_batch_device(d_in.data_ptr() + off * rec, form, n, d_out.data_ptr() + off * 96)
            out = d_out.cpu().numpy()
            same(out[off * 96: (off + n) * 96].view(np.uint64).reshape(n, 12), want)
            assert (out[: off * 96] == 0x5A).all() and (out[(off + n) * 96:] == 0x5A).all()


def test_counters_and_the_threshold_between_the_builds(gpu, oracle, pool):
    """out[0] grows by n per call; out[1] by at least 1 and at most ceil(n / 64) per launch -- the inversion really is
    shared.  65,536 points still take one per lane (1,024 groups), 65,537 eight (129 groups), and both are exact."""
    for form in (JAC, XYZZ):
        small, want_small = batch(oracle, pool, 1000, form, 77 + form)
        for n in SIZES + [65536, 65537]:
            limbs, want = (np.tile(small, (66, 1))[:n], np.tile(want_small, (66, 1))[:n])
            limbs = np.ascontiguousarray(limbs)
            for lp in LANE_POINTS:
                with gpu.knobs(NORMALIZE_LANE_POINTS=lp):
                    a = gpu.stat_normalize()
                    got = gpu.g1_normalize_batch(limbs, form)
                    b = gpu.stat_normalize()
                same(got, want)
                assert b["points"] - a["points"] == n
                assert 1 <= b["groups"] - a["groups"] <= (n + 63) // 64
                if lp is None:
                    assert b["groups"] - a["groups"] == ((n + 63) // 64 if n <= 65536 else (n + 511) // 512)
                else:
                    assert b["groups"] - a["groups"] == (n + 511) // 512


# ---------------------------------------------------------------------------
# curdle_g1_scalar_mul_batch_device
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def products(gpu, oracle, pool):
    """Six points of G1 and infinity times six scalars (0, 1, r - 1 among them), from the oracle, once."""
    rand = oracle.Rand(99)
    pts = pool[:6] + [None]                                                    # points of G1: the chain splits its scalar with the endomorphism
    scal = [0, 1, oracle.R - 1] + [rand.get_fr() for _ in range(3)]
    table = {(si, pi): oracle.scalar_mul(s, p) if p is not None else None for si, s in enumerate(scal) for pi, p in enumerate(pts)}
    return pts, scal, table


def mul_case(oracle, products, n, shared, with_addends):
    """points, scalars, addends (or None) as gnark limbs, and the expected affine records."""
    pts, scal, table = products
    pi = [i % len(pts) for i in range(n)]
    si = [shared] * n if shared is not None else [(i // len(pts) + i) % len(scal) for i in range(n)]
    prod = [table[(s, p)] for s, p in zip(si, pi)]
    adds = None
    if with_addends:
        adds = []
        for i in range(n):
            if i % 11 == 4:
                adds.append(oracle.neg(prod[i]) if prod[i] is not None else None)      # the result is infinity
            else:
                adds.append(pts[(5 * i + 3) % len(pts)])                               # infinity as an addend too
        want = [oracle.add(a, p) for a, p in zip(adds, prod)]
        assert n < 5 or prod[4] is None or want[4] is None
    else:
        want = prod
    lim = lambda ps: np.array([oracle.affine_to_mont_limbs(p) for p in ps], dtype=np.uint64)
    sc = np.array([oracle.fr_to_mont_limbs(scal[s]) for s in (si if shared is None else si[:1])], dtype=np.uint64)
    return lim([pts[p] for p in pi]), sc, (lim(adds) if adds is not None else None), lim(want)


@pytest.mark.parametrize("n", [1, 16, 17, 300])
@pytest.mark.parametrize("with_addends", [False, True])
@pytest.mark.parametrize("shared", [None, 0, 2, 4])
def test_scalar_mul_batch_device(gpu, oracle, products, n, with_addends, shared):
    """Per-point scalars (0, 1, r - 1 and random ones in turn) and one shared scalar, with and without addends, against
    the oracle and g1_scalar_mul_batch; then in place over the points and over the addends."""
    import torch
    points, sc, adds, want = mul_case(oracle, products, n, shared, with_addends)
    same(gpu.g1_scalar_mul_batch(points, sc[0] if shared is not None else sc, adds), want)
    dev = lambda a: torch.from_numpy(a.view(np.int64)).to("cuda:0")
    back = lambda t: t.cpu().numpy().view(np.uint64).reshape(n, 12)
    d_sc = dev(sc)
    for place in ("apart", "points") + (("addends",) if with_addends else ()):
        d_p, d_a = dev(points), (dev(adds) if with_addends else None)
        d_out = {"apart": torch.zeros(n * 12, dtype=torch.int64, device="cuda:0"), "points": d_p, "addends": d_a}[place]
        torch.cuda.synchronize()
        gpu.g1_scalar_mul_batch_device(d_p.data_ptr(), d_sc.data_ptr(), sc.shape[0], d_a.data_ptr() if with_addends else 0,
                                       n, d_out.data_ptr())
        same(back(d_out), want)
        if place != "points":
            same(back(d_p), points)                                                    # ... and the inputs are as they were
        if with_addends and place != "addends":
            same(back(d_a), adds)


def test_resident_results_are_msm_bases(gpu, oracle, coracle, products):
    """The 300 results go straight, still resident, to curdle_msm_g1_device as bases, on the caller's stream: the MSM
    equals the oracle's sum of t_i (s_i P_i)."""
    import torch
    n = 300
    points, sc, _, want = mul_case(oracle, products, n, None, False)
    rng = np.random.default_rng(5)
    t = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    t[:, 3] &= np.uint64((1 << 62) - 1)                                                # < r
    exp = coracle.msm_pippenger(want, t, threads=4)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_p = torch.from_numpy(points.view(np.int64)).to("cuda:0")
        d_sc = torch.from_numpy(sc.view(np.int64)).to("cuda:0")
        d_t = torch.from_numpy(t.view(np.int64)).to("cuda:0")
        d_out = torch.zeros(n * 12, dtype=torch.int64, device="cuda:0")
        gpu.g1_scalar_mul_batch_device(d_p.data_ptr(), d_sc.data_ptr(), n, 0, n, d_out.data_ptr(), stream=s.cuda_stream)
        got = gpu.msm_g1_device(d_out.data_ptr(), d_t.data_ptr(), n, stream=s.cuda_stream)
    assert (got == exp).all()
    same(d_out.cpu().numpy().view(np.uint64).reshape(n, 12), want)


def test_two_threads_normalise_beside_an_msm(gpu, oracle, coracle, pool):
    batches = [batch(oracle, pool, 1000, form, 300 + form) + (form,) for form in (JAC, XYZZ)]
    k, q = oracle.Rand(1).get_frs(2)
    pts = coracle.points_walk(k, q, 4096)
    rng = np.random.default_rng(4096)
    sc = rng.integers(0, 1 << 64, size=(4096, 4), dtype=np.uint64)
    sc[:, 3] &= np.uint64((1 << 62) - 1)
    exp = coracle.msm_pippenger(pts, sc, threads=4)
    errors = []

    def worker(which):
        try:
            for r in range(4):
                limbs, want, form = batches[(which + r) % 2]
                same(gpu.g1_normalize_batch(limbs, form), want)
                same(on_device(gpu, limbs, form), want)
        except BaseException as e:  # noqa: BLE001 - reported by the main thread
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(w,)) for w in range(2)]
    for th in threads:
        th.start()
    msms = [gpu.msm_g1(pts, sc) for _ in range(3)]
    for th in threads:
        th.join()
    assert not errors, errors
    for got in msms:
        assert (got == exp).all()
