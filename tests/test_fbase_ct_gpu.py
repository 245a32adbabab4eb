"""CURDLE_FBASE_CONSTANT_TIME on the GPU (k_fbase_mul_ct, csrc/fbase_ct_kernels.hip): the flagged entry points against
the big-integer model of tests/fbase_ct_model.py, bit for bit -- the expected arrays come from the C oracle, not from
the library -- and, second, against the untouched default path on the same inputs.  Both output forms, host and
resident entry, the generator's table and a second base (7 G through curdle_fbase_create).  The kernel takes one lane
per scalar in blocks of 256 and walks 64 unsigned 4-bit digits, selecting among the 15 multiples of every window, so the
scalars are the model's digit families (every window as the first addition, odd ones included; runs of zero digits;
every digit 0xf; each half of the subset mapping alone; the top nibble of r - 1) and the sizes straddle a wave, a block
and a pass (FBASE_PASS = 256).  The counters prove which kernel ran."""
import threading

import numpy as np
import pytest

import fbase_ct_model as cm4
import fbase_model as fm

pytestmark = pytest.mark.gpu

AFF, COMP = 0, 1
CT = 1
INF48 = bytes([0xC0]) + bytes(47)


def same(got, want, names=None):
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} rows differ, first at {bad[0]}" + (f" ({names[bad[0]]})" if names else "")


class Env:
    def __init__(self, gpu, oracle, coracle):
        self.gpu, self.o, self.co = gpu, oracle, coracle
        self.other = gpu.FBase(coracle.scalar_mul_gen(fm.OTHER_BASE))
        self.bases = ((None, None), (self.other, fm.OTHER_BASE))

    def want(self, ks, ms=None, base_int=None):
        prod = [fm.product(k, None if ms is None else ms[i]) for i, k in enumerate(ks)]
        for p in prod:
            cm4.check_exact(p)
        return cm4.expected_arrays(self.o, self.co, prod, base_int)

    def stats(self):
        return self.gpu.stat_fbase(), self.gpu.stat_fbase_ct()

    def resident(self, sc, mu, form, base=None, stream=None, off=0, flags=CT):
        """The resident call; compressed output at byte offset `off` between guard bytes.  Returns the output rows."""
        import torch
        n, rec = len(sc), (48 if form == COMP else 96)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1)).to("cuda:0")
        d_sc, d_mu = dev(sc), (dev(mu) if mu is not None else None)
        d_out = torch.full((n * rec + 32,), 0x5A, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        self.gpu.g1_fixed_base_mul_batch_device(d_sc.data_ptr(), d_mu.data_ptr() if mu is not None else 0, n,
                                                d_out.data_ptr() + 16 + off, base=base, out_form=form, stream=stream, flags=flags)
        out = d_out.cpu().numpy()
        assert (out[:16 + off] == 0x5A).all() and (out[16 + off + n * rec:] == 0x5A).all()     # nothing outside the rows
        assert (d_sc.cpu().numpy().view(np.uint64).reshape(-1, 4) == sc).all()                 # the caller's scalars are as they were
        if mu is not None:
            assert (d_mu.cpu().numpy().view(np.uint64).reshape(-1, 4) == mu).all()
        body = out[16 + off: 16 + off + n * rec].copy()
        return body.reshape(n, 48) if form == COMP else body.view(np.uint64).reshape(n, 12)

    def every_way(self, ks, ms=None, bases=None, names=None):
        """Host and resident entry, both forms, over `bases`: the flagged call against the model, the default call
        against the flagged one.  Returns the last base's expected arrays."""
        sc = fm.to_limbs(self.o, ks)
        mu = fm.to_limbs(self.o, ms) if ms is not None else None
        for base, base_int in (bases or self.bases):
            aff, comp = self.want(ks, ms, base_int)
            for form, want in ((AFF, aff), (COMP, comp)):
                got = self.gpu.g1_fixed_base_mul_batch(sc, mu, base=base, out_form=form, flags=CT)
                same(got, want, names)
                same(self.gpu.g1_fixed_base_mul_batch(sc, mu, base=base, out_form=form), got, names)    # the default path
                got = self.resident(sc, mu, form, base)
                same(got, want, names)
                same(self.resident(sc, mu, form, base, flags=0), got, names)
        return aff, comp


@pytest.fixture(scope="module")
def env(gpu, oracle, coracle):
    e = Env(gpu, oracle, coracle)
    yield e
    e.other.free()


@pytest.fixture(scope="module")
def families(oracle):
    return cm4.digit_families(oracle)


@pytest.mark.parametrize("family", ["small_and_top", "single_digits", "all_f", "zero_runs", "low_zero", "half_zero", "randoms"])
def test_digit_families(env, families, family):
    cases = families[family]
    assert 8 <= len(cases) < 1000
    a, b = env.stats()
    aff, comp = env.every_way([k for _, k in cases], names=[n for n, _ in cases])
    a2, b2 = env.stats()
    # 2 bases x 2 forms x 2 entries, once per kernel: the flag chose the kernel every time
    assert (b2["scalars"] - b["scalars"], b2["launches"] - b["launches"]) == (8 * len(cases), 8)
    assert (a2["scalars"] - a["scalars"], a2["launches"] - a["launches"]) == (8 * len(cases), 8)
    if family == "small_and_top":
        assert not aff[0].any() and bytes(comp[0]) == INF48                              # 0 * P
        assert bytes(comp[1]) == env.o.compress(env.o.scalar_mul(fm.OTHER_BASE, env.o.G1))


def test_multiplier_form(env):
    cases = cm4.multiplier_cases(env.o)
    ks, ms = [s for _, s, _ in cases], [m for _, _, m in cases]
    aff, _ = env.every_way(ks, ms, names=[n for n, _, _ in cases])
    by = {n: j for j, (n, _, _) in enumerate(cases)}
    assert not aff[by["m=0"]].any() and not aff[by["s=0"]].any() and aff[by["m=1"]].any()
    # a null multiplier array against an array of ones: identical output
    sc, ones = fm.to_limbs(env.o, ks), fm.to_limbs(env.o, [1] * len(ks))
    for form in (AFF, COMP):
        a = env.gpu.g1_fixed_base_mul_batch(sc, None, out_form=form, flags=CT)
        b = env.gpu.g1_fixed_base_mul_batch(sc, ones, out_form=form, flags=CT)
        assert (a == b).all()
        same(a, env.want(ks)[form])
        assert (env.resident(sc, None, form) == env.resident(sc, ones, form)).all() and (a == env.resident(sc, ones, form)).all()


HOLES = {"none": lambda n: set(), "first": lambda n: {0}, "last": lambda n: {n - 1},
         "a run of 64": lambda n: set(range(n // 2, min(n, n // 2 + 64))), "everywhere": lambda n: set(range(n))}


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_sizes_with_infinity_results(env, families, n):
    """The edges of a wave and of a block; scalar 0 (an infinity result, stored through the mask) first, last, in a run
    of 64 and everywhere."""
    pool = [k for _, k in families["randoms"]]
    for where, holes in HOLES.items():
        at = holes(n)
        ks = [0 if i in at else pool[(i * 7 + n) % len(pool)] for i in range(n)]
        bases = env.bases if where in ("none", "a run of 64") else env.bases[:1]
        aff, _ = env.every_way(ks, bases=bases)
        assert int((~aff.any(axis=1)).sum()) == len(at), where


@pytest.mark.parametrize("n", [256, 257, 513])
def test_the_pass_boundary_and_the_counters(env, families, n):
    """FBASE_PASS = 256: both sides of the boundary are exact, a flagged call moves curdle_stat_fbase_ct by n and
    ceil(n / 256) and curdle_stat_fbase[0..1] not at all -- and the converse for flags = 0 and for the entry points
    without flags: a flag that is accepted and quietly routed to the old kernel fails here."""
    pool = [k for _, k in families["randoms"]]
    ks = [pool[(3 * i + n) % len(pool)] for i in range(n)]
    ms = [pool[(5 * i + 1) % len(pool)] for i in range(n)]
    ks[255], ms[0] = 0, 0
    passes = (n + 255) // 256
    sc, mu = fm.to_limbs(env.o, ks), fm.to_limbs(env.o, ms)
    with env.gpu.knobs(FBASE_PASS=256):
        for m, mlimbs in ((None, None), (ms, mu)):
            aff, comp = env.want(ks, m)
            for form, want in ((AFF, aff), (COMP, comp)):
                for call in (lambda f: env.gpu.g1_fixed_base_mul_batch(sc, mlimbs, out_form=form, flags=f),
                             lambda f: env.resident(sc, mlimbs, form, flags=f)):
                    a, b = env.stats()
                    same(call(CT), want)
                    a2, b2 = env.stats()
                    assert (b2["scalars"] - b["scalars"], b2["launches"] - b["launches"]) == (n, passes)
                    assert a2 == a                                     # tables included: the table is shared
                    for flags in (0, None):
                        same(call(flags), want)
                        a3, b3 = env.stats()
                        assert (a3["scalars"] - a2["scalars"], a3["launches"] - a2["launches"]) == (n, passes)
                        assert b3 == b2 and a3["tables"] == a2["tables"]
                        a2 = a3
    a, b = env.stats()
    env.gpu.g1_fixed_base_mul_batch(sc, flags=CT)                      # the default pass size: one launch
    assert env.gpu.stat_fbase_ct()["launches"] - b["launches"] == 1 and env.gpu.stat_fbase() == a


@pytest.mark.parametrize("off", [0, 1, 3])
def test_resident_on_a_callers_stream_and_at_byte_offsets(env, families, off):
    """The scalars are written on the caller's stream immediately before the call; the compressed output starts `off`
    bytes into its array between guard bytes; the caller's arrays are as they were afterwards."""
    import torch
    ks = [k for _, k in families["low_zero"]] + [k for _, k in families["randoms"]][:70]
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
                                               out_form=COMP, stream=s.cuda_stream, flags=CT)
        env.gpu.g1_fixed_base_mul_batch_device(d_in.data_ptr(), d_in.data_ptr() + 32 * n, n, d_a.data_ptr(),
                                               out_form=AFF, stream=s.cuda_stream, flags=CT)
        out = d_c.cpu().numpy()
        got_a = d_a.cpu().numpy().view(np.uint64).reshape(n, 12)
        back = d_in.cpu().numpy()
    same(out[16 + off: 16 + off + 48 * n].reshape(n, 48), comp)
    assert (out[:16 + off] == 0x5A).all() and (out[16 + off + 48 * n:] == 0x5A).all()
    same(got_a, aff)
    assert (back == src.numpy()).all()                                 # scalars and multipliers unchanged
    torch.cuda.synchronize()
    same(env.resident(sc, mu, COMP, off=off), comp)                    # the library's own stream
    same(env.resident(sc, mu, COMP, env.other, off=off), env.want(ks, ms, fm.OTHER_BASE)[1])


ONE = np.array([0x00000001fffffffe, 0x5884b7fa00034802, 0x998c4fefecbc4ff5, 0x1824b159acc5056f], dtype=np.uint64)  # 1 as an fr.Element


def test_the_tracker_batch_with_the_flag(env):
    """curdle_whisk_compute_trackers_batch_ex with the flag on the 19 x 19 matrix of fbase_model.whisk_scalars: byte for
    byte what curdle_whisk_compute_tracker / curdle_whisk_k_commitment write, with rs null and with k_commitments_out
    null too; the three columns of a pass are ONE launch of the constant-time kernel."""
    gpu, o = env.gpu, env.o
    assert o.fr_to_mont_limbs(1) == [int(v) for v in ONE]
    vals = fm.whisk_scalars(o)
    assert len(vals) == 19
    pairs = [(k, r) for _, k in vals for _, r in vals]
    ks, rs = fm.to_limbs(o, [k for k, _ in pairs]), fm.to_limbs(o, [r for _, r in pairs])
    n = len(pairs)
    want_t = np.frombuffer(b"".join(gpu.whisk_compute_tracker(ks[i], rs[i]) for i in range(n)), dtype=np.uint8).reshape(n, 96)
    want_c = np.frombuffer(b"".join(gpu.whisk_k_commitment(ks[i]) for i in range(n)), dtype=np.uint8).reshape(n, 48)
    a, b = env.stats()
    trk, com = gpu.whisk_compute_trackers_batch(ks, rs, flags=CT)
    a2, b2 = env.stats()
    assert (b2["scalars"] - b["scalars"], b2["launches"] - b["launches"]) == (3 * n, 1) and a2 == a
    assert (trk == want_t).all() and (com == want_c).all()
    for i in (0, 1, 20, 79, 200, n - 1):                                                # ... and the model directly
        assert (bytes(trk[i]), bytes(com[i])) == fm.tracker_bytes(o, env.co, *pairs[i]), i
    assert bytes(trk[0]) == INF48 + INF48 and bytes(com[0]) == INF48                    # k = r = 0
    t0, c0 = gpu.whisk_compute_trackers_batch(ks, rs, flags=0)                          # the default path: the same bytes
    a3, b3 = env.stats()
    assert (t0 == trk).all() and (c0 == com).all()
    assert (a3["scalars"] - a2["scalars"], a3["launches"] - a2["launches"]) == (3 * n, 1) and b3 == b2
    # rs null: r = 1, the fork's initial trackers (G, k G)
    t1, c1 = gpu.whisk_compute_trackers_batch(ks, None, flags=CT)
    want_1 = np.frombuffer(b"".join(gpu.whisk_compute_tracker(ks[i], ONE) for i in range(n)), dtype=np.uint8).reshape(n, 96)
    assert (t1 == want_1).all() and (c1 == want_c).all()
    assert (t1[:, :48] == np.frombuffer(o.compress(o.G1), dtype=np.uint8)).all() and (t1[:, 48:] == want_c).all()
    # k_commitments_out null: two columns
    b = gpu.stat_fbase_ct()
    t2, c2 = gpu.whisk_compute_trackers_batch(ks, rs, commitments=False, flags=CT)
    b2 = gpu.stat_fbase_ct()
    assert c2 is None and (t2 == want_t).all()
    assert (b2["scalars"] - b["scalars"], b2["launches"] - b["launches"]) == (2 * n, 1)
    t3, _ = gpu.whisk_compute_trackers_batch(ks, None, commitments=False, flags=CT)
    assert (t3 == want_1).all()
    with gpu.knobs(FBASE_PASS=256):                                                     # 85 members a pass
        b = gpu.stat_fbase_ct()
        t4, c4 = gpu.whisk_compute_trackers_batch(ks, rs, flags=CT)
        assert (t4 == want_t).all() and (c4 == want_c).all()
        assert gpu.stat_fbase_ct()["launches"] - b["launches"] == (n + 84) // 85


def test_one_thread_beside_an_msm(env, families):
    ks = ([k for _, k in families["randoms"]] + [k for _, k in families["single_digits"]] + [0, 1, fm.R - 1])[:300]
    ks[17] = 0
    sc = fm.to_limbs(env.o, ks)
    want_a, want_c = env.want(ks)
    want_o = env.want(ks, None, fm.OTHER_BASE)[0]
    k, q = env.o.Rand(1).get_frs(2)
    pts = env.co.points_walk(k, q, 4096)
    rng = np.random.default_rng(4096)
    t = rng.integers(0, 1 << 64, size=(4096, 4), dtype=np.uint64)
    t[:, 3] &= np.uint64((1 << 62) - 1)
    exp = env.co.msm_pippenger(pts, t, threads=4)
    errors = []

    def worker():
        try:
            for r in range(3):
                same(env.gpu.g1_fixed_base_mul_batch(sc, out_form=COMP, flags=CT), want_c)
                same(env.resident(sc, None, AFF, env.other), want_o)
                same(env.gpu.g1_fixed_base_mul_batch(sc, flags=CT), want_a)
        except BaseException as e:  # noqa: BLE001 - reported by the main thread
            errors.append(e)

    th = threading.Thread(target=worker)
    th.start()
    msms = [env.gpu.msm_g1(pts, t) for _ in range(3)]
    th.join()
    assert not errors, errors
    for got in msms:
        assert (got == exp).all()
