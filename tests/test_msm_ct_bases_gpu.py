"""The constant-time MSM over a resident base set on the GPU (csrc/msm_ct_bases_kernels.hip: k_ct_bases_shift,
k_msm_ct_walk_rows; csrc/msm_ct_bases_api.hip): the exported table rows against the C oracle, the results bit for bit
against curdle_msm_g1_ct, curdle_msm_g1 and the point of the big-integer model (tests/msm_ct_bases_model.py, whose
expected words come from the C oracle, not from the library), for every chunk width.  Small shapes only; the reference
results of a case are computed once and shared by the four chunk widths."""
import ctypes as C
import threading

import numpy as np
import pytest

import msm_ct_bases_model as cb
import msm_ct_model as mm
from msm_ct_model import R

pytestmark = pytest.mark.gpu
GUARD = 0x5A
_refs = {}


class Env:
    def __init__(self, gpu, oracle, coracle):
        self.gpu, self.o, self.co = gpu, oracle, coracle
        self.inf = np.array(oracle.jac_to_mont_limbs(oracle.INF), dtype=np.uint64)

    def stats(self):
        g = self.gpu
        return g.stat_msm_ct_bases(), g.stat_msm_ct(), g.stat_msm_ct_batch(), g.stat_g1_mul_ct()

    def moved(self, before, lanes, msms, tables=0, calls=1, batch=None):
        """The counters of `calls` completed calls: curdle_stat_msm_ct_bases by the model's counts, curdle_stat_msm_ct
        (its walk counter above all) and curdle_stat_g1_mul_ct not at all, curdle_stat_msm_ct_batch by `batch` only."""
        after = self.stats()
        d = {n: after[0][n] - before[0][n] for n in after[0]}
        assert d == {"tables": tables, "calls": calls, "lanes": lanes, "msms": msms}, d
        assert after[1] == before[1] and after[3] == before[3]
        bt = {n: after[2][n] - before[2][n] for n in after[2]}
        assert bt == (batch or {"calls": 0, "msms": 0, "levels": 0}), bt

    def arrays(self, case):
        """(points of the set, rows uint32 | None, the pairs' points, scalars) of a model case."""
        name, gs, rows, ks, bits = case
        pts = cb.set_limbs(self.o, self.co, gs)
        r = None if rows is None else np.array(rows, dtype=np.uint32)
        pair_pts = pts[:len(ks)] if r is None else pts[r]
        return pts, r, np.ascontiguousarray(pair_pts), mm.to_limbs(self.o, ks)

    def references(self, case, pair_pts, sc):
        """The model's point, checked ONCE per set of pairs against curdle_msm_g1_ct and curdle_msm_g1."""
        name, gs, rows, ks, bits = case
        key = (name, bits, tuple(ks))
        if key not in _refs:
            want = mm.expected_jac(self.o, self.co, sum(k * g for k, g in cb.pairs_of(case) if g is not None) % R)
            assert (self.gpu.msm_g1_ct(pair_pts, sc, bits) == want).all(), name
            assert (self.gpu.msm_g1(pair_pts, sc) == want).all(), name
            _refs[key] = want
        return _refs[key]

    def resident(self, handle, sc, rows, bits, stream=0, offsets=None):
        """The resident call on scalars that sit between guard bytes; scalars and guards are as they were afterwards."""
        import torch
        lead, tail = 32 * 3, 32 * 5
        raw = np.full(lead + sc.nbytes + tail, GUARD, dtype=np.uint8)
        raw[lead:lead + sc.nbytes] = sc.view(np.uint8).reshape(-1)
        d = torch.from_numpy(raw).to("cuda:0")
        assert d.data_ptr() % 16 == 0
        torch.cuda.synchronize()
        try:
            if offsets is None:
                return handle.msm_device(d.data_ptr() + lead, len(sc), rows, bits, stream=stream)
            return handle.msm_batch_device(d.data_ptr() + lead, offsets, rows, bits, stream=stream)
        finally:
            assert (d.cpu().numpy() == raw).all()

    def check(self, c, case, forms=("host",), handle=None):
        name, gs, rows, ks, bits = case
        pts, r, pair_pts, sc = self.arrays(case)
        want = self.references(case, pair_pts, sc)
        assert (want == cb.expected(self.o, self.co, case, c)).all(), (c, name)   # the fold over the chunk terms
        h = handle or self.gpu.CtBases(pts, c)
        try:
            for form in forms:
                before = self.stats()
                got = h.msm(sc, r, bits) if form == "host" else self.resident(h, sc, r, bits)
                assert (got == want).all(), (c, name, form)
                self.moved(before, len(ks) * cb.chunks(bits, c), 1)
        finally:
            if handle is None:
                h.free()


@pytest.fixture(scope="module")
def env(gpu, oracle, coracle):
    return Env(gpu, oracle, coracle)


@pytest.mark.parametrize("c", cb.CHUNK_BITS)
def test_the_exported_rows_match_the_oracle(env, c):
    """Row j is 2^(c j) P_i for every j, with infinity bases at the start, in the middle and at the end; both creators;
    one table built per handle."""
    import torch
    for n in cb.EXPORT_SIZES:
        base = cb.Bases(env.o, n, (0, n // 2, n - 1) if n > 1 else ())
        pts = base.limbs(env.co)
        before = env.stats()
        h = env.gpu.CtBases(pts, c)
        d_pts = torch.from_numpy(pts.view(np.int64)).to("cuda:0")
        h2 = env.gpu.CtBases(d_pts.data_ptr(), c, n=n, device=True)
        env.moved(before, 0, 0, tables=2, calls=0)
        assert (h.n, h.chunk_bits, h.chunks) == (n, c, cb.chunks(255, c)) == (h2.n, h2.chunk_bits, h2.chunks)
        for j in range(h.chunks):
            want = base.limbs(env.co, c, j)
            assert (h.export(j) == want).all(), (n, j)
            assert (h2.export(j) == want).all(), (n, j)
            assert not want[list(base.inf)].any()
        with pytest.raises(env.gpu.CurdleError) as e:
            h.export(h.chunks)
        assert e.value.code == env.gpu.EINVAL
        h.free()
        h2.free()
    assert env.gpu.CtBases(np.zeros((1, 12), dtype=np.uint64)).chunk_bits == cb.DEFAULT_CHUNK_BITS


@pytest.mark.parametrize("c", cb.CHUNK_BITS)
def test_the_arms_between_chunk_terms(env, c):
    for case in cb.arm_cases(env.o, c):
        env.check(c, case, forms=("host", "device"))


@pytest.mark.parametrize("c", cb.CHUNK_BITS)
def test_the_sizes_the_edges_and_the_row_lists(env, c):
    """n = 1 ... 513: random scalars with rows null, scalars 0 / 1 / r - 1 and infinity rows at the edges, all pairs on
    one row, a reversal, repeats."""
    for n in cb.SIZES:
        handles = {}
        for case in cb.size_cases(env.o, n):
            key = tuple(case[1])
            if key not in handles:
                handles[key] = env.gpu.CtBases(cb.set_limbs(env.o, env.co, case[1]), c)
            env.check(c, case, forms=("host", "device") if case[2] is None else ("host",), handle=handles[key])
        for h in handles.values():
            h.free()


@pytest.mark.parametrize("c", cb.CHUNK_BITS)
def test_scalar_bits_at_the_chunk_edges(env, c):
    """c - 1, c, c + 1, 2c, 254, 255 and 1 with the scalars' top bit set; a scalar of exactly 2^bits refused with the
    guard words around out_jac intact, in both forms, and the same call one lower accepted afterwards."""
    gpu = env.gpu
    assert {1, c, c + 1, 254, 255} <= set(cb.bits_list(c))
    cases = cb.bits_cases(env.o, c)
    h = gpu.CtBases(cb.set_limbs(env.o, env.co, cases[0][1]), c)
    for case in cases:
        env.check(c, case, forms=("host", "device"), handle=h)
    for case in cb.violation_cases(env.o, c):
        name, gs, rows, ks, bits = case
        sc = mm.to_limbs(env.o, ks)
        before = env.stats()
        out = np.full(18 + 4, 77, dtype=np.uint64)
        rc = gpu._lib.curdle_msm_g1_ct_bases(h._h, None, C.c_void_p(sc.ctypes.data), C.c_size_t(len(ks)), C.c_uint(bits),
                                             C.c_void_p(out[2:].ctypes.data))
        assert rc == gpu.EINVAL and "scalar_bits" in gpu.last_error(), name
        assert (out == 77).all(), name
        with pytest.raises(gpu.CurdleError) as e:
            env.resident(h, sc, None, bits)
        assert e.value.code == gpu.EINVAL and "scalar_bits" in e.value.msg, name
        assert env.stats() == before, name
        env.check(c, (name + ", one lower", gs, rows, ks[:-1] + [ks[-1] - 1], bits), handle=h)
    h.free()


def test_the_limits(env):
    """c = 64 at 255 bits is 4 chunks: 16,384 pairs over a set of 16,384 bases are 65,536 terms and 65,536 table records,
    accepted once; one more pair, one more base and a row index equal to the size are refused before device work."""
    gpu = env.gpu
    n = cb.MAX_TERMS // 4
    a, q = env.o.Rand(31).get_frs(2)
    pts = env.co.points_walk(a, q, n)
    sc = np.random.default_rng(31).integers(0, 1 << 64, size=(n + 1, 4), dtype=np.uint64)
    sc[:, 3] &= np.uint64((1 << 62) - 1)                                    # Montgomery words of canonical scalars: < r
    before = env.stats()
    h = gpu.CtBases(pts, 64)
    got = h.msm(sc[:n])
    env.moved(before, cb.MAX_TERMS, 1, tables=1)
    assert (got == gpu.msm_g1(pts, sc[:n])).all()
    assert (got == env.co.msm_pippenger(pts, sc[:n], threads=4)).all()
    after = env.stats()
    rows = np.arange(n + 1, dtype=np.uint32) % np.uint32(n)
    for call in (lambda: h.msm(sc, rows), lambda: h.msm_batch(sc, [0, 1, n + 1], rows)):
        with pytest.raises(gpu.CurdleError) as e:
            call()
        assert e.value.code == gpu.EINVAL and "65,536" in e.value.msg
    rows[5] = n
    for call in (lambda: h.msm(sc[:9], rows[:9]), lambda: h.msm_batch(sc[:9], [0, 4, 9], rows[:9]),
                 lambda: h.msm(sc[:3], np.array([0, n, 1], dtype=np.uint32))):
        with pytest.raises(gpu.CurdleError) as e:
            call()
        assert e.value.code == gpu.EINVAL and "not below" in e.value.msg
    with pytest.raises(gpu.CurdleError) as e:
        gpu.CtBases(np.zeros((n + 1, 12), dtype=np.uint64), 64)
    assert e.value.code == gpu.EINVAL and "65,536" in e.value.msg
    # a misaligned device pointer over a real handle: behind the rows
    out = np.full(20, 77, dtype=np.uint64)
    dev = gpu._lib.curdle_msm_g1_ct_bases_device
    for off in (4, 8):
        rc = dev(h._h, None, C.c_void_p(0x7000_0000_1000 + off), C.c_size_t(3), C.c_uint(255), C.c_void_p(out[1:].ctypes.data), None)
        assert rc == gpu.EINVAL and "multiples of 16" in gpu.last_error()
    assert (out == 77).all() and env.stats() == after
    h.free()


def _batch_expected(env, base, rows, sc, offs):
    return np.array([mm.expected_jac(env.o, env.co, sum(k * base.g[r] for k, r in zip(sc[a:b], rows[a:b]) if base.g[r] is not None) % R)
                     for a, b in zip(offs[:-1].astype(int), offs[1:].astype(int))], dtype=np.uint64).reshape(-1, 18)


@pytest.mark.parametrize("c", cb.CHUNK_BITS)
def test_the_batch_with_empty_msms_first_in_the_middle_and_last(env, c):
    """Counts [0, 1, 2, 3, 5, 0, 64, 65, 127, 0], rows wandering over a set of 300 with infinity bases: the model's point
    per MSM, curdle_msm_g1_ct_batch on the gathered pairs, both forms, the counters."""
    counts = list(cb.MIXED_COUNTS)
    base, rows, ks, offs = cb.batch_case(env.o, counts, 40)
    pts, sc, r = base.limbs(env.co), mm.to_limbs(env.o, ks), np.array(rows, dtype=np.uint32)
    want = _batch_expected(env, base, rows, ks, offs)
    if "mixed" not in _refs:
        _refs["mixed"] = env.gpu.msm_g1_ct_batch(np.ascontiguousarray(pts[r]), sc, offs)
    assert (_refs["mixed"] == want).all()
    assert all((want[j] == env.inf).all() for j in (0, 5, 9))
    h = env.gpu.CtBases(pts, c)
    moved = {"calls": 1, "msms": len(counts), "levels": cb.level_launches(counts, c, 255)}
    for form in ("host", "device"):
        before = env.stats()
        got = h.msm_batch(sc, offs, r) if form == "host" else env.resident(h, sc, r, 255, offsets=offs)
        assert (got == want).all(), form
        env.moved(before, sum(counts) * cb.chunks(255, c), 7, batch=moved)
    # pairs in front of the call's first pair belong to no MSM: offsets[0] = 3
    assert int(offs[3]) == 3
    assert (h.msm_batch(sc, offs[3:], r) == want[3:]).all()
    assert (env.resident(h, sc, r, 255, offsets=offs[3:]) == want[3:]).all()
    h.free()


def test_the_level_path_at_sixteen_bits(env):
    """[513, 3, 1025, 0, 512] at c = 16 against the single call per MSM; the level launches, read from
    curdle_stat_msm_ct_batch, are msm_ct_batch_model's rule on count x 16 terms."""
    counts = list(cb.LEVEL_COUNTS)
    base, rows, ks, offs = cb.batch_case(env.o, counts, 100)
    pts, sc, r = base.limbs(env.co), mm.to_limbs(env.o, ks), np.array(rows, dtype=np.uint32)
    want = _batch_expected(env, base, rows, ks, offs)
    h = env.gpu.CtBases(pts, 16)
    levels = cb.level_launches(counts, 16, 255)
    assert levels == 6
    before = env.stats()
    got = h.msm_batch(sc, offs, r)
    env.moved(before, sum(counts) * 16, 4, batch={"calls": 1, "msms": 5, "levels": levels})
    assert (got == want).all()
    for j, (a, b) in enumerate(zip(offs[:-1].astype(int), offs[1:].astype(int))):
        assert (got[j] == h.msm(sc[a:b], r[a:b])).all(), j
    h.free()


def test_a_violation_in_the_last_msm_fails_the_whole_call(env):
    gpu = env.gpu
    counts = [3, 65, 2]
    base, rows, ks, offs = cb.batch_case(env.o, counts, 700)
    pts, r = base.limbs(env.co), np.array(rows, dtype=np.uint32)
    h = gpu.CtBases(pts, 16)
    for bits in (9, 16, 17, 254):
        low = [k & ((1 << bits) - 1) for k in ks]
        bad = mm.to_limbs(env.o, low[:-1] + [1 << bits])
        before = env.stats()
        out = np.full(18 * 3 + 4, 77, dtype=np.uint64)
        rc = gpu._lib.curdle_msm_g1_ct_bases_batch(h._h, C.c_void_p(r.ctypes.data), C.c_void_p(bad.ctypes.data),
                                                   C.c_void_p(offs.ctypes.data), C.c_size_t(3), C.c_uint(bits),
                                                   C.c_void_p(out[2:].ctypes.data))
        assert rc == gpu.EINVAL and "scalar_bits" in gpu.last_error(), bits
        assert (out == 77).all(), bits
        with pytest.raises(gpu.CurdleError) as e:
            env.resident(h, bad, r, bits, offsets=offs)
        assert e.value.code == gpu.EINVAL and "scalar_bits" in e.value.msg
        assert env.stats() == before
        assert (h.msm_batch(mm.to_limbs(env.o, low), offs, r, bits) == _batch_expected(env, base, rows, low, offs)).all(), bits
    h.free()


def test_streams_two_handles_a_shutdown_and_a_second_context(env):
    """A caller's stream and the library's; two handles of different chunk widths alive at once; both used after
    curdle_shutdown and re-init, and first used on a second context of the same GPU: the table is uploaded again from
    the handle's rows, not built again."""
    import torch
    gpu = env.gpu
    counts = [5, 0, 130]
    base, rows, ks, offs = cb.batch_case(env.o, counts, 900)
    pts, sc, r = base.limbs(env.co), mm.to_limbs(env.o, ks), np.array(rows, dtype=np.uint32)
    want = _batch_expected(env, base, rows, ks, offs)
    total = mm.expected_jac(env.o, env.co, sum(k * base.g[i] for k, i in zip(ks, rows) if base.g[i] is not None) % R)
    h16, h64 = gpu.CtBases(pts, 16), gpu.CtBases(pts, 64)
    s = torch.cuda.Stream()
    src = torch.from_numpy(sc.view(np.int64).reshape(-1)).pin_memory()
    with torch.cuda.stream(s):                                     # the scalars are written on the caller's stream
        d_sc = torch.zeros_like(src, device="cuda:0")
        d_sc.copy_(src, non_blocking=True)
        got = h16.msm_batch_device(d_sc.data_ptr(), offs, r, stream=s.cuda_stream)
        one = h64.msm_device(d_sc.data_ptr(), len(ks), r, stream=s.cuda_stream)
    assert (got == want).all() and (one == total).all()
    torch.cuda.synchronize()
    assert (env.resident(h64, sc, r, 255, stream=s.cuda_stream, offsets=offs) == want).all()
    assert (env.resident(h16, sc, r, 255) == total).all()
    del d_sc
    tables = gpu.stat_msm_ct_bases()["tables"]
    gpu.shutdown()
    gpu.init(0)
    assert (h16.msm_batch(sc, offs, r) == want).all() and (h64.msm(sc, r) == total).all()
    errors = []

    def second():
        try:
            gpu.set_device(1)
            assert (h64.msm_batch(sc, offs, r) == want).all() and (h16.msm(sc, r) == total).all()
            fresh = gpu.CtBases(pts, 32)                          # made on context 1, used on both
            assert (fresh.msm(sc, r) == total).all()
            box.append(fresh)
        except BaseException as e:  # noqa: BLE001 - reported by the main thread
            errors.append(e)

    box = []
    gpu.init_devices([0, 0])
    try:
        assert gpu.device_count() == 2
        th = threading.Thread(target=second)
        th.start()
        th.join()
        assert not errors, errors
        assert (box[0].msm_batch(sc, offs, r) == want).all()       # context 0
    finally:
        gpu.set_device(-1)
        gpu.shutdown()
        gpu.init(0)
    assert gpu.device_count() == 1
    assert (h16.msm(sc, r) == total).all() and (box[0].msm(sc, r) == total).all()
    assert gpu.stat_msm_ct_bases()["tables"] == tables + 1         # `fresh` alone was built
    for h in (h16, h64, box[0]):
        h.free()


def test_one_thread_beside_a_bucket_msm(env):
    counts = [129, 128]
    base, rows, ks, offs = cb.batch_case(env.o, counts, 500)
    pts, sc, r = base.limbs(env.co), mm.to_limbs(env.o, ks), np.array(rows, dtype=np.uint32)
    want = _batch_expected(env, base, rows, ks, offs)
    h = env.gpu.CtBases(pts)
    a, q = env.o.Rand(1).get_frs(2)
    bases = env.co.points_walk(a, q, 4096)
    t = np.random.default_rng(4096).integers(0, 1 << 62, size=(4096, 4), dtype=np.uint64)
    exp = env.co.msm_pippenger(bases, t, threads=4)
    errors = []

    def worker():
        try:
            for _ in range(3):
                assert (h.msm_batch(sc, offs, r) == want).all()
                assert (env.resident(h, sc, r, 255, offsets=offs) == want).all()
        except BaseException as e:  # noqa: BLE001 - reported by the main thread
            errors.append(e)

    th = threading.Thread(target=worker)
    th.start()
    msms = [env.gpu.msm_g1(bases, t) for _ in range(3)]
    th.join()
    assert not errors, errors
    for got in msms:
        assert (got == exp).all()
    h.free()


def test_the_counters(env):
    """curdle_stat_msm_ct_bases moves by (tables built, calls, pairs x chunks walked, MSMs that are not empty); a refused
    call and a call that needs no device count nothing; curdle_stat_msm_ct does not move at all."""
    gpu = env.gpu
    base, rows, ks, offs = cb.batch_case(env.o, [4, 0, 6], 20)
    pts, sc, r = base.limbs(env.co), mm.to_limbs(env.o, ks), np.array(rows, dtype=np.uint32)
    before = env.stats()
    h = gpu.CtBases(pts, 8)
    env.moved(before, 0, 0, tables=1, calls=0)
    before = env.stats()
    h.msm(sc, r, 255)                                             # 10 pairs x 32 chunks
    h.msm(sc[:4] & np.uint64(0), r[:4], 9)                        # 4 pairs x 2 chunks
    env.moved(before, 10 * 32 + 4 * 2, 2, calls=2)
    before = env.stats()
    h.msm_batch(sc, offs, r, 255)
    env.moved(before, 10 * 32, 2, batch={"calls": 1, "msms": 3, "levels": 0})
    before = env.stats()
    h.msm(sc[:0], r[:0])
    h.msm_batch(sc, [3, 3, 3], r)
    h.msm_batch(sc, [3], r)
    with pytest.raises(gpu.CurdleError):
        h.msm_batch(sc, [0, 5, 4], r)
    with pytest.raises(gpu.CurdleError):
        h.msm(sc, r, 0)
    assert env.stats() == before
    h.free()
