"""The constant-time MSM over up to four resident base sets in one call on the GPU (curdle_msm_g1_ct_bases_sets_batch /
_device; k_msm_ct_walk_rows with its sets by value): bit for bit against curdle_msm_g1_ct_bases_batch over ONE handle of
the concatenated points, against curdle_msm_g1_batch on the gathered pairs and against the big-integer model
(tests/msm_ct_sets_model.py, whose expected words come from the C oracle).  Small shapes; a case's references are
computed once and shared by the chunk widths."""
import ctypes as C
import threading

import numpy as np
import pytest

import msm_ct_bases_model as cb
import msm_ct_model as mm
import msm_ct_sets_model as sm

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

    def delta(self, before):
        after = self.stats()
        assert after[1] == before[1] and after[3] == before[3]     # the unchunked walk and the multiplication: never
        return ({n: after[0][n] - before[0][n] for n in after[0]}, {n: after[2][n] - before[2][n] for n in after[2]})

    def handles(self, case, c):
        """(the sets' handles, the single handle over the concatenation, the points)."""
        name, sizes, gs, rows, ks, counts, bits = case
        pts = cb.set_limbs(self.o, self.co, gs)
        b = sm.firsts(sizes)
        sets = [self.gpu.CtBases(np.ascontiguousarray(pts[b[s]:b[s + 1]]), c) for s in range(len(sizes))]
        return sets, self.gpu.CtBases(pts, c), pts

    def resident(self, sets, sc, rows, offs, bits, stream=0):
        """The _device form on scalars between guard bytes, which are as they were afterwards."""
        import torch
        lead, tail = 32 * 3, 32 * 5
        raw = np.full(lead + sc.nbytes + tail, GUARD, dtype=np.uint8)
        raw[lead:lead + sc.nbytes] = sc.view(np.uint8).reshape(-1)
        d = torch.from_numpy(raw).to("cuda:0")
        assert d.data_ptr() % 16 == 0
        torch.cuda.synchronize()
        try:
            return self.gpu.msm_g1_ct_bases_sets_batch_device(sets, rows, d.data_ptr() + lead, offs, bits, stream=stream)
        finally:
            assert (d.cpu().numpy() == raw).all()

    def check(self, c, case, forms=("host", "device")):
        """Both forms against the model, the single handle and (once per set of pairs) the bucket MSM; the counters move
        exactly as the single-handle batch's on the same pairs."""
        name, sizes, gs, rows, ks, counts, bits = case
        sets, one, pts = self.handles(case, c)
        try:
            r, sc, offs = np.array(rows, dtype=np.uint32), mm.to_limbs(self.o, ks), sm.offsets_of(counts)
            want = sm.expected(self.o, self.co, case, c)
            key = (name, bits, tuple(ks))
            if key not in _refs:
                _refs[key] = self.gpu.msm_g1_batch(np.ascontiguousarray(pts[r]), sc, offs)
            assert (_refs[key] == want).all(), (c, name)
            before = self.stats()
            single = one.msm_batch(sc, offs, r, bits)
            moved = self.delta(before)
            assert (single == want).all(), (c, name)
            cbits = cb.chunks(bits, c)
            assert moved[0] == {"tables": 0, "calls": 1, "lanes": len(ks) * cbits, "msms": sum(1 for n in counts if n)}
            assert moved[1] == {"calls": 1, "msms": len(counts), "levels": cb.level_launches(counts, c, bits)}
            for form in forms:
                before = self.stats()
                got = (self.gpu.msm_g1_ct_bases_sets_batch(sets, r, sc, offs, bits) if form == "host"
                       else self.resident(sets, sc, r, offs, bits))
                assert (got == want).all(), (c, name, form)
                assert self.delta(before) == moved, (c, name, form)
        finally:
            for h in sets + [one]:
                h.free()


@pytest.fixture(scope="module")
def env(gpu, oracle, coracle):
    return Env(gpu, oracle, coracle)


@pytest.mark.parametrize("sizes", sm.SET_SIZES, ids=lambda s: "+".join(map(str, s)))
def test_the_row_lists_over_the_set_shapes(env, sizes):
    """Rows at both ends of every set, reversed, repeated, alternating between the sets lane by lane, infinity records;
    c = 8 / 16 / 32 / 64 at the first three shapes, 16 at the others."""
    for case in sm.row_cases(env.o, sizes):
        for c in sm.widths_of(sizes):
            env.check(c, case, forms=("host", "device") if c == 16 else ("host",))


@pytest.mark.parametrize("c", cb.CHUNK_BITS)
def test_the_arms_with_one_point_in_two_sets(env, c):
    for case in sm.arm_cases(env.o, c):
        env.check(c, case)


def test_the_long_batches_cycling_over_three_sets(env):
    """[0, 1, 2, 3, 5, 0, 64, 65, 127, 0] and [513, 3, 1025, 0, 512] at c = 16: the level path of the segmented sum."""
    for counts, start in ((sm.MIXED_COUNTS, 40), (sm.LEVEL_COUNTS, 100)):
        env.check(16, sm.batch_case(env.o, counts, start))
    assert cb.level_launches(sm.LEVEL_COUNTS, 16, 255) == 6


def test_scalar_bits_and_a_violation_in_the_last_msm(env):
    """scalar_bits 1 / 9 / 16 / 17 / 255 with the scalars' top bit set; a scalar of exactly 2^bits in the last MSM fails
    the whole call, in both forms, with the guard words around out_jac intact and nothing counted."""
    gpu = env.gpu
    for case in sm.bits_cases(env.o):
        env.check(16, case)
        if case[6] == 255:
            continue
        name, sizes, gs, rows, ks, counts, bits = bad = sm.violation_case(case)
        sets, one, _ = env.handles(bad, 16)
        r, sc, offs = np.array(rows, dtype=np.uint32), mm.to_limbs(env.o, ks), sm.offsets_of(counts)
        arr = (C.c_void_p * len(sets))(*[h._h for h in sets])
        before = env.stats()
        out = np.full(18 * len(counts) + 4, 77, dtype=np.uint64)
        rc = gpu._lib.curdle_msm_g1_ct_bases_sets_batch(arr, C.c_size_t(len(sets)), C.c_void_p(r.ctypes.data), C.c_void_p(sc.ctypes.data),
                                                        C.c_void_p(offs.ctypes.data), C.c_size_t(len(counts)), C.c_uint(bits),
                                                        C.c_void_p(out[2:].ctypes.data))
        assert rc == gpu.EINVAL and "scalar_bits" in gpu.last_error(), name
        assert (out == 77).all(), name
        with pytest.raises(gpu.CurdleError) as e:
            env.resident(sets, sc, r, offs, bits)
        assert e.value.code == gpu.EINVAL and "scalar_bits" in e.value.msg, name
        assert env.stats() == before, name
        for h in sets + [one]:
            h.free()


def test_the_limits(env):
    """c = 64 at 255 bits is 4 chunks: 16,384 pairs over two sets of 8,192 are 65,536 terms, accepted once; one more pair
    and a row equal to the total are refused before device work; so is a misaligned device pointer, behind the rows."""
    gpu = env.gpu
    n = cb.MAX_TERMS // 4
    a, q = env.o.Rand(35).get_frs(2)
    pts = env.co.points_walk(a, q, n)
    sc = np.random.default_rng(35).integers(0, 1 << 64, size=(n + 1, 4), dtype=np.uint64)
    sc[:, 3] &= np.uint64((1 << 62) - 1)                                    # Montgomery words of canonical scalars: < r
    sets = [gpu.CtBases(np.ascontiguousarray(pts[:n // 2]), 64), gpu.CtBases(np.ascontiguousarray(pts[n // 2:]), 64)]
    rows = np.arange(n + 1, dtype=np.uint32)[::-1].copy() % np.uint32(n)
    before = env.stats()
    got = gpu.msm_g1_ct_bases_sets_batch(sets, rows[:n], sc[:n], [0, n // 3, n])
    assert env.delta(before)[0] == {"tables": 0, "calls": 1, "lanes": cb.MAX_TERMS, "msms": 2}
    want = gpu.msm_g1_batch(np.ascontiguousarray(pts[rows[:n]]), sc[:n], [0, n // 3, n])
    assert (got == want).all()
    assert (got[1] == env.co.msm_pippenger(np.ascontiguousarray(pts[rows[n // 3:n]]), sc[n // 3:n], threads=4)).all()
    after = env.stats()
    with pytest.raises(gpu.CurdleError) as e:
        gpu.msm_g1_ct_bases_sets_batch(sets, rows, sc, [0, 1, n + 1])
    assert e.value.code == gpu.EINVAL and "65,536" in e.value.msg
    rows[5] = n
    with pytest.raises(gpu.CurdleError) as e:
        gpu.msm_g1_ct_bases_sets_batch(sets, rows[:9], sc[:9], [0, 4, 9])
    assert e.value.code == gpu.EINVAL and "not below" in e.value.msg
    out = np.full(20, 77, dtype=np.uint64)
    arr = (C.c_void_p * 2)(*[h._h for h in sets])
    offs = sm.offsets_of([3])
    dev = gpu._lib.curdle_msm_g1_ct_bases_sets_batch_device
    for off in (4, 8):
        rc = dev(arr, C.c_size_t(2), C.c_void_p(rows.ctypes.data + 64), C.c_void_p(0x7000_0000_1000 + off), C.c_void_p(offs.ctypes.data),
                 C.c_size_t(1), C.c_uint(255), C.c_void_p(out[1:].ctypes.data), None)
        assert rc == gpu.EINVAL and "multiples of 16" in gpu.last_error()
    assert (out == 77).all() and env.stats() == after
    for h in sets:
        h.free()


def test_streams_a_shutdown_and_a_second_context(env):
    """The _device form on a caller's stream and on the library's; the sets used after curdle_shutdown and re-init and
    first used on a second context of the same GPU: the copies are made again from the handles' rows, no table is built
    again."""
    import torch
    gpu = env.gpu
    case = sm.batch_case(env.o, [5, 0, 130], 900)
    name, sizes, gs, rows, ks, counts, bits = case
    sets, one, pts = env.handles(case, 16)
    r, sc, offs = np.array(rows, dtype=np.uint32), mm.to_limbs(env.o, ks), sm.offsets_of(counts)
    want = sm.expected(env.o, env.co, case, 16)
    s = torch.cuda.Stream()
    src = torch.from_numpy(sc.view(np.int64).reshape(-1)).pin_memory()
    with torch.cuda.stream(s):                                     # the scalars are written on the caller's stream
        d_sc = torch.zeros_like(src, device="cuda:0")
        d_sc.copy_(src, non_blocking=True)
        got = gpu.msm_g1_ct_bases_sets_batch_device(sets, r, d_sc.data_ptr(), offs, stream=s.cuda_stream)
    assert (got == want).all()
    torch.cuda.synchronize()
    assert (env.resident(sets, sc, r, offs, 255, stream=s.cuda_stream) == want).all()
    assert (env.resident(sets, sc, r, offs, 255) == want).all()
    del d_sc
    tables = gpu.stat_msm_ct_bases()["tables"]
    gpu.shutdown()
    gpu.init(0)
    assert (gpu.msm_g1_ct_bases_sets_batch(sets, r, sc, offs) == want).all()
    errors = []

    def second():
        try:
            gpu.set_device(1)
            assert (gpu.msm_g1_ct_bases_sets_batch(sets, r, sc, offs) == want).all()
            assert (one.msm_batch(sc, offs, r) == want).all()
        except BaseException as e:  # noqa: BLE001 - reported by the main thread
            errors.append(e)

    gpu.init_devices([0, 0])
    try:
        assert gpu.device_count() == 2
        th = threading.Thread(target=second)
        th.start()
        th.join()
        assert not errors, errors
        assert (gpu.msm_g1_ct_bases_sets_batch(sets, r, sc, offs) == want).all()   # context 0
    finally:
        gpu.set_device(-1)
        gpu.shutdown()
        gpu.init(0)
    assert gpu.device_count() == 1
    assert (gpu.msm_g1_ct_bases_sets_batch(sets, r, sc, offs) == want).all()
    assert gpu.stat_msm_ct_bases()["tables"] == tables
    for h in sets + [one]:
        h.free()


def test_one_thread_beside_a_bucket_msm(env):
    case = sm.batch_case(env.o, [129, 128], 500)
    name, sizes, gs, rows, ks, counts, bits = case
    sets, one, pts = env.handles(case, 16)
    r, sc, offs = np.array(rows, dtype=np.uint32), mm.to_limbs(env.o, ks), sm.offsets_of(counts)
    want = sm.expected(env.o, env.co, case, 16)
    a, q = env.o.Rand(1).get_frs(2)
    bases = env.co.points_walk(a, q, 4096)
    t = np.random.default_rng(4096).integers(0, 1 << 62, size=(4096, 4), dtype=np.uint64)
    exp = env.co.msm_pippenger(bases, t, threads=4)
    errors = []

    def worker():
        try:
            for _ in range(3):
                assert (env.gpu.msm_g1_ct_bases_sets_batch(sets, r, sc, offs) == want).all()
                assert (env.resident(sets, sc, r, offs, 255) == want).all()
        except BaseException as e:  # noqa: BLE001 - reported by the main thread
            errors.append(e)

    th = threading.Thread(target=worker)
    th.start()
    msms = [env.gpu.msm_g1(bases, t) for _ in range(3)]
    th.join()
    assert not errors, errors
    for got in msms:
        assert (got == exp).all()
    for h in sets + [one]:
        h.free()


def test_the_counters_of_calls_that_do_nothing(env):
    """A refused call and a call that needs no device count nothing; the same handle may stand for two sets."""
    gpu = env.gpu
    case = sm.bits_cases(env.o)[-1]
    name, sizes, gs, rows, ks, counts, bits = case
    sets, one, pts = env.handles(case, 16)
    r, sc, offs = np.array(rows, dtype=np.uint32), mm.to_limbs(env.o, ks), sm.offsets_of(counts)
    before = env.stats()
    assert gpu.msm_g1_ct_bases_sets_batch(sets, r, sc, [3]).shape == (0, 18)
    assert (gpu.msm_g1_ct_bases_sets_batch(sets, r, sc, [3, 3, 3]) == env.inf).all()
    for call in (lambda: gpu.msm_g1_ct_bases_sets_batch(sets, r, sc, [0, 5, 4]),
                 lambda: gpu.msm_g1_ct_bases_sets_batch(sets, r, sc, offs, 0),
                 lambda: gpu.msm_g1_ct_bases_sets_batch(sets + [gpu.CtBases(np.zeros((0, 12), dtype=np.uint64), 32)], r, sc, offs),
                 lambda: gpu.msm_g1_ct_bases_sets_batch(sets * 3, r, sc, offs)):
        with pytest.raises(gpu.CurdleError) as e:
            call()
        assert e.value.code == gpu.EINVAL
    assert env.stats() == before
    # sets (3, 3): the first handle twice, rows into the second copy
    twice = gpu.msm_g1_ct_bases_sets_batch([sets[0], sets[0]], np.array([3, 1, 5], dtype=np.uint32), sc[:3], [0, 3])
    assert (twice == sets[0].msm_batch(sc[:3], [0, 3], np.array([0, 1, 2], dtype=np.uint32))).all()
    for h in sets + [one]:
        h.free()
