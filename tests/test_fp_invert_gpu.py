"""curdle_fp_invert_batch / _device on the GPU (k_fp_invert, csrc/fp_invert_kernels.hip): the division-step inversion
of csrc/invert_ds.h against the big-integer model of tests/fp_divsteps_model.py AND against the same call under
CURDLE_FP_INVERT_FERMAT (the exponent chain of invert28.h), bit for bit.  The inputs are the model's case families; the
sizes straddle a wave and a block with 0 and p - 1 at the first and last index; the raw form feeds representatives in
[p, 2p) as the exit of the constant-time MSM may; the resident form runs on the library's stream and on a caller's,
between 0x5A guard bytes and in place; an element at or above p in the last position fails the call with CURDLE_EINVAL
and leaves the output (host form) and the guards untouched; the counters move by calls and elements."""
import threading

import numpy as np
import pytest

import fp_divsteps_model as m

pytestmark = pytest.mark.gpu

P = m.P
FERMAT, RAW = 1, 2


def gnark_rows(vals):
    return np.array([m.limbs(v, 64, 6) for v in vals], dtype=np.uint64).reshape(-1, 6)


def raw_rows(vals):
    """14 u32 limbs of 28 bits as 7 little-endian u64."""
    return np.array([m.limbs28(v) for v in vals], dtype=np.uint32).reshape(-1, 14).view(np.uint64)


def same(got, want, what=None):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (what, "%d rows differ, first at %d" % (bad.size, bad[0]))


@pytest.fixture(scope="module")
def cases():
    """Every case family once, as gnark elements, with the model's words for them (computed once, never changed)."""
    vals = m.all_cases()
    want = []
    for a in vals:
        y, viol = m.invert_gnark(a)
        assert viol == 0 and y == m.want_gnark(a)
        want.append(y)
    return vals, gnark_rows(vals), gnark_rows(want)


def resident(gpu, rows, flags=0, stream=None, off=0, in_place=False):
    """The resident call: the items start `off` items into their array (a multiple of 16 bytes), between guard bytes."""
    import torch
    n, item = rows.shape[0], rows.shape[1] * 8
    d_in = torch.from_numpy(np.ascontiguousarray(rows).view(np.int64).reshape(-1).copy()).to("cuda:0")
    d_out = torch.full((item * (n + off) + 32,), 0x5A, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    lo, hi = 16 + item * off, 16 + item * (off + n)
    gpu.fp_invert_batch_device(d_in.data_ptr(), n, d_in.data_ptr() if in_place else d_out.data_ptr() + lo, flags=flags, stream=stream)
    out = d_out.cpu().numpy()
    if in_place:
        assert (out == 0x5A).all()
        return d_in.cpu().numpy().view(np.uint64).reshape(rows.shape)
    assert (d_in.cpu().numpy().view(np.uint64).reshape(rows.shape) == rows).all()
    assert (out[:lo] == 0x5A).all() and (out[hi:] == 0x5A).all()             # nothing outside the rows
    return out[lo:hi].copy().view(np.uint64).reshape(rows.shape)


def test_every_case_family_against_the_model_and_the_fermat_flag(gpu, cases):
    vals, rows, want = cases
    a = gpu.stat_fp_invert()
    got = gpu.fp_invert_batch(rows)
    b = gpu.stat_fp_invert()
    same(got, want, "division steps")
    assert (b["calls"] - a["calls"], b["elements"] - a["elements"]) == (1, len(vals))
    same(gpu.fp_invert_batch(rows, flags=FERMAT), want, "fermat")
    c = gpu.stat_fp_invert()
    assert (c["calls"] - b["calls"], c["elements"] - b["elements"]) == (1, len(vals))
    assert (c["finish_divsteps"], c["finish_fermat"]) == (a["finish_divsteps"], a["finish_fermat"])
    same(resident(gpu, rows), want, "resident")
    same(resident(gpu, rows, flags=FERMAT), want, "resident fermat")
    # x x^-1 = 1 through the model's own product: the words are inverses, not merely equal to the model's
    rinv = pow(m.R384, -1, P)
    for x, row in list(zip(vals, got))[:40]:
        y = m.value([int(w) for w in row], 64)
        assert x == 0 and y == 0 or (x * rinv) * (y * rinv) % P == 1


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1000])
def test_sizes_with_zero_and_p_minus_1_at_the_edges(gpu, cases, n):
    vals, rows, want = cases
    idx = (np.arange(n) * 7 + n) % len(vals)
    idx[0] = vals.index(0)
    idx[-1] = vals.index(P - 1) if n > 1 else idx[0]
    r, w = rows[idx], want[idx]
    if n > 1:
        assert not w[0].any() and (r[-1] == gnark_rows([P - 1])[0]).all()
    same(gpu.fp_invert_batch(r), w, "host")
    same(gpu.fp_invert_batch(r, flags=FERMAT), w, "host fermat")
    same(resident(gpu, r, off=1), w, "resident")
    same(resident(gpu, r, flags=FERMAT, off=1), w, "resident fermat")


def test_the_raw_form_on_representatives_in_p_to_2p(gpu):
    """CURDLE_FP_INVERT_RAW28: invert_ds(F28&, const F28&) as the exit calls it, on [0, 2p)."""
    base = m.fixed_cases() + m.random_cases(80)
    vals = base + [c + P for c in base] + list(m.RAW_EXTRA)
    assert all(v < 2 * P for v in vals) and sum(v >= P for v in vals) >= len(base)
    want = []
    for a in vals:
        y, viol = m.invert_raw28(a)
        assert viol == 0 and y % P == m.want_raw28(a % P)
        want.append(y % P)                                                   # the kernel stores the canonical limbs
    rows, want = raw_rows(vals), raw_rows(want)
    same(gpu.fp_invert_batch(rows, flags=RAW), want, "raw")
    same(gpu.fp_invert_batch(rows, flags=RAW | FERMAT), want, "raw fermat")
    same(resident(gpu, rows, flags=RAW, off=2), want, "raw resident")        # 2 x 56 bytes: a multiple of 16
    same(resident(gpu, rows, flags=RAW, in_place=True), want, "raw in place")
    for bad, what in ((2 * P, "2p"), (2 * P + 5, "above 2p")):
        with pytest.raises(gpu.CurdleError) as e:
            gpu.fp_invert_batch(raw_rows(vals[:64] + [bad]), flags=RAW)
        assert e.value.code == gpu.EINVAL, what
    wide = raw_rows(vals[:65]).copy()
    wide.view(np.uint32)[64, 3] |= 1 << 28                                   # a limb at 2^28
    with pytest.raises(gpu.CurdleError):
        gpu.fp_invert_batch(wide, flags=RAW)


def test_in_place_and_streams(gpu, cases):
    import torch
    vals, rows, want = cases
    r, w = rows[:300], want[:300]
    buf = r.copy()
    assert gpu.fp_invert_batch(buf, out=buf) is buf                          # the host form, out == in
    same(buf, w, "host in place")
    s = torch.cuda.Stream()
    for stream in (None, s.cuda_stream):
        for flags in (0, FERMAT):
            same(resident(gpu, r, flags=flags, stream=stream, off=1), w, (stream, flags))
            same(resident(gpu, r, flags=flags, stream=stream, in_place=True), w, (stream, flags, "in place"))
    # written on the caller's stream immediately before the call
    src = torch.from_numpy(r.view(np.int64).reshape(-1).copy()).pin_memory()
    with torch.cuda.stream(s):
        d = torch.zeros_like(src, device="cuda:0")
        d.copy_(src, non_blocking=True)
        gpu.fp_invert_batch_device(d.data_ptr(), len(r), d.data_ptr(), stream=s.cuda_stream)
        back = d.cpu().numpy()
    same(back.view(np.uint64).reshape(r.shape), w, "behind the caller's copy")
    torch.cuda.synchronize()


@pytest.mark.parametrize("bad", [P, P + 1, (1 << 384) - 1])
def test_an_element_out_of_range_in_the_last_position(gpu, cases, bad):
    import torch
    vals, rows, want = cases
    r = np.concatenate([rows[:256], gnark_rows([bad])])
    for flags in (0, FERMAT):
        out = np.full(r.shape, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
        a = gpu.stat_fp_invert()
        with pytest.raises(gpu.CurdleError) as e:
            gpu.fp_invert_batch(r, flags=flags, out=out)
        assert e.value.code == gpu.EINVAL and "below p" in str(e.value)
        assert (out == 0x5A5A5A5A5A5A5A5A).all()                             # untouched
        assert gpu.stat_fp_invert() == a                                     # not a completed call
        d_in = torch.from_numpy(r.view(np.int64).reshape(-1).copy()).to("cuda:0")
        d_out = torch.full((48 * len(r) + 32,), 0x5A, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        with pytest.raises(gpu.CurdleError) as e:
            gpu.fp_invert_batch_device(d_in.data_ptr(), len(r), d_out.data_ptr() + 16, flags=flags)
        assert e.value.code == gpu.EINVAL
        o = d_out.cpu().numpy()
        assert (o[:16] == 0x5A).all() and (o[-16:] == 0x5A).all()            # the guard words
        assert (d_in.cpu().numpy().view(np.uint64).reshape(r.shape) == r).all()
    same(gpu.fp_invert_batch(rows[:256]), want[:256], "the call after a refusal")


def test_one_call_beside_a_thread_running_a_bucket_msm(gpu, oracle, coracle, cases):
    vals, rows, want = cases
    k, q = oracle.Rand(1).get_frs(2)
    bases = coracle.points_walk(k, q, 4096)
    t = np.random.default_rng(4096).integers(0, 1 << 62, size=(4096, 4), dtype=np.uint64)
    exp = coracle.msm_pippenger(bases, t, threads=4)
    errors, msms = [], []

    def worker():
        try:
            for _ in range(3):
                msms.append(gpu.msm_g1(bases, t))
        except BaseException as e:  # noqa: BLE001 - reported by the main thread
            errors.append(e)

    th = threading.Thread(target=worker)
    th.start()
    same(gpu.fp_invert_batch(rows), want, "beside an MSM")
    same(resident(gpu, rows[:257], flags=FERMAT), want[:257], "beside an MSM, resident")
    th.join()
    assert not errors, errors
    assert len(msms) == 3 and all((g == exp).all() for g in msms)


def test_a_second_context(gpu, cases):
    """Both contexts on one GPU: the slot, the stream and the staging are the second context's."""
    vals, rows, want = cases
    r, w = rows[:257], want[:257]
    gpu.init_devices([0, 0])
    try:
        assert gpu.device_count() == 2
        box = {}

        def run():
            try:
                gpu.set_device(1)
                a = gpu.stat_fp_invert()
                box["host"] = gpu.fp_invert_batch(r)
                box["fermat"] = gpu.fp_invert_batch(r, flags=FERMAT)
                box["resident"] = resident(gpu, r, off=1)
                b = gpu.stat_fp_invert()
                box["moved"] = (b["calls"] - a["calls"], b["elements"] - a["elements"])
            except BaseException as e:  # noqa: BLE001 - reported by the test's thread
                box["e"] = e

        th = threading.Thread(target=run)
        th.start()
        th.join()
        assert "e" not in box, box.get("e")
        for key in ("host", "fermat", "resident"):
            same(box[key], w, key)
        assert box["moved"] == (3, 3 * len(r))
        same(gpu.fp_invert_batch(r), w, "context 0 beside it")
    finally:
        gpu.set_device(-1)
        gpu.shutdown()
        gpu.init(0)
    assert gpu.device_count() == 1
    same(gpu.fp_invert_batch(r), w, "after the contexts were closed")
