"""Keccak-f[1600] on the device, both forms (curdle_keccak_permute_batch: a state per lane, csrc/keccak_dev.h, and a
state spread over the lanes of a wave half, csrc/keccak_sheet.h), against the model's permutation
(tests/merlin_model.py): the zero state, all ones, the 50 states with one word set to 1 or to 2^63 (every rho offset
across the word boundary, every pi route), random states; 1, 2 and 24 dependent permutations; counts that leave the
last wave half, wave and block partly empty."""
import numpy as np
import pytest

import merlin_model as mm

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 63, 64, 65, 129)
REPS = (1, 2, 24)
_cache = {}


def inputs():
    """129 states: zero, all ones, one word = 1 (25), one word = 2^63 (25), 64 + 13 random."""
    rows = [np.zeros(25, dtype=np.uint64), np.full(25, np.uint64((1 << 64) - 1))]
    for v in (1, 1 << 63):
        for w in range(25):
            s = np.zeros(25, dtype=np.uint64)
            s[w] = np.uint64(v)
            rows.append(s)
    rnd = np.random.default_rng(1600).integers(0, 1 << 64, size=(77, 25), dtype=np.uint64)
    a = np.concatenate([np.array(rows), rnd])
    assert a.shape == (129, 25)
    return a


def reference():
    """(inputs, {reps: the model's states}), computed once and read-only."""
    if not _cache:
        a = inputs()
        want, cur = {}, [[int(v) for v in row] for row in a]
        for r in range(1, max(REPS) + 1):
            cur = [mm.keccak_f1600(s) for s in cur]
            if r in REPS:
                want[r] = np.array(cur, dtype=np.uint64)
                want[r].setflags(write=False)
        a.setflags(write=False)
        _cache["ref"] = (a, want)
    return _cache["ref"]


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_both_forms_equal_the_model(gpu, form, n):
    a, want = reference()
    for reps in REPS:
        got, ms = gpu.keccak_permute_batch(a[:n], form, reps, want_ms=True)
        assert (got == want[reps][:n]).all(), (form, n, reps)
        assert ms > 0
    # the same states one place on: every input on the other half of its wave
    if n == 129:
        for reps in REPS:
            assert (gpu.keccak_permute_batch(a[1:], form, reps) == want[reps][1:]).all(), (form, reps)


def test_the_forms_agree_on_a_thousand_states(gpu):
    a = np.random.default_rng(24).integers(0, 1 << 64, size=(1000, 25), dtype=np.uint64)
    lane = gpu.keccak_permute_batch(a, gpu.KECCAK_LANE, 24)
    sheet = gpu.keccak_permute_batch(a, gpu.KECCAK_SHEET, 24)
    assert (lane == sheet).all()
    for i in (0, 999):
        s = [int(v) for v in a[i]]
        for _ in range(24):
            s = mm.keccak_f1600(s)
        assert [int(v) for v in sheet[i]] == s


def test_in_place_and_refusals_on_the_device(gpu):
    import ctypes as C
    a, want = reference()
    buf = a[:65].copy()
    f = gpu._lib.curdle_keccak_permute_batch
    assert f(buf.ctypes.data_as(C.c_void_p), 65, 1, 2, buf.ctypes.data_as(C.c_void_p), None) == gpu.OK
    assert (buf == want[2][:65]).all()
    before = buf.copy()
    assert f(buf.ctypes.data_as(C.c_void_p), 65, 2, 2, buf.ctypes.data_as(C.c_void_p), None) == gpu.EINVAL
    assert f(buf.ctypes.data_as(C.c_void_p), 65, 1, 0, buf.ctypes.data_as(C.c_void_p), None) == gpu.EINVAL
    assert (buf == before).all()
