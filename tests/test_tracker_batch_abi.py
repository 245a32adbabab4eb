"""curdle_whisk_is_valid_tracker_proof_batch at its C ABI, without a GPU: the empty batch, null
arguments, and a loud ENODEV (never a verdict) when no device is visible."""
import ctypes as C
import os

import numpy as np
import pytest


def _fn(cm):
    f = cm._lib.curdle_whisk_is_valid_tracker_proof_batch
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    return f


def _args(k):
    return (np.zeros(96 * k, np.uint8), np.zeros(48 * k, np.uint8), np.zeros(128 * k, np.uint8))


def test_empty_batch_is_ok_and_writes_nothing(cm):
    f = _fn(cm)
    res = np.full(4, 77, dtype=np.int32)
    t, kc, p = _args(1)
    assert f(t.ctypes.data, kc.ctypes.data, p.ctypes.data, 0, res.ctypes.data) == cm.OK
    assert f(None, None, None, 0, None) == cm.OK
    assert (res == 77).all()
    assert len(cm.whisk_is_valid_tracker_proof_batch([], [], [])) == 0


def test_null_arguments_are_einval(cm):
    f = _fn(cm)
    t, kc, p = _args(2)
    res = np.full(2, 77, dtype=np.int32)
    for args in ((None, kc.ctypes.data, p.ctypes.data), (t.ctypes.data, None, p.ctypes.data),
                 (t.ctypes.data, kc.ctypes.data, None)):
        res[:] = 77
        assert f(*args, 2, res.ctypes.data) == cm.EINVAL
        assert (res == cm.EINVAL).all()
    assert f(t.ctypes.data, kc.ctypes.data, p.ctypes.data, 2, None) == cm.EINVAL


def test_binding_checks_lengths(cm):
    t, kc, p = bytes(96), bytes(48), bytes(128)
    with pytest.raises(ValueError):
        cm.whisk_is_valid_tracker_proof_batch([t], [kc], [])
    with pytest.raises(ValueError):
        cm.whisk_is_valid_tracker_proof_batch([t[:95]], [kc], [p])


@pytest.mark.skipif(os.environ.get("CURDLE_EXPECT_GPU") == "1", reason="GPU box")
def test_no_device_is_enodev_in_every_result(cm):
    if cm.device_available():
        pytest.skip("a device is visible")
    f = _fn(cm)
    for k in (1, 3, 1000):
        t, kc, p = _args(k)
        res = np.full(k, 77, dtype=np.int32)
        assert f(t.ctypes.data, kc.ctypes.data, p.ctypes.data, k, res.ctypes.data) == cm.ENODEV
        assert (res == cm.ENODEV).all()
    with pytest.raises(cm.CurdleError) as e:
        cm.whisk_is_valid_tracker_proof_batch([bytes(96)], [bytes(48)], [bytes(128)])
    assert e.value.code == cm.ENODEV
