"""CPU tests of the LP batch's early-fixing window that takes its scores on the device (lpbox_get_x_iters_rows_device,
lpbox_iterate_l2f_scores; LpBatch.x_iters_rows_torch / solve_iter_l2f_scores; l2f.run_l2f_batch_device): the symbols and their
bindings, every argument and call-order check that comes before a device call, with its status and message, and -- without a
device -- that the compute calls fail with LPBOX_E_NODEVICE (no CPU fallback).  tests/test_lp_l2f_scores_gpu.py has the rest."""
import ctypes as C

import numpy as np
import pytest

from helpers import lp_instances

E_BADARG, E_STATE, E_NODEVICE = -2, -3, -6
NAMES = ["lpbox_get_x_iters_rows_device", "lpbox_iterate_l2f_scores"]
FAKE = C.c_void_p(64)            # a non-null "device pointer" that no check may read


def batch(k=2):
    from lpbox_hip.lp import LpBatch
    return LpBatch(lp_instances("lp_20_60_seed0.npz")[:k])


def scores_call(L, h, i, j, ptr, hi=0.9, lo=0.1, min_fix=10, B=2):
    rets, fixed = np.zeros(B, np.int32), np.zeros(B, np.int32)
    rc = L.lpbox_iterate_l2f_scores(h, i, j, ptr, hi, lo, min_fix, rets.ctypes.data_as(C.c_void_p), fixed.ctypes.data_as(C.c_void_p))
    return rc, L.lpbox_last_status(), L.lpbox_last_error()


def test_library_exports_and_python_binds_the_two_functions():
    from lpbox_hip import _lib, l2f
    from lpbox_hip.lp import LpBatch
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), f"liblpbox_hip.so does not export {name}"
        assert name in _lib.SYMBOLS
    assert hasattr(LpBatch, "x_iters_rows_torch") and hasattr(LpBatch, "solve_iter_l2f_scores")
    assert hasattr(l2f, "run_l2f_batch_device")


def test_every_check_comes_before_the_device_with_its_status_and_message():
    from lpbox_hip import _lib
    L = _lib.load()
    b = batch()
    # a segmentation handle
    seg = C.c_void_p(L.lpbox_create(_lib.FLAVOUR_SEG, 1, 0))
    assert seg
    rc, st, msg = scores_call(L, seg, 0, 100, None, B=1)
    assert rc == st == E_STATE and b"LP flavour" in msg
    ptr = C.c_void_p()
    assert L.lpbox_get_x_iters_rows_device(seg, 100, C.byref(ptr), None) == E_STATE and b"LP flavour" in L.lpbox_last_error()
    L.lpbox_destroy(seg)
    # the window is longer than x_iters (the text of lpbox_iterate_l2f)
    rc, st, msg = scores_call(L, b._h, 0, 501, None)
    assert rc == st == E_BADARG and b"window of 501 iterations exceeds the 500 columns of x_iters" in msg
    # min_fix
    rc, st, msg = scores_call(L, b._h, 0, 100, None, min_fix=-1)
    assert rc == st == E_BADARG and b"min_fix = -1 is negative" in msg
    # thresholds
    for hi, lo in ((np.nan, 0.1), (0.9, np.nan), (np.inf, 0.1), (0.9, -np.inf), (0.1, 0.9)):
        rc, st, msg = scores_call(L, b._h, 0, 100, None, hi=hi, lo=lo)
        assert rc == st == E_BADARG and b"thresholds" in msg and b"finite and hi >= lo" in msg, (hi, lo)
    rc, st, msg = scores_call(L, b._h, 0, 100, None, hi=0.5, lo=0.5)          # hi == lo is allowed: the next check answers
    assert rc == st == E_STATE and b"solve_init has not been called" in msg
    # scores without a row table: the pointer is never read
    rc, st, msg = scores_call(L, b._h, 0, 100, FAKE)
    assert rc == st == E_STATE and b"lpbox_get_x_iters_rows_device has not been called since the last window" in msg
    # no scores, not initialised: the text of lpbox_iterate_l2f
    rc, st, msg = scores_call(L, b._h, 0, 100, None)
    assert rc == st == E_STATE and msg == b"solve_init has not been called"
    # the table itself needs a window
    assert L.lpbox_get_x_iters_rows_device(b._h, 100, C.byref(ptr), None) == E_STATE
    assert L.lpbox_last_error() == b"solve_iter_l2f has not been called"
    assert L.lpbox_iterate_l2f_scores(None, 0, 100, None, 0.9, 0.1, 10, None, None) < 0
    assert L.lpbox_get_x_iters_rows_device(None, 100, None, None) < 0
    b.close()


def test_python_refuses_scores_that_are_no_float32_device_tensor_before_the_library():
    import torch
    b = batch()
    for bad in (np.zeros(120, np.float32), torch.zeros(120, dtype=torch.float32), torch.zeros(120, dtype=torch.float64), [0.5] * 120):
        with pytest.raises(ValueError, match="float32 CUDA tensor"):          # (the library would have said "solve_init has not been called")
            b.solve_iter_l2f_scores(0, 100, bad)
    b.close()


def test_active_mask_change_invalidates_the_table_and_a_repeat_does_not():
    """Needs a table, hence a device: without one the check cannot be reached (tests/test_lp_l2f_scores_gpu.py runs it too)."""
    from lpbox_hip import _lib
    L = _lib.load()
    if L.lpbox_device_count() < 1:
        return
    b = batch()
    b.solve_init()
    b.solve_iter_l2f_scores(0, 10)
    ptr, first = C.c_void_p(), np.zeros(3, np.int32)
    assert L.lpbox_get_x_iters_rows_device(b._h, 10, C.byref(ptr), first.ctypes.data_as(C.c_void_p)) == 120
    assert first.tolist() == [0, 60, 120]
    b.set_active([True, True])                                                # repeats the mask: the table stays
    b.set_active([True, False])
    rc, st, msg = scores_call(L, b._h, 10, 20, FAKE)
    assert rc == st == E_STATE and b"lpbox_set_active changed the active instances after the row table was built" in msg
    b.close()


def test_no_device_no_compute():
    from lpbox_hip import _lib
    from lpbox_hip.l2f import run_l2f_batch_device
    from lpbox_hip.lp import LpboxError
    L = _lib.load()
    b = batch()
    if L.lpbox_device_count() > 0:                          # with a device the same calls work
        assert b.solve_init() == 1
        rets, fixed = b.solve_iter_l2f_scores(0, 100)
        assert set(rets) <= {0, 1} and not fixed.any()
        b.close()
        return
    with pytest.raises(LpboxError, match="no HIP device") as e:
        b.solve_init()
    assert e.value.code == E_NODEVICE
    with pytest.raises(LpboxError, match="solve_init has not been called"):      # nobody was flagged initialised
        b.solve_iter_l2f_scores(0, 100)
    with pytest.raises(LpboxError, match="no HIP device") as e:
        run_l2f_batch_device(b, lambda x: x[:, -1, -1])
    assert e.value.code == E_NODEVICE
    b.close()
