"""CPU tests of the batched early-fixing boundary of the segmentation flavour (lpbox_seg_batch_*, lpbox_hip.seg.SegBatch): what
_create refuses (status and offending index), the argument and call-order checks that come before any device call, and -- without a
device -- that the compute calls fail with LPBOX_E_NODEVICE (no CPU fallback)."""
import ctypes as C

import numpy as np
import pytest

from helpers import banded_seg_problem

E_BADARG, E_STATE, E_NODEVICE, E_UNSUPPORTED = -2, -3, -6, -7
NAMES = ["lpbox_seg_batch_create", "lpbox_seg_batch_destroy", "lpbox_seg_batch_init", "lpbox_seg_batch_set_active",
         "lpbox_seg_batch_iterate_l2f", "lpbox_seg_batch_get_x_iters_device", "lpbox_seg_batch_iterate_l2f_scores"]


def solver(n=40, seed=0):
    from lpbox_hip.seg import PyLPboxADMMsolver
    s = PyLPboxADMMsolver(0, n, seed)
    s.write_files = False
    s.set_problem(banded_seg_problem(n, seed))
    return s


def refused(solvers):
    from lpbox_hip.lp import LpboxError
    from lpbox_hip.seg import SegBatch
    with pytest.raises(LpboxError) as e:
        SegBatch(solvers)
    return e.value


def test_library_exports_and_python_binds_the_batch_functions():
    from lpbox_hip import _lib, l2f, seg
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), f"liblpbox_hip.so does not export {name}"
        assert name in _lib.SYMBOLS
    assert hasattr(seg, "SegBatch") and hasattr(l2f, "run_l2f_seg_batch")


def test_create_refuses_with_status_and_index():
    from lpbox_hip import _lib
    from lpbox_hip.seg import PyLPboxADMMsolver, SegBatch
    L = _lib.load()
    with pytest.raises(ValueError):
        SegBatch([])
    assert not L.lpbox_seg_batch_create(None, 0)
    assert L.lpbox_last_status() == E_BADARG and b"empty" in L.lpbox_last_error()
    a, b = solver(40, 0), solver(48, 1)

    lp = L.lpbox_create(_lib.FLAVOUR_LP, 1, 0)              # an LP-flavour handle at index 1
    assert lp
    hs = (C.c_void_p * 2)(a._h, C.c_void_p(lp))
    assert not L.lpbox_seg_batch_create(hs, 2)
    msg = L.lpbox_last_error()
    assert L.lpbox_last_status() == E_STATE and b"problem 1" in msg and b"LP" in msg

    class Fake:                                             # the same refusal through the Python class
        _have_problem = True
        _h = hs[1]
        _L = L
    e = refused([a, b, Fake()])
    assert e.code == E_STATE and "problem 2" in str(e)

    empty = PyLPboxADMMsolver(0, 40, 0)                      # no image, no problem
    empty._have_problem = True                              # (keep SegBatch from looking for <problem>.jpg)
    e = refused([a, empty])
    assert e.code == E_STATE and "problem 1" in str(e) and "no image" in str(e)

    e = refused([a, b, a])
    assert e.code == E_BADARG and "problem 0 and problem 2" in str(e) and "same handle" in str(e)

    assert L.lpbox_set_record(b._h, 1) == 0
    e = refused([a, b])
    assert e.code == E_UNSUPPORTED and "problem 1" in str(e) and "recording" in str(e)
    assert L.lpbox_set_record(b._h, 0) == 0
    SegBatch([a, b]).close()                                # and now it is accepted -- without a device call
    L.lpbox_destroy(C.c_void_p(lp))


def test_argument_and_call_order_checks_come_before_the_device():
    from lpbox_hip import _lib
    from lpbox_hip.lp import LpboxError
    from lpbox_hip.seg import SegBatch
    a, b = solver(40, 0), solver(48, 1)
    B = SegBatch([a, b])
    zeros = np.zeros(2, np.int32)
    with pytest.raises(LpboxError, match="solve_init has not been called") as e:
        B.solve_iter_l2f(0, 10, None, zeros)                # before _init
    assert e.value.code == E_STATE
    with pytest.raises(LpboxError, match="exceeds the 10 columns") as e:
        B.solve_iter_l2f(0, 11, None, zeros)                # longer than SEG_XITERS_COLS
    assert e.value.code == E_BADARG
    with pytest.raises(LpboxError, match="exceeds the 10 columns") as e:
        B.solve_iter_l2f_scores(0, 11, None)
    assert e.value.code == E_BADARG
    vecs = -np.ones((2, 48))
    vecs[1, :3] = (1.0, 0.0, 1.0)
    for nums, what in (((0, 2), "problem 1 of the batch: vec fixes 3 variables but num = 2"),      # disagrees with its vector
                       ((0, -1), "problem 1 of the batch: fix count -1"),                           # negative
                       ((41, 3), "problem 0 of the batch: fix count 41 outside \\[0,40\\]")):         # more than the live count
        with pytest.raises(LpboxError, match=what) as e:
            B.solve_iter_l2f(0, 10, vecs, np.array(nums, np.int32))
        assert e.value.code == E_BADARG, nums
    with pytest.raises(LpboxError, match="fix vector missing") as e:
        B.solve_iter_l2f(0, 10, None, np.array((0, 3), np.int32))
    assert e.value.code == E_BADARG
    # scores without a preceding pack: the pointer is never read
    L = _lib.load()
    rets, fixed = np.zeros(2, np.int32), np.zeros(2, np.int32)
    rc = L.lpbox_seg_batch_iterate_l2f_scores(B._h, 0, 10, C.c_void_p(64), 0.9, 0.1, 10, rets.ctypes.data_as(C.c_void_p),
                                              fixed.ctypes.data_as(C.c_void_p))
    assert rc == E_STATE and b"lpbox_seg_batch_get_x_iters_device has not been called" in L.lpbox_last_error()
    # an inactive problem's arguments are not looked at
    B.set_active([True, False])
    with pytest.raises(LpboxError, match="solve_init has not been called"):
        B.solve_iter_l2f(0, 10, vecs, np.array((0, -1), np.int32))
    with pytest.raises(ValueError):
        B.set_active([True])
    assert L.lpbox_seg_batch_init(None) < 0 and L.lpbox_seg_batch_iterate_l2f(None, 0, 10, None, 0, None, None) < 0
    B.close()


def test_no_device_no_compute():
    from lpbox_hip import _lib
    from lpbox_hip.l2f import run_l2f_seg_batch
    from lpbox_hip.lp import LpboxError
    from lpbox_hip.seg import SegBatch
    L = _lib.load()
    a, b = solver(40, 0), solver(48, 1)
    B = SegBatch([a, b])
    if L.lpbox_device_count() > 0:                          # with a device the same calls work (tests/test_seg_l2f_batch_gpu.py has the rest)
        assert B.solve_init() == 1
        assert set(B.solve_iter_l2f(0, 10, None, np.zeros(2, np.int32))) <= {0, 1}
        B.close()
        return
    with pytest.raises(LpboxError, match="no HIP device") as e:
        B.solve_init()
    assert e.value.code == E_NODEVICE
    with pytest.raises(LpboxError, match="solve_init has not been called"):      # nobody was flagged initialised
        B.solve_iter_l2f(0, 10, None, np.zeros(2, np.int32))
    B.close()
    with pytest.raises(LpboxError, match="no HIP device") as e:
        run_l2f_seg_batch([a, b], lambda x: x[:, 0, 0])
    assert e.value.code == E_NODEVICE
