"""Call-order rules of the large-instance path's reference summation order (lpbox_big_set_order / lpbox_big_set_problem_vals) that
answer without a device: lpbox_big_create and the problem upload are host-only."""
import ctypes as C

import numpy as np
import pytest

from lpbox_hip import _lib

E_BADARG, E_STATE, E_UNSUPPORTED = -2, -3, -7


@pytest.fixture
def L():
    return _lib.load()


def tiny():
    colptr = np.array([0, 1, 3, 4], np.int32)
    rowidx = np.array([0, 0, 1, 1], np.int32)
    return 3, 2, colptr, rowidx, np.array([-1.0, -2.0, -3.0])


def create(L, world=1):
    h = C.c_void_p(L.lpbox_big_create(0, world, 0))
    assert h
    return h


def order_of(L, h):
    v = C.c_double(-1.0)
    assert L.lpbox_big_get_scalar(h, b"order", C.byref(v)) == 0
    return v.value


def set_vals(L, h, vals):
    n, l, cp, ri, b = tiny()
    vals = np.ascontiguousarray(vals, np.float64)
    return L.lpbox_big_set_problem_vals(h, n, 0, n, l, cp, ri, b, None, vals.ctypes.data_as(C.c_void_p))


def test_order_is_set_before_the_problem(L):
    h = create(L)
    assert order_of(L, h) == 0.0
    assert L.lpbox_big_set_order(h, 1) == 0 and order_of(L, h) == 1.0
    assert L.lpbox_big_set_order(h, 0) == 0 and order_of(L, h) == 0.0
    assert L.lpbox_big_set_order(h, 7) == E_BADARG
    n, l, cp, ri, b = tiny()
    assert L.lpbox_big_set_problem(h, n, 0, n, l, cp, ri, b, None) == 0
    assert L.lpbox_big_set_order(h, 1) == E_STATE
    assert order_of(L, h) == 0.0
    L.lpbox_big_destroy(h)


def test_one_rank_without_transport_and_with_the_reference_pcg(L):
    h = create(L, world=2)
    assert L.lpbox_big_set_order(h, 1) == E_UNSUPPORTED
    assert L.lpbox_big_set_order(h, 0) == 0
    L.lpbox_big_destroy(h)
    cb = _lib.ALLGATHER_FN(lambda *a: 0)
    for first in ("order", "other"):
        for other in ("allgather", "lean", "rccl"):
            if other == "rccl" and first == "other":
                continue                                   # creating a communicator needs a device: test_communicator_first in tests/test_big_ref_order_gpu.py
            h = create(L)
            call = {"allgather": lambda: L.lpbox_big_set_allgather(h, C.cast(cb, C.c_void_p), None),
                    "lean": lambda: L.lpbox_big_set_pcg_mode(h, 1),
                    "rccl": lambda: L.lpbox_big_rccl_init(h, (C.c_ubyte * 128)())}[other]
            if first == "order":
                assert L.lpbox_big_set_order(h, 1) == 0
                assert call() == E_UNSUPPORTED, (first, other)
                assert order_of(L, h) == 1.0
            else:
                assert call() == 0
                assert L.lpbox_big_set_order(h, 1) == E_UNSUPPORTED, (first, other)
                assert order_of(L, h) == 0.0
            L.lpbox_big_destroy(h)


def test_stored_values(L):
    h = create(L)                                          # default order: unit values only
    assert set_vals(L, h, [1.0, 2.0, 1.0, 1.0]) == E_UNSUPPORTED
    assert b"lpbox_big_set_order" in L.lpbox_last_error()
    assert set_vals(L, h, [1.0, 1.0, 1.0, 1.0]) == 0
    L.lpbox_big_destroy(h)
    for bad in (np.inf, -np.inf, np.nan):
        h = create(L)
        assert L.lpbox_big_set_order(h, 1) == 0
        assert set_vals(L, h, [1.0, bad, 1.0, 1.0]) == E_BADARG
        assert set_vals(L, h, [0.0, -2.5, 1e-300, 1.0]) == 0     # an explicit zero, a negative and a tiny value are stored entries
        v = C.c_double()
        assert L.lpbox_big_get_scalar(h, b"valued", C.byref(v)) == 0 and v.value == 1.0
        L.lpbox_big_destroy(h)
    h = create(L)
    assert L.lpbox_big_set_order(h, 1) == 0
    assert set_vals(L, h, [1.0, 1.0, 1.0, 1.0]) == 0
    v = C.c_double()
    assert L.lpbox_big_get_scalar(h, b"valued", C.byref(v)) == 0 and v.value == 0.0
    L.lpbox_big_destroy(h)


def test_non_finite_objective_entry_is_a_bad_argument(L):
    """b is checked on the host like the stored values, by both entry points and in both orders; a subnormal, a
    zero and 1e300 are values like any other."""
    n, l, cp, ri, b = tiny()
    ones = np.ones(4)
    for order in (0, 1):
        for bad in (np.nan, np.inf, -np.inf):
            for with_vals in (False, True):
                h = create(L)
                assert L.lpbox_big_set_order(h, order) == 0
                v = b.copy()
                v[1] = bad
                # a shard that starts at global column 5 of 9: the message carries both indices
                rc = (L.lpbox_big_set_problem_vals(h, 9, 5, n, l, cp, ri, v, None, ones.ctypes.data_as(C.c_void_p)) if with_vals
                      else L.lpbox_big_set_problem(h, 9, 5, n, l, cp, ri, v, None))
                assert rc == E_BADARG, (order, bad, with_vals)
                msg = L.lpbox_last_error()
                assert b"local index 1" in msg and b"global 6" in msg, msg
                ok = np.array([-1e-310, 0.0, 1e300])
                assert L.lpbox_big_set_problem(h, n, 0, n, l, cp, ri, ok, None) == 0       # the refused call left the handle usable
                L.lpbox_big_destroy(h)
        h = create(L)
        assert L.lpbox_big_set_order(h, order) == 0
        assert L.lpbox_big_set_problem_vals(h, n, 0, n, l, cp, ri, np.array([5e-324, -0.0, -1e300]), None, ones.ctypes.data_as(C.c_void_p)) == 0
        L.lpbox_big_destroy(h)


def test_dropin_class_keeps_the_refusal_by_default():
    from lpbox_hip.lp import PyLPboxADMMsolver
    s = PyLPboxADMMsolver(0)
    s.set_order("reference")
    assert s.large_ok is False
    s.set_order("reference", large_ok=True)
    assert s.large_ok is True and s.order == "reference"


def test_dropin_class_refuses_the_iteration_log_on_the_large_route():
    """Refused at solve_init, before any device call, with LPBOX_E_UNSUPPORTED."""
    import numpy as np
    from lpbox_hip._lib import LpboxError
    from lpbox_hip.lp import PyLPboxADMMsolver
    n, l = 2100, 700
    colptr = np.arange(n + 1, dtype=np.int32)
    rowidx = (np.arange(n) % l).astype(np.int32)
    s = PyLPboxADMMsolver(0)
    s.set_order("reference", large_ok=True)
    s.write_log = True
    s.set_problem(n, l, colptr, rowidx, -np.ones(n))
    with pytest.raises(LpboxError) as e:
        s.solve_init()
    assert e.value.code == E_UNSUPPORTED and not s.large
