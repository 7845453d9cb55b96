"""CPU tests of the reference-order mode of the BQP batch (lpbox_bqp_batch_set_order, BqpBatch(order=...)):
the header declares the function and the library exports it, an unknown order is refused in Python before the library is touched, a
null handle is refused -- and the pins the GPU file (tests/test_bqp_batch_ref_order_gpu.py) rests on: the oracle's two orders differ
on its cases where the case module says they do, so a kernel in the wrong association cannot pass there."""
import ctypes
import os
import re

import numpy as np
import pytest

import bqp_ref_cases as K
from helpers import bits_equal, bqp_problem
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_set_order():
    from lpbox_hip import _lib
    txt = open(os.path.join(ROOT, "include", "lpbox_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"int\s+lpbox_bqp_batch_set_order\s*\(\s*lpbox_bqp_batch_t\s*\*h,\s*int mode\s*\)\s*;", txt)
    assert re.search(r"#define\s+LPBOX_ORDER_DEFAULT\s+0\b", txt) and re.search(r"#define\s+LPBOX_ORDER_REFERENCE\s+1\b", txt)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "lpbox_bqp_batch_set_order")
    assert "lpbox_bqp_batch_set_order" in _lib.SYMBOLS


def test_unknown_order_is_refused_before_the_library_is_touched(monkeypatch):
    from lpbox_hip import _lib, bqp

    def touched(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", touched)
    P = bqp_problem(6, 1, 1, seed=1)
    for bad in ("eigen", "Reference", 1, None):
        with pytest.raises(ValueError, match="order"):
            bqp.BqpBatch([P], order=bad)
        with pytest.raises(ValueError, match="order"):
            bqp.solve_many([P], order=bad)
    shell = bqp.BqpBatch.__new__(bqp.BqpBatch)            # no handle, no library: set_order refuses the name first
    with pytest.raises(ValueError, match="order"):
        shell.set_order("eigen")
    assert bqp.ORDERS == {"default": 0, "reference": 1}


def test_null_handle_is_refused():
    from lpbox_hip import _lib
    L = _lib.load()
    assert L.lpbox_bqp_batch_set_order(None, 1) == -1 and b"handle" in L.lpbox_last_error()      # LPBOX_E_BADHANDLE
    assert L.lpbox_bqp_batch_set_order(None, 7) == -1


@pytest.mark.parametrize("n", K.PIN_SIZES)
def test_the_two_orders_differ_where_the_cases_claim_it(n):
    """At most REDUX_K iterations of the size case on the oracle in both orders: x differs in at least one bit at the sizes of ORDERS_DIFFER
    (every size of the GPU file's three batches is in one of the two lists)."""
    assert set(sum(K.REDUX_SIZES.values(), ())) <= set(K.PIN_SIZES)
    i = K.PIN_SIZES.index(n)
    (e, it_e), (g, it_g) = K.eigen("pin", i), K.kernel_order("pin", i)
    assert 0 < it_e <= K.REDUX_K and 0 < it_g <= K.REDUX_K          # (the smallest problems stop before the cap)
    assert np.isfinite(e.vec("x")).all()
    if n in K.ORDERS_DIFFER:
        assert not bits_equal(e.vec("x"), g.vec("x")), f"n = {n}: the two orders give the same x"
    else:
        assert n in K.ORDERS_AGREE


def test_the_two_orders_end_on_different_binary_objectives():
    """bqp_problem(400, 25, 20, seed=1) to 10^4 iterations: the association decides the answer."""
    i = K.SEED1_INDEX
    assert K.STOPPING[i] == (400, 25, 20, 1, None)
    (e, it_e), (g, it_g) = K.eigen("stopping", i), K.kernel_order("stopping", i)
    assert it_e == it_g == 10000
    assert e.scalar("best_bin_obj") == K.SEED1_BEST_BIN_OBJ[O.ORDER_EIGEN]
    assert g.scalar("best_bin_obj") == K.SEED1_BEST_BIN_OBJ[O.ORDER_GPU]
    assert int(((e.vec("x") >= 0.5) != (g.vec("x") >= 0.5)).sum()) == 3


def test_the_stopping_cases_cover_the_three_stops():
    stops = {int(K.eigen("stopping", i)[0].scalar("stop")) for i in range(len(K.STOPPING))}
    assert stops == {0, 1, 2}
