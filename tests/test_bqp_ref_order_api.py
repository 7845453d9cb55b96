"""CPU tests of the reference-order mode of the one-problem BQP chain (lpbox_bqp_set_order, BqpSolver(order=...); DESIGN.md section
14.3): the header declares the function and the library exports it, an unknown order is refused in Python before the library is
touched, a null handle is refused -- and the pins the GPU file (tests/test_bqp_ref_order_gpu.py) rests on: the oracle's two orders
differ on its cases where the case module says they do, so a chain in the wrong association cannot pass there."""
import ctypes
import os
import re

import numpy as np
import pytest

import bqp_chain_ref_cases as R
from chain_cases import BQP_KMAX_START, PAIRS_PER_RESUME, bqp_case, bqp_case_params
from helpers import bqp_problem
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_set_order():
    from lpbox_hip import _lib
    txt = open(os.path.join(ROOT, "include", "lpbox_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"int\s+lpbox_bqp_set_order\s*\(\s*lpbox_bqp_t\s*\*h,\s*int mode\s*\)\s*;", txt)
    assert re.search(r"#define\s+LPBOX_ORDER_DEFAULT\s+0\b", txt) and re.search(r"#define\s+LPBOX_ORDER_REFERENCE\s+1\b", txt)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "lpbox_bqp_set_order")
    assert "lpbox_bqp_set_order" in _lib.SYMBOLS


def test_unknown_order_is_refused_before_the_library_is_touched(monkeypatch):
    from lpbox_hip import _lib, bqp

    def touched(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", touched)
    P = bqp_problem(6, 1, 1, seed=1)
    for bad in ("eigen", "Reference", 1, None):
        with pytest.raises(ValueError, match="order"):
            bqp.BqpSolver(P["n"], P["A"], P["b"], P["x0"], P["C"], P["d"], P["E"], P["f"], order=bad)
        with pytest.raises(ValueError, match="order"):
            bqp.ADMM_bqp_unconstrained(P["n"], P["A"], P["b"], P["x0"], order=bad)
        with pytest.raises(ValueError, match="order"):
            bqp.ADMM_bqp_linear_eq(P["n"], P["A"], P["b"], P["x0"], 1, P["C"], P["d"], order=bad)
        with pytest.raises(ValueError, match="order"):
            bqp.ADMM_bqp_linear_ineq(P["n"], P["A"], P["b"], P["x0"], 1, P["E"], P["f"], order=bad)
        with pytest.raises(ValueError, match="order"):
            bqp.ADMM_bqp_linear_eq_and_uneq(P["n"], P["A"], P["b"], P["x0"], 1, P["C"], P["d"], 1, P["E"], P["f"], order=bad)
    shell = bqp.BqpSolver.__new__(bqp.BqpSolver)            # no handle, no library: set_order refuses the name first
    with pytest.raises(ValueError, match="order"):
        shell.set_order("eigen")


def test_null_handle_and_unknown_mode_are_refused():
    from lpbox_hip import _lib
    L = _lib.load()
    assert L.lpbox_bqp_set_order(None, 1) == -1 and b"handle" in L.lpbox_last_error()      # LPBOX_E_BADHANDLE
    assert L.lpbox_bqp_set_order(None, 7) == -1
    h = ctypes.c_void_p(L.lpbox_bqp_create(0))              # no device call before a solve
    try:
        assert L.lpbox_bqp_set_order(h, 2) == -2 and L.lpbox_bqp_set_order(h, -1) == -2    # LPBOX_E_BADARG
        assert L.lpbox_bqp_set_order(h, 1) == 0 and L.lpbox_bqp_set_order(h, 1) == 0 and L.lpbox_bqp_set_order(h, 0) == 0
    finally:
        L.lpbox_bqp_destroy(h)


@pytest.mark.parametrize("n", R.SIZES)
def test_the_two_orders_differ_where_the_cases_claim_it(n):
    """60 iterations of the size case on the oracle in both orders: x differs in at least one bit at every size of the GPU file's
    list but those of ORDERS_AGREE."""
    assert set(R.ORDERS_AGREE) <= set(R.SIZES) and {2, 3} <= set(R.ORDERS_AGREE)
    (e, it_e), (g, it_g) = R.size_oracle(n, O.ORDER_EIGEN), R.size_oracle(n, O.ORDER_GPU)
    assert 0 < it_e <= 60 and 0 < it_g <= 60                 # (the smallest problems stop before the cap)
    assert np.isfinite(e.vec("x")).all()
    differing = int((e.vec("x").view(np.uint64) != g.vec("x").view(np.uint64)).sum())
    if n in R.ORDERS_AGREE:
        assert differing == 0
    else:
        assert differing > 0, f"n = {n}: the two orders give the same x"
        if n >= 255:                                         # not a bit here and there: nearly every entry
            assert n - 108 <= differing <= n


def test_the_two_orders_end_on_different_binary_answers_above_the_batch_limit():
    """bqp_problem(2100, 64, 64, seed=1) under preset 3 to the 10^4-iteration cap: the association decides the answer."""
    from lpbox_hip.bqp import BATCH_MAX_DIM
    assert R.BIG[0] > BATCH_MAX_DIM
    (e, it_e), (g, it_g) = R.big_oracle(O.ORDER_EIGEN), R.big_oracle(O.ORDER_GPU)
    assert it_e == it_g == 10000 and e.scalar("stop") == g.scalar("stop") == 0
    assert e.scalar("best_bin_obj") == R.BIG_BEST_BIN_OBJ[O.ORDER_EIGEN]
    assert g.scalar("best_bin_obj") == R.BIG_BEST_BIN_OBJ[O.ORDER_GPU]
    assert e.scalar("total_pcg") == R.BIG_PCG_STEPS[O.ORDER_EIGEN] and g.scalar("total_pcg") == R.BIG_PCG_STEPS[O.ORDER_GPU]
    assert int(((e.vec("best_sol") >= 0.5) != (g.vec("best_sol") >= 0.5)).sum()) == R.BIG_BINARY_DIFFERENCES


def test_the_resume_case_needs_more_pairs_than_the_chain_enqueues():
    """G4 in the reference's order: iteration 0 needs more than the 12 + 16 launch groups of a fresh chain and one resume, and every
    iteration more than one group."""
    P, _ = bqp_case("G4")
    o = O.BqpOracle(P, params=bqp_case_params("G4"), order=O.ORDER_EIGEN)
    assert o.solve() == 30
    trace = [int(k) for k in o.pcg_trace()]
    assert len(trace) == 30 and trace[0] > BQP_KMAX_START + PAIRS_PER_RESUME and min(trace) > 1
