"""The direct x-update on odd structures and at its limits, the half that needs no GPU (cases:
tests/direct_cases.py).  The host's row split is compared, element for element, with its restatement (greedy_split), and the C oracle's
mirror of the kernel arithmetic with NumpyLpBox(x_update="direct"), whose x-update is numpy.linalg.solve on the same system: windows
[0, 50) and [50, 100) with a fix at 50, where a rho update is pending, so that c = dI / r4Et moves at iteration 75 and the mirror rebuilds
its inverse inside the window.  The bar is the 1e-9 of tests/test_direct_x_update.py.  GPU half: tests/test_lp_direct_edges_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import direct_cases as D
from lpbox_hip.lp import LpBatch
from oracle import oracle as O
from oracle.lpbox_numpy import NumpyLpBox

BAR = 1e-9


def base_of(I):
    b = LpBatch([I])
    try:
        return b.config()["lds_bytes"]                # answered by the host planner: no device
    finally:
        b.close()


def library_split(I):
    """(|G| as lpbox_get_direct_rows returns it, the dense index per row) -- no device, no mode."""
    b = LpBatch([I])
    try:
        out = np.zeros(I["l"], np.int32)
        ng = b._L.lpbox_get_direct_rows(b._h, 0, out.ctypes.data_as(C.c_void_p))
        assert np.array_equal(out, b.direct_rows(0))
        return ng, out
    finally:
        b.close()


@pytest.fixture(scope="module")
def lds_pair():
    return D.lds_pair(base_of)


@pytest.fixture(scope="module")
def random_cases():
    return D.random_cases()


def _check_split(I, expect=None):
    ng, g = library_split(I)
    want = D.greedy_split(I)
    assert np.array_equal(g, want), "row split differs from the restated greedy rule at rows %s" % np.nonzero(g != want)[0][:8]
    assert ng == int((want >= 0).sum()) and (expect is None or ng == expect)
    hit = np.zeros(I["n"], int)                       # the D rows are column-disjoint
    for cols, gi in zip(D.rows_of(I), g):
        if gi < 0:
            hit[cols] += 1
    assert hit.max(initial=0) <= 1
    return ng


@pytest.mark.parametrize("name", list(D.FITTING) + list(D.REFUSED))
def test_row_split_is_the_restated_greedy_rule(name):
    _check_split(D.case(name), (D.FITTING.get(name) or D.REFUSED[name])[1])


def test_row_split_of_the_lds_pair_and_the_random_cases(lds_pair, random_cases):
    for I in lds_pair:
        assert _check_split(I) == D.MAX_G
    sizes = {_check_split(I) for I, _ in random_cases}
    assert 0 in sizes and max(sizes) > D.MAX_G        # the draw holds both ends


def test_lds_pair_straddles_the_limit_by_one_step(lds_pair):
    fit, over = lds_pair
    need = [D.direct_need(base_of(I), D.MAX_G) for I in (fit, over)]
    print("lds_fit: nnz %d need %d B; lds_over: nnz %d need %d B" % (len(fit["rowidx"]), need[0], len(over["rowidx"]), need[1]))
    assert need[0] <= D.LDS_LIMIT < need[1]
    assert need[1] - need[0] == 32                    # one step of the two index pools (eight uint16 entries each)
    assert D.refusal([fit], base_of(fit)) is None and D.refusal([over], base_of(over)) == "%d B of LDS" % need[1]


def test_restated_limits_on_the_named_cases():
    for name in D.FITTING:
        assert D.refusal([D.case(name)], base_of(D.case(name))) is None, name
    mixed = [D.case(name) for name in D.MIXED]
    b = LpBatch(mixed)
    assert D.refusal(mixed, b.config()["lds_bytes"]) is None        # HL = 128 with the batch's own l and index pools
    b.close()
    assert D.refusal([D.case("g_129")], base_of(D.case("g_129"))) == "129 rows of E share columns"
    assert D.refusal([D.case("n_513")], base_of(D.case("n_513"))) == "n <= 512"


def mirror_vs_dense(I):
    """Worst |x_mirror - x_dense| after the two windows, over the mirror in Eigen order with the library's split and with the descending
    split."""
    ref = NumpyLpBox(I["n"], I["l"], I["colptr"], I["rowidx"], I["b"], I.get("f"), x_update="direct")
    ref.solve_init()
    orcs = []
    for g in (library_split(I)[1], D.greedy_split(I, False)):
        o = O.LpOracle(0, order=O.ORDER_EIGEN, x_update="direct", direct_rows=g)
        o.set_problem(I["n"], I["l"], I["colptr"], I["rowidx"], I["b"], I.get("f"))
        o.solve_init()
        orcs.append(o)
    worst = [0.0, 0.0]
    vec, num = -np.ones(I["n"]), 0
    for w, (a, e) in enumerate(((0, 50), (50, 100))):
        rr = ref.solve_iter_l2f(a, e, vec, num)
        for o in orcs:
            assert o.solve_iter_l2f(a, e, vec, num) == rr and o.get_n() == ref.n, (w, rr)
            if ref.n:
                worst[w] = max(worst[w], np.abs(o.vec("x") - ref.x).max())
            assert o.total_pcg_iters == 0
        assert worst[w] < BAR, (w, worst)
        if rr:
            break
        vec, num = D.fix_with_kill(I, ref.x)
        if "kill" in I:
            assert num >= len(I["kill"]) and np.all(vec[I["kill"]] == 0.0)
    return worst


@pytest.mark.parametrize("name", list(D.FITTING))
def test_mirror_solves_the_dense_system_on_the_named_cases(name):
    worst = mirror_vs_dense(D.case(name))
    assert worst[1] > 0.0 or D.case(name)["n"] <= 5   # the window after the fix ran
    print("%s: worst |x_mirror - x_dense| %.2e before the fix, %.2e after it" % (name, worst[0], worst[1]))


def test_mirror_solves_the_dense_system_on_the_lds_pair_and_the_random_cases(lds_pair, random_cases):
    """lds_over is refused by the kernel, not by the mirror: its math is checked all the same; the random cases that the restated rule
    refuses are left out (up to 460 dense rows)."""
    worst = np.zeros(2)
    ran = 0
    for I in list(lds_pair) + [I for I, _ in random_cases if D.refusal([I], base_of(I)) is None]:
        worst = np.maximum(worst, mirror_vs_dense(I))
        ran += 1
    print("lds pair and %d random cases: worst |x_mirror - x_dense| %.2e before the fix, %.2e after it" % (ran - 2, worst[0], worst[1]))
    assert ran - 2 >= 18
