"""The opt-in DIRECT x-update (lpbox_set_x_update) has no reference counterpart: the reference solves its
x-update by Jacobi-PCG to 1e-3 (LPcpp:251-335, :894).  What can be pinned on the CPU: the C oracle's mirror of the kernel arithmetic
(closed-form inverse over the column-disjoint rows + Woodbury over the rest) solves the SAME linear system as a plain dense solve
(oracle/lpbox_numpy.py, written without that algebra), for any admissible row split, and the ADMM around it is unchanged."""
import numpy as np
import pytest

from direct_cases import greedy_split
from helpers import lp_instances
from oracle import oracle as O
from oracle.lpbox_numpy import NumpyLpBox


def direct_oracle(I, rows=None):
    s = O.LpOracle(0, order=O.ORDER_EIGEN, x_update="direct", direct_rows=rows)
    s.set_problem(I["n"], I["l"], I["colptr"], I["rowidx"], I["b"], I.get("f"))
    s.solve_init()
    return s


@pytest.mark.parametrize("name,idx", [("lp_20_60_seed0.npz", 0), ("lp_20_60_seed0.npz", 3), ("lp_100_500_seed0.npz", 1)])
def test_mirror_solves_the_same_system_as_a_dense_solve(name, idx):
    I = lp_instances(name)[idx]
    ref = NumpyLpBox(I["n"], I["l"], I["colptr"], I["rowidx"], I["b"], I.get("f"), x_update="direct")
    ref.solve_init()
    splits = [None, greedy_split(I, True), greedy_split(I, False)]
    assert (splits[1] < 0).any()                      # the auction's XOR rows are found
    orcs = [direct_oracle(I, g) for g in splits]
    for w in range(3):
        ref.solve_iter(w * 20, (w + 1) * 20)
        for o in orcs:
            o.solve_iter(w * 20, (w + 1) * 20)
            assert np.abs(o.vec("x") - ref.x).max() < 1e-9, w
            assert o.total_pcg_iters == 0
    assert orcs[1].total_outer_iters == 60


def test_direct_mode_converges_like_the_pcg_mode_on_the_small_batch():
    """Different x-update, same ADMM: on the 20/60 fixtures both modes stop by a reference stop rule with feasible roundings and
    objectives of the same size (the direct mode is NOT expected to reproduce the PCG iterates)."""
    insts = lp_instances("lp_20_60_seed0.npz")
    obj = {"pcg": [], "direct": []}
    for I in insts:
        for mode in obj:
            s = O.LpOracle(0, order=O.ORDER_EIGEN, x_update=mode, direct_rows=greedy_split(I) if mode == "direct" else None)
            s.set_problem(I["n"], I["l"], I["colptr"], I["rowidx"], I["b"], I.get("f"))
            s.solve_init()
            s.solve_iter(0, 20000)
            assert s.last_stop_reason in (1, 2) and s.check_infeasible_l2f() == 0, mode
            obj[mode].append(-s.cal_Obj())
    p, d = np.array(obj["pcg"]), np.array(obj["direct"])
    assert abs(d.mean() - p.mean()) < 0.05 * abs(p.mean())


def test_fix_rebuilds_the_inverse():
    """After an early fix E loses columns: the mirror rebuilds H and W and still matches the dense solve on the reduced problem."""
    I = lp_instances("lp_100_500_seed0.npz")[2]
    o = direct_oracle(I, greedy_split(I))
    ref = NumpyLpBox(I["n"], I["l"], I["colptr"], I["rowidx"], I["b"], I.get("f"), x_update="direct")
    ref.solve_init()
    z = -np.ones(I["n"])
    assert o.solve_iter_l2f(0, 30, z, 0) == ref.solve_iter_l2f(0, 30, z, 0)
    x = o.vec("x")
    vec = -np.ones(I["n"])
    vec[np.argsort(x)[:40]] = 0.0
    assert o.solve_iter_l2f(30, 60, vec, 40) == ref.solve_iter_l2f(30, 60, vec, 40)
    assert o.get_n() == I["n"] - 40
    assert np.abs(o.vec("x") - ref.x).max() < 1e-9


def test_plain_schedule_keeps_c_far_below_the_rebuild_threshold():
    """The direct mode rebuilds its inverse when c = dI / r4Et moved by more than 1e-9 relative at a rho update (kernel and mirror).  The
    schedule's own scalar arithmetic (LPcpp:851-866, :951-970: dI += rcr (prev_rho1 + prev_rho2), r4Et = learning_fact r4Et) moves c by
    rounding only: over 800 updates (20 000 iterations) never by more than a few ulp per update and 1e-13 in all, so runs without a
    fix at a pending update never rebuild and keep their bits.  After such a fix (the double count) the first update moves c by 1e-4."""
    lf = 1 + 1.0 / 100
    rcr = lf - 1.0

    def run(dI, r4Et, rho, updates):
        worst, c0 = 0.0, dI / r4Et
        for _ in range(updates):
            prev, rho = rho, lf * rho
            before = dI / r4Et
            dI += rcr * (prev + prev)
            r4Et = lf * r4Et
            worst = max(worst, abs(dI / r4Et - before) / before)
        return worst, abs(dI / r4Et - c0) / c0
    step, total = run(0.0 + (25.0 + 25.0), 25.0, 25.0, 800)
    print(step, total)
    assert step < 1e-14 and total < 1e-13
    # a fix while the update after iteration 24 is pending: update_expression's fresh values, then the pending increment on top
    rho, prev = lf * 25.0, 25.0
    dI, r4Et = (0.0 + (rho + rho)) + rcr * (prev + prev), lf * rho
    step, _ = run(dI, r4Et, rho, 1)
    assert 5e-5 < step < 5e-4

    # the oracle's mirror follows the rule: a plain 20 000-iteration solve in direct mode never rebuilds, i.e. equals the parent's bits
    # is pinned by the objective-study fixture; here: c as the mirror reports it stays 2 to rounding over the first 4 updates
    I = lp_instances("lp_20_60_seed0.npz")[0]
    o = direct_oracle(I)
    o.solve_iter(0, 101)
    assert abs(o.scalar("dI") / o.scalar("rho4Et") - 2.0) < 1e-14
