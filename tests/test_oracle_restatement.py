"""CPU tests: the C oracles of the generic BQP (oracle/bqp_oracle.c) and of the segmentation loops (oracle/seg_oracle.c) against the
independent numpy restatement oracle/bqp_numpy.py, written from the reference source alone.

Tolerance rule (NOT the LP path's: along an LP trajectory the two oracle orders agree by luck at iteration 0 and B collapses, so the LP
path is held step by step to a bound from the restatement's own rounding spread, tests/lp_steplock.py): over the prefix of outer iterations where the PCG iteration counts of
both oracle orders and of the restatement agree, every compared vector and scalar is within B of the restatement, B = 10 x the
oracle's own Eigen-order vs GPU-order spread at that point plus 1e-12 max(1, |v|).  Each prefix must hold a rho / gamma update that
has reached the matrix, the y3 / z3 / z4 updates of its type and a std_obj evaluation."""
import os

import numpy as np
import pytest

from helpers import (BQP_SCALARS, BQP_VECS, GOLDEN, assert_within_bound, bqp_params, bqp_problem, common_prefix, scripted_fix_vec,
                     synthetic_seg_problem)
from oracle import oracle as O
from oracle.bqp_numpy import NumpyBqp, NumpySeg

SEG_SCALARS = ("rho1", "gamma", "std_obj", "cvg1", "cvg2", "obj_val", "best_bin_obj", "cur_obj")


def bqp_oracles(P, params, T=256, chunk=512):
    e = O.BqpOracle(P, params=params)
    g = O.BqpOracle(P, params=params, order=O.ORDER_GPU, T=T, chunk=chunk)
    return e, g, e.solve(), g.solve()


def restated_prefix(P, params, T=256, chunk=512):
    """(restatement run with snapshots, length of the prefix on which all three PCG traces agree)."""
    r = NumpyBqp(P, params=params)
    r.solve(record=True)
    e, g, _, _ = bqp_oracles(P, params, T, chunk)
    return r, common_prefix(e.pcg_trace(), g.pcg_trace(), r.pcg)


def check_bqp_state(got, snap, e, g, tag):
    """got: an object with vec() / scalar() (oracle or HIP) after k iterations; snap: the restatement after k; e, g: the oracle in
    both orders after k (the spread)."""
    for name in BQP_VECS:
        if name in snap:
            assert_within_bound(got.vec(name), snap[name], e.vec(name), g.vec(name), f"{tag} {name}")
    for name in BQP_SCALARS:
        assert_within_bound(got.scalar(name), snap[name], e.scalar(name), g.scalar(name), f"{tag} {name}")


def assert_prefix_matters(P, params, prefix):
    step, hist = int(params[4]), int(params[7])
    assert prefix >= step + 1, f"prefix {prefix}: no rho / gamma update reached the matrix (rho_change_step {step})"
    assert prefix >= hist, f"prefix {prefix}: no std_obj evaluation (history_size {hist})"


def compare_bqp_prefix(P, params, ks=None):
    r, prefix = restated_prefix(P, params)
    assert_prefix_matters(P, params, prefix)
    for k in (ks or range(1, prefix + 1)):
        if k > prefix:
            continue
        prm = list(params)
        prm[5] = k
        e, g, ie, ig = bqp_oracles(P, prm)
        assert ie == ig == k
        for o, tag in ((e, "eigen"), (g, "gpu")):
            check_bqp_state(o, r.trace[k - 1], e, g, f"{tag} k={k}")
    return r, prefix


# one problem of each type; the parameters are the type's own preset with the rho schedule shortened to 3 so that K = 8 holds an update
BQP_CASES = {
    "unconstrained": dict(n=300, m=0, l=0, seed=11),
    "equality": dict(n=300, m=30, l=0, seed=12),
    "inequality": dict(n=300, m=0, l=40, seed=13),
    "both": dict(n=300, m=20, l=30, seed=14),
}


@pytest.mark.parametrize("kind", list(BQP_CASES))
def test_bqp_oracle_both_orders_within_bound_of_restatement(kind):
    c = BQP_CASES[kind]
    P = bqp_problem(c["n"], c["m"], c["l"], c["seed"])
    ptype = (1 if c["m"] else 0) | (2 if c["l"] else 0)
    r, prefix = compare_bqp_prefix(P, bqp_params(ptype, 8))
    assert prefix == 8
    if ptype & 2:
        assert np.abs(r.trace[-1]["z4"]).max() > 0 and np.any(r.trace[-1]["y3"] > 0)
    if ptype & 1:
        assert np.abs(r.trace[-1]["z3"]).max() > 0
    # the rho schedule of the type (SolverInstruction, SEGcpp:1845-2046): rho3 moves only when both kinds of constraint are present
    t = r.trace[-1]
    assert t["rho1"] > r.trace[0]["rho1"] and t["gamma"] < r.trace[0]["gamma"] or ptype == 0
    assert (t["rho3"] != r.initial_rho) == (ptype == 3)
    assert (t["rho4"] != r.initial_rho) == bool(ptype & 2)


def test_bqp_presets_and_schedule_from_the_reference():
    """The four *_init presets (SEGcpp:587-672) each run K iterations on a problem of their type, with their own rho_change_step."""
    for ptype, (m, l) in enumerate(((0, 0), (25, 0), (0, 25), (15, 20))):
        P = bqp_problem(120, m, l, 30 + ptype)
        params = bqp_params(ptype, 7, rho_change_step=5)
        compare_bqp_prefix(P, params, ks=(1, 5, 6, 7))


def test_bqp_equality_type_keeps_rho3():
    """ADMM_bqp_linear_eq sets update_rho3 = 0 (SEGcpp:1903-1906): rho3 stays initial_rho, rho3 C' keeps its first scale and the
    preconditioner gets no Csq increment, while rho1 / rho2 grow.  (The oracle and the kernels used to scale rho3 as well.)"""
    P = bqp_problem(200, 20, 0, 40)
    params = bqp_params(1, 9, rho_change_step=2)
    e, g, _, _ = bqp_oracles(P, params)
    r = NumpyBqp(P, params=params)
    r.solve()
    assert e.scalar("rho3") == g.scalar("rho3") == r.state["rho3"] == params[6]
    assert e.scalar("rho1") == r.state["rho1"] > params[6]
    compare_bqp_prefix(P, params, ks=(9,))


def test_bqp_edge_shapes_against_restatement():
    """Small and awkward sizes: n below a wave, m = l = 1, more inequality rows than variables, A diagonal-only."""
    for n, m, l, offdiag in ((2, 1, 1, True), (3, 1, 0, True), (5, 0, 1, True), (40, 0, 60, True), (64, 8, 8, False)):
        P = bqp_problem(n, m, l, 50 + n, offdiag=offdiag)
        ptype = (1 if m else 0) | (2 if l else 0)
        params = bqp_params(ptype, 6)
        r, prefix = restated_prefix(P, params)
        k = min(prefix, 6)
        assert k >= 4, (n, m, l, r.pcg)
        prm = list(params)
        prm[5] = k
        e, g, _, _ = bqp_oracles(P, prm)
        check_bqp_state(e, r.trace[k - 1], e, g, f"n={n} m={m} l={l}")


def test_bqp_indefinite_operator_first_iterations():
    """2A + (rho1 + rho2) I indefinite at the starting rho: Eigen's CG (SEGcpp:415-485) has no curvature test and walks on."""
    P = bqp_problem(150, 15, 0, 60, indefinite=True)
    params = bqp_params(1, 3)
    r = NumpyBqp(P, params=params)
    r.solve(record=True)
    assert r.min_curvature[0] < 0
    assert all(np.isfinite(s["x"]).all() for s in r.trace)
    e, g, _, _ = bqp_oracles(P, params)
    prefix = common_prefix(e.pcg_trace(), g.pcg_trace(), r.pcg)
    assert prefix >= 2
    prm = list(params)
    prm[5] = prefix
    e, g, _, _ = bqp_oracles(P, prm)
    check_bqp_state(e, r.trace[prefix - 1], e, g, "indefinite")


# ---- segmentation -------------------------------------------------------------------------------------------------------
def seg_problem(name="7.jpg", nodes=2500):
    from lpbox_hip.seg import load_gray
    g = load_gray(os.path.join(GOLDEN, "seg", name))
    return O.seg_build_costs(O.seg_resize_u8(g, np.sqrt(nodes / g.size)).astype(float))


def seg_trio(P):
    e = O.SegOracle(0, P["n"], 0); e.set_problem(P); e.solve_init()
    g = O.SegOracle(0, P["n"], 0, order=O.ORDER_GPU); g.set_problem(P); g.solve_init()
    r = NumpySeg(P); r.solve_init()
    return e, g, r


def check_seg_window(e, g, r, tag, x_iters=True):
    if x_iters:
        xe, xg, xr = e.get_x_iters_2d(10), g.get_x_iters_2d(10), r.get_x_iters_2d(10)
        for c in range(xe.shape[1]):
            assert_within_bound(xe[:, c], xr[:, c], xe[:, c], xg[:, c], f"{tag} x_iters[{c}]")
            assert_within_bound(xg[:, c], xr[:, c], xe[:, c], xg[:, c], f"{tag} x_iters[{c}] gpu")
    assert np.array_equal(e.vec("left_idx").astype(int), r.left_idx)
    for name in ("x", "z1", "z2", "b"):
        assert_within_bound(e.vec(name), getattr(r, name), e.vec(name), g.vec(name), f"{tag} {name}")
    for name in SEG_SCALARS:
        assert_within_bound(e.scalar(name), getattr(r, "std" if name == "std_obj" else name), e.scalar(name), g.scalar(name), f"{tag} {name}")


def test_seg_legacy_loop_matches_restatement_to_convergence():
    """ADMM_bqp_unconstrained_legacy (SEGcpp:1200-1380) on a small synthetic image: the PCG traces agree all the way, so the energy,
    stop reason, iteration count, labelling and final state must too."""
    P = synthetic_seg_problem(3)
    e, g, r = seg_trio(P)
    en, gn, rn = e.solve_iter(), g.solve_iter(), r.solve_iter()
    assert np.array_equal(e.pcg_trace(), r.pcg) and np.array_equal(g.pcg_trace(), r.pcg) and len(r.pcg) > 300
    assert en == gn == rn and e.legacy_iter_plus1 == r.legacy_iter_plus1 and e.last_stop == r.last_stop
    assert np.array_equal(e.get_x_sol().ravel(), r.get_x_sol())
    check_seg_window(e, g, r, "legacy", x_iters=False)


def test_seg_l2f_windows_without_fixes():
    P = seg_problem("7.jpg", 2500)
    e, g, r = seg_trio(P)
    z = np.zeros(P["n"])
    for w in range(3):
        assert e.solve_iter_l2f(10 * w, 10 * w + 10, z, 0) == g.solve_iter_l2f(10 * w, 10 * w + 10, z, 0) \
            == r.solve_iter_l2f(10 * w, 10 * w + 10, z, 0) == 0
        assert common_prefix(e.pcg_trace(), g.pcg_trace(), r.pcg[-10:]) == 10        # the oracle's trace is per call
        check_seg_window(e, g, r, f"window {w}")
    # the legacy loop is the l2f loop without fixes: the restatement's own two loops agree over the same iterations
    q = NumpySeg(P); q.solve_init(); q.max_iters = 30
    q.solve_iter()
    assert np.array_equal(q.x, r.x) and q.pcg == r.pcg


def test_seg_window_after_a_scripted_fix():
    """The fix step of SEGcpp:927-1058: A compacted onto the live variables, b = 2 Mb x2 + b1, temp_mat rebuilt at the current rho."""
    P = seg_problem("7.jpg", 2500)
    e, g, r = seg_trio(P)
    vec, num, fixed = np.zeros(P["n"]), 0, 0
    for w in range(3):
        rets = {e.solve_iter_l2f(10 * w, 10 * w + 10, vec, num), g.solve_iter_l2f(10 * w, 10 * w + 10, vec, num),
                r.solve_iter_l2f(10 * w, 10 * w + 10, vec, num)}
        assert rets == {0}
        assert common_prefix(e.pcg_trace(), g.pcg_trace(), r.pcg[-10:]) == 10
        check_seg_window(e, g, r, f"window {w} (fixed before it: {num})")
        fixed += num
        vec, num = scripted_fix_vec(e.get_x_iters_2d(10), lo=0.05, hi=0.95, last=5)
    assert fixed > 500 and r.n == P["n"] - fixed
    b0 = np.asarray(P["b"], float)
    assert not np.array_equal(r.b, b0[r.left_idx])           # the shift moved b
