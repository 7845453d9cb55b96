"""CPU tests of the oracle (the checker): pinned against the reference's own importable pieces, an independent numpy
restatement, analytic known answers and an exact MILP bound.  The reference ships no golden vectors for the solver
itself, so with respect to the reference BINARY parity stays unpinned -- see DESIGN.md."""
import os

import numpy as np
import pytest

import lp_steplock as S
from helpers import GOLDEN, lp_instances, make_oracle, scripted_fix_vec
from oracle import oracle as O
from oracle.lpbox_numpy import NumpyLpBox


def test_sphere_projection_matches_reference_golden():
    """Golden vector produced by the reference's SA/utils.py:8-16 (tests/golden/make_sphere_fixture.py)."""
    d = np.load(os.path.join(GOLDEN, "sphere_proj_reference.npz"))
    for n in (5, 60, 500, 2000):
        y = O.project_shifted_lp_ball(d[f"x{n}"])
        np.testing.assert_allclose(y, d[f"y{n}"], rtol=0, atol=4e-16 * np.sqrt(n))
        # analytic properties: on the sphere of radius sqrt(n)/2 around 1/2, same direction as x - 1/2
        assert abs(np.linalg.norm(y - 0.5) - np.sqrt(n) / 2) < 1e-12 * np.sqrt(n)
        t = d[f"x{n}"] - 0.5
        assert np.allclose((y - 0.5) / np.linalg.norm(y - 0.5), t / np.linalg.norm(t), atol=1e-14)


def test_box_projection_known_answers():
    x = np.array([-1.0, -0.0, 0.0, 0.25, 1.0, 1.0 + 1e-16, 7.0, np.nan])
    y = O.project_box(x)
    assert np.array_equal(y[:7], np.array([0.0, -0.0, 0.0, 0.25, 1.0, 1.0, 1.0]))
    assert np.isnan(y[7])                      # LPcpp:409-421: NaN falls through both comparisons
    assert np.array_equal(O.project_box(y[:7]), y[:7])   # idempotent


def test_file_reader_equals_fixture_arrays():
    """readFile restatement (LPcpp:2407-2545) on the generator's own text files vs the same instances in the npz."""
    insts = lp_instances("lp_100_500_seed0.npz")
    for k in (1, 2):
        s = O.LpOracle(0)
        s.read_files(os.path.join(GOLDEN, "instance", "100_500", f"instance_{k}_C.txt"),
                     os.path.join(GOLDEN, "instance", "100_500", f"instance_{k}_b.txt"), 100)
        s.solve_init()
        I = insts[k - 1]
        assert s.get_n() == I["n"] and len(s.vec("f")) == I["l"]
        assert np.array_equal(s.vec("b"), I["b"])          # b = -price (LPcpp:2520)
        assert np.all(s.vec("f") == 1.0)                   # LPcpp:2522
        t = make_oracle(I)
        s.solve_iter(0, 50)
        t.solve_iter(0, 50)
        assert np.array_equal(s.vec("x"), t.vec("x"))


def test_oracle_regression_seed0_instance1():
    """Config 1 of BASELINE.json (./test 1 100 500): full solve by the oracle in Eigen reduction order.  The numbers pin the
    oracle against accidental change (they are the oracle's own, not reference outputs)."""
    I = lp_instances("lp_100_500_seed0.npz")[0]
    s = make_oracle(I)
    ret = s.solve_iter(0, 20000)
    assert (ret, s.last_stop_reason, s.last_plain_iter_plus1) == (0, 1, 8175)
    assert s.total_pcg_iters == 119531 or abs(s.total_pcg_iters / s.total_outer_iters - 14.62) < 0.01
    assert abs(-s.cal_Obj() - 6749.027316656483) < 1e-9
    assert s.check_infeasible_l2f() == 0 and s.check_infeasible_lpbox() == 0
    x = s.get_x_sol().ravel()
    assert set(np.unique(x)) <= {0.0, 1.0}
    assert abs(I["b"] @ x - s.cal_Obj()) < 1e-9


def test_objective_bounded_by_exact_milp():
    from scipy.optimize import Bounds, LinearConstraint, milp
    import scipy.sparse as sp
    I = lp_instances("lp_20_60_seed0.npz")[0]
    E = sp.csc_matrix((np.ones(len(I["rowidx"])), I["rowidx"], I["colptr"]), shape=(I["l"], I["n"]))
    res = milp(I["b"], constraints=LinearConstraint(E, -np.inf, np.ones(I["l"])), integrality=np.ones(I["n"]),
               bounds=Bounds(0, 1))
    s = make_oracle(I)
    s.solve_iter(0, 20000)
    assert s.check_infeasible_l2f() == 0
    assert s.cal_Obj() >= res.fun - 1e-9          # minimisation: ADMM's feasible point cannot beat the optimum
    assert s.cal_Obj() <= 0.8 * res.fun           # and is a decent heuristic (within 20 % on this instance)


@pytest.mark.parametrize("idx", [0, 3])
def test_c_oracle_agrees_with_numpy_restatement(idx):
    """Two independent restatements of LPcpp agree to rounding while their PCG iteration counts agree (afterwards the
    1e-3 PCG exit threshold amplifies rounding differences: the algorithm is chaotic)."""
    I = lp_instances("lp_100_500_seed0.npz")[idx]
    c = make_oracle(I)
    p = NumpyLpBox(I["n"], I["l"], I["colptr"], I["rowidx"], I["b"])
    p.solve_init()
    vec = np.zeros(I["n"])
    c.solve_iter_l2f(0, 40, vec, 0)
    p.solve_iter_l2f(0, 40, vec, 0)
    xc, xp = c.get_x_iters_2d(40), p.x_iters[:, :40]
    kc, kp = c.pcg_trace(), np.array(p.pcg_trace)
    same = int(np.argmax(kc[:40] != kp[:40])) if np.any(kc[:40] != kp[:40]) else 40
    assert same >= 4, "PCG iteration counts diverge immediately"
    for it in range(same):
        assert np.abs(xc[:, it] - xp[:, it]).max() < 5e-5 * max(1.0, np.abs(xc[:, it]).max()), it
    assert np.abs(xc[:, 0] - xp[:, 0]).max() < 1e-7
    # beyond the first flipped PCG exit the two trajectories stay within the inexact-solve tolerance for a while
    assert np.abs(xc[:, same:same + 5] - xp[:, same:same + 5]).max() < 5e-2


def test_tiny_instances_inexact_solve_tolerance():
    """On 60-variable instances the PCG residual hovers at its 1e-3 exit threshold, so even the first outer iteration may
    take a different number of PCG steps under a different summation order; iterates then agree to the PCG tolerance."""
    for idx in range(4):
        I = lp_instances("lp_20_60_seed0.npz")[idx]
        c = make_oracle(I)
        p = NumpyLpBox(I["n"], I["l"], I["colptr"], I["rowidx"], I["b"])
        p.solve_init()
        vec = np.zeros(I["n"])
        c.solve_iter_l2f(0, 3, vec, 0)
        p.solve_iter_l2f(0, 3, vec, 0)
        assert np.abs(c.pcg_trace()[:3] - np.array(p.pcg_trace[:3])).max() <= 3
        assert np.abs(c.get_x_iters_2d(3) - p.x_iters[:, :3]).max() < 5e-2


def test_gpu_order_close_to_eigen_order_early():
    I = lp_instances("lp_100_500_seed0.npz")[0]
    a = make_oracle(I, O.ORDER_EIGEN)
    g = make_oracle(I, O.ORDER_GPU, 512)
    vec = np.zeros(I["n"])
    a.solve_iter_l2f(0, 6, vec, 0)
    g.solve_iter_l2f(0, 6, vec, 0)
    assert np.array_equal(a.pcg_trace(), g.pcg_trace())
    d = np.abs(a.get_x_iters_2d(6) - g.get_x_iters_2d(6)).max(axis=0)
    assert d[0] < 1e-7 and d.max() < 5e-5        # rounding-level at first, growing like the PCG's error amplification


def test_early_fix_bookkeeping_c_vs_numpy():
    """Fix block LPcpp:1124-1335: same index bookkeeping, fixed objective and shrunken problem in both restatements."""
    I = lp_instances("lp_100_500_seed0.npz")[2]
    c = make_oracle(I)
    p = NumpyLpBox(I["n"], I["l"], I["colptr"], I["rowidx"], I["b"])
    p.solve_init()
    vec, num = np.zeros(I["n"]), 0
    for w in range(12):
        rc = c.solve_iter_l2f(w * 100, (w + 1) * 100, vec, num)
        xit = c.get_x_iters_2d(100)
        vec, num = scripted_fix_vec(xit)
        if num > 10:
            break
        num = 0
        assert rc == 0
    assert num > 10, "scripted policy did not fire"
    # replay: both restatements from scratch with the same (window, vec, num) script
    c2 = make_oracle(I)
    z = np.zeros(I["n"])
    for ww in range(w + 1):
        c2.solve_iter_l2f(ww * 100, (ww + 1) * 100, z, 0)
        p.solve_iter_l2f(ww * 100, (ww + 1) * 100, z, 0)
    n_before = c2.get_n()
    c2.solve_iter_l2f((w + 1) * 100, (w + 1) * 100 + 1, vec, num)
    p.solve_iter_l2f((w + 1) * 100, (w + 1) * 100 + 1, vec, num)
    assert c2.get_n() == p.n == n_before - num
    assert np.array_equal(c2.vec("left_idx").astype(int), p.left_idx)
    assert abs(c2.scalar("sum_fix_obj") - p.sum_fix_obj) < 1e-9 * max(1.0, abs(p.sum_fix_obj))
    assert c2.get_x_iters_2d(1).shape == (n_before - num, 1)
    # Q1: the pending rho update is applied on top of update_expression's fresh values (LPcpp:1329 then :1392-1405)
    rho1 = c2.scalar("rho1")
    assert abs(c2.scalar("dI") - (2 * rho1 + (1.01 - 1.0) * 2 * c2.scalar("prev_rho1"))) < 1e-9
    fixed = np.setdiff1d(np.arange(I["n"]), p.left_idx)
    xs = c2.get_x_sol().ravel()
    assert set(np.unique(xs[fixed])) <= {0.0, 1.0}
    # feed numpy the C oracle's state so that chaos cannot separate them: the same script step-locked
    case = steplocked_across_fix(I, fix_it=(w + 1) * 100, vec=vec, num=num)
    assert case.checked == 21 and case.fixed == num and np.array_equal(np.sort(case.members[0].left_idx), p.left_idx)


def steplocked_across_fix(I, fix_it, vec, num, before=20):
    """The oracle driven one iteration at a time up to fix_it, the fix (vec, num) applied there and one iteration run, with the
    restatement step-locked to it (tests/lp_steplock.py).  The last `before` iterations ahead of the fix and the one after it are held
    to the restatement's own rounding spread: the shrunken problem, the pending rho update on top of update_expression's fresh values
    and the iterates after the fix.  (The earlier iterations only carry the restatement's own rho schedule and objective history there;
    tests/test_lp_steplock.py compares them.)"""
    o = make_oracle(I)
    case = S.Case(I, S.OracleSubject(o), "bookkeeping", check_from=fix_it - before)
    S.run_cases(S.OracleGroup([o]), [case], S.l2f_steps(0, fix_it) + S.l2f_steps(fix_it, fix_it + 1, (vec, num)))
    S.assert_clean([case])
    return case


def test_all_fixed_and_bad_vec():
    I = lp_instances("lp_20_60_seed0.npz")[2]
    c = make_oracle(I)
    z = np.zeros(I["n"])
    c.solve_iter_l2f(0, 10, z, 0)
    with pytest.raises(RuntimeError):
        c.solve_iter_l2f(10, 20, -np.ones(I["n"]), 3)          # num does not match vec
    vec = (c.get_x_iters_2d(10)[:, -1] >= 0.5).astype(float)
    ret = c.solve_iter_l2f(10, 20, vec, I["n"])                # fix everything (LPcpp:1212-1217)
    assert ret == 1 and c.get_n() == 0 and c.last_stop_reason == 4
    assert np.array_equal(c.get_x_sol().ravel(), vec)
    assert c.cal_Obj() == 0.0                                  # reference quirk: sum_fix_obj is not updated on the all-fixed path


def test_summation_order_changes_trajectories_not_solution_quality():
    """What "parity with the reference's final x and objective" can mean for this algorithm: the iteration is
    chaotic in rounding, so the Eigen summation order and the kernels' order end on DIFFERENT binary points (a few % of the bits, up to
    ~15 % objective on single instances) -- but of the same quality: both feasible, mean objective within 4 % over 8 instances
    (the spread of the per-instance differences is ~5 %, i.e. ~2 % on a mean of 8)."""
    from helpers import make_oracle
    insts = lp_instances("lp_100_500_seed0.npz")[:8]
    objs, bits = [], []
    for I in insts:
        a = make_oracle(I, O.ORDER_EIGEN)
        a.solve_iter(0, 20000)
        b = make_oracle(I, O.ORDER_GPU, 512)
        b.solve_iter(0, 20000)
        assert a.check_infeasible_l2f() == 0 and b.check_infeasible_l2f() == 0
        objs.append((-a.cal_Obj(), -b.cal_Obj()))
        bits.append(float(np.mean(a.get_x_sol() != b.get_x_sol())))
    objs = np.array(objs)
    assert 0 < np.mean(bits) < 0.15                                   # different end points ...
    assert abs(objs[:, 1].mean() - objs[:, 0].mean()) < 0.04 * objs[:, 0].mean()    # ... of the same quality


def test_instance_file_writer_roundtrip(tmp_path):
    """lpbox_hip.synth.write_instance_files reproduces the reference generator's files byte for byte (the committed fixture) and the
    oracle's reader (LPcpp:2407-2545) reads them back to the same problem."""
    import filecmp
    from lpbox_hip.synth import write_instance_files
    I = lp_instances("lp_100_500_seed0.npz")[0]
    pc, pb = str(tmp_path / "instance_1_C.txt"), str(tmp_path / "instance_1_b.txt")
    write_instance_files(I, pc, pb)
    assert filecmp.cmp(pc, os.path.join(GOLDEN, "instance/100_500/instance_1_C.txt"), shallow=False)
    assert filecmp.cmp(pb, os.path.join(GOLDEN, "instance/100_500/instance_1_b.txt"), shallow=False)
    o = O.LpOracle(0)
    o.read_files(pc, pb, 100)
    o.solve_init()
    assert o.get_n() == I["n"] and np.array_equal(o.vec("b"), I["b"])


def test_oracle_pool_worker_under_spawn():
    """The -m gpu parity test of every benchmark instance runs its oracle solves in a SPAWNED pool (a process that has initialised the GPU
    must not fork): the worker has to be importable and picklable from a fresh interpreter, and equal an in-process solve."""
    import multiprocessing
    from concurrent.futures import ProcessPoolExecutor
    from helpers import oracle_full_solve
    insts = lp_instances("lp_20_60_seed0.npz")[:3]
    jobs = [(I, 512, 512, None, None, None) for I in insts]
    with ProcessPoolExecutor(2, mp_context=multiprocessing.get_context("spawn")) as ex:
        res = list(ex.map(oracle_full_solve, jobs, chunksize=2))
    for job, r in zip(jobs, res):
        here = oracle_full_solve(job)
        assert r[:4] == here[:4] and np.array_equal(r[4], here[4]) and np.array_equal(r[5], here[5])


def test_pcg_lean_mirror_is_the_same_algebra_with_another_rounding():
    """lpo_set_pcg_lean (mirror of the large-instance kernels' opt-in comm-lean PCG): p.Mp = dI (p.p) + r4Et (q.q) is the reference's
    p.(M p) in exact arithmetic -- the first iterates agree to rounding and the PCG counts are the same; further on it is a different
    trajectory of the same heuristic (different bits), and the grouping of the q.q partials matters to the last bit only."""
    I = lp_instances("lp_100_500_seed0.npz")[0]
    ref = make_oracle(I, O.ORDER_GPU, 256)
    lean = O.LpOracle(0, order=O.ORDER_GPU, T=256)
    lean.set_pcg_lean(True, 512)
    lean.set_problem(I["n"], I["l"], I["colptr"], I["rowidx"], I["b"])
    lean.solve_init()
    other = O.LpOracle(0, order=O.ORDER_GPU, T=256)
    other.set_pcg_lean(True, 64)
    other.set_problem(I["n"], I["l"], I["colptr"], I["rowidx"], I["b"])
    other.solve_init()
    for o in (ref, lean, other):
        o.solve_iter(0, 1)
    d1 = np.abs(ref.vec("x") - lean.vec("x")).max()
    assert 0 < d1 < 1e-7, d1                                  # rounding of alpha only
    for o in (ref, lean, other):
        o.solve_iter(1, 6)
    assert np.array_equal(ref.pcg_trace(), lean.pcg_trace())
    assert np.abs(ref.vec("x") - lean.vec("x")).max() < 5e-4  # ... amplified like any other rounding difference (cf. the summation-order test above)
    assert np.abs(other.vec("x") - lean.vec("x")).max() < 5e-4
    for o in (ref, lean):
        o.solve_iter(6, 20000)
    for o in (ref, lean):
        x = o.vec("x")
        assert np.all((x == 0) | (x == 1))
