"""GPU tests of the opt-in DIRECT x-update (lpbox_set_x_update).  The mode has no reference counterpart -- the
reference's x-update is Jacobi-PCG to 1e-3 (LPcpp:251-335, :894) and the default mode is held to it bit for bit elsewhere.  Here the
kernel is held, bit for bit, to the C oracle's mirror of the same arithmetic (whose math tests/test_direct_x_update.py pins against a
plain dense solve), and the whole benchmark batch to size-independent properties."""
import numpy as np
import pytest

from helpers import bits_equal, lp_instances, oracle_for, scripted_fix_vec
from lpbox_hip.lp import LpBatch, LpboxError

pytestmark = pytest.mark.gpu


def _pair(insts):
    b = LpBatch(insts)
    b.set_x_update("direct")
    b.solve_init()
    return b, [oracle_for(b, i, I, x_update="direct", direct_rows=b.direct_rows(i)) for i, I in enumerate(insts)]


def _same_state(b, os_, tag):
    for i, o in enumerate(os_):
        left = o.vec("left_idx").astype(int)             # the kernels never compact: fixed variables stay in place, masked
        for name in ("x", "z1", "z2"):               # (once every variable is fixed the oracle keeps its last arrays: none of it is live)
            assert bits_equal(b.debug_vec(name, i)[left], o.vec(name) if len(left) else np.zeros(0)), (tag, i, name)
        assert bits_equal(b.debug_vec("z4", i), o.vec("z4")), (tag, i)
        assert b.counters(i) == (o.total_outer_iters, o.total_pcg_iters) == (o.total_outer_iters, 0), (tag, i)
        for name in ("rho1", "cvg1", "cvg2", "std_obj", "obj_val", "cur_obj", "best_bin_obj"):
            assert b.debug_scalar(name, i) == o.scalar(name), (tag, i, name)


def test_row_split_finds_the_xor_rows():
    insts = lp_instances("lp_100_500_seed0.npz")[:8]
    b = LpBatch(insts)
    b.set_x_update("direct")
    for i, I in enumerate(insts):
        g = b.direct_rows(i)
        dense = int((g >= 0).sum())
        assert 0 < dense <= 128 and (g < 0).sum() >= I["l"] - 128
        assert sorted(g[g >= 0]) == list(range(dense))
        # the closed-form rows really are column-disjoint
        hit = np.zeros(I["n"], int)
        for j in range(I["n"]):
            for e in range(I["colptr"][j], I["colptr"][j + 1]):
                hit[j] += g[I["rowidx"][e]] < 0
        assert hit.max() <= 1


def test_plain_windows_and_full_solve_bit_exact_vs_mirror():
    insts = lp_instances("lp_100_500_seed0.npz")[:3] + lp_instances("lp_20_60_seed0.npz")[:2]
    b, os_ = _pair(insts)
    for (a, e) in ((0, 30), (30, 200), (200, 20000)):
        rets = b.solve_iter(a, e)
        for i, o in enumerate(os_):
            assert rets[i] == o.solve_iter(a, e), (i, a, e)
        _same_state(b, os_, (a, e))
    for i, o in enumerate(os_):
        assert b.stop(i)[0] == o.last_stop_reason and np.array_equal(b.get_x_sol(i), np.ravel(o.get_x_sol()))
        assert b.cal_obj(i) == o.cal_Obj()


def test_l2f_windows_with_fixes_rebuild_the_inverse():
    """The early-fixing loop (LP/trainer.py:216-252 shape) on the direct mode: every fix removes columns of E, the kernel rebuilds its
    inverse inside the next window and stays bit-identical to the mirror; windows without a fix reload the saved inverse.  The fix at
    iteration 100 meets a pending rho update (the double count): from there c = dI / r4Et moves at every rho update, and the
    update at iteration 125, in the middle of a window, makes kernel and mirror rebuild the inverse."""
    insts = lp_instances("lp_100_500_seed0.npz")[4:7]
    b, os_ = _pair(insts)
    B = len(insts)
    vecs, nums = [np.zeros(0)] * B, [0] * B
    fixed_any = 0
    for w in range(40):
        stride = max(b.get_n(i) for i in range(B))
        V = -np.ones((B, stride))
        for i in range(B):
            V[i, :len(vecs[i])] = vecs[i]
        rets = b.solve_iter_l2f(w * 20, (w + 1) * 20, V, np.array(nums, np.int32))
        done = True
        for i, o in enumerate(os_):
            ro = o.solve_iter_l2f(w * 20, (w + 1) * 20, vecs[i] if nums[i] else -np.ones(o.get_n()), nums[i])
            assert rets[i] == ro and b.get_n(i) == o.get_n(), (w, i)
            xg, xo = b.get_x_iters_2d(20, i), o.get_x_iters_2d(20)
            assert bits_equal(xg, xo), (w, i)
            if ro:
                vecs[i], nums[i] = np.zeros(0), 0
                continue
            done = False
            v, k = scripted_fix_vec(xo, last=10)
            if w % 3 == 2 or k < 5:              # every third window without a fix: the saved inverse is reloaded
                v, k = -np.ones(len(v)), 0
            vecs[i], nums[i] = v, k
            fixed_any += k
        _same_state(b, os_, w)
        if done:
            break
    assert fixed_any > 50


def test_switching_modes_between_calls():
    I = lp_instances("lp_100_500_seed0.npz")[9]
    b = LpBatch([I])
    b.solve_init()
    o = oracle_for(b, 0, I)
    plan = (("pcg", 0, 40), ("direct", 40, 90), ("pcg", 90, 120), ("direct", 120, 300))
    for mode, a, e in plan:
        b.set_x_update(mode)
        o.set_x_update(mode, b.direct_rows(0) if mode == "direct" else None)
        assert b.solve_iter(a, e)[0] == o.solve_iter(a, e)
        assert bits_equal(b.debug_vec("x", 0), o.vec("x")), (mode, a, e)
    assert b.counters(0) == (o.total_outer_iters, o.total_pcg_iters)


def test_batches_that_do_not_fit_are_refused_loudly():
    big = lp_instances("lp_500_2000_seed0.npz")[:1]
    b = LpBatch(big)
    with pytest.raises(LpboxError, match="direct x-update"):
        b.set_x_update("direct")
    b.solve_init()                                   # the handle stays usable in the default mode
    b.solve_iter(0, 5)
    with pytest.raises(ValueError):
        b.set_x_update("cholesky")


def test_full_256_batch_properties():
    """No oracle at this size: determinism, every instance that stops does so by a reference stop rule with a feasible rounding,
    and the mean objective within 1 % of the default mode's (the modes are statistically equivalent
    in quality, tools/objective_study.py; a rare instance may run into max_iters, which the reference's loop bound allows too)."""
    insts = lp_instances("lp_100_500_seed0.npz")

    def run(mode):
        b = LpBatch(insts)
        b.set_x_update(mode)
        b.solve_init()
        b.solve_iter(0, 20000)
        return b
    d1, d2, p = run("direct"), run("direct"), run("pcg")
    stopped = 0
    for i, I in enumerate(insts):
        assert bits_equal(d1.debug_vec("x", i), d2.debug_vec("x", i)), i
        assert d1.counters(i)[1] == 0
        reason = d1.stop(i)[0]
        if reason in (1, 2):
            stopped += 1
            assert d1.check_infeasible_l2f(i) == 0, i
        x = d1.get_x_sol(i)
        assert set(np.unique(x)) <= {0.0, 1.0}
    assert stopped >= len(insts) - 2
    od = np.array([d1.cal_obj(i) for i in range(len(insts))])
    op = np.array([p.cal_obj(i) for i in range(len(insts))])
    assert abs(od.mean() - op.mean()) <= 0.01 * abs(op.mean())
    assert d1.kernel_time()[0] < p.kernel_time()[0]
