"""The opt-in reference summation order (LpBatch.set_order("reference")) against the oracle's model of the
reference's Eigen path (LPO_ORDER_EIGEN).  Bar: bit-exact on every iterate, counter and stop reason; the one documented deviation is
the std stop test, where the kernel takes sqrt and the reference pow(v, 1/2): where the oracle counted a pow/sqrt disagreement the
deviation differs by 1 ulp and std_obj (deviation / |objective|) by at most 2."""
import multiprocessing as mp
import os

import numpy as np
import pytest

from helpers import GOLDEN, bits_equal, lp_instances, make_oracle, scripted_fix_vec
from oracle import oracle as O

pytestmark = pytest.mark.gpu

FX = np.load(os.path.join(GOLDEN, "objective_study_100_500.npz"))


def ref_batch(insts):
    from lpbox_hip.lp import LpBatch
    B = LpBatch(insts)
    B.set_order("reference")
    B.solve_init()
    return B


def compare_state(B, idx, o, tag):
    left = o.vec("left_idx").astype(int)
    for name in ("x", "z1", "z2", "z4", "f"):
        gv, ov = B.debug_vec(name, idx), o.vec(name)
        if name in ("x", "z1", "z2"):            # the device keeps the original order; the oracle compacts
            gv = gv[left] if len(ov) == len(left) else gv
        assert bits_equal(gv, ov), f"{tag}: state vector {name} differs (max abs {np.abs(gv - ov).max():.3e})"
    for name in ("rho1", "rho4", "gamma", "dI", "rho4Et", "cur_obj", "sum_fix_obj", "best_bin_obj", "cvg1", "cvg2", "obj_val"):
        assert bits_equal([B.debug_scalar(name, idx)], [o.scalar(name)]), f"{tag}: scalar {name}"
    g, e = B.debug_scalar("std_obj", idx), o.scalar("std_obj")
    if o.scalar("pow_sqrt_mismatch") > 0:        # the kernel's sqrt against glibc's pow(v, 1/2): 1 ulp in the deviation, <= 2 after / |obj|
        assert abs(g - e) <= 2 * np.spacing(abs(e)), f"{tag}: std_obj {g!r} vs {e!r}"
    else:
        assert bits_equal([g], [e]), f"{tag}: std_obj"


def run_windows(B, idx_insts, oracles, ws, nwin, tag):
    """l2f windows without fixes on the batch and on one oracle per instance: x_iters, state, counters and the PCG trace."""
    vec = np.zeros((B.B, max(I["n"] for I in idx_insts)))
    done = [False] * B.B
    for w in range(nwin):
        pcg0 = [B.counters(i)[1] for i in range(B.B)]
        rg = B.solve_iter_l2f(w * ws, (w + 1) * ws, vec, np.zeros(B.B, np.int32))
        for i, o in enumerate(oracles):
            if done[i]:
                continue
            ro = o.solve_iter_l2f(w * ws, (w + 1) * ws, np.zeros(idx_insts[i]["n"]), 0)
            t = f"{tag} instance {i} window {w}"
            assert rg[i] == ro, t
            assert B.get_iter(i) == o.get_iter(), t
            xg, xo = B.get_x_iters_2d(ws, i), o.get_x_iters_2d(ws)
            if not bits_equal(xg, xo):
                bad = np.where((xg != xo).any(axis=0))[0]
                raise AssertionError(f"{t}: x_iters differ from iteration {bad[0]}")
            trace = o.pcg_trace()
            assert B.counters(i) == (o.total_outer_iters, o.total_pcg_iters), t
            assert B.counters(i)[1] - pcg0[i] == int(trace.sum()), t
            if len(trace):
                assert B.debug_scalar("last_pcg", i) == trace[-1], t
            compare_state(B, i, o, t)
            done[i] = bool(ro)
        if all(done):
            break


def test_headline_batch_matches_recorded_eigen_order_results():
    """All 256 instances of the headline batch to convergence: objective, outer and PCG iterations, stop reason and infeasibility equal
    the Eigen-order oracle's recorded results (the fixture's oracle half, reproduced on CPU by test_objective_gap)."""
    insts = lp_instances("lp_100_500_seed0.npz")
    B = ref_batch(insts)
    B.solve_iter(0, 20000)
    obj = np.array([-B.cal_obj(i) for i in range(256)])
    outer = np.array([B.counters(i)[0] for i in range(256)])
    pcg = np.array([B.counters(i)[1] for i in range(256)])
    stop = np.array([B.stop(i)[0] for i in range(256)])
    inf = np.array([B.check_infeasible_l2f(i) for i in range(256)])
    assert int((obj == FX["eigen_obj"]).sum()) == 256, f"{int((obj == FX['eigen_obj']).sum())} of 256 objectives match"
    assert np.array_equal(outer, FX["eigen_iters"])
    assert np.array_equal(pcg, FX["eigen_pcg"])
    assert np.array_equal(stop, FX["eigen_stop"])
    assert np.array_equal(inf, FX["eigen_infeasible"])


def test_windows_bit_exact_headline_and_config4():
    for fixture, picks in (("lp_100_500_seed0.npz", (0, 7, 100, 255)), ("lp_500_2000_seed0.npz", (0, 1))):
        all_insts = lp_instances(fixture)
        insts = [all_insts[i] for i in picks]
        B = ref_batch(insts)
        cfg = B.config()
        assert cfg["threads"] == 512
        for i, I in enumerate(insts):
            assert np.array_equal(B.layout(i), np.arange(I["n"]))
            assert np.all(B.row_split(i) == 1)
            own, help4 = B.col_split(i)
            assert np.array_equal(own, np.diff(I["colptr"])) and not np.any(help4)
        run_windows(B, insts, [make_oracle(I, O.ORDER_EIGEN) for I in insts], 50, 6, fixture)


def _oracle_full(I):
    s = O.LpOracle(0, order=O.ORDER_EIGEN)
    s.set_problem(I["n"], I["l"], I["colptr"], I["rowidx"], I["b"])
    s.solve_init()
    ret = s.solve_iter(0, 20000)
    return ret, s.total_outer_iters, s.total_pcg_iters, s.last_stop_reason, s.vec("x"), s.get_x_sol().ravel(), s.cal_Obj()


def test_full_solves_config4_match_oracle():
    from lpbox_hip.lp import PyLPboxADMMsolver
    insts = [lp_instances("lp_500_2000_seed0.npz")[i] for i in (2, 3)]
    with mp.get_context("spawn").Pool(2) as pool:
        pending = pool.map_async(_oracle_full, insts)
        got = []
        for I in insts:
            s = PyLPboxADMMsolver(0)
            s.set_order("reference")
            s.set_problem(I["n"], I["l"], I["colptr"], I["rowidx"], I["b"])
            s.solve_init()
            ret = s.solve_iter(0, 20000)
            got.append((ret, s.batch.counters(0), s.batch.stop(0)[0], s.get_final_x_sol(I["n"]).ravel(), s.get_x_sol(I["n"]).ravel(),
                        s.cal_Obj()))
        want = pending.get(timeout=600)
    for (ret, cnt, stop, x, xs, obj), (ro, outer, pcg, ostop, ox, oxs, oobj) in zip(got, want):
        assert ret == ro and cnt == (outer, pcg) and stop == ostop
        assert bits_equal(x, ox)
        assert np.array_equal(xs, oxs) and obj == oobj


def test_l2f_windows_with_fixes_match_oracle_compaction():
    """The product loop of LP/trainer.py:504-545 with a scripted policy: every fix shifts the live ranks of the reductions."""
    from lpbox_hip.lp import PyLPboxADMMsolver
    for fixture, idx in (("lp_100_500_seed0.npz", 4), ("lp_500_2000_seed0.npz", 5)):
        I = lp_instances(fixture)[idx]
        g = PyLPboxADMMsolver(0)
        g.set_order("reference")
        g.set_problem(I["n"], I["l"], I["colptr"], I["rowidx"], I["b"])
        g.solve_init()
        o = make_oracle(I, O.ORDER_EIGEN)
        ws = 50
        vec, num, fixes = np.zeros(I["n"]), 0, 0
        for w in range(60):
            rg = g.solve_iter_l2f(w * ws, (w + 1) * ws, vec, num)
            ro = o.solve_iter_l2f(w * ws, (w + 1) * ws, vec, num)
            tag = f"{fixture}[{idx}] window {w}"
            assert rg == ro, tag
            assert g.get_n() == o.get_n() and g.get_iter() == o.get_iter(), tag
            assert g.cal_Obj() == o.cal_Obj(), tag
            if rg:
                break
            xg, xo = g.get_x_iters_2d(ws), o.get_x_iters_2d(ws)
            assert bits_equal(xg, xo), f"{tag}: x_iters differ"
            compare_state(g.batch, 0, o, tag)
            vec, num = scripted_fix_vec(xo)
            if num <= 10:                       # LP/trainer.py:533-535
                num = 0
            fixes += num > 0
        assert fixes >= 1, f"{fixture}: the scripted policy never fixed anything; the re-ranking is not exercised"
        assert np.array_equal(g.get_x_sol(I["n"]).ravel(), o.get_x_sol().ravel())
        assert g.check_infeasible_l2f() == o.check_infeasible_l2f()


def odd_instance(n, rs):
    """tools/fuzz_lp.py's generator pattern at a given n: empty rows in the middle, one-entry columns, l != n."""
    l = max(2, int(n * rs.uniform(0.3, 0.9)))
    if l == n:
        l = n + 1
    cols = []
    for j in range(n):
        k = 1 if j % 3 == 0 else int(rs.randint(1, min(l, 5) + 1))
        cols.append(sorted(set(rs.choice(l, size=k, replace=False).tolist())))
    dead = set(rs.choice(l, size=max(1, l // 5), replace=False).tolist()) - {l - 1}
    cols = [[r for r in c if r not in dead] or [l - 1] for c in cols]
    colptr = np.zeros(n + 1, np.int32)
    colptr[1:] = np.cumsum([len(c) for c in cols])
    rowidx = np.array([r for c in cols for r in c], np.int32)
    return dict(n=n, l=l, colptr=colptr, rowidx=rowidx, b=-rs.uniform(1, 500, n))


def test_odd_sizes_every_redux_branch():
    rs = np.random.RandomState(11)
    insts = [odd_instance(n, rs) for n in (2, 3, 4, 5, 6, 7, 9, 513, 1023, 2047)]
    assert all(I["n"] != I["l"] for I in insts)
    B = ref_batch(insts)
    run_windows(B, insts, [make_oracle(I, O.ORDER_EIGEN) for I in insts], 50, 3, "odd sizes")


def test_refusals_and_default_handle_unchanged():
    from lpbox_hip.lp import LpBatch, PyLPboxADMMsolver
    from lpbox_hip._lib import LpboxError
    insts = lp_instances("lp_100_500_seed0.npz")[:2]
    # after the upload: LPBOX_E_STATE
    B = LpBatch(insts)
    B.solve_init()
    with pytest.raises(LpboxError) as e:
        B.set_order("reference")
    assert e.value.code == -3
    # with the direct x-update or the iteration log, in either call order: LPBOX_E_UNSUPPORTED
    for first in ("direct", "log"):
        B = LpBatch(insts)
        B.set_order("reference")
        with pytest.raises(LpboxError) as e:
            B.set_x_update("direct") if first == "direct" else B.set_log(True)
        assert e.value.code == -7
        B = LpBatch(insts)
        if first == "direct":
            B.set_x_update("direct")
        else:
            B.set_log(True)
        with pytest.raises(LpboxError) as e:
            B.set_order("reference")
        assert e.value.code == -7
    # beyond the on-chip limit: LPBOX_E_TOOLARGE, no silent switch to the large-instance path
    rs = np.random.RandomState(3)
    big = odd_instance(2100, rs)
    B = LpBatch([big])
    B.set_order("reference")
    with pytest.raises(LpboxError) as e:
        B.solve_init()
    assert e.value.code == -9
    s = PyLPboxADMMsolver(0)
    s.set_order("reference")
    s.set_problem(big["n"], big["l"], big["colptr"], big["rowidx"], big["b"])
    with pytest.raises(LpboxError) as e:
        s.solve_init()
    assert e.value.code == -9 and not s.large
    # a default-order handle in the same process still matches the oracle in the kernels' own order
    from helpers import oracle_for
    R = ref_batch(insts)
    D = LpBatch(insts)
    D.solve_init()
    o = oracle_for(D, 0, insts[0])
    R.solve_iter_l2f(0, 100, None, None)
    D.solve_iter_l2f(0, 100, None, None)
    o.solve_iter_l2f(0, 100, np.zeros(insts[0]["n"]), 0)
    assert bits_equal(D.get_x_iters_2d(100, 0), o.get_x_iters_2d(100))
    assert D.counters(0) == (o.total_outer_iters, o.total_pcg_iters)
