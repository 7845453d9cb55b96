"""Constraint matrices with stored values on the reference-order kernels against the oracle in the reference's
Eigen order with the same values (LpOracle(order=ORDER_EIGEN), vals).  Bar: bit-exact on every iterate, state vector, scalar, counter and
stop decision, as tests/test_lp_ref_order_gpu.py holds the unit kernels to; the one allowance carried over from there: std_obj may
differ by at most 2 ulp where the oracle counted a pow/sqrt disagreement.  Both placements of the values run: LDS (headline shapes,
small instances) and global memory (config 4, and small instances forced there)."""
import multiprocessing as mp
import os
import subprocess

import numpy as np
import pytest

from helpers import GOLDEN, bits_equal, lp_instances, scripted_fix_vec
from oracle import oracle as O
from valued_cases import FAMILIES, edge_instance, oracle_full_valued, valued, valued_oracle

pytestmark = pytest.mark.gpu

FX = np.load(os.path.join(GOLDEN, "objective_study_100_500.npz"))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEARNING_FACT = 1 + 1.0 / 100


def ref_batch(insts, placement=None, monkeypatch=None):
    """A reference-order batch; placement "lds" / "global" forces where the values sit (None: the library's rule)."""
    from lpbox_hip.lp import LpBatch
    if placement is not None:
        monkeypatch.setenv("LPBOX_LP_REF_VALS", placement)
    B = LpBatch(insts, order="reference")
    B.solve_init()
    if placement is not None:
        monkeypatch.delenv("LPBOX_LP_REF_VALS")
    return B


def vals_lds_bytes(B, insts):
    """LDS bytes of the launch beyond the unit kernels' carve-up for the same shapes: 3 x 8 x ZS when the values sit in LDS, else 0."""
    from lpbox_hip.lp import LpBatch
    U = LpBatch([{k: v for k, v in I.items() if k != "vals"} for I in insts], order="reference")
    return B.config()["lds_bytes"] - U.config()["lds_bytes"]


def compare_state(B, idx, o, tag, vals=None, applied=None):
    left = o.vec("left_idx").astype(int)
    for name in ("x", "z1", "z2", "z4", "f", "pd"):
        gv, ov = B.debug_vec(name, idx), o.vec(name)
        if name in ("x", "z1", "z2", "pd"):      # the device keeps the original order; the oracle compacts
            gv = gv[left] if len(ov) == len(left) else gv
        assert bits_equal(gv, ov), f"{tag}: state vector {name} differs (max abs {np.abs(gv - ov).max():.3e})"
    for name in ("rho1", "rho4", "gamma", "dI", "cur_obj", "sum_fix_obj", "best_bin_obj", "cvg1", "cvg2", "obj_val"):
        assert bits_equal([B.debug_scalar(name, idx)], [o.scalar(name)]), f"{tag}: scalar {name}"
    g, e = B.debug_scalar("std_obj", idx), o.scalar("std_obj")
    if o.scalar("pow_sqrt_mismatch") > 0:        # the kernel's sqrt against glibc's pow(v, 1/2): 1 ulp in the deviation, <= 2 after / |obj|
        assert abs(g - e) <= 2 * np.spacing(abs(e)), f"{tag}: std_obj {g!r} vs {e!r}"
    else:
        assert bits_equal([g], [e]), f"{tag}: std_obj"
    if vals is not None and applied is not None:
        # rho4_E_transpose, entry by entry: rho4_0 * val, then scaled in place once per rho update that an iteration has consumed
        want = 25.0 * np.asarray(vals, np.float64)
        for _ in range(applied):
            want = LEARNING_FACT * want
        assert bits_equal(B.debug_vec("r4v", idx), want), f"{tag}: rho4_E_transpose after {applied} updates"


def run_windows(B, insts, oracles, ws, nwin, tag):
    """l2f windows without fixes on the batch and on one oracle per instance: x_iters, state, counters and the PCG trace."""
    vec = np.zeros((B.B, max(I["n"] for I in insts)))
    done = [False] * B.B
    for w in range(nwin):
        pcg0 = [B.counters(i)[1] for i in range(B.B)]
        rg = B.solve_iter_l2f(w * ws, (w + 1) * ws, vec, np.zeros(B.B, np.int32))
        for i, o in enumerate(oracles):
            if done[i]:
                continue
            ro = o.solve_iter_l2f(w * ws, (w + 1) * ws, np.zeros(insts[i]["n"]), 0)
            t = f"{tag} instance {i} window {w}"
            assert rg[i] == ro, t
            assert B.get_iter(i) == o.get_iter(), t
            assert B.stop(i)[0] == o.last_stop_reason, t
            xg, xo = B.get_x_iters_2d(ws, i), o.get_x_iters_2d(ws)
            if not bits_equal(xg, xo):
                bad = np.where((xg != xo).any(axis=0))[0]
                raise AssertionError(f"{t}: x_iters differ from iteration {bad[0]}")
            trace = o.pcg_trace()
            assert B.counters(i) == (o.total_outer_iters, o.total_pcg_iters), t
            assert B.counters(i)[1] - pcg0[i] == int(trace.sum()), t
            if len(trace):
                assert B.debug_scalar("last_pcg", i) == trace[-1], t
            full = o.get_iter() == (w + 1) * ws and o.last_stop_reason == 0
            compare_state(B, i, o, t, insts[i].get("vals", np.ones(len(insts[i]["rowidx"]))), ((w + 1) * ws - 1) // 25 if full else None)
            done[i] = bool(ro)
        if all(done):
            break


def test_windows_headline_values_in_lds():
    H = lp_instances("lp_100_500_seed0.npz")
    insts = [valued(H[p], fam, p) for p in (0, 7, 100, 255) for fam in FAMILIES]
    B = ref_batch(insts)
    cfg = B.config()
    assert (cfg["threads"], cfg["elems_per_thread"]) == (512, 1)
    zs = (max(len(I["rowidx"]) for I in insts) + 7) & ~7
    assert vals_lds_bytes(B, insts) == 24 * zs, "the headline shape keeps its values in LDS"
    run_windows(B, insts, [valued_oracle(I) for I in insts], 50, 6, "headline")


def test_windows_config4_values_in_global_memory():
    C4 = lp_instances("lp_500_2000_seed0.npz")
    insts = [valued(C4[0], "uniform", 0), valued(C4[1], "signed", 1)]
    B = ref_batch(insts)
    cfg = B.config()
    assert (cfg["threads"], cfg["elems_per_thread"]) == (512, 4)
    assert vals_lds_bytes(B, insts) == 0, "config 4 leaves no room in LDS: the values stay in global memory"
    run_windows(B, insts, [valued_oracle(I) for I in insts], 50, 6, "config 4")


def test_windows_two_slots_per_thread_both_placements(monkeypatch):
    I = edge_instance(700, 3)
    assert 512 < I["n"] <= 1024 and I["n"] != I["l"]
    for placement in ("lds", "global"):
        B = ref_batch([I], placement, monkeypatch)
        assert B.config()["elems_per_thread"] == 2
        assert (vals_lds_bytes(B, [I]) > 0) == (placement == "lds")
        run_windows(B, [I], [valued_oracle(I)], 50, 6, f"n = 700, values in {placement}")


def test_full_solves_match_oracle():
    """To the stop or the 20 000 cap: return value, outer and PCG counts, stop reason, raw x, binary x, objective, both infeasibility counts."""
    S, H = lp_instances("lp_20_60_seed0.npz"), lp_instances("lp_100_500_seed0.npz")
    groups = [[valued(S[p], fam, p) for p in range(4) for fam in FAMILIES], [valued(H[3], "set", 3), valued(H[200], "signed", 200)]]
    with mp.get_context("spawn").Pool(4) as pool:
        pending = [pool.map_async(oracle_full_valued, g) for g in groups]
        got = []
        for g in groups:
            B = ref_batch(g)
            rets = B.solve_iter(0, 20000)
            got.append([(int(rets[i]), B.counters(i), B.stop(i)[0], B.get_final_x_sol(i), B.get_x_sol(i), B.cal_obj(i),
                         B.check_infeasible_lpbox(i), B.check_infeasible_l2f(i)) for i in range(B.B)])
        want = [p.get(timeout=600) for p in pending]
    for gi, (gg, ww) in enumerate(zip(got, want)):
        for i, ((ret, cnt, stop, x, xs, obj, inf1, inf2), (ro, outer, pcg, ostop, ox, oxs, oobj, oinf1, oinf2)) in enumerate(zip(gg, ww)):
            t = f"group {gi} instance {i}"
            assert ret == ro and cnt == (outer, pcg) and stop == ostop, t
            assert bits_equal(x, ox), t
            assert np.array_equal(xs, oxs) and obj == oobj, t
            assert (inf1, inf2) == (oinf1, oinf2), t


@pytest.mark.parametrize("placement", ["lds", "global"])
def test_l2f_windows_with_fixes_match_oracle_compaction(placement, monkeypatch):
    """A scripted policy fixes variables between windows: the kernel masks, the oracle really compacts E (values included), f loses
    E_fix x_fix, rho4_E_transpose and Esq_diag are rebuilt from the live columns."""
    from lpbox_hip.lp import PyLPboxADMMsolver
    I = valued(lp_instances("lp_100_500_seed0.npz")[4], "set", 4)
    monkeypatch.setenv("LPBOX_LP_REF_VALS", placement)
    g = PyLPboxADMMsolver(0)
    g.set_order("reference")
    g.set_problem(I["n"], I["l"], I["colptr"], I["rowidx"], I["b"], vals=I["vals"])
    g.solve_init()
    o = valued_oracle(I)
    ws = 50
    vec, num, fixes = np.zeros(I["n"]), 0, 0
    for w in range(60):
        rg = g.solve_iter_l2f(w * ws, (w + 1) * ws, vec, num)
        ro = o.solve_iter_l2f(w * ws, (w + 1) * ws, vec, num)
        tag = f"values in {placement}, window {w}"
        assert rg == ro, tag
        assert g.get_n() == o.get_n() and g.get_iter() == o.get_iter(), tag
        assert g.batch.stop(0)[0] == o.last_stop_reason, tag
        assert g.cal_Obj() == o.cal_Obj(), tag
        if rg:
            break
        xg, xo = g.get_x_iters_2d(ws), o.get_x_iters_2d(ws)
        assert bits_equal(xg, xo), f"{tag}: x_iters differ"
        compare_state(g.batch, 0, o, tag)
        vec, num = scripted_fix_vec(xo)
        if num <= 10:
            num = 0
        fixes += num > 0
    assert fixes >= 1, "the scripted policy never fixed anything; the compaction is not exercised"
    assert np.array_equal(g.get_x_sol(I["n"]).ravel(), o.get_x_sol().ravel())
    assert g.check_infeasible_l2f() == o.check_infeasible_l2f()
    assert g.check_infeasible_lpbox() == o.check_infeasible_lpbox()


def test_mixed_batch_unit_instances_keep_their_recorded_results():
    """The 256 headline instances with values on instance 0 only: the whole batch runs the valued kernels, instances 1 .. 255 (every
    value 1.0) must still give the recorded Eigen-order results exactly, instance 0 must equal its oracle."""
    insts = lp_instances("lp_100_500_seed0.npz")
    insts[0] = valued(insts[0], "uniform", 0)
    with mp.get_context("spawn").Pool(1) as pool:
        pending = pool.map_async(oracle_full_valued, [insts[0]])
        B = ref_batch(insts)
        assert vals_lds_bytes(B, insts) > 0
        rets = B.solve_iter(0, 20000)
        obj = np.array([-B.cal_obj(i) for i in range(256)])
        outer = np.array([B.counters(i)[0] for i in range(256)])
        pcg = np.array([B.counters(i)[1] for i in range(256)])
        stop = np.array([B.stop(i)[0] for i in range(256)])
        inf = np.array([B.check_infeasible_l2f(i) for i in range(256)])
        (ro, oouter, opcg, ostop, ox, oxs, oobj, oinf1, oinf2), = pending.get(timeout=600)
    u = slice(1, 256)
    assert int((obj[u] == FX["eigen_obj"][u]).sum()) == 255
    assert np.array_equal(outer[u], FX["eigen_iters"][u]) and np.array_equal(pcg[u], FX["eigen_pcg"][u])
    assert np.array_equal(stop[u], FX["eigen_stop"][u]) and np.array_equal(inf[u], FX["eigen_infeasible"][u])
    assert int(rets[0]) == ro and (outer[0], pcg[0], stop[0]) == (oouter, opcg, ostop)
    assert bits_equal(B.get_final_x_sol(0), ox) and np.array_equal(B.get_x_sol(0), oxs)
    assert -obj[0] == oobj and inf[0] == oinf2 and B.check_infeasible_lpbox(0) == oinf1


@pytest.mark.parametrize("k", [2, 3])
def test_fixture_file_through_the_dropin_class(k, tmp_path):
    """tests/golden/instance/<k>_7: values other than 1, duplicates, a cancelling pair; k == 2 takes the reader's negation path."""
    from lpbox_hip.lp import PyLPboxADMMsolver
    d = os.path.join(GOLDEN, "instance", "%d_7" % k)
    o = O.LpOracle(0, order=O.ORDER_EIGEN)
    o.read_files(os.path.join(d, "instance_1_C.txt"), os.path.join(d, "instance_1_b.txt"), k)
    o.solve_init()
    g = PyLPboxADMMsolver(0)
    g.data_root = GOLDEN
    g.write_files = False
    g.set_order("reference")
    g.read_File(1, k, 7)
    g.solve_init()
    n = g.get_n()
    assert n == o.get_n() and "vals" in g.batch.get_problem(0)
    rg, ro = g.solve_iter_l2f(0, 100, np.zeros(n), 0), o.solve_iter_l2f(0, 100, np.zeros(n), 0)
    assert rg == ro and bits_equal(g.get_x_iters_2d(100), o.get_x_iters_2d(100))
    compare_state(g.batch, 0, o, f"k = {k} after the window")
    rg, ro = g.solve_iter(100, 5000), o.solve_iter(100, 5000)
    assert rg == ro and g.batch.counters(0) == (o.total_outer_iters, o.total_pcg_iters) and g.batch.stop(0)[0] == o.last_stop_reason
    assert bits_equal(g.get_final_x_sol(n).ravel(), o.vec("x"))
    assert np.array_equal(g.get_x_sol(n).ravel(), o.get_x_sol().ravel()) and g.cal_Obj() == o.cal_Obj()
    assert g.check_infeasible_lpbox() == o.check_infeasible_lpbox() and g.check_infeasible_l2f() == o.check_infeasible_l2f()
    # the C++ class takes the same road: set_order, then readFile through lpbox_read_file
    cxx = os.path.join(ROOT, "accelerated-lpbox-admm_amd", "cxx", "LinearProgramming", "cython_solver")
    exe = str(tmp_path / "lp_solve")
    subprocess.check_call(["make", "-s", "-C", cxx, "OUT=" + exe])
    p = subprocess.run([exe, "1", str(k), "7", "5000", "0", "0", "0", "1"], env=dict(os.environ, LPBOX_DATA_ROOT=GOLDEN, LPBOX_QUIET="1"),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    res = dict(kv.split("=") for kv in [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][0][7:].split())
    f = O.LpOracle(0, order=O.ORDER_EIGEN)
    f.read_files(os.path.join(d, "instance_1_C.txt"), os.path.join(d, "instance_1_b.txt"), k)
    f.solve_init()
    rf = f.solve_iter(0, 5000)
    assert int(res["ret"]) == rf and float(res["objective"]) == -f.cal_Obj() and int(res["iterations"]) == f.total_outer_iters
    assert int(res["stop"]) == f.last_stop_reason and int(res["infeasible"]) == f.check_infeasible_l2f()
    # without the order the driver fails loudly and names the missing call
    p = subprocess.run([exe, "1", str(k), "7"], env=dict(os.environ, LPBOX_DATA_ROOT=GOLDEN), capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "lpbox_set_order" in p.stderr


@pytest.mark.parametrize("placement", ["lds", "global"])
def test_edges_and_every_redux_branch(placement, monkeypatch):
    """An explicit zero, 1e-3 next to 1e3 in one row, a one-entry row, an empty row; n = 2 .. 9 walk every branch of the redux."""
    insts = [edge_instance(n, 20 + n) for n in (2, 3, 4, 5, 6, 7, 9, 40)]
    for I in insts:
        rows = np.bincount(I["rowidx"], minlength=I["l"])
        assert I["n"] != I["l"] and np.any(rows == 0) and np.any(rows == 1) and np.any(I["vals"] == 0.0)
        assert np.any(I["vals"] == 1e-3) and np.any(I["vals"] == 1e3)
    B = ref_batch(insts, placement, monkeypatch)
    run_windows(B, insts, [valued_oracle(I) for I in insts], 50, 3, f"edges, values in {placement}")
