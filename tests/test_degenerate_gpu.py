"""GPU tests of the degenerate scalar branches and out-of-range data of the segmentation and generic-BQP kernels (the cases of
tests/degenerate_cases.py; DESIGN.md section 26 holds the branch table B1-B7).  Every case is compared bit for bit against the C oracle in
the kernels' order (built from the solver's threads / chunk read-outs), or in Eigen order for the reference-order routes; scalars are
compared by bit pattern too, so that NaN == NaN and -0.0 != +0.0 are judged.  tests/test_degenerate_cases.py pins on the CPU that each
case enters its branch on the oracle, so a kernel that equals the oracle here has taken the branch."""
import functools

import numpy as np
import pytest

import degenerate_cases as D
from bqp_ref_cases import EXACT_SCALARS, STD_OBJ_ULPS
from chain_cases import expected_resumes
from helpers import BQP_SCALARS, BQP_VECS, bits_equal_nan, bqp_params, bqp_problem, scalar_bits_equal
from oracle import oracle as O
from seg_harness import SCALARS as SEG_SCALARS

pytestmark = pytest.mark.gpu

ALL_BQP_SCALARS = BQP_SCALARS + ("iters", "stop", "total_pcg", "last_pcg")
ORDINARY = (("ordinary-t3", bqp_problem(200, 15, 20, seed=801), bqp_params(3, 8)), ("ordinary-t0", bqp_problem(257, seed=802), bqp_params(0, 8)))


def vec_names(P):
    return [v for v in BQP_VECS if (v != "z3" or P.get("C") is not None) and (v not in ("z4", "y3") or P.get("E") is not None)]


def ulps_apart(a, b):
    a, b = np.array([a], np.float64), np.array([b], np.float64)
    if np.isnan(a[0]) or np.isnan(b[0]):
        return 0 if np.isnan(a[0]) and np.isnan(b[0]) else 2 ** 62
    return abs(int(a.view(np.int64)[0]) - int(b.view(np.int64)[0]))


def bqp_same(vec, scalar, P, ref, tag, ref_order=False):
    """A solved problem (vec(name), scalar(name)) against a solved oracle: every vector of its type and every scalar by bit pattern; in
    reference order std_obj within the documented 2 ulps."""
    for name in vec_names(P):
        got, want = vec(name), ref.vec(name)
        assert bits_equal_nan(got, want), f"{tag} {name}: max diff {np.nanmax(np.abs(got - want)):.3e}, NaN at {np.isnan(got).sum()} / {np.isnan(want).sum()}"
    for name in (EXACT_SCALARS if ref_order else ALL_BQP_SCALARS):
        assert scalar_bits_equal(scalar(name), ref.scalar(name)), f"{tag} {name}: {scalar(name)!r} vs {ref.scalar(name)!r}"
    if ref_order:
        d = ulps_apart(scalar("std_obj"), ref.scalar("std_obj"))
        assert d <= STD_OBJ_ULPS, f"{tag} std_obj: {d} ulps apart"


def bqp_oracle(P, prm, order, T=256, chunk=512):
    o = O.BqpOracle(P, params=prm, order=order, T=T, chunk=chunk)
    with np.errstate(invalid="ignore"):
        return o, o.solve()


def assert_pinned(name, it, o):
    iters, stop, trace = D.BQP_PINS[name]
    assert it == iters and o.scalar("stop") == stop and list(o.pcg_trace()) == list(trace), (name, it, o.scalar("stop"), list(o.pcg_trace()))


# ---- BqpSolver: the launch chain ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["default", "reference"])
@pytest.mark.parametrize("name", D.BQP_NAMES)
def test_bqp_solver_case(monkeypatch, name, order):
    from lpbox_hip.bqp import BqpSolver
    P, prm = D.bqp_case(name)
    centre = name.startswith("centre_start")
    if centre:
        monkeypatch.setenv("LPBOX_BQP_KMAX", "4")       # a fixed launch count makes the number of resumes exact
    g = BqpSolver(P["n"], P["A"], P["b"], P["x0"], P.get("C"), P.get("d"), P.get("E"), P.get("f"), params=prm, order=order)
    it = g.solve()                                      # (an LPBOX_E_STATE of the resume guard would raise here)
    assert g.scalar("threads") == 256 and g.scalar("chunk") == 512 and g.scalar("order") == (order == "reference")
    o, it_o = bqp_oracle(P, prm, O.ORDER_EIGEN if order == "reference" else O.ORDER_GPU, int(g.scalar("threads")), int(g.scalar("chunk")))
    assert_pinned(name, it_o, o)
    assert it == it_o, f"{name} {order}: iterations {it} vs {it_o}"
    bqp_same(g.vec, g.scalar, P, o, f"{name} {order}", ref_order=order == "reference")
    if centre:
        trace = [int(k) for k in o.pcg_trace()]
        assert trace == [int(prm[10])] * 2 and g.scalar("kmax") == 4
        assert g.scalar("pcg_resumes") == expected_resumes(trace, 4) == 4
        assert np.array_equal(np.isnan(g.vec("x")), np.isnan(o.vec("x"))) and np.isnan(g.vec("x")).all()
    g.close()


# ---- BqpBatch: one workgroup per problem, every case in one batch ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def batch_solved(order):
    from lpbox_hip.bqp import BqpBatch
    cases = [(name,) + tuple(D.bqp_case(name)) for name in D.BQP_NAMES]
    cases[20:20] = [ORDINARY[0]]                        # the ordinary problems sit between degenerate neighbours
    cases.append(ORDINARY[1])
    B = BqpBatch([P for _, P, _ in cases], params=[prm for _, _, prm in cases], order=order)
    return B, B.solve(), cases


@pytest.mark.parametrize("order", ["default", "reference"])
def test_bqp_batch_holds_every_case_and_leaves_the_neighbours_alone(order):
    from lpbox_hip.bqp import BqpSolver
    B, its, cases = batch_solved(order)
    assert {D.bqp_ptype(P) for _, P, _ in cases} == {0, 1, 2, 3} and len(cases) == len(D.BQP_NAMES) + 2
    assert B.scalar(0, "threads") == 256 and B.scalar(0, "chunk") == 512 and B.scalar(0, "order") == (order == "reference")
    for i, (name, P, prm) in enumerate(cases):
        o, it_o = bqp_oracle(P, prm, O.ORDER_EIGEN if order == "reference" else O.ORDER_GPU)
        if name in D.BQP_PINS:
            assert_pinned(name, it_o, o)
        assert int(its[i]) == it_o, f"batch [{i}] {name} {order}: iterations {its[i]} vs {it_o}"
        bqp_same(functools.partial(B.vec, i), functools.partial(B.scalar, i), P, o, f"batch [{i}] {name} {order}", ref_order=order == "reference")
        if name.startswith("ordinary"):                 # ... and bit for bit what the problem gives on its own
            g = BqpSolver(P["n"], P["A"], P["b"], P["x0"], P.get("C"), P.get("d"), P.get("E"), P.get("f"), params=prm, order=order)
            assert g.solve() == int(its[i]) == 8 and np.isfinite(B.vec(i, "x")).all()
            for v in vec_names(P):
                assert bits_equal_nan(B.vec(i, v), g.vec(v)), f"batch [{i}] {name} {order} {v} vs its solo run"
            for s in ALL_BQP_SCALARS + ("outer_total",):
                assert scalar_bits_equal(B.scalar(i, s), g.scalar(s)), f"batch [{i}] {name} {order} {s} vs its solo run"
            g.close()


def test_bqp_batch_refuses_non_finite_data_on_the_host():
    """lpbox_bqp_batch_set_problem / _set_params share the host checks of the one-problem handle (tests/test_degenerate_cases.py); a batch
    handle exists only where a device does, hence here."""
    import ctypes as C

    from lpbox_hip import _lib
    from lpbox_hip.bqp import BqpBatch
    from lpbox_hip.lp import LpboxError
    P = bqp_problem(12, 3, 4, seed=2)
    L = _lib.load()
    for key in ("A", "b", "x0", "C", "d", "E", "f"):
        for bad in (float("nan"), float("inf"), float("-inf")):
            Q = dict(P)
            if key in ("A", "C", "E"):
                v = np.array(P[key][2], np.float64); v[2] = bad
                Q[key] = (P[key][0], P[key][1], v)
            else:
                v = np.array(P[key], np.float64); v[2] = bad
                Q[key] = v
            with pytest.raises(LpboxError, match=f"{key} has a non-finite") as err:
                BqpBatch([P, Q])
            assert err.value.code == -2                  # LPBOX_E_BADARG
    B = BqpBatch([P, P], params=bqp_params(3, 4))
    prm = np.array(bqp_params(3, 4), np.float64)
    prm[6] = float("nan")
    assert L.lpbox_bqp_batch_set_params(B._h, 1, prm) == -2 and b"index 6, initial_rho" in L.lpbox_last_error()
    bad_b = np.array(P["b"], np.float64); bad_b[7] = float("inf")
    A, Cm, Em = [[np.ascontiguousarray(a) for a in P[k]] for k in ("A", "C", "E")]
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    d, f, x0 = (np.ascontiguousarray(P[k], np.float64) for k in ("d", "f", "x0"))
    rc = L.lpbox_bqp_batch_set_problem(B._h, 1, 12, ptr(A[0]), ptr(A[1]), ptr(A[2]), ptr(bad_b), ptr(x0), 3, ptr(Cm[0]), ptr(Cm[1]), ptr(Cm[2]),
                                       ptr(d), 4, ptr(Em[0]), ptr(Em[1]), ptr(Em[2]), ptr(f))
    assert rc == -2 and L.lpbox_last_error() == b"b has a non-finite entry (index 7)"
    its = B.solve()                                      # the batch stays usable, with the problems and parameters it had
    assert list(its) == [4, 4] and bits_equal_nan(B.vec(0, "x"), B.vec(1, "x"))
    B.close()


# ---- segmentation -------------------------------------------------------------------------------------------------------------------
def seg_solver(P, init=True):
    from lpbox_hip.seg import PyLPboxADMMsolver
    g = PyLPboxADMMsolver(0, P["n"], 0)
    g.write_files = False
    g.set_problem(P)
    if init:
        g.solve_init()
    return g


def seg_pair(monkeypatch, name):
    """The case on a handle that may hold the matrix as diagonals and on one that keeps ELL, with the storage each ended up in asserted."""
    P = D.seg_case(name)
    dia = seg_solver(P)
    monkeypatch.setenv("LPBOX_SEG_NODIA", "1")
    ell = seg_solver(P)
    monkeypatch.delenv("LPBOX_SEG_NODIA")
    assert dia.debug_scalar("matrix_as_diagonals") == (1.0 if D.seg_as_diagonals(name) else 0.0), name
    assert ell.debug_scalar("matrix_as_diagonals") == 0.0
    width = int(np.diff(P["rowptr"]).max())
    assert ell.debug_scalar("ell_width") == width and (D.seg_as_diagonals(name) or dia.debug_scalar("ell_width") == width)
    return P, dia, ell


def seg_oracle(g, P):
    cfg = g.config()
    o = O.SegOracle(0, P["n"], 0, order=O.ORDER_GPU, T=cfg["threads"], chunk=cfg["threads"] * cfg["elems_per_thread"])
    o.set_problem(P)
    o.solve_init()
    return o


def seg_state_same(g, o, ws, tag, stopped=False):
    """The state of a HIP handle after a window against the oracle's (and, o being a HIP handle, against another handle's)."""
    hip = not isinstance(o, O.SegOracle)
    xg, xo = g.get_x_iters_2d(ws), o.get_x_iters_2d(ws)
    assert bits_equal_nan(xg, xo), f"{tag}: x_iters differ, max diff {np.nanmax(np.abs(xg - xo)):.3e}"
    if hip:
        assert g.counters() == o.counters() and g.get_n() == o.get_n()
        left = slice(None)
    else:
        assert g.counters() == (o.total_outer_iters, o.total_pcg_iters) and g.get_n() == o.get_n()
        left = o.vec("left_idx").astype(int)
    for v in ("x", "z1", "z2", "b"):
        got, want = g.debug_vec(v)[left], (o.debug_vec(v) if hip else o.vec(v))
        assert bits_equal_nan(got, want), f"{tag}: {v} differs, max diff {np.nanmax(np.abs(got - want)):.3e}"
    for s in SEG_SCALARS:
        if stopped and not hip and s in ("obj_val", "cur_obj", "std_obj"):        # a window that stops on the residual test in its first
            continue                                                              # iteration never computes them (placeholders differ)
        a, b = g.debug_scalar(s), (o.debug_scalar(s) if hip else o.scalar(s))
        assert scalar_bits_equal(a, b), f"{tag}: {s} {a!r} vs {b!r}"


@pytest.mark.parametrize("name", D.SEG_NAMES)
def test_seg_window_in_both_storages(monkeypatch, name):
    P, dia, ell = seg_pair(monkeypatch, name)
    o = seg_oracle(dia, P)
    z = np.zeros(P["n"])
    ret, trace = D.SEG_WINDOW_PINS[name]
    assert (dia.solve_iter_l2f(0, 3, z, 0), ell.solve_iter_l2f(0, 3, z, 0), o.solve_iter_l2f(0, 3, z, 0)) == (ret,) * 3
    assert list(o.pcg_trace()) == list(trace)
    seg_state_same(dia, o, 3, f"{name} vs oracle", stopped=bool(ret))
    seg_state_same(ell, o, 3, f"{name} ELL vs oracle", stopped=bool(ret))
    seg_state_same(dia, ell, 3, f"{name} diagonals vs ELL")
    assert dia.stop() == ell.stop() and (not ret or dia.stop()[0] == o.last_stop == 1)


@pytest.mark.parametrize("name", sorted(D.SEG_LEGACY_PINS))
def test_seg_legacy_solve_in_both_storages(monkeypatch, name):
    P, dia, ell = seg_pair(monkeypatch, name)
    o = seg_oracle(dia, P)
    energy, it1, stop, pcg_total = D.SEG_LEGACY_PINS[name]
    eo = o.solve_iter()
    assert (eo, o.legacy_iter_plus1, o.last_stop, o.total_pcg_iters) == (energy, it1, stop, pcg_total)
    for g, tag in ((dia, "diagonals"), (ell, "ELL")):
        assert g.solve_iter() == energy, f"{name} {tag}"          # at b x 1e6: the defined out-of-range int, the oracle's
        assert scalar_bits_equal(g.get_obj(), o.get_obj()), f"{name} {tag}: get_obj {g.get_obj()!r} vs {o.get_obj()!r}"
        assert g.counters() == (o.total_outer_iters, o.total_pcg_iters) and g.stop() == (stop, it1), f"{name} {tag}"
        assert np.array_equal(g.get_x_sol(), o.get_x_sol()) and bits_equal_nan(g.debug_vec("x"), o.vec("x")), f"{name} {tag}"
    if name == "b-x1e6":
        assert energy == D.SEG_1E6_ENERGY_INT and dia.get_obj() == D.SEG_1E6_OBJ


@pytest.mark.parametrize("name", D.SEG_FIX_CASES)
def test_seg_fix_step_in_both_storages(monkeypatch, name):
    """b := 2 Mb x2 + b with bytes up to 255 (seg_b_fix), td rebuilt on the live rows."""
    P, dia, ell = seg_pair(monkeypatch, name)
    o = seg_oracle(dia, P)
    z = np.zeros(P["n"])
    assert {s.solve_iter_l2f(*D.SEG_FIX_FIRST, z, 0) for s in (dia, ell, o)} == {0}
    seg_state_same(dia, o, 5, f"{name} first window")
    seg_state_same(ell, o, 5, f"{name} first window, ELL")
    vec, num = D.seg_fix_vec(o.get_x_iters_2d(5)[:, 4])
    fixed, ret, trace = D.SEG_FIX_PINS[name]
    assert num == fixed
    assert {s.solve_iter_l2f(*D.SEG_FIX_SECOND, vec, num) for s in (dia, ell, o)} == {ret}
    assert list(o.pcg_trace()) == list(trace) and dia.get_n() == ell.get_n() == P["n"] - fixed
    seg_state_same(dia, o, 3, f"{name} after the fix")
    seg_state_same(ell, o, 3, f"{name} after the fix, ELL")
    seg_state_same(dia, ell, 3, f"{name} after the fix, diagonals vs ELL")
    assert np.array_equal(dia.get_x_sol(), o.get_x_sol())


def test_seg_legacy_batch_equals_the_single_solves():
    from lpbox_hip.seg import solve_batch
    names = sorted(D.SEG_LEGACY_PINS)
    single = [seg_solver(D.seg_case(n)) for n in names]
    ref = [(s.solve_iter(), s.get_obj(), s.counters(), s.stop(), s.get_x_sol().copy(), s.debug_vec("x")) for s in single]
    batch = [seg_solver(D.seg_case(n), init=False) for n in names]
    en = solve_batch(batch)
    for k, (name, s) in enumerate(zip(names, batch)):
        assert en[k] == ref[k][0] == D.SEG_LEGACY_PINS[name][0], name
        assert scalar_bits_equal(s.get_obj(), ref[k][1]) and s.counters() == ref[k][2] and s.stop() == ref[k][3], name
        assert np.array_equal(s.get_x_sol(), ref[k][4]) and bits_equal_nan(s.debug_vec("x"), ref[k][5]), name


def test_seg_batched_window_over_every_case_equals_the_single_handles():
    """One lockstep window (0, 3) of lpbox_hip.seg.SegBatch -- the engine of run_l2f_seg_batch -- over all cases at once: problems that
    stop in iteration 0 beside problems that run on, diagonal storage beside ELL, n = 1 and n = 2 beside n = 600."""
    from lpbox_hip.seg import SegBatch
    single = [seg_solver(D.seg_case(n)) for n in D.SEG_NAMES]
    want = [s.solve_iter_l2f(0, 3, np.zeros(s.get_org_n()), 0) for s in single]
    members = [seg_solver(D.seg_case(n), init=False) for n in D.SEG_NAMES]
    batch = SegBatch(members)
    batch.solve_init()
    rets = batch.solve_iter_l2f(0, 3, None, np.zeros(len(members), np.int32))
    assert [m.debug_scalar("matrix_as_diagonals") for m in members] == [1.0 if D.seg_as_diagonals(n) else 0.0 for n in D.SEG_NAMES]
    for k, name in enumerate(D.SEG_NAMES):
        assert int(rets[k]) == want[k] == D.SEG_WINDOW_PINS[name][0], name
        seg_state_same(members[k], single[k], 3, f"batched window, {name}")
        assert members[k].stop() == single[k].stop(), name
    batch.close()
