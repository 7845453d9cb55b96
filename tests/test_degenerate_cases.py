"""CPU tests of the degenerate-branch cases (tests/degenerate_cases.py): the premises the GPU file
(tests/test_degenerate_gpu.py) rests on.  Per case the branch condition itself is asserted from the data, the PCG trace, stop reason,
return value and iteration count are pinned on BqpOracle / SegOracle in both orders and on NumpyBqp / NumpySeg, and the oracle is held
to the restatement within the bound B of tests/test_oracle_restatement.py (a NaN on every side counts as agreement, a NaN on one side
alone as a failure).  Then the host-side refusal of non-finite data through the C-ABI (no device is touched)."""
import ctypes as C
import math

import numpy as np
import pytest

import degenerate_cases as D
from helpers import BQP_SCALARS, BQP_VECS, assert_within_bound_nan, bqp_params, bqp_problem, banded_seg_problem
from oracle import oracle as O
from oracle.bqp_numpy import NumpyBqp, NumpySeg, col_sq, csr, project_box, project_sphere

E_BADARG = -2
SEG_SCALARS = ("rho1", "gamma", "std_obj", "cvg1", "cvg2", "obj_val", "best_bin_obj", "cur_obj")
FLOOR = 2.2204e-16                                     # the floor under norm(x) in the stop test (B4)


def fsum_sq(v):
    return math.fsum((np.asarray(v, np.float64) ** 2).tolist())


def test_the_tables_hold_every_case_and_the_sizes_stay_small():
    assert set(D.BQP_PINS) == set(D.BQP_NAMES) and set(D.SEG_WINDOW_PINS) == set(D.SEG_NAMES)
    assert set(D.SEG_LEGACY_PINS) == {f"b-x{t}" for t in D.SEG_FULL_SOLVE} | {"b-x1e6"}
    assert all(D.bqp_case(name)[0]["n"] <= 400 for name in D.BQP_NAMES) and all(D.seg_case(name)["n"] <= 600 for name in D.SEG_NAMES)
    assert {D.bqp_case(name)[0]["n"] for name in D.BQP_NAMES} >= {2, 3, 257}
    for family in ("zero_rhs", "scaled", "zero_precond_diag", "centre_start"):
        assert {D.bqp_ptype(D.bqp_case(name)[0]) for name in D.BQP_NAMES if name.startswith(family)} == {0, 1, 2, 3}
    for name in D.BQP_NAMES:                            # the NaN case never runs with the presets' 10^7 PCG iterations
        P, prm = D.bqp_case(name)
        assert prm[5] <= 12 and (not name.startswith("centre_start") or (prm[5], prm[10]) == (2, 30))


# ---- generic BQP ---------------------------------------------------------------------------------------------------------------------
def first_rhs(P, prm):
    """The right-hand side of the first x-update, from the formulas of oracle/bqp_numpy.py (NumpyBqp.solve, iteration 0)."""
    n, rho = P["n"], float(prm[6])
    x0 = np.asarray(P["x0"], float)
    y1, y2 = project_box(x0), project_sphere(x0, n)
    rhs = (rho * y1 + rho * y2) - ((np.asarray(P["b"], float) + np.zeros(n)) + np.zeros(n))
    if P.get("C") is not None:
        Cm = csr(P["C"], len(P["d"]), n)
        rhs = rhs + (rho * Cm.T.tocsr()) @ np.asarray(P["d"], float) - Cm.T @ np.zeros(len(P["d"]))
    if P.get("E") is not None:
        Em = csr(P["E"], len(P["f"]), n)
        t = (P["f"] - Em @ x0) - np.zeros(len(P["f"])) / rho
        y3 = np.where(t < 0, 0.0, t)
        rhs = rhs + (rho * Em.T.tocsr()) @ (P["f"] - y3) - Em.T @ np.zeros(len(P["f"]))
    return rhs


def precond_diag(P, prm):
    """The diagonal the first preconditioner is built from: 2 a_ii + rho1 + rho2 (+ rho3 Csq + rho4 Esq), as NumpyBqp.solve has it."""
    n, rho = P["n"], float(prm[6])
    d = (2 * csr(P["A"], n, n)).diagonal() + (rho + rho)
    if P.get("C") is not None:
        d = d + rho * col_sq(csr(P["C"], len(P["d"]), n))
    if P.get("E") is not None:
        d = d + rho * col_sq(csr(P["E"], len(P["f"]), n))
    return d


def assert_bqp_branch(name, P, prm, r):
    family = name.split("-")[0]
    if family == "zero_rhs":                            # B1 in iteration 0, then B4
        assert np.all(first_rhs(P, prm) == 0.0), name
        assert r.pcg[0] == 0 and np.all(r.state["x"] == 0.0) and r.state["cvg1"] == 0.0
    elif family == "tiny_b":
        s, tol, tag = fsum_sq(P["b"]), float(prm[9]), name[len("tiny_b-x"):name.rindex("-n")]
        assert np.all(np.asarray(P["x0"]) == 0.0)
        if tag == "1e-150":
            assert tol * tol * s >= D.DBL_MIN                               # the ordinary threshold
        elif tag == "1e-153":
            assert tol * tol * s < D.DBL_MIN <= s                           # B3: the clamp
        elif tag == "1e-160":
            assert 0.0 < s < D.DBL_MIN                                      # B2 under the clamped threshold: x stays y1 = 0
        else:
            assert s == 0.0                                                 # B1
        assert math.sqrt(fsum_sq(r.state["x"])) < FLOOR                     # B4
    elif family == "zero_precond_diag":                 # B5
        d = precond_diag(P, prm)
        assert np.array_equal(np.nonzero(d == 0.0)[0], D.zero_precond_rows(P)) and len(D.zero_precond_rows(P)) == 3, name
        assert set(D.zero_precond_rows(P)) <= set(D.empty_columns(P))
    elif family == "centre_start":                      # B6
        assert math.sqrt(fsum_sq(np.asarray(P["x0"]) - 0.5)) == 0.0
        assert np.isnan(r.state["x"]).all() and np.isnan(r.state["y2"]).all() and r.pcg == [int(prm[10])] * 2
    else:
        assert family == "scaled"
        assert np.isfinite(r.state["x"]).all()


@pytest.mark.parametrize("name", D.BQP_NAMES)
def test_bqp_case_is_pinned_and_enters_its_branch(name):
    P, prm = D.bqp_case(name)
    e = O.BqpOracle(P, params=prm)
    g = O.BqpOracle(P, params=prm, order=O.ORDER_GPU, T=256, chunk=512)
    r = NumpyBqp(P, params=prm)
    with np.errstate(invalid="ignore"):
        its = (e.solve(), g.solve(), r.solve())
    iters, stop, trace = D.BQP_PINS[name]
    assert its == (iters,) * 3, (name, its)
    assert (e.scalar("stop"), g.scalar("stop"), r.stop) == (stop,) * 3, name
    assert list(e.pcg_trace()) == list(g.pcg_trace()) == r.pcg == list(trace), (name, list(e.pcg_trace()), list(g.pcg_trace()), r.pcg)
    assert e.scalar("total_pcg") == g.scalar("total_pcg") == sum(trace)
    assert_bqp_branch(name, P, prm, r)
    # oracle against restatement: the three traces agree over the whole run, so the final state lies inside the agreeing prefix
    for o, tag in ((e, "eigen"), (g, "gpu")):
        for v in BQP_VECS:
            if v in r.state:
                assert_within_bound_nan(o.vec(v), r.state[v], e.vec(v), g.vec(v), f"{name} {tag} {v}")
        for v in BQP_SCALARS:
            if iters == 0 and v in ("obj_val", "cur_obj"):    # stopped inside iteration 0, before either is assigned (the restatement's
                continue                                      # placeholder is NaN, the oracle's 0: neither is a computed value)
            assert_within_bound_nan(o.scalar(v), r.state[v], e.scalar(v), g.scalar(v), f"{name} {tag} {v}")


# ---- segmentation --------------------------------------------------------------------------------------------------------------------
def seg_trio(P):
    e = O.SegOracle(0, P["n"], 0); e.set_problem(P); e.solve_init()
    g = O.SegOracle(0, P["n"], 0, order=O.ORDER_GPU); g.set_problem(P); g.solve_init()
    r = NumpySeg(P); r.solve_init()
    return e, g, r


def storage_predicate(P):
    """as_diagonals() and the rule around it restated: n >= 2, rows of at most 7 entries, a stored diagonal in every row, at most three
    distinct offsets either side, every off-diagonal value -w for an integer w in 0..255."""
    n = P["n"]
    i = np.repeat(np.arange(n), np.diff(P["rowptr"]))
    off = np.asarray(P["colidx"]) - i
    v = np.asarray(P["vals"], float)[off != 0]
    return bool(n >= 2 and np.diff(P["rowptr"]).max() <= 7 and np.all(np.bincount(i[off == 0], minlength=n) == 1)
                and len(set(off[off < 0])) <= 3 and len(set(off[off > 0])) <= 3
                and np.all((v <= 0.0) & (v >= -255.0) & (v == np.floor(v))))


def assert_seg_branch(name, P):
    assert storage_predicate(P) == D.seg_as_diagonals(name), name
    i = np.repeat(np.arange(P["n"]), np.diff(P["rowptr"]))
    diag = np.asarray(P["vals"])[np.asarray(P["colidx"]) == i]
    td = 2 * diag + (5.0 + 5.0)                         # the first preconditioner diagonal at rho1 = rho2 = 5
    if name.startswith("b-x"):
        s, tol, tag = fsum_sq(P["b"]), 1e-3, name[3:]
        if tag in ("0", "1e-310"):
            assert s == 0.0                                                 # B1
        elif tag == "1e-160":
            assert 0.0 < s < D.DBL_MIN                                      # B2 under the clamp
        elif tag == "1e-155":
            assert tol * tol * s < D.DBL_MIN <= s                           # B3
        else:
            assert tol * tol * s >= D.DBL_MIN
        if tag == "1e6":
            assert D.SEG_1E6_OBJ < -2147483648.0                            # the energy does not fit an int
    if name == "zero_td":                                                   # B5
        assert np.array_equal(np.nonzero(td == 0.0)[0], D.ZERO_TD_ROWS)
    else:
        assert np.all(td != 0.0)
    if name.startswith("weights255"):                                       # B7: large bytes in every band
        off = np.asarray(P["colidx"]) - i
        for o in set(off[off != 0]):
            w = -np.asarray(P["vals"])[off == o]
            assert w.max() == 255.0 and (P["n"] == 2 or {255.0, 128.0, 0.0} <= set(w)), (name, o)
    if name.startswith("boundary-") and name != "boundary-n1":
        base = banded_seg_problem(D.BOUNDARY_N, 9)
        k = base["rowptr"][D.BOUNDARY_AT[0]] + list(base["colidx"][base["rowptr"][D.BOUNDARY_AT[0]]:]).index(D.BOUNDARY_AT[1])
        want = {"m255": -255.0, "m256": -256.0, "mhalf": -0.5, "p1": 1.0, "mzero": -0.0, "pzero": 0.0}[name.split("-")[1]]
        got = P["vals"][k]
        assert got == want and np.signbit(got) == np.signbit(want) and np.array_equal(P["colidx"], base["colidx"])
        changed = np.nonzero(np.asarray(P["vals"]) != np.asarray(base["vals"]))[0]
        assert len(changed) <= 4                        # the entry, its mirror and the two diagonals


@pytest.mark.parametrize("name", D.SEG_NAMES)
def test_seg_case_window_is_pinned_and_enters_its_branch(name):
    P = D.seg_case(name)
    assert_seg_branch(name, P)
    e, g, r = seg_trio(P)
    z = np.zeros(P["n"])
    ret, trace = D.SEG_WINDOW_PINS[name]
    assert (e.solve_iter_l2f(0, 3, z, 0), g.solve_iter_l2f(0, 3, z, 0), r.solve_iter_l2f(0, 3, z, 0)) == (ret,) * 3, name
    assert list(e.pcg_trace()) == list(g.pcg_trace()) == r.pcg == list(trace), (name, list(e.pcg_trace()), r.pcg)
    if name.startswith("b-x") and name[3:] in D.SEG_FULL_SOLVE:            # B4: the iterate has no norm to speak of
        assert math.sqrt(fsum_sq(r.x)) < FLOOR and e.last_stop == g.last_stop == r.last_stop == 1
    k = len(trace)
    xe, xg, xr = e.get_x_iters_2d(10), g.get_x_iters_2d(10), r.get_x_iters_2d(10)
    for c in range(k):
        for got, tag in ((xe, "eigen"), (xg, "gpu")):
            assert_within_bound_nan(got[:, c], xr[:, c], xe[:, c], xg[:, c], f"{name} {tag} x_iters[{c}]")
    for o, tag in ((e, "eigen"), (g, "gpu")):
        for v in ("x", "z1", "z2", "b"):
            assert_within_bound_nan(o.vec(v), getattr(r, v), e.vec(v), g.vec(v), f"{name} {tag} {v}")
        for v in SEG_SCALARS:
            if ret and v in ("obj_val", "cur_obj", "std_obj"):             # a window that stops on the residual test never computes them
                continue
            assert_within_bound_nan(o.scalar(v), getattr(r, "std" if v == "std_obj" else v), e.scalar(v), g.scalar(v), f"{name} {tag} {v}")


@pytest.mark.parametrize("name", sorted(D.SEG_LEGACY_PINS))
def test_seg_legacy_solve_is_pinned(name):
    """The full legacy solves of the GPU file: a few iterations (b x 0 ... 1e-150), and b x 1e6, whose energy is below INT_MIN: the
    returned int is the defined out-of-range value on the oracle and on the restatement alike."""
    P = D.seg_case(name)
    e, g, r = seg_trio(P)
    energy, it1, stop, pcg_total = D.SEG_LEGACY_PINS[name]
    assert (e.solve_iter(), g.solve_iter(), r.solve_iter()) == (energy,) * 3
    assert (e.legacy_iter_plus1, g.legacy_iter_plus1, r.legacy_iter_plus1) == (it1,) * 3
    assert (e.last_stop, g.last_stop, r.last_stop) == (stop,) * 3
    assert (e.total_pcg_iters, g.total_pcg_iters, sum(r.pcg)) == (pcg_total,) * 3
    assert np.array_equal(e.get_x_sol().ravel(), r.get_x_sol()) and np.array_equal(g.get_x_sol().ravel(), r.get_x_sol())
    if name == "b-x1e6":
        assert energy == D.SEG_1E6_ENERGY_INT and e.get_obj() == g.get_obj() == D.SEG_1E6_OBJ
        assert r.cur_obj + r.c == D.SEG_1E6_OBJ


@pytest.mark.parametrize("name", D.SEG_FIX_CASES)
def test_seg_fix_step_is_pinned(name):
    """b := 2 Mb x2 + b with bytes up to 255, and td rebuilt on the live rows (a zero td row ends up non-zero or fixed)."""
    P = D.seg_case(name)
    e, g, r = seg_trio(P)
    z = np.zeros(P["n"])
    assert {s.solve_iter_l2f(*D.SEG_FIX_FIRST, z, 0) for s in (e, g, r)} == {0}
    assert list(e.pcg_trace()) == list(g.pcg_trace()) == r.pcg
    vec, num = D.seg_fix_vec(g.get_x_iters_2d(5)[:, 4])
    fixed, ret, trace = D.SEG_FIX_PINS[name]
    assert num == fixed and P["n"] // 3 == fixed                            # a third of the variables
    b_before = g.vec("b")
    assert {s.solve_iter_l2f(*D.SEG_FIX_SECOND, vec, num) for s in (e, g, r)} == {ret}
    assert list(e.pcg_trace()) == list(g.pcg_trace()) == r.pcg[-3:] == list(trace)
    assert e.get_n() == g.get_n() == r.n == P["n"] - fixed
    left = g.vec("left_idx").astype(int)
    assert np.array_equal(left, r.left_idx) and not np.array_equal(g.vec("b"), b_before[left])      # the shift moved b
    if name == "zero_td":
        assert set(D.ZERO_TD_ROWS) - set(left) and set(D.ZERO_TD_ROWS) & set(left)                  # zero-td rows fixed, and live
    for o, tag in ((e, "eigen"), (g, "gpu")):
        for v in ("x", "z1", "z2", "b"):
            assert_within_bound_nan(o.vec(v), getattr(r, v), e.vec(v), g.vec(v), f"{name} after the fix {tag} {v}")


# ---- non-finite data is refused on the host, before anything reaches a device -----------------------------------------------------------
BAD = (float("nan"), float("inf"), float("-inf"))


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def bqp_set_problem(L, h, P):
    keep = []

    def arr(v, dt):
        if v is None:
            return None
        keep.append(np.ascontiguousarray(v, dt))
        return _ptr(keep[-1])

    def mat(M):
        return [None] * 3 if M is None else [arr(M[0], np.int32), arr(M[1], np.int32), arr(M[2], np.float64)]
    m = len(P["d"]) if P.get("C") is not None else 0
    l = len(P["f"]) if P.get("E") is not None else 0
    return L.lpbox_bqp_set_problem(h, P["n"], *mat(P["A"]), arr(P["b"], np.float64), arr(P["x0"], np.float64), m, *mat(P.get("C")),
                                   arr(P.get("d"), np.float64), l, *mat(P.get("E")), arr(P.get("f"), np.float64))


def poisoned(P, key, at, bad):
    """A copy of the BQP problem P with entry `at` of the array `key` (A, C, E: of its stored values) replaced."""
    Q = dict(P)
    if key in ("A", "C", "E"):
        v = np.array(P[key][2], np.float64)
        v[at] = bad
        Q[key] = (P[key][0], P[key][1], v)
    else:
        v = np.array(P[key], np.float64)
        v[at] = bad
        Q[key] = v
    return Q


def stored_position(M, at):
    """(row, column) of the stored entry `at` of a CSR triple."""
    row = int(np.searchsorted(M[0], at, side="right") - 1)
    return row, int(M[1][at])


def test_bqp_set_problem_refuses_non_finite_data_and_stays_usable():
    from lpbox_hip import _lib
    L = _lib.load()
    P = bqp_problem(12, 3, 4, seed=2)
    h = C.c_void_p(L.lpbox_bqp_create(0))              # no device call before a solve
    try:
        for key in ("A", "b", "x0", "C", "d", "E", "f"):
            size = len(P[key][2]) if key in ("A", "C", "E") else len(P[key])
            for at in (0, size - 1):
                for bad in BAD:
                    assert bqp_set_problem(L, h, poisoned(P, key, at, bad)) == E_BADARG, (key, at, bad)
                    assert L.lpbox_last_status() == E_BADARG
                    msg = L.lpbox_last_error().decode()
                    if key in ("A", "C", "E"):
                        row, col = stored_position(P[key], at)
                        assert msg == f"{key} has a non-finite stored value (row {row}, column {col})", msg
                    else:
                        assert msg == f"{key} has a non-finite entry (index {at})", msg
                    assert L.lpbox_bqp_solve(h, None) == -3 and b"no problem set" in L.lpbox_last_error()      # nothing was kept
        assert bqp_set_problem(L, h, P) == 0            # the handle stays usable
        assert bqp_set_problem(L, h, poisoned(P, "b", 5, BAD[0])) == E_BADARG       # ... and a refused call leaves the problem that was set
        assert bqp_set_problem(L, h, P) == 0
    finally:
        L.lpbox_bqp_destroy(h)


def test_bqp_set_params_refuses_non_finite_values_and_keeps_the_old_ones():
    from lpbox_hip import _lib
    from lpbox_hip.bqp import PARAM_NAMES
    L = _lib.load()
    h = C.c_void_p(L.lpbox_bqp_create(0))
    try:
        good = np.array(bqp_params(3, 4), np.float64)
        assert L.lpbox_bqp_set_params(h, good) == 0
        for i, pname in enumerate(PARAM_NAMES):
            for bad in BAD:
                p = good.copy()
                p[i] = bad
                assert L.lpbox_bqp_set_params(h, p) == E_BADARG, (pname, bad)
                assert L.lpbox_last_error().decode() == f"params has a non-finite entry (index {i}, {pname})"
        assert L.lpbox_bqp_set_params(h, good) == 0
    finally:
        L.lpbox_bqp_destroy(h)


def seg_set_problem(L, h, P, c=None):
    return L.lpbox_set_problem_bqp(h, int(P["n"]), len(P["colidx"]), np.ascontiguousarray(P["rowptr"], np.int32),
                                   np.ascontiguousarray(P["colidx"], np.int32), np.ascontiguousarray(P["vals"], np.float64),
                                   np.ascontiguousarray(P["b"], np.float64), float(P["c"] if c is None else c), 1, int(P["n"]))


def test_seg_set_problem_refuses_non_finite_data_and_stays_usable():
    from lpbox_hip import _lib
    L = _lib.load()
    P = banded_seg_problem(30, 4)
    h = C.c_void_p(L.lpbox_create(_lib.FLAVOUR_SEG, 1, 0))
    try:
        for key in ("vals", "b"):
            for at in (0, len(P[key]) - 1):
                for bad in BAD:
                    v = np.array(P[key], np.float64)
                    v[at] = bad
                    assert seg_set_problem(L, h, dict(P, **{key: v})) == E_BADARG, (key, at, bad)
                    msg = L.lpbox_last_error().decode()
                    if key == "vals":
                        row, col = stored_position((P["rowptr"], P["colidx"]), at)
                        assert msg == f"vals has a non-finite stored value (row {row}, column {col})", msg
                    else:
                        assert msg == f"b has a non-finite entry (index {at})", msg
                    assert L.lpbox_init(h) == -3 and b"no problem set" in L.lpbox_last_error()
        for bad in BAD:
            assert seg_set_problem(L, h, P, c=bad) == E_BADARG and L.lpbox_last_error() == b"c is not finite"
        assert seg_set_problem(L, h, P) == 0            # the handle stays usable
    finally:
        L.lpbox_destroy(h)


def test_the_python_classes_raise_lpbox_error_with_the_code():
    from lpbox_hip.bqp import BqpSolver
    from lpbox_hip.lp import LpboxError
    from lpbox_hip.seg import PyLPboxADMMsolver
    P = bqp_problem(12, 3, 4, seed=2)
    for key, what in (("A", "A has a non-finite stored value"), ("b", "b has a non-finite entry"), ("x0", "x0 has"), ("C", "C has"),
                      ("d", "d has"), ("E", "E has"), ("f", "f has")):
        Q = poisoned(P, key, 1, float("nan"))
        with pytest.raises(LpboxError, match=what) as err:
            BqpSolver(Q["n"], Q["A"], Q["b"], Q["x0"], Q["C"], Q["d"], Q["E"], Q["f"])
        assert err.value.code == E_BADARG
    prm = bqp_params(3, 4)
    prm[9] = float("inf")
    with pytest.raises(LpboxError, match="pcg_tol") as err:
        BqpSolver(P["n"], P["A"], P["b"], P["x0"], P["C"], P["d"], P["E"], P["f"], params=prm)
    assert err.value.code == E_BADARG
    S = banded_seg_problem(30, 4)
    for key in ("vals", "b"):
        v = np.array(S[key], np.float64)
        v[3] = float("-inf")
        g = PyLPboxADMMsolver(0, S["n"], 0)
        with pytest.raises(LpboxError, match=f"{key} has a non-finite") as err:
            g.set_problem(dict(S, **{key: v}))
        assert err.value.code == E_BADARG
        g.set_problem(S)                                # the solver stays usable
        g.close()
