"""CPU tests of the lockstep batch of generic BQPs (lpbox_bqp_lockstep_*, lpbox_hip.bqp.BqpLockstep / solve_large_many / solve_any): the
declarations, what _create refuses without a device, solve_any's partition on stub results, and the oracle pins
tests/test_bqp_lockstep_gpu.py rests on -- so that a later change to a helper cannot turn its batches into ones whose members all end
alike, whose chain never halts or whose best_sol copy is never due."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bqp_lockstep_cases as BC
from chain_cases import BQP_KMAX_START, PAIRS_PER_RESUME, expected_resumes

E_BADARG, E_STATE, E_NODEVICE, E_UNSUPPORTED = -2, -3, -6, -7
NAMES = ["lpbox_bqp_lockstep_create", "lpbox_bqp_lockstep_destroy", "lpbox_bqp_lockstep_solve", "lpbox_bqp_lockstep_get_scalar"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def solver(P, params=None, **kw):
    from lpbox_hip.bqp import BqpSolver
    return BqpSolver(P["n"], P["A"], P["b"], P["x0"], P.get("C"), P.get("d"), P.get("E"), P.get("f"), params=params, **kw)


def test_header_declares_library_exports_python_binds():
    from lpbox_hip import _lib, bqp
    header = open(os.path.join(ROOT, "include", "lpbox_hip.h")).read()
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), f"include/lpbox_hip.h does not declare {name}"
        assert hasattr(lib, name), f"liblpbox_hip.so does not export {name}"
        assert name in _lib.SYMBOLS
    assert "typedef struct lpbox_bqp_lockstep lpbox_bqp_lockstep_t;" in header
    assert hasattr(bqp, "BqpLockstep") and hasattr(bqp, "solve_large_many") and hasattr(bqp, "solve_any")


def test_argument_errors_come_before_the_library(monkeypatch):
    from lpbox_hip import _lib
    from lpbox_hip.bqp import BqpLockstep, solve_any, solve_large_many

    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_load)
    P = BC.extents()[0][0]
    for bad in ([], None):
        with pytest.raises(ValueError):
            BqpLockstep(bad)
    with pytest.raises(TypeError, match="member 1"):
        BqpLockstep([P, "not a problem"])
    with pytest.raises(TypeError, match="member 0"):
        BqpLockstep([dict(n=3, b=[0, 0, 0])])
    with pytest.raises(ValueError):
        BqpLockstep([P, P], presets=[0])
    with pytest.raises(ValueError):
        solve_large_many([])
    with pytest.raises(ValueError):
        solve_any([])
    with pytest.raises(TypeError, match="problem 1"):
        solve_any([P, 7])


def test_create_refuses_without_a_device_call():
    from lpbox_hip import _lib
    from lpbox_hip._lib import LpboxError
    from lpbox_hip.bqp import BqpLockstep
    L = _lib.load()
    (P0, p0), (P1, p1) = BC.extents()[0], BC.extents()[1]
    assert not L.lpbox_bqp_lockstep_create(None, 0)
    assert L.lpbox_last_status() == E_BADARG and b"empty" in L.lpbox_last_error()
    a, b = solver(P0, p0), solver(P1, p1)
    assert not L.lpbox_bqp_lockstep_create((C.c_void_p * 1)(a._h), 0)
    assert L.lpbox_last_status() == E_BADARG and b"empty" in L.lpbox_last_error()
    assert not L.lpbox_bqp_lockstep_create(None, 2)
    assert L.lpbox_last_status() == E_BADARG

    def refused(members):
        with pytest.raises(LpboxError) as e:
            BqpLockstep(members)
        return e.value

    e = refused([a, b, a])
    assert e.code == E_BADARG and "problem 0 and problem 2" in str(e) and "same handle" in str(e)
    e = refused([a, solver(P1, p1, device=1)])
    assert e.code == E_BADARG and "problem 1" in str(e) and "another device" in str(e)
    raw = C.c_void_p(L.lpbox_bqp_create(0))                  # a handle without a problem
    assert not L.lpbox_bqp_lockstep_create((C.c_void_p * 3)(a._h, b._h, raw), 3)
    assert L.lpbox_last_status() == E_STATE and b"problem 2" in L.lpbox_last_error() and b"no problem" in L.lpbox_last_error()
    L.lpbox_bqp_destroy(raw)
    assert not L.lpbox_bqp_lockstep_create((C.c_void_p * 2)(a._h, None), 2)      # a null member
    assert L.lpbox_last_status() == E_STATE and b"problem 1" in L.lpbox_last_error()
    e = refused([a, solver(P1, p1, order="reference")])
    assert e.code == E_UNSUPPORTED and "problem 1" in str(e) and "reference summation order" in str(e)
    e = refused([solver(P1, p1, order="reference"), a])
    assert e.code == E_UNSUPPORTED and "problem 0" in str(e)

    B = BqpLockstep([a, b])                                  # and now it is accepted -- without a device call
    assert len(B) == 2 and B[1] is b and B.scalar("count") == 2.0 and B.scalar("pcg_resumes_1") == 0.0
    assert B.scalar("graph") == 0.0 and B.scalar("launches") == 0.0 and B.scalar("kmax") == float(BQP_KMAX_START)
    for name in ("pcg_resumes_2", "pcg_resumes_", "pcg_resumes_x", "nothing"):
        with pytest.raises(LpboxError) as e:
            B.scalar(name)
        assert e.value.code == E_BADARG
    b.set_order("reference")                                 # a member changed after create: the solve refuses before anything changes
    with pytest.raises(LpboxError) as e:
        B.solve()
    assert e.value.code == E_UNSUPPORTED and "problem 1" in str(e.value)
    b.set_order("default")
    if L.lpbox_device_count() < 1:                           # no CPU fallback
        with pytest.raises(LpboxError, match="no HIP device") as e:
            B.solve()
        assert e.value.code == E_NODEVICE
    B.close()
    assert a.scalar("order") == 0.0                          # the members are still there: borrowed, not closed with the batch
    assert L.lpbox_bqp_lockstep_solve(None, None) < 0 and L.lpbox_bqp_lockstep_get_scalar(None, b"count", C.byref(C.c_double())) < 0
    L.lpbox_bqp_lockstep_destroy(None)


def test_members_built_by_the_batch_take_presets_and_params_and_close_with_it():
    from lpbox_hip.bqp import BqpLockstep, BqpSolver
    (P0, p0), (P1, p1) = BC.extents()[0], BC.extents()[1]
    B = BqpLockstep([P0, (P1["n"], P1["A"], P1["b"], P1["x0"], P1["C"], P1["d"])], params=[p0, p1])
    assert all(isinstance(s, BqpSolver) for s in B.solvers) and (B[1].n, B[1].m, B[1].l) == (255, 1, 0)
    B.close()
    assert B[0]._h is None and B[1]._h is None
    mine = solver(P0, p0)
    B = BqpLockstep([mine, P1])
    B.close()
    assert mine._h is not None and B[1]._h is None


# ---- the oracle pins behind the GPU file ---------------------------------------------------------------------------------------------
def test_extents_batch_covers_the_grid_edges():
    G = [BC.groups(P) for (P, _) in BC.extents()]
    assert [g[0] for g in G] == [1, 1, 1, 2, 3, 4]
    assert {BC.ptype_of(P) for (P, _) in BC.extents()} == {0, 1, 2, 3}
    dims = [(P["n"], len(P.get("d", ())), len(P.get("f", ()))) for (P, _) in BC.extents()]
    assert any(m == 1 for (_, m, _) in dims) and any(l == 1 for (_, _, l) in dims)
    assert any(g[2] > g[0] for g in G) and any(g[1] > 1 and g[2] == 0 for g in G)      # Gl > G: the y and rows extents; Gm = 2 beside no E
    assert len({max(g[0], g[2], 1) for g in G}) > 1 and len({max(g[1], g[2], 1) for g in G}) > 1
    for r in BC.oracle_runs("extents"):
        assert r["iterations"] == BC.EXTENTS_K and r["stop"] == 0 and len(r["trace"]) == BC.EXTENTS_K and min(r["trace"]) >= 1


STOP_ENDS = [(54, 1), (120, 1), (33, 2), (26, 2), (7, 0), (19, 0), (40, 0)]       # (iterations, stop): 1 x/y, 2 objective std, 0 max_iters


def test_stop_members_end_pairwise_differently_by_all_three_ends():
    runs = BC.oracle_runs("stops")
    assert [(r["iterations"], int(r["stop"])) for r in runs] == STOP_ENDS
    assert len({r["iterations"] for r in runs}) == len(runs)
    assert {int(r["stop"]) for r in runs} == {0, 1, 2}
    params = [p for (_, p) in BC.stops()]
    ended_by_cap = [(r["iterations"], p[5]) for r, p in zip(runs, params) if r["stop"] == 0]
    assert all(it == cap for it, cap in ended_by_cap) and len({cap for _, cap in ended_by_cap}) >= 2
    assert all(r["iterations"] < p[5] for r, p in zip(runs, params) if r["stop"] != 0)
    assert {BC.groups(P)[0] for (P, _) in BC.stops()} == {1, 2}
    for r in runs:                                                                  # no halt at the starting kmax: the ends alone are under test
        assert max(r["trace"]) <= BQP_KMAX_START


def test_best_member_improves_in_its_last_iteration():
    """The member whose best_sol copy is due after the loop: it ends at its max_iters, and that last iteration lowered best_bin_obj."""
    i = BC.BEST_MEMBER
    last, before = BC.oracle_runs("stops")[i], BC.oracle_run_with("stops", i, STOP_ENDS[i][0] - 1)
    assert last["stop"] == 0 and last["iterations"] == before["iterations"] + 1
    assert last["cur_obj"] == last["best_bin_obj"] < before["best_bin_obj"]
    assert np.array_equal(last["best_sol"], last["x"]) and not np.array_equal(last["best_sol"], before["best_sol"])
    assert not np.array_equal(before["x"], last["x"])


def test_resume_members_halt_under_the_forced_counts():
    runs = BC.oracle_runs("resume")
    assert [r["iterations"] for r in runs] == [30, 30, 30]
    for r in runs:
        assert min(r["trace"]) > 3                                                  # kmax 1 and 3: every iteration of every member halts
    want = {k: [expected_resumes(r["trace"], k) for r in runs] for k in (1, 3)}
    assert want[1] == [59, 30, 30] and want[3] == [54, 30, 30]                      # G4: one or two resumes per iteration, the others one
    g4 = runs[0]["trace"]
    assert g4[0] > BQP_KMAX_START + PAIRS_PER_RESUME and max(runs[1]["trace"]) < BQP_KMAX_START   # adaptive: G4 halts twice at once, G1 never
    assert len({r["total_pcg"] for r in runs}) == 3


def test_many_and_wide_members():
    many = BC.many()
    assert len(many) == 300 and max(P["n"] for (P, _) in many) <= 64 and min(P["n"] for (P, _) in many) == 2
    assert {BC.ptype_of(P) for (P, _) in many} == {0, 1, 2, 3}
    assert all(r["iterations"] == BC.MANY_K for r in BC.oracle_runs("many"))
    (P, p), (Q, q) = BC.wide()
    assert (P["n"], len(P["d"]), len(P["f"]), Q["n"]) == (2100, 64, 64, 2) and p[5] == q[5] == BC.WIDE_K
    assert BC.groups(P) == (5, 1, 1) and BC.groups(Q) == (1, 0, 0)
    assert [r["iterations"] for r in BC.oracle_runs("wide")] == [30, 30]


# ---- solve_any: partition and ordering, on stub results ------------------------------------------------------------------------------
def test_solve_any_partitions_by_size_and_keeps_the_order(monkeypatch):
    from lpbox_hip import bqp

    def prob(n, m=0, l=0):
        P = dict(n=n, A="A%d" % n, b="b", x0="x0")
        if m:
            P.update(C="C", d=[0.0] * m)
        if l:
            P.update(E="E", f=[0.0] * l)
        return P
    problems = [prob(40), prob(2049), prob(2048, 2048, 2048), prob(10, 2049), prob(2048), prob(7, 0, 5000), prob(3)]
    assert bqp.split_by_size(problems) == ([0, 2, 4, 6], [1, 3, 5])
    calls = []

    def stub(tag):
        def run(ps, presets=None, params=None, device=0):
            calls.append((tag, [P["n"] for P in ps], list(presets), list(params), device))
            return [dict(route=tag, n=P["n"], m=len(P.get("d", ()))) for P in ps]
        return run
    monkeypatch.setattr(bqp, "solve_many", stub("batch"))
    monkeypatch.setattr(bqp, "solve_large_many", stub("lockstep"))
    presets = [0, 0, 3, 1, 0, 2, 0]
    params = [[float(k)] * 11 for k in range(7)]
    out = bqp.solve_any(problems, presets=presets, params=params, device=2)
    assert [(s["route"], s["n"], s["m"]) for s in out] == [("batch", 40, 0), ("lockstep", 2049, 0), ("batch", 2048, 2048), ("lockstep", 10, 2049),
                                                          ("batch", 2048, 0), ("lockstep", 7, 0), ("batch", 3, 0)]
    assert calls == [("batch", [40, 2048, 2048, 3], [0, 3, 0, 0], [params[0], params[2], params[4], params[6]], 2),
                     ("lockstep", [2049, 10, 7], [0, 1, 2], [params[1], params[3], params[5]], 2)]
    calls.clear()
    out = bqp.solve_any(problems[:1] + problems[4:5])                               # nothing for the lockstep batch: it is not built
    assert [c[0] for c in calls] == ["batch"] and calls[0][2] == [None, None] and [s["n"] for s in out] == [40, 2048]
    calls.clear()
    out = bqp.solve_any([problems[1]], presets=0)
    assert [c[0] for c in calls] == ["lockstep"] and calls[0][2] == [0] and out[0]["n"] == 2049
