"""GPU tests of the reference-order mode of the BQP batch (BqpBatch(order="reference"), lpbox_bqp_batch_set_order; DESIGN.md section
14.2).  Every comparison is against oracle/bqp_oracle.c in ORDER_EIGEN, the oracle's model of the reference: the vectors x, y1, y2,
z1..z4, y3, best_sol bit for bit, the scalars of EXACT_SCALARS exactly, std_obj within 2 ulps (sqrt where the reference calls
pow(v, 1/2), the bound of section 18).  The problems and the oracle's solves live in tests/bqp_ref_cases.py;
tests/test_bqp_batch_ref_order_api.py pins on the CPU that the oracle's two orders differ on them.

Run as a script (`python test_bqp_batch_ref_order_gpu.py OUT.npy`) the file solves the eight-slot size batch in reference order and
writes every result byte to OUT: the window test starts it as a fresh child process with LPBOX_BQP_BATCH_WINDOW=3."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    _ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_ROOT, os.path.join(_ROOT, "accelerated-lpbox-admm_amd")]

import bqp_ref_cases as K
from helpers import BQP_SCALARS, assert_within_bound, bits_equal, common_prefix
from oracle import oracle as O
from oracle.bqp_numpy import NumpyBqp

pytestmark = pytest.mark.gpu


def batch_of(cases, order="reference"):
    from lpbox_hip.bqp import BqpBatch
    return BqpBatch([P for P, _, _ in cases], presets=[t for _, t, _ in cases], params=[list(p) for _, _, p in cases], order=order)


def ulps_apart(a, b):
    a, b = np.array([a], np.float64), np.array([b], np.float64)
    assert np.isfinite(a).all() and np.isfinite(b).all() and a[0] >= 0 and b[0] >= 0
    return abs(int(a.view(np.int64)[0]) - int(b.view(np.int64)[0]))


def same_scalar(a, b):
    return bits_equal(np.array([a], np.float64), np.array([b], np.float64))


def check_against(B, i, its, P, ref, it_ref, tag, std_ulps=K.STD_OBJ_ULPS):
    """Problem i of the solved batch B against a solved oracle."""
    assert int(its[i]) == it_ref, f"{tag}: iterations {its[i]} vs {it_ref}"
    for name in K.vec_names(P):
        got, want = B.vec(i, name), ref.vec(name)
        assert bits_equal(got, want), f"{tag} {name}: max diff {np.abs(got - want).max():.3e}"
    for name in K.EXACT_SCALARS:
        assert same_scalar(B.scalar(i, name), ref.scalar(name)), f"{tag} {name}: {B.scalar(i, name)!r} vs {ref.scalar(name)!r}"
    d = ulps_apart(B.scalar(i, "std_obj"), ref.scalar("std_obj"))
    assert d <= std_ulps, f"{tag} std_obj: {d} ulps apart"


def check_group(B, its, group, picks=None):
    cases = K.cases(group)
    for i in (range(len(cases)) if picks is None else picks):
        o, it_o = K.eigen(group, i)
        check_against(B, i, its, cases[i][0], o, it_o, f"{group} [{i}] n={cases[i][0]['n']} vs the Eigen-order oracle")


def all_bytes(B, cases, its):
    parts = [np.asarray(its, np.float64)]
    for i, (P, _, _) in enumerate(cases):
        parts += [B.vec(i, v) for v in K.vec_names(P)]
        parts.append(np.array([B.scalar(i, s) for s in K.EXACT_SCALARS + ("std_obj", "outer_total")]))
    return np.concatenate(parts).view(np.uint64)


@functools.lru_cache(maxsize=None)
def redux_solved(group):
    B = batch_of(K.cases(group))
    its = B.solve()
    return B, its


# ---- 1. the branches of the redux, in each slot count ---------------------------------------------------------------------------------
@pytest.mark.parametrize("group", ["slots2", "slots4", "slots8"])
def test_redux_branches_in_each_slot_count(group):
    B, its = redux_solved(group)
    assert B.order == "reference" and B.scalar(0, "order") == 1 and B.scalar(0, "slots") == K.REDUX_SLOTS[group]
    assert B.scalar(0, "threads") == 256 and B.scalar(0, "chunk") == 512
    assert [d[0] for d in B.dims] == list(K.REDUX_SIZES[group]) and max(its) == K.REDUX_K
    check_group(B, its, group)


# ---- 2. all four types in one batch ---------------------------------------------------------------------------------------------------
def test_all_four_types_with_the_edge_shapes():
    M = K.mixed_cases()
    assert {t for _, t, _ in M} == {0, 1, 2, 3}
    assert {(P["n"], len(P.get("d", ())), len(P.get("f", ()))) for P, _, _ in M} >= {(257, 1, 0), (257, 0, 1), (257, 1, 1), (256, 0, 300), (200, 20, 260)}
    for key in ("C", "E"):                                   # the empty row and column, the row lengths 1, 2, 3 mod 4, values of both signs
        P = M[13][0]
        lens = np.diff(P[key][0])
        assert lens[0] == 0 and {1, 2, 3} <= set(lens % 4) and 299 not in set(P[key][1]) and np.any(P[key][2] < 0)
    B = batch_of(M)
    its = B.solve()
    assert B.scalar(0, "slots") == 2
    check_group(B, its, "mixed")
    assert np.isfinite(B.vec(14, "x")).all() and its[14] == 3      # the indefinite operator


# ---- 3. problems to their own stops ---------------------------------------------------------------------------------------------------
def test_problems_to_their_own_stops():
    S = K.stopping_cases()
    B = batch_of(S)
    its = B.solve()
    check_group(B, its, "stopping")
    stops = [int(B.scalar(i, "stop")) for i in range(B.count)]
    assert set(stops) == {0, 1, 2} and max(its) == 10000 and min(its) == 8, (list(its), stops)
    assert B.scalar(0, "launches") >= 1 + -(-10000 // B.scalar(0, "window"))
    i = K.SEED1_INDEX                                          # the answer of the reference's order, not the default order's
    assert B.scalar(i, "best_bin_obj") == K.SEED1_BEST_BIN_OBJ[O.ORDER_EIGEN] != K.SEED1_BEST_BIN_OBJ[O.ORDER_GPU]


# ---- 4. window independence -----------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_the_window(tmp_path):
    """The eight-slot size batch again in a fresh process with 3 outer iterations per launch, byte for byte."""
    B, its = redux_solved("slots8")
    assert B.scalar(0, "window") != 3
    want = all_bytes(B, K.cases("slots8"), its)
    out = str(tmp_path / "slots8_w3.npy")
    env = dict(os.environ, LPBOX_BQP_BATCH_WINDOW="3")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.load(out)
    assert got[-1] == 3 and got[-2] == 1 + -(-int(max(its)) // 3)      # the window the child ran with, and its launches (init + 20 windows)
    assert np.array_equal(got[:-2], want)


# ---- 5. one handle, both orders -------------------------------------------------------------------------------------------------------
def test_one_handle_both_orders():
    cases = K.cases("slots2")
    B = batch_of(cases)
    its = B.solve()
    first = all_bytes(B, cases, its)
    B.set_order("default")
    assert B.order == "default"
    import ctypes as C
    v = C.c_double()
    assert B._L.lpbox_bqp_batch_get_scalar(B._h, 0, b"order", C.byref(v)) < 0       # set_order marks the batch as not solved
    its_d = B.solve()
    assert B.scalar(0, "order") == 0
    for i, (P, _, _) in enumerate(cases):
        o, it_o = K.kernel_order("slots2", i)
        check_against(B, i, its_d, P, o, it_o, f"default order [{i}] n={P['n']} vs the kernel-order oracle", std_ulps=0)
    assert B._L.lpbox_bqp_batch_set_order(B._h, 2) == -2 and B.scalar(0, "order") == 0      # LPBOX_E_BADARG leaves the batch as it was
    B.set_order("reference")
    its2 = B.solve()
    assert B.scalar(0, "order") == 1 and np.array_equal(all_bytes(B, cases, its2), first)
    check_group(B, its2, "slots2")


# ---- 6. more problems than compute units ----------------------------------------------------------------------------------------------
def test_300_problems_at_once():
    from lpbox_hip.bqp import solve_many
    cases = K.many_cases()
    B = batch_of(cases)
    its = B.solve()
    assert B.count == 300
    check_group(B, its, "many", K.MANY_CHECKED)
    sols = solve_many([P for P, _, _ in cases[:3]], params=[list(p) for _, _, p in cases[:3]], order="reference")
    assert all(bits_equal(sols[i]["x_sol"], B.vec(i, "x")) and sols[i]["iterations"] == its[i] for i in range(3))


# ---- 7. not pinned to the C oracle alone: the numpy restatement -----------------------------------------------------------------------
def test_one_problem_within_the_bound_of_the_restatement():
    """The state after the prefix over which the PCG counts of the two oracle orders and the restatement agree, within B of
    oracle/bqp_numpy.py (tests/test_oracle_restatement.py states the rule)."""
    P, t, params = K.mixed_cases()[K.RESTATEMENT_PICK]
    e, _ = K.eigen("mixed", K.RESTATEMENT_PICK)
    g, _ = K.kernel_order("mixed", K.RESTATEMENT_PICK)
    r = NumpyBqp(P, params=list(params))
    r.solve(record=True)
    k = common_prefix(g.pcg_trace(), e.pcg_trace(), r.pcg)
    assert k >= 4, f"PCG counts agree over {k} iterations only: {list(e.pcg_trace())} vs {r.pcg}"
    prm = list(params); prm[5] = k
    case = (P, t, tuple(prm))
    B = batch_of([case])
    its = B.solve()
    (e, it_e), (g, _) = K.solve_oracle(case, O.ORDER_EIGEN), K.solve_oracle(case, O.ORDER_GPU)
    check_against(B, 0, its, P, e, it_e, f"prefix k={k}")
    snap = r.trace[k - 1]
    for name in K.vec_names(P):
        assert_within_bound(B.vec(0, name), snap[name], e.vec(name), g.vec(name), f"k={k} {name}")
    for name in BQP_SCALARS:
        assert_within_bound(B.scalar(0, name), snap[name], e.scalar(name), g.scalar(name), f"k={k} {name}")


def _child(out):
    B, its = redux_solved("slots8")
    tail = np.array([B.scalar(0, "launches"), B.scalar(0, "window")]).astype(np.uint64)
    np.save(out, np.concatenate([all_bytes(B, K.cases("slots8"), its), tail]))


if __name__ == "__main__":
    _child(sys.argv[1])
