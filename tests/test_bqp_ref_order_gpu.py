"""GPU tests of the reference-order mode of the one-problem BQP chain (BqpSolver(order="reference"), lpbox_bqp_set_order; DESIGN.md
section 14.3).  Every comparison is against oracle/bqp_oracle.c in ORDER_EIGEN, the oracle's model of the reference: the vectors x,
y1, y2, z1..z4, y3, best_sol bit for bit, the scalars of EXACT_SCALARS exactly, std_obj within 2 ulps (sqrt where the reference
calls pow(v, 1/2), the bound of section 18).  The comparison sets come from tests/bqp_ref_cases.py, the problems and the oracle's
solves from tests/bqp_chain_ref_cases.py; tests/test_bqp_ref_order_api.py pins on the CPU that the oracle's two orders differ on them.

Run as a script (`python test_bqp_ref_order_gpu.py KIND NAME OUT.npy`) the file solves one case in reference order under the
environment as it stands and writes every result byte to OUT: the resume and eager-launch tests start it as a fresh child process
with LPBOX_BQP_KMAX / LPBOX_BQP_NOGRAPH set (a handle reads them when it is created)."""
import functools
import os
import subprocess
import sys
import time

import numpy as np
import pytest

if __name__ == "__main__":
    _ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_ROOT, os.path.join(_ROOT, "accelerated-lpbox-admm_amd")]

import bqp_chain_ref_cases as R
import bqp_ref_cases as K
from chain_cases import BQP_KMAX_START, bqp_case, bqp_case_params, expected_resumes
from helpers import bits_equal
from oracle import oracle as O

pytestmark = pytest.mark.gpu

CHILD_TAIL = ("pcg_resumes", "kmax", "launches", "order")


def hip(case, order="reference"):
    from lpbox_hip.bqp import BqpSolver
    P, preset, params = case
    g = BqpSolver(P["n"], P["A"], P["b"], P["x0"], P.get("C"), P.get("d"), P.get("E"), P.get("f"), preset=preset, params=list(params),
                  order=order)
    return g, g.solve()


def ulps_apart(a, b):
    a, b = np.array([a], np.float64), np.array([b], np.float64)
    assert np.isfinite(a).all() and np.isfinite(b).all() and a[0] >= 0 and b[0] >= 0
    return abs(int(a.view(np.int64)[0]) - int(b.view(np.int64)[0]))


def same_scalar(a, b):
    return bits_equal(np.array([a], np.float64), np.array([b], np.float64))


def check_against(g, it_g, P, ref, it_ref, tag, std_ulps=K.STD_OBJ_ULPS):
    """A solved handle against a solved oracle."""
    assert it_g == it_ref, f"{tag}: iterations {it_g} vs {it_ref}"
    for name in K.vec_names(P):
        got, want = g.vec(name), ref.vec(name)
        assert bits_equal(got, want), f"{tag} {name}: max diff {np.abs(got - want).max():.3e}"
    for name in K.EXACT_SCALARS:
        assert same_scalar(g.scalar(name), ref.scalar(name)), f"{tag} {name}: {g.scalar(name)!r} vs {ref.scalar(name)!r}"
    d = ulps_apart(g.scalar("std_obj"), ref.scalar("std_obj"))
    assert d <= std_ulps, f"{tag} std_obj: {d} ulps apart"


def all_bytes(g, P, it):
    parts = [np.array([it], np.float64)] + [g.vec(v) for v in K.vec_names(P)]
    parts.append(np.array([g.scalar(s) for s in K.EXACT_SCALARS + ("std_obj", "outer_total")]))
    return np.concatenate(parts).view(np.uint64)


def oracle_bytes(o, P, it):
    parts = [np.array([it], np.float64)] + [o.vec(v) for v in K.vec_names(P)]
    parts.append(np.array([o.scalar(s) for s in K.EXACT_SCALARS]))
    return np.concatenate(parts).view(np.uint64)


@functools.lru_cache(None)
def size_solved(n):
    return hip(R.size_case(n))


# ---- 1. the branches of the redux and the walker's tile edges ------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.SIZES)
def test_redux_branches_and_walker_tile_edges(n):
    assert {t + k for t in (R.WALK_TILE, 2 * R.WALK_TILE) for k in (-1, 0, 1)} | {R.WALK_TILE + 3, 2 * R.WALK_TILE + 2, 2 * R.WALK_TILE + 3,
                                                                                 3 * R.WALK_TILE + 1, 4 * R.WALK_TILE + 1} <= set(R.SIZES)
    g, it = size_solved(n)
    assert g.order == "reference" and g.scalar("order") == 1
    assert g.scalar("threads") == 256 and g.scalar("chunk") == 512
    o, it_o = R.size_oracle(n, O.ORDER_EIGEN)
    check_against(g, it, R.size_case(n)[0], o, it_o, f"n={n} vs the Eigen-order oracle")


# ---- 2. all four types, the edge shapes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(K.mixed_cases())))
def test_all_four_types_with_the_edge_shapes(i):
    M = K.mixed_cases()
    assert {t for _, t, _ in M} == {0, 1, 2, 3}
    assert {(P["n"], len(P.get("d", ())), len(P.get("f", ()))) for P, _, _ in M} >= {(257, 1, 0), (257, 0, 1), (257, 1, 1), (256, 0, 300), (200, 20, 260)}
    g, it = hip(M[i])
    o, it_o = K.eigen("mixed", i)
    check_against(g, it, M[i][0], o, it_o, f"mixed [{i}] n={M[i][0]['n']} vs the Eigen-order oracle")
    if i == 14:
        assert np.isfinite(g.vec("x")).all() and it == 3          # the indefinite operator


# ---- 3. problems to their own stops --------------------------------------------------------------------------------------------------
def test_problems_to_their_own_stops():
    S = K.stopping_cases()
    stops, its = [], []
    for i, case in enumerate(S):
        g, it = hip(case)
        o, it_o = K.eigen("stopping", i)
        check_against(g, it, case[0], o, it_o, f"stopping [{i}] vs the Eigen-order oracle")
        stops.append(int(g.scalar("stop"))); its.append(it)
        if i == K.SEED1_INDEX:                                     # the answer of the reference's order, not the default order's
            assert g.scalar("best_bin_obj") == K.SEED1_BEST_BIN_OBJ[O.ORDER_EIGEN] != K.SEED1_BEST_BIN_OBJ[O.ORDER_GPU]
    assert set(stops) == {0, 1, 2} and max(its) == 10000 and min(its) == 8, (its, stops)


# ---- 4. above the batch limit --------------------------------------------------------------------------------------------------------
def test_above_the_batch_limit_ends_on_the_reference_answer():
    """bqp_problem(2100, 64, 64, seed=1), preset 3, to its stop at the 10^4-iteration cap: 147.6795702348325, not the default order's
    148.33867126179442.  BqpBatch refuses the problem (n > 2048)."""
    case = R.big_case()
    t0 = time.perf_counter()
    g, it = hip(case)
    wall = time.perf_counter() - t0
    print(f"n=2100 to the cap: wall {wall:.2f} s, kernel {g.scalar('kernel_ms'):.0f} ms, {g.scalar('launches'):.0f} launches, "
          f"pcg_resumes {g.scalar('pcg_resumes'):.0f}, kmax {g.scalar('kmax'):.0f}")
    o, it_o = R.big_oracle(O.ORDER_EIGEN)
    assert g.scalar("best_bin_obj") == R.BIG_BEST_BIN_OBJ[O.ORDER_EIGEN] != R.BIG_BEST_BIN_OBJ[O.ORDER_GPU]
    assert bits_equal(g.vec("best_sol"), o.vec("best_sol"))
    check_against(g, it, case[0], o, it_o, "n=2100 vs the Eigen-order oracle")
    assert it == 10000 and g.scalar("total_pcg") == R.BIG_PCG_STEPS[O.ORDER_EIGEN]


# ---- 5. halt and resume, in fresh child processes ------------------------------------------------------------------------------------
def run_child(tmp_path, kind, name, env_extra):
    assert not any(os.environ.get(k) for k in ("LPBOX_BQP_KMAX", "LPBOX_BQP_NOGRAPH"))
    out = str(tmp_path / f"{kind}_{name}.npy")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), kind, str(name), out], env=dict(os.environ, **env_extra),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.load(out)
    return got[:-len(CHILD_TAIL)], dict(zip(CHILD_TAIL, (int(v) for v in got[-len(CHILD_TAIL):])))


@pytest.mark.parametrize("kmax", [1, None])
def test_halt_and_resume(tmp_path, kmax):
    """G4 of tests/chain_cases.py: 31 ... 17 PCG iterations per outer iteration.  One launch group per iteration: every iteration halts
    and is resumed, the walkers behind the halt fall through and the resumed PCG finds the sums of its last update.  No knob: the
    chain starts at 12 groups, iteration 0 halts at least twice."""
    P, _ = bqp_case("G4")
    params = bqp_case_params("G4")
    o = O.BqpOracle(P, params=params, order=O.ORDER_EIGEN)
    it_o = o.solve()
    trace = [int(k) for k in o.pcg_trace()]
    got, tail = run_child(tmp_path, "chain", "G4", {"LPBOX_BQP_KMAX": str(kmax)} if kmax else {})
    want = oracle_bytes(o, P, it_o)
    assert np.array_equal(got[:len(want)], want), "G4 in the child vs the Eigen-order oracle"
    std_obj = float(got[len(want):len(want) + 1].view(np.float64)[0])
    assert ulps_apart(std_obj, o.scalar("std_obj")) <= K.STD_OBJ_ULPS and tail["order"] == 1
    print(f"G4 kmax {kmax}: pcg_resumes {tail['pcg_resumes']}, kmax after {tail['kmax']}, launches {tail['launches']}")
    if kmax:
        assert tail["pcg_resumes"] == expected_resumes(trace, kmax) > 30 and tail["kmax"] == kmax
    else:
        # the adaptive chain, from the trace and the rules of lpbox_chain.h (CHAIN_RULES_GEN: start 12, 16 groups per resume, halt bump 8,
        # margin 1, 16 iterations per batch).  Iteration 0 halts at 12 and at 28 groups (31 > 28): two resumes, kmax max(12 + 8, 28 + 8) =
        # 36, which the other 15 iterations of the first batch stay below; the second and last batch (30 iterations in all) runs at the
        # largest count of the first + 1 = 32, which nothing there reaches.  So: exactly two resumes, kmax 32 at the end.
        batch = 16
        assert len(trace) == 30 and trace[0] == max(trace) == 31 and max(trace[1:batch]) <= 36 and max(trace[batch:]) <= max(trace[:batch]) + 1
        assert expected_resumes(trace[:1], BQP_KMAX_START) == 2
        assert tail["pcg_resumes"] == 2 and tail["kmax"] == max(trace[:batch]) + 1 == 32


# ---- 6. above 2^21 variables: four slots per thread in the producers, a walk of 2049 tiles -------------------------------------------
def test_above_2_pow_21_variables():
    case = R.two_pow_21_case()
    P = case[0]
    g, it = hip(case)
    assert g.scalar("chunk") == 1024 and g.scalar("threads") == 256 and g.scalar("order") == 1
    o, it_o = K.solve_oracle(case, O.ORDER_EIGEN)
    check_against(g, it, P, o, it_o, "n > 2^21 vs the Eigen-order oracle")
    assert it == 2 and g.scalar("total_pcg") > 0


# ---- 7. one handle, both orders ------------------------------------------------------------------------------------------------------
def test_one_handle_both_orders():
    import ctypes as C
    n = 1025
    case = R.size_case(n)
    P = case[0]
    g, it = hip(case)
    first = all_bytes(g, P, it)
    g.set_order("default")
    assert g.order == "default"
    v = C.c_double()
    assert g.scalar("order") == 0                                           # the setting follows the switch at once ...
    assert g._L.lpbox_bqp_get_scalar(g._h, b"best_bin_obj", C.byref(v)) < 0 # ... and the other order's results are refused until a solve
    it_d = g.solve()
    assert g.scalar("order") == 0 and (g.scalar("threads"), g.scalar("chunk")) == (256, 512)
    o, it_o = R.size_oracle(n, O.ORDER_GPU)
    check_against(g, it_d, P, o, it_o, f"default order n={n} vs the kernel-order oracle", std_ulps=0)
    assert not np.array_equal(all_bytes(g, P, it_d), first)
    assert g._L.lpbox_bqp_set_order(g._h, 2) == -2 and g.scalar("order") == 0      # LPBOX_E_BADARG leaves the handle as it was
    g.set_order("reference")
    assert g.scalar("order") == 1
    it2 = g.solve()
    assert g.scalar("order") == 1 and np.array_equal(all_bytes(g, P, it2), first)
    e, it_e = R.size_oracle(n, O.ORDER_EIGEN)
    check_against(g, it2, P, e, it_e, f"reference order again, n={n}")


# ---- 8. against the batch: two implementations of one association ---------------------------------------------------------------------
def test_same_bits_as_the_batch_in_reference_order():
    from lpbox_hip.bqp import BqpBatch
    sizes = (7, 513, 2048)
    cases = [R.size_case(n) for n in sizes]
    B = BqpBatch([P for P, _, _ in cases], presets=[t for _, t, _ in cases], params=[list(p) for _, _, p in cases], order="reference")
    its = B.solve()
    for i, n in enumerate(sizes):
        g, it = size_solved(n)
        assert it == its[i]
        for name in K.vec_names(cases[i][0]):
            assert bits_equal(g.vec(name), B.vec(i, name)), f"n={n} {name}"
        for name in K.EXACT_SCALARS + ("std_obj",):
            assert same_scalar(g.scalar(name), B.scalar(i, name)), f"n={n} {name}"


# ---- 9. eager launches ---------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_graph_replay(tmp_path):
    n = 2049
    g, it = size_solved(n)
    got, tail = run_child(tmp_path, "size", n, {"LPBOX_BQP_NOGRAPH": "1"})
    assert np.array_equal(got, all_bytes(g, R.size_case(n)[0], it))
    assert tail["order"] == 1 and tail["launches"] == g.scalar("launches") and tail["pcg_resumes"] == g.scalar("pcg_resumes")


def _child(kind, name, out):
    if kind == "chain":
        P, t = bqp_case(name)
        case = (P, None, tuple(bqp_case_params(name)))
    else:
        case = R.size_case(int(name))
    g, it = hip(case)
    tail = np.array([g.scalar(s) for s in CHILD_TAIL]).astype(np.uint64)
    np.save(out, np.concatenate([all_bytes(g, case[0], it), tail]))


if __name__ == "__main__":
    _child(*sys.argv[1:4])
