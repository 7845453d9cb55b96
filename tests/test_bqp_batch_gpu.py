"""GPU tests of the batch of small generic constrained BQPs (lpbox_hip.bqp.BqpBatch, lpbox_bqp_batch_*): one persistent workgroup per
problem.  Every comparison has two references: oracle/bqp_oracle.c in the kernels' order (T = threads, chunk = chunk as the batch
reports them) and a BqpSolver (the large-instance kernel chain) on the same problem in the same process -- bitwise on every vector
that exists for the type and on the scalars, equality on iters / stop / total_pcg.  Three problems are also held within B of the
numpy restatement oracle/bqp_numpy.py over the prefix where the PCG counts agree (tests/test_oracle_restatement.py states the rule).

Run as a script (`python test_bqp_batch_gpu.py OUT.npy`) the file solves the size batch and writes every result byte to OUT: the
window test starts it as a fresh child process with LPBOX_BQP_BATCH_WINDOW=3."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    _ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_ROOT, os.path.join(_ROOT, "accelerated-lpbox-admm_amd")]

from helpers import BQP_SCALARS, BQP_VECS, assert_within_bound, bits_equal, bqp_params, bqp_problem, common_prefix
from oracle import oracle as O
from oracle.bqp_numpy import NumpyBqp

pytestmark = pytest.mark.gpu

SIZES = [2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1025, 2047, 2048]
ALL_SCALARS = BQP_SCALARS + ("iters", "stop", "total_pcg", "last_pcg")
SOLVER_ONLY_SCALARS = ("outer_total",)          # the oracle does not count it


def ptype_of(P):
    return (1 if P.get("C") is not None else 0) | (2 if P.get("E") is not None else 0)


def names(P):
    return [v for v in BQP_VECS if v not in ("z3",) or P.get("C") is not None
            if v not in ("z4", "y3") or P.get("E") is not None]


def single(P, preset=None, params=None):
    from lpbox_hip.bqp import BqpSolver
    g = BqpSolver(P["n"], P["A"], P["b"], P["x0"], P.get("C"), P.get("d"), P.get("E"), P.get("f"), preset=preset, params=params)
    return g, g.solve()


def oracle_gpu(B, P, preset=None, params=None):
    o = O.BqpOracle(P, preset=preset, params=params, order=O.ORDER_GPU, T=int(B.scalar(0, "threads")), chunk=int(B.scalar(0, "chunk")))
    return o, o.solve()


def same_scalar(a, b):
    return bits_equal(np.array([a], np.float64), np.array([b], np.float64))


def check_against(B, i, its, P, ref, it_ref, scalars, tag):
    assert int(its[i]) == it_ref, f"{tag}: iterations {its[i]} vs {it_ref}"
    for name in names(P):
        got, want = B.vec(i, name), ref.vec(name)
        assert bits_equal(got, want), f"{tag} {name}: max diff {np.abs(got - want).max():.3e}"
    for name in scalars:
        assert same_scalar(B.scalar(i, name), ref.scalar(name)), f"{tag} {name}: {B.scalar(i, name)!r} vs {ref.scalar(name)!r}"


def check_problem(B, i, its, P, preset=None, params=None, tag=""):
    """Problem i of the solved batch B against its two references."""
    assert B.scalar(i, "threads") == 256 and B.scalar(i, "chunk") == 512
    o, it_o = oracle_gpu(B, P, preset, params)
    check_against(B, i, its, P, o, it_o, ALL_SCALARS, f"{tag} [{i}] n={P['n']} vs oracle")
    g, it_g = single(P, preset, params)
    assert g.scalar("threads") == 256 and g.scalar("chunk") == 512
    check_against(B, i, its, P, g, it_g, ALL_SCALARS + SOLVER_ONLY_SCALARS, f"{tag} [{i}] n={P['n']} vs BqpSolver")
    g.close()
    return o


# ---- 1. sizes: every edge of the tree (one lane, one wave, one slot, one chunk, two, three and four chunks) ------------------------
@functools.lru_cache(maxsize=None)
def size_problems():
    return tuple(bqp_problem(n, max(1, n // 12), max(1, n // 9), seed=n) for n in SIZES)


def solve_sizes():
    from lpbox_hip.bqp import BqpBatch
    B = BqpBatch(size_problems(), params=bqp_params(3, 8))
    return B, B.solve()


def all_bytes(B, problems, its):
    parts = [np.asarray(its, np.float64)]
    for i, P in enumerate(problems):
        parts += [B.vec(i, v) for v in names(P)]
        parts.append(np.array([B.scalar(i, s) for s in ALL_SCALARS + SOLVER_ONLY_SCALARS]))
    return np.concatenate(parts).view(np.uint64)


@functools.lru_cache(maxsize=None)
def sizes_solved():
    B, its = solve_sizes()
    return B, its, all_bytes(B, size_problems(), its), B.scalar(0, "window")


def test_sizes_across_the_tree():
    B, its, _, _ = sizes_solved()
    assert B.scalar(0, "slots") == 8 and B.scalar(0, "launches") >= 2 and B.scalar(0, "kernel_ms") > 0
    for i, P in enumerate(size_problems()):
        assert B.dims[i] == (P["n"], max(1, P["n"] // 12), max(1, P["n"] // 9))
        check_problem(B, i, its, P, params=bqp_params(3, 8), tag="sizes")
        assert its[i] == 8


def test_results_do_not_depend_on_the_window(tmp_path):
    """The same batch in a fresh process with 3 outer iterations per launch: state saved and restored across launch boundaries, the
    halt (8 = 3 + 3 + 2) in mid-window."""
    _, _, want, window = sizes_solved()
    assert window != 3
    out = str(tmp_path / "sizes_w3.npy")
    env = dict(os.environ, LPBOX_BQP_BATCH_WINDOW="3")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.load(out)
    assert got[-1] == 3 and got[-2] >= 4          # the window the child ran with, and its launches (init + three windows)
    assert np.array_equal(got[:-2], want)


# ---- 2. mixed batch: four types, diagonal-only and general A, single rows, more rows than variables, empty rows / columns ---------
@functools.lru_cache(maxsize=None)
def mixed_problems():
    """(problem, type, K) triples"""
    out = []
    for ptype in (0, 1, 2, 3):
        for offdiag in (False, True):
            m, l = (0, 25, 0, 15)[ptype], (0, 0, 25, 20)[ptype]
            out.append((bqp_problem(400, m, l, seed=90 + ptype, offdiag=offdiag), ptype, 8))
    for n, m, l in [(257, 1, 0), (257, 0, 1), (257, 1, 1), (256, 0, 300), (200, 20, 260)]:
        out.append((bqp_problem(n, m, l, seed=7 * n + m + l), (1 if m else 0) | (2 if l else 0), 8))
    out.append((bqp_problem(300, 40, 50, seed=5), 3, 8))
    out.append((bqp_problem(150, 15, 0, 60, indefinite=True), 1, 3))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def mixed_solved():
    from lpbox_hip.bqp import BqpBatch
    M = mixed_problems()
    B = BqpBatch([P for P, _, _ in M], presets=[t for _, t, _ in M], params=[bqp_params(t, K) for _, t, K in M])
    return B, B.solve()


def test_mixed_batch_of_all_four_types():
    B, its = mixed_solved()
    M = mixed_problems()
    assert {ptype_of(P) for P, _, _ in M} == {0, 1, 2, 3} and B.scalar(0, "slots") == 2
    for key in ("C", "E"):                                   # the edge shapes are what they claim to be
        P = M[13][0]
        lens = np.diff(P[key][0])
        assert lens[0] == 0 and {1, 2, 3} <= set(lens % 4) and 299 not in set(P[key][1]) and np.any(P[key][2] < 0)
    for i, (P, t, K) in enumerate(M):
        assert t == ptype_of(P)
        check_problem(B, i, its, P, preset=t, params=bqp_params(t, K), tag="mixed")
    r0 = NumpyBqp(M[14][0], params=bqp_params(1, 3))
    r0.solve(record=True)
    assert r0.min_curvature[0] < 0 and np.isfinite(B.vec(14, "x")).all() and its[14] == 3      # the indefinite operator


# ---- 3. not pinned to the C oracle alone: the numpy restatement over the agreeing prefix -------------------------------------------
def test_three_problems_against_the_restatement():
    from lpbox_hip.bqp import BqpBatch
    M = mixed_problems()
    picks = [M[7], M[12], M[13]]                              # type 3 with a general A, more rows than variables, empty rows / columns
    B0 = BqpBatch([P for P, _, _ in picks], params=[bqp_params(t, K) for _, t, K in picks])
    B0.solve()
    ks, rs = [], []
    for i, (P, t, K) in enumerate(picks):
        params = bqp_params(t, K)
        o, _ = oracle_gpu(B0, P, params=params)
        e = O.BqpOracle(P, params=params)
        e.solve()
        r = NumpyBqp(P, params=params)
        r.solve(record=True)
        k = common_prefix(o.pcg_trace(), e.pcg_trace(), r.pcg)
        assert k >= 4, f"n={P['n']}: PCG counts agree over {k} iterations only: {list(o.pcg_trace())} vs {r.pcg}"
        ks.append(k); rs.append(r)
    prms = []
    for (P, t, K), k in zip(picks, ks):
        prm = list(bqp_params(t, K)); prm[5] = k
        prms.append(prm)
    B = BqpBatch([P for P, _, _ in picks], params=prms)
    its = B.solve()
    for i, (P, t, K) in enumerate(picks):
        k = ks[i]
        o, it_o = oracle_gpu(B, P, params=prms[i])
        e = O.BqpOracle(P, params=prms[i])
        e.solve()
        check_against(B, i, its, P, o, it_o, ALL_SCALARS, f"prefix k={k}")
        snap = rs[i].trace[k - 1]
        for name in names(P):
            assert_within_bound(B.vec(i, name), snap[name], e.vec(name), o.vec(name), f"n={P['n']} k={k} {name}")
        for name in BQP_SCALARS:
            assert_within_bound(B.scalar(i, name), snap[name], e.scalar(name), o.scalar(name), f"n={P['n']} k={k} {name}")


# ---- 4. different stopping points: each problem runs to its own stop, an early finisher is not disturbed by later windows ---------
# (n, m, l, seed, max_iters or None): chosen on the CPU with the oracle -- iteration counts 95 ... 997, stops 1, 2 and max_iters
STOPPING = [(120, 0, 0, 1000, None), (160, 12, 0, 1000, None), (160, 12, 0, 1002, None), (200, 0, 15, 1001, None),
            (280, 0, 0, 1002, None), (360, 0, 24, 1002, None), (200, 0, 15, 1000, 8), (400, 25, 20, 1000, 40)]


def test_problems_that_stop_at_different_points():
    from lpbox_hip.bqp import BqpBatch
    from oracle.bqp_numpy import PRESETS
    problems, params = [], []
    for n, m, l, seed, cap in STOPPING:
        P = bqp_problem(n, m, l, seed=seed)
        prm = None
        if cap is not None:
            prm = list(PRESETS[ptype_of(P)]); prm[5] = cap
        problems.append(P); params.append(prm)
    B = BqpBatch(problems, params=params)          # presets: from the constraints present
    its = B.solve()
    stops = []
    for i, P in enumerate(problems):
        o = check_problem(B, i, its, P, params=params[i], tag="stopping")
        stops.append(int(o.scalar("stop")))
    assert max(its) >= 2 * min(its) and {0, 1, 2} <= set(stops), (list(its), stops)
    assert B.scalar(0, "launches") >= 1 + -(-max(its) // B.scalar(0, "window"))
    # problem 6 ends on max_iters right after an iteration that improved the binary objective: best_sol is that x (the trailing copy)
    assert stops[6] == 0 and its[6] == 8 and bits_equal(B.vec(6, "best_sol"), B.vec(6, "x"))
    assert B.scalar(6, "cur_obj") == B.scalar(6, "best_bin_obj")


# ---- 5. more problems than compute units, determinism, a batch of one --------------------------------------------------------------
def test_more_problems_than_compute_units_and_a_batch_of_one():
    from lpbox_hip.bqp import BqpBatch, solve_many
    problems, params = [], []
    for i in range(300):
        n = 5 + i % 36
        t = i % 4
        P = bqp_problem(n, max(1, n // 6) if t & 1 else 0, max(1, n // 5) if t & 2 else 0, seed=3000 + i, offdiag=bool(i % 5))
        problems.append(P); params.append(bqp_params(t, 8))
    B = BqpBatch(problems, params=params)
    its = B.solve()
    first = all_bytes(B, problems, its)
    for i in range(0, 300, 10):
        check_problem(B, i, its, problems[i], params=params[i], tag="300")
    its2 = B.solve()                                # a second solve starts again from x0
    assert np.array_equal(all_bytes(B, problems, its2), first)
    one = BqpBatch([problems[7]], params=params[7])
    its1 = one.solve()
    assert one.count == 1 and its1.shape == (1,)
    check_problem(one, 0, its1, problems[7], params=params[7], tag="one")
    for name in names(problems[7]):
        assert bits_equal(one.vec(0, name), B.vec(7, name))
    sols = solve_many(problems[:3], params=params[:3])
    assert len(sols) == 3 and all(bits_equal(sols[i]["x_sol"], B.vec(i, "x")) and sols[i]["iterations"] == its[i] for i in range(3))
    assert sorted(sols[0]) == sorted(["x_sol", "y1", "y2", "best_sol", "iterations", "stop", "best_bin_obj", "time_elapsed_ms"])
    assert sorted(B.solution(0)) == sorted(["x_sol", "y1", "y2", "best_sol"])


def test_four_slot_instantiation():
    """513 <= the largest n <= 1024: four slots per thread, two chunks (the size batch runs on eight, the others on two)."""
    from lpbox_hip.bqp import BqpBatch
    problems = [bqp_problem(n, max(1, n // 12), max(1, n // 9), seed=n) for n in (513, 1024)] + [bqp_problem(40, 3, 0, seed=4)]
    params = [bqp_params(3, 5), bqp_params(3, 5), bqp_params(1, 5)]
    B = BqpBatch(problems, params=params)
    its = B.solve()
    assert B.scalar(0, "slots") == 4
    for i, P in enumerate(problems):
        check_problem(B, i, its, P, params=params[i], tag="slots4")


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals():
    import ctypes as C
    from lpbox_hip import _lib
    from lpbox_hip.bqp import BqpBatch
    from lpbox_hip.lp import LpboxError
    L = _lib.load()
    small = bqp_problem(6, 1, 1, seed=1)
    n = 2049
    big = dict(n=n, A=(np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n)), b=np.zeros(n), x0=np.full(n, 0.5))
    with pytest.raises(LpboxError, match="lpbox_bqp_") as e:
        BqpBatch([small, big])
    assert e.value.code == _lib.E_TOOLARGE
    # through the C boundary: the refused index stays unset, the other problem is untouched, solve wants every index
    h = C.c_void_p(L.lpbox_bqp_batch_create(2, 0))
    assert h

    def set_problem(idx, P):
        keep = [np.ascontiguousarray(a) for a in P["A"]] + [np.ascontiguousarray(P["b"], np.float64), np.ascontiguousarray(P["x0"], np.float64)]
        p = [a.ctypes.data_as(C.c_void_p) for a in keep]
        return L.lpbox_bqp_batch_set_problem(h, idx, P["n"], p[0], p[1], p[2], p[3], p[4], 0, None, None, None, None, 0, None, None, None, None)
    free = bqp_problem(6, 0, 0, seed=2)
    out, v = np.zeros(4096), C.c_double()
    assert set_problem(0, free) == 0
    assert set_problem(1, big) == _lib.E_TOOLARGE and b"lpbox_bqp_" in L.lpbox_last_error()
    assert set_problem(2, free) == -2 and b"range" in L.lpbox_last_error()
    assert L.lpbox_bqp_batch_solve(h, None) == _lib.E_STATE and b"index 1" in L.lpbox_last_error()
    assert L.lpbox_bqp_batch_get_vec(h, 0, b"x", out, len(out)) == _lib.E_STATE            # getter before solve
    assert L.lpbox_bqp_batch_get_scalar(h, 0, b"iters", C.byref(v)) == _lib.E_STATE
    assert set_problem(1, free) == 0 and L.lpbox_bqp_batch_preset(h, -1, 0) == 0 and L.lpbox_bqp_batch_preset(h, 0, 7) == -2
    bad = np.array(bqp_params(0, 4), np.float64); bad[7] = 9
    assert L.lpbox_bqp_batch_set_params(h, 1, bad) == -2 and b"history_size" in L.lpbox_last_error()
    assert L.lpbox_bqp_batch_set_params(h, -1, np.array(bqp_params(0, 4), np.float64)) == 0
    its = np.zeros(2, np.int32)
    assert L.lpbox_bqp_batch_solve(h, its.ctypes.data_as(C.c_void_p)) == 0 and list(its) == [4, 4]
    assert L.lpbox_bqp_batch_get_vec(h, 0, b"x", out, len(out)) == 6 and L.lpbox_bqp_batch_get_vec(h, 0, b"x", out, 3) == -2
    assert L.lpbox_bqp_batch_get_vec(h, 5, b"x", out, len(out)) == -2 and L.lpbox_bqp_batch_get_vec(h, 0, b"nope", out, len(out)) == -2
    x0 = out[:6].copy()
    assert L.lpbox_bqp_batch_get_vec(h, 1, b"x", out, len(out)) == 6 and bits_equal(out[:6], x0)    # the same problem twice: the same bits
    # validation: the one-problem solver's cases and messages; a rejected call leaves the problem that was set untouched
    i32, f64 = (lambda *v: np.array(v, np.int32)), (lambda *v: np.array(v, np.float64))

    def raw(n, Ap, Ai, Av, m=0, Cp=None, Ci=None, Cv=None, d=None):
        keep = [Ap, Ai, Av, f64(*[0.0] * n), f64(*[0.5] * n), Cp, Ci, Cv, d]
        p = [None if a is None else a.ctypes.data_as(C.c_void_p) for a in keep]
        return L.lpbox_bqp_batch_set_problem(h, 0, n, p[0], p[1], p[2], p[3], p[4], m, p[5], p[6], p[7], p[8], 0, None, None, None, None)
    for rc_msg, args in [
            (b"A: columns must ascend", dict(n=2, Ap=i32(0, 2, 3), Ai=i32(1, 0, 1), Av=f64(1, 1, 1))),
            (b"A: row pointer not monotone", dict(n=2, Ap=i32(0, 2, 1), Ai=i32(0, 1, 1), Av=f64(1, 1, 1))),
            (b"A: column index out of range", dict(n=2, Ap=i32(0, 1, 2), Ai=i32(0, 2), Av=f64(1, 1))),
            (b"A has no stored diagonal entry in row 0", dict(n=2, Ap=i32(0, 1, 2), Ai=i32(1, 1), Av=f64(1, 1))),
            (b"d missing", dict(n=2, Ap=i32(0, 1, 2), Ai=i32(0, 1), Av=f64(1, 1), m=1, Cp=i32(0, 1), Ci=i32(0), Cv=f64(1.0)))]:
        assert raw(**args) == -2 and rc_msg in L.lpbox_last_error(), rc_msg
    assert L.lpbox_bqp_batch_solve(h, its.ctypes.data_as(C.c_void_p)) == 0 and list(its) == [4, 4]
    assert L.lpbox_bqp_batch_get_vec(h, 0, b"x", out, len(out)) == 6 and bits_equal(out[:6], x0)
    L.lpbox_bqp_batch_destroy(h)


def _child(out):
    B, its = solve_sizes()
    tail = np.array([B.scalar(0, "launches"), B.scalar(0, "window")]).astype(np.uint64)
    np.save(out, np.concatenate([all_bytes(B, size_problems(), its), tail]))


if __name__ == "__main__":
    _child(sys.argv[1])
