"""GPU tests of the lockstep batch of generic BQPs (lpbox_hip.bqp.BqpLockstep, lpbox_bqp_lockstep_*): every member of every batch is
bit for bit the oracle in the kernels' order (tests/bqp_lockstep_cases.py runs it once per member) and a solo `BqpSolver` twin solved in
this process -- at the smallest shapes at which the batch entries of the kernels can go wrong: members with 1 ... 4 column workgroups in
one grid, row extents above the column extent, members that stop while others run on, a PCG that halts and resumes in lockstep, one
member, 300 members, a member above BqpBatch's limit, handles used again, graph replay, and the front doors.  The CPU file
tests/test_bqp_lockstep_api.py pins what these batches are made of."""
import numpy as np
import pytest

import bqp_lockstep_cases as BC
from chain_cases import expected_resumes
from helpers import BQP_SCALARS, bits_equal

pytestmark = pytest.mark.gpu

_twins = {}


def snapshot(g, P, it):
    """Everything the tests compare, read from a solved BqpSolver."""
    r = dict(iterations=int(it), iters=g.scalar("iters"))
    for name in BC.names(P):
        r[name] = g.vec(name)
    for name in BQP_SCALARS + BC.INT_SCALARS:
        r[name] = g.scalar(name)
    return r


def solo(P, params):
    from lpbox_hip.bqp import BqpSolver
    g = BqpSolver(P["n"], P["A"], P["b"], P["x0"], P.get("C"), P.get("d"), P.get("E"), P.get("f"), params=params)
    assert (g.scalar("order"), BC.T, BC.CHUNK) == (0.0, 256, 512)
    r = snapshot(g, P, g.solve())
    assert (g.scalar("threads"), g.scalar("chunk")) == (BC.T, BC.CHUNK)
    g.close()
    return r


def twin(set_name, i):
    """The solo run of member i of a set, solved once in this process."""
    if (set_name, i) not in _twins:
        _twins[(set_name, i)] = solo(*BC.SETS[set_name]()[i])
    return _twins[(set_name, i)]


def same(got, want, P, tag):
    assert got["iterations"] == want["iterations"], f"{tag}: iterations {got['iterations']} vs {want['iterations']}"
    assert got["stop"] == want["stop"] and got["total_pcg"] == want["total_pcg"], tag
    for name in BC.names(P):
        assert bits_equal(got[name], want[name]), f"{tag} {name}: max diff {np.abs(got[name] - want[name]).max():.3e}"
    for name in BQP_SCALARS:
        assert got[name] == want[name], f"{tag} {name}: {got[name]!r} vs {want[name]!r}"


def lockstep(members):
    from lpbox_hip.bqp import BqpLockstep
    return BqpLockstep([P for (P, _) in members], params=[p for (_, p) in members])


def solve_set(set_name, order=None, twins=True):
    """The set as one batch (members in `order`): every member against its oracle run and its solo twin.  Returns the batch, solved."""
    members, runs = BC.SETS[set_name](), BC.oracle_runs(set_name)
    order = list(range(len(members))) if order is None else list(order)
    B = lockstep([members[i] for i in order])
    its = B.solve()
    assert B.scalar("count") == len(order)
    for k, i in enumerate(order):
        P = members[i][0]
        got = snapshot(B[k], P, its[k])
        assert got["iters"] == its[k]
        same(got, runs[i], P, f"{set_name}[{i}] in slot {k} vs oracle")
        if twins:
            same(got, twin(set_name, i), P, f"{set_name}[{i}] in slot {k} vs solo")
    return B


def test_grid_extents_in_one_batch():
    B = solve_set("extents")
    G = [BC.groups(P) for (P, _) in BC.extents()]
    assert B.scalar("grid_cols") == max(g[0] for g in G) == 4
    assert B.scalar("grid_y") == max(max(g[0], g[2], 1) for g in G) == 4 and B.scalar("grid_rows") == max(max(g[1], g[2], 1) for g in G) == 3
    assert B.scalar("graph") == 0.0 and B.scalar("launches") > 0 and B.scalar("kernel_ms") > 0
    assert all(B.scalar("pcg_resumes_%d" % i) == 0 for i in range(len(G)))
    for s in B.solvers:                                   # the chain's launches belong to the batch
        assert s.scalar("kernel_ms") == 0.0 and s.scalar("launches") == 0.0 and s.scalar("pcg_resumes") == 0.0
    B.close()


def test_reversed_member_order_gives_the_same_bits():
    solve_set("extents", order=reversed(range(len(BC.extents())))).close()


def test_members_stop_on_their_own_while_others_run_on():
    B = solve_set("stops")
    ends = [(int(s.scalar("iters")), int(s.scalar("stop"))) for s in B.solvers]
    assert len({e[0] for e in ends}) == len(ends) and {e[1] for e in ends} == {0, 1, 2}
    i = BC.BEST_MEMBER                                    # the copy after the loop: best_sol is the final x, not the one before it
    assert bits_equal(B[i].vec("best_sol"), B[i].vec("x"))
    assert not bits_equal(B[i].vec("best_sol"), BC.oracle_run_with("stops", i, ends[i][0] - 1)["best_sol"])
    assert B[i].solution()["best_sol"].shape == (BC.stops()[i][0]["n"],) and B[i].scalar("best_bin_obj") == B[i].scalar("cur_obj")
    B.close()


@pytest.mark.parametrize("kmax", [1, 3])
def test_pcg_halts_and_resumes_in_lockstep(monkeypatch, kmax):
    """LPBOX_BQP_KMAX forced: every iteration of every member halts in `post`, the chain resumes for all, and each member's count of
    resumes is the one its own oracle PCG trace gives."""
    monkeypatch.setenv("LPBOX_BQP_KMAX", str(kmax))
    B = solve_set("resume")
    assert B.scalar("kmax") == kmax
    for i, r in enumerate(BC.oracle_runs("resume")):
        want = expected_resumes(r["trace"], kmax)
        assert want > 0 and B.scalar("pcg_resumes_%d" % i) == want == B[i].scalar("pcg_resumes"), (i, want)
    B.close()


def test_adaptive_chain_on_the_resume_members():
    B = solve_set("resume")
    res = [B.scalar("pcg_resumes_%d" % i) for i in range(3)]
    assert res[0] >= 2 and res[1] == res[2] == 0          # G4 needs 31 PCG iterations at once (12 + 16 do not reach it); G1, G3 never halt
    assert B.scalar("kmax") > 12
    B.close()


def test_batch_of_one_equals_the_solver():
    from lpbox_hip.bqp import BqpLockstep, BqpSolver
    P, p = BC.extents()[3]
    g = BqpSolver(P["n"], P["A"], P["b"], P["x0"], P.get("C"), P.get("d"), P.get("E"), P.get("f"), params=p)
    B = BqpLockstep([g])
    its = B.solve()
    got = snapshot(g, P, its[0])
    same(got, BC.oracle_runs("extents")[3], P, "batch of one vs oracle")
    same(got, twin("extents", 3), P, "batch of one vs solo")
    same(snapshot(g, P, g.solve()), got, P, "the same handle solved on its own afterwards")
    assert g.scalar("launches") > 0
    B.close()
    g.close()


def test_300_small_members():
    solve_set("many", twins=False).close()


def test_member_above_2048_beside_a_tiny_one():
    B = solve_set("wide")
    assert (B.scalar("grid_cols"), B.scalar("grid_y"), B.scalar("grid_rows")) == (5, 5, 1)
    B.close()


def test_handles_used_again():
    members, runs = BC.stops(), BC.oracle_runs("stops")
    B = lockstep(members)
    first = B.solve()
    second = B.solve()                                    # the batch again: every member re-initialised
    assert list(first) == list(second) == [r["iterations"] for r in runs]
    for i, (P, _) in enumerate(members):
        same(snapshot(B[i], P, second[i]), runs[i], P, f"second batch solve, member {i}")
    i = BC.BEST_MEMBER
    P = members[i][0]
    same(snapshot(B[i], P, B[i].solve()), runs[i], P, "a member solved on its own after the batch")
    assert B[i].scalar("launches") > 0
    third = B.solve()                                     # and the batch after that
    for k in (0, i):
        same(snapshot(B[k], members[k][0], third[k]), runs[k], members[k][0], f"third batch solve, member {k}")
    B.close()


def test_graph_replay_gives_the_bits_of_eager_launches(monkeypatch):
    monkeypatch.setenv("LPBOX_BQP_LOCKSTEP_GRAPH", "1")
    B = solve_set("extents")
    assert B.scalar("graph") == 1.0 and B.scalar("graph_entries") >= 1
    B.close()


def test_front_doors():
    from lpbox_hip import bqp
    members = BC.doors()
    problems, params = [P for (P, _) in members], [p for (_, p) in members]
    assert bqp.split_by_size(problems) == ([0, 2], [1])
    out = bqp.solve_any(problems, params=params)
    large = bqp.solve_large_many(problems[1:2], params=params[1:2])
    for i, (P, p) in enumerate(members):
        ptype = BC.ptype_of(P)
        want = bqp._run(P["n"], P["A"], P["b"], P["x0"], P.get("C"), P.get("d"), P.get("E"), P.get("f"), preset=ptype, params=p)
        for got in [out[i]] + (large if i == 1 else []):
            assert set(got) == set(want)
            for key in ("iterations", "stop", "best_bin_obj"):
                assert got[key] == want[key], (i, key)
            for key in ("x_sol", "y1", "y2", "best_sol"):
                assert bits_equal(got[key], want[key]), (i, key)
        r = BC.oracle_runs("doors")[i]
        assert out[i]["iterations"] == r["iterations"] and bits_equal(out[i]["x_sol"], r["x"]) and bits_equal(out[i]["best_sol"], r["best_sol"])
