"""GPU tests of the batched large route (lpbox_big_batch_*, BigLpBatch): a batch of instances in one lockstep
launch chain, every member on its own control state.  The contract is that a member gets the same bits in a batch as alone, so every
comparison is bit for bit -- against the CPU oracle in the kernels' reduction order and against a solo BigLp twin."""
import ctypes as C

import numpy as np
import pytest

import big_batch_cases as BC
from chain_cases import expected_resumes
from helpers import bits_equal

pytestmark = pytest.mark.gpu

E_BADARG, E_STATE, E_UNSUPPORTED = -2, -3, -7


def make_batch(cases):
    from lpbox_hip.big import BigLpBatch
    B = BigLpBatch([BC.problem(n, s) for (n, s) in cases])
    assert B.solve_init() == 1
    for g in B.solvers:                                     # the geometry the shared oracle runs were made with
        assert (int(g.scalar("threads")), int(g.scalar("chunk"))) == (BC.T, BC.CHUNK) and g.scalar("folded_reductions") == 1.0
    return B


def solo(n, seed):
    from lpbox_hip.big import BigLp
    g = BigLp(BC.problem(n, seed))
    g.solve_init()
    return g


def test_mixed_sizes_windows_bit_exact():
    """G = 1, 2, 3, 5, 6 and Gl = 1 ... 3 in one grid: workgroups beyond a member's own extent leave, per kernel kind."""
    B = make_batch(BC.MIXED)
    assert [int(B.scalar(k)) for k in ("grid_cols", "grid_y", "grid_rows", "grid_z4")] == [6, 6, 3, 3]
    assert sorted(int(g.scalar("groups")) for g in B.solvers) == [1, 2, 3, 5, 6]
    twins = [solo(n, s) for (n, s) in BC.MIXED]
    for w, (a, b) in enumerate(BC.WINDOWS):
        rets = B.solve_iter(a, b)
        assert rets.dtype == np.int32 and len(rets) == len(BC.MIXED)
        for k, (n, s) in enumerate(BC.MIXED):
            tag = f"n={n} seed={s} [{a},{b})"
            snap = BC.oracle_windows(n, s)[w]
            assert rets[k] == snap["ret"] == twins[k].solve_iter(a, b), tag
            BC.same_as_snapshot(B[k], snap, tag)
            BC.same_as_twin(B[k], twins[k], tag)
    assert B.scalar("parity_copies") == 0 and B.scalar("launches") > 0 and B.scalar("kernel_ms") > 0
    for t in twins:
        t.close()
    B.close()


def test_own_stops():
    """Four members that stop at four different iterations, by both rules: each falls through from its own stop on."""
    cases = sorted(BC.OWN_STOPS)
    B = make_batch(cases)
    rets = B.solve_iter(0, 20000)
    for k, (n, s) in enumerate(cases):
        snap, g = BC.oracle_solve(n, s), B[k]
        tag = f"n={n} seed={s}"
        assert (int(rets[k]), int(g.scalar("stop")), int(g.scalar("plain_iter_p1"))) == (snap["ret"], snap["stop"], snap["plain_iter_p1"]), tag
        assert (snap["stop"], snap["plain_iter_p1"], snap["ret"]) == BC.OWN_STOPS[(n, s)], tag
        assert bits_equal(g.local_x(), snap["x"]) and bits_equal(g.local_x_sol(), snap["x_sol"]), tag
        assert g.cal_Obj() == snap["obj"], tag
        assert (g.scalar("outer_total"), g.scalar("pcg_total")) == (snap["outer_total"], snap["pcg_total"]), tag   # its own count
    assert len({B[k].scalar("outer_total") for k in range(len(cases))}) == len(cases)
    B.close()


def test_solve_many():
    from lpbox_hip.big import solve_many
    cases = [(300, 1), (513, 2)]
    rets, xs, objs = solve_many([BC.problem(n, s) for (n, s) in cases])
    for k, (n, s) in enumerate(cases):
        snap = BC.oracle_solve(n, s)
        assert rets[k] == snap["ret"] and bits_equal(xs[k], snap["x_sol"]) and objs[k] == snap["obj"]


def test_resumed_pcg_in_lockstep(monkeypatch):
    """LPBOX_BIG_KMAX=4: every iteration of every member halts in `post` (its PCG needs 9 ... 22 iterations), the chain resumes for all
    and a member whose PCG is complete falls through the resumes the others still need."""
    monkeypatch.setenv("LPBOX_BIG_KMAX", "4")
    cases = [(300, 0), (1100, 4), (2600, 7)]
    B = make_batch(cases)
    assert int(B.scalar("kmax")) == 4
    rets = B.solve_iter(0, 40)
    windows = ((0, 40),)
    want = []
    for k, (n, s) in enumerate(cases):
        snap = BC.oracle_windows(n, s, windows)[0]
        assert rets[k] == snap["ret"]
        BC.same_as_snapshot(B[k], snap, f"kmax 4, n={n}")
        want.append(expected_resumes(snap["trace"], 4))
        assert int(B[k].scalar("kmax")) == 4 and B[k].scalar("pcg_resumes") == want[-1] == B.scalar(f"pcg_resumes_{k}"), (n, want)
    assert int(B.scalar("kmax")) == 4 and min(want) >= 40       # forced: the launch count never adapts; every iteration halted
    B.close()


def test_captured_batch_chain(monkeypatch):
    """LPBOX_BIG_BATCH_GRAPH=1: the iterations of a batch are replays of captured graphs (two iterations each) plus an eager tail, and a
    second window comes back to the cache at another kmax.  Same bits as eager launches; the batch must not have fallen back to them."""
    monkeypatch.setenv("LPBOX_BIG_BATCH_GRAPH", "1")
    cases = [(300, 0), (1100, 4)]
    windows = ((0, 7), (7, 40))
    B = make_batch(cases)
    assert B.scalar("graph") == 1.0
    twins = [solo(n, s) for (n, s) in cases]
    for w, (a, b) in enumerate(windows):
        rets = B.solve_iter(a, b)
        for k, (n, s) in enumerate(cases):
            tag = f"captured, n={n} seed={s} [{a},{b})"
            snap = BC.oracle_windows(n, s, windows)[w]
            assert rets[k] == snap["ret"] == twins[k].solve_iter(a, b), tag
            BC.same_as_snapshot(B[k], snap, tag)
            BC.same_as_twin(B[k], twins[k], tag)
    assert B.scalar("graph") == 1.0 and B.scalar("launches") > 0
    for t in twins:
        t.close()
    B.close()


def test_batch_of_one_equals_the_solo_handle():
    (n, s) = BC.MIXED[2]
    B, t = make_batch([(n, s)]), solo(n, s)
    for w, (a, b) in enumerate(BC.WINDOWS[:2]):
        assert B.solve_iter(a, b)[0] == t.solve_iter(a, b)
        BC.same_as_twin(B[0], t, f"B = 1 [{a},{b})")
        BC.same_as_snapshot(B[0], BC.oracle_windows(n, s)[w], f"B = 1 [{a},{b})")
    t.close()
    B.close()


def test_many_small_problems():
    """300 members: the grid's y-extent exceeds the CU count."""
    cases = [(300, seed) for seed in range(300)]
    B = make_batch(cases)
    rets = B.solve_iter(0, 20)
    assert B.scalar("count") == 300.0
    windows = ((0, 20),)
    for k, (n, s) in enumerate(cases):
        snap = BC.oracle_windows(n, s, windows)[0]
        assert rets[k] == snap["ret"]
        BC.same_as_snapshot(B[k], snap, f"member {k}")
    B.close()


def test_interleaved_with_a_window_of_its_own(monkeypatch):
    """A member runs a window alone between two batch windows.  With an even forced launch count a window of a handle's own flips its
    state ping-pong an odd number of times (1 + rounds x (2 + iterations x (8 + 3 kmax)), resumes 52 each), so the member comes back on
    the other parity and the batch copies its state across first."""
    monkeypatch.setenv("LPBOX_BIG_KMAX", "24")
    cases = BC.MIXED[:3]
    B = make_batch(cases)
    rets = B.solve_iter(0, 7)
    for k, (n, s) in enumerate(cases):
        assert rets[k] == BC.oracle_windows(n, s)[0]["ret"]
        BC.same_as_snapshot(B[k], BC.oracle_windows(n, s)[0], f"first batch window, member {k}")
    (n1, s1) = cases[1]
    assert B[1].solve_iter(7, 60) == BC.oracle_windows(n1, s1)[1]["ret"]
    BC.same_as_snapshot(B[1], BC.oracle_windows(n1, s1)[1], "own window")                  # the solo getters answer in between
    assert bits_equal(B[1].local_x_sol(), (BC.oracle_windows(n1, s1)[1]["x"] >= 0.5).astype(float)) and B[1].cal_Obj() == BC.oracle_windows(n1, s1)[1]["cur_obj"]
    BC.same_as_snapshot(B[0], BC.oracle_windows(*cases[0])[0], "member 0 untouched")
    rets = B.solve_iter(60, 130)
    assert B.scalar("parity_copies") == 1.0
    for k, (n, s) in enumerate(cases):
        snap = BC.oracle_windows(n, s)[2] if k == 1 else BC.oracle_windows(n, s, ((0, 7), (60, 130)))[1]
        assert rets[k] == snap["ret"]
        BC.same_as_snapshot(B[k], snap, f"second batch window, member {k}")
    assert B[2].solve_iter(130, 140) in (0, 1) and int(B[2].scalar("iter")) == 140         # and a member goes on alone afterwards
    B.close()


def test_refusals(monkeypatch):
    from lpbox_hip import _lib
    from lpbox_hip._lib import LpboxError
    from lpbox_hip.big import BigLp, BigLpBatch
    L = _lib.load()
    P0, P1 = BC.problem(300, 0), BC.problem(300, 1)
    a, b = BigLp(P0), BigLp(P1)

    def refused(members, code, text):
        with pytest.raises(LpboxError) as e:
            BigLpBatch(members)
        assert e.value.code == code and text in str(e.value), str(e.value)

    assert not L.lpbox_big_batch_create(None, 0) and L.lpbox_last_status() == E_BADARG
    assert not L.lpbox_big_batch_create((C.c_void_p * 1)(a._h), 0) and L.lpbox_last_status() == E_BADARG
    refused([a, b, a], E_BADARG, "same handle")
    refused([a, BigLp(P1, device=1)], E_BADARG, "another device")
    raw = C.c_void_p(L.lpbox_big_create(0, 1, 0))
    assert not L.lpbox_big_batch_create((C.c_void_p * 2)(a._h, raw), 2) and L.lpbox_last_status() == E_STATE
    L.lpbox_big_destroy(raw)
    refused([a, BigLp(P1, order="reference")], E_UNSUPPORTED, "reference summation order")
    n = P1["n"]
    half = C.c_void_p(L.lpbox_big_create(0, 2, 0))           # rank 0 of 2: the first half of the columns
    cp = np.ascontiguousarray(P1["colptr"][:n // 2 + 1], np.int32)
    assert L.lpbox_big_set_problem(half, n, 0, n // 2, P1["l"], cp, np.ascontiguousarray(P1["rowidx"][:cp[-1]], np.int32),
                                   np.ascontiguousarray(P1["b"][:n // 2], np.float64), None) == 0
    assert not L.lpbox_big_batch_create((C.c_void_p * 2)(a._h, half), 2)
    assert L.lpbox_last_status() == E_UNSUPPORTED and b"2 ranks" in L.lpbox_last_error()
    L.lpbox_big_destroy(half)
    cb = _lib.ALLGATHER_FN(lambda send, count, recv, user: 1)
    t = BigLp(P1)
    assert L.lpbox_big_set_allgather(t._h, C.cast(cb, C.c_void_p), None) == 0
    refused([a, t], E_UNSUPPORTED, "transport")             # (one check covers the callback and an RCCL communicator; creating one takes ~10 s)
    refused([a, BigLp(P1, pcg_mode="lean")], E_UNSUPPORTED, "comm-lean")
    assert L.lpbox_big_set_record(b._h, 1) == 0
    refused([a, b], E_UNSUPPORTED, "recording")
    assert L.lpbox_big_set_record(b._h, 0) == 0

    # decided by the upload: a member without folded reductions is refused by solve_init (fresh) or by create (initialised before)
    a.solve_init()                                           # a has uploaded: it keeps its folded reductions
    c = BigLp(P1)
    B = BigLpBatch([a, c])
    monkeypatch.setenv("LPBOX_BIG_NOFOLD", "1")              # read when a handle uploads its problem
    with pytest.raises(LpboxError) as e:
        B.solve_init()
    monkeypatch.delenv("LPBOX_BIG_NOFOLD")
    assert e.value.code == E_UNSUPPORTED and "problem 1" in str(e.value) and "folded reductions" in str(e.value)
    with pytest.raises(LpboxError) as e:
        B.solve_iter(0, 5)                                   # the batch stays unusable
    assert e.value.code == E_STATE
    B.close()
    assert c.scalar("folded_reductions") == 0.0
    refused([a, c], E_UNSUPPORTED, "folded reductions")

    # iterate before init; a member with recording switched on, or with fixed variables, between two calls
    B = BigLpBatch([a, b])
    with pytest.raises(LpboxError) as e:
        B.solve_iter(0, 5)
    assert e.value.code == E_STATE and "lpbox_big_batch_init" in str(e.value)
    B.solve_init()
    assert L.lpbox_big_set_record(b._h, 1) == 0
    with pytest.raises(LpboxError) as e:
        B.solve_iter(0, 5)
    assert e.value.code == E_UNSUPPORTED and "recording" in str(e.value)
    assert L.lpbox_big_set_record(b._h, 0) == 0
    assert int(a.scalar("iter")) == 0 and int(b.scalar("iter")) == 0       # refused: nobody moved
    vec = -np.ones(P1["n"])
    vec[:3] = (1.0, 0.0, 0.0)
    b.solve_iter_l2f(0, 5, vec, 3)
    with pytest.raises(LpboxError) as e:
        B.solve_iter(5, 10)
    assert e.value.code == E_UNSUPPORTED and "problem 1" in str(e.value) and "fixed variables" in str(e.value)
    B.close()

    # the members are usable alone afterwards (a ran nothing so far; c keeps its reduction launches)
    for g, (n_, s_) in ((a, (300, 0)), (c, (300, 1))):
        snap = BC.oracle_windows(n_, s_, ((0, 20),))[0]
        assert g.solve_iter(0, 20) == snap["ret"]
        BC.same_as_snapshot(g, snap, "alone after the refusals")
