"""GPU tests of the batched large route in the reference summation order (BigLpBatch(order="reference")): unit
and valued members in one lockstep chain, one walker per member.  The contract is section 28's: a member gets the bits it gets alone,
hence the bits of the oracle in ORDER_EIGEN.  Every comparison is bit for bit -- against a solo BigLp(order="reference") twin without
exception, against the oracle with the one documented deviation (std_obj within 2 ulp where the oracle's pow_sqrt_mismatch moved)."""
import ctypes as C

import numpy as np
import pytest

import big_ref_batch_cases as RC
from chain_cases import expected_resumes
from helpers import bits_equal

pytestmark = pytest.mark.gpu

E_UNSUPPORTED = -7


def make_batch(members):
    """members: (key, family) pairs -> a batch built from problem dicts, initialised."""
    from lpbox_hip.big import BigLpBatch
    B = BigLpBatch([RC.problem(key, fam) for (key, fam) in members], order="reference")
    assert B.solve_init() == 1
    assert B.scalar("order") == 1.0 and B.scalar("valued_members") == sum(1 for (_, fam) in members if fam)
    for g in B.solvers:
        assert g.scalar("order") == 1.0 and g.scalar("folded_reductions") == 0.0 and int(g.scalar("row_slices")) == 1
    return B


def solo(key, fam):
    from lpbox_hip.big import BigLp
    g = BigLp(RC.problem(key, fam), order="reference")
    g.solve_init()
    return g


def check_valued_vectors(g, P, snap, b, tag):
    if snap["stop"] == 0:
        assert bits_equal(g.vec("r4v"), RC.want_r4v(P["vals"], b)), f"{tag}: rho4_E_transpose"
    assert bits_equal(g.vec("vals"), P["vals"]), f"{tag}: vals"


def run_windows(members, windows, check_twins=True):
    """Every member after every window against its oracle snapshot and against a solo twin that runs the same windows."""
    B = make_batch(members)
    twins = [solo(key, fam) for (key, fam) in members] if check_twins else None
    walks = 0.0
    for w, (a, b) in enumerate(windows):
        rets = B.solve_iter(a, b)
        assert rets.dtype == np.int32 and len(rets) == len(members)
        assert B.scalar("walks") > walks
        walks = B.scalar("walks")
        for k, (key, fam) in enumerate(members):
            tag = f"{key} {fam} [{a},{b})"
            snap = RC.oracle_windows(key, fam, windows)[w]
            assert rets[k] == snap["ret"], tag
            RC.compare(B[k], snap, tag, unit=fam is None)
            if fam:
                check_valued_vectors(B[k], RC.problem(key, fam), snap, b, tag)
            if twins:
                assert rets[k] == twins[k].solve_iter(a, b), tag
                RC.same_as_twin(B[k], twins[k], tag, valued=fam is not None)
    assert B.scalar("parity_copies") == 0 and B.scalar("launches") > B.scalar("walks") > 0
    for t in twins or ():
        t.close()
    return B


def test_unit_mixed_sizes():
    """G = 1, 2, 3, 5, 6 and Gl = 1 ... 3 in one grid; a batch that ran the default order would differ after every window."""
    B = run_windows([(key, None) for key in RC.MIXED], RC.WINDOWS)
    assert [int(B.scalar(k)) for k in ("grid_cols", "grid_y", "grid_rows", "grid_z4")] == [6, 6, 3, 3]
    for k, key in enumerate(RC.MIXED):
        assert not bits_equal(B[k].vec("x"), RC.default_order_x(key)[-1]), key
    B.close()


@pytest.mark.parametrize("family", ["set", "uniform"])
def test_valued_mixed_sizes(family):
    run_windows([(key, family) for key in RC.MIXED], RC.WINDOWS).close()


def test_unit_and_valued_members_in_one_batch():
    """Alternating kinds: the entries branch per member, y runs once per kind.  A member whose vals are all ones is a unit instance."""
    from lpbox_hip.big import BigLp, BigLpBatch
    members = [(RC.MIXED[0], None), (RC.MIXED[1], "set"), (RC.MIXED[2], None), (RC.MIXED[3], "uniform"), (RC.MIXED[0], "set")]
    B = run_windows(members, RC.WINDOWS[:2])
    B.close()
    key = RC.MIXED[1]
    P = RC.problem(key)
    ones = dict(P, vals=np.ones(len(P["rowidx"])))
    B = BigLpBatch([RC.problem(RC.MIXED[0], "set"), ones, RC.problem(key, "uniform")], order="reference")
    B.solve_init()
    assert B.scalar("valued_members") == 2.0 and B[1].scalar("valued") == 0.0
    t = BigLp(ones, order="reference")
    t.solve_init()
    for w, (a, b) in enumerate(RC.WINDOWS[:2]):
        rets = B.solve_iter(a, b)
        assert rets[1] == t.solve_iter(a, b)
        RC.same_as_twin(B[1], t, f"all-ones vals [{a},{b})")
        RC.compare(B[1], RC.oracle_windows(key, None, RC.WINDOWS[:2])[w], f"all-ones vals [{a},{b})")
        RC.compare(B[0], RC.oracle_windows(RC.MIXED[0], "set", RC.WINDOWS[:2])[w], "valued beside it", unit=False)
        RC.compare(B[2], RC.oracle_windows(key, "uniform", RC.WINDOWS[:2])[w], "valued beside it", unit=False)
    t.close()
    B.close()


@pytest.mark.parametrize("family", [None, "set"])
def test_every_redux_branch_and_the_tile_edges(family):
    """Twelve odd instances in one batch: live counts 2 ... 9 (every short branch, the left-over pair, the odd element), 511 / 513 beside
    the rank chunk, 1025 / 1027 beside the walker's tile, 2049 over three tiles.  The smallest members stop inside the second window
    while the others run on."""
    members = [(("odd", n), family) for n in RC.ODD_NS]
    B = run_windows(members, RC.ODD_WINDOWS)
    for k, n in enumerate(RC.ODD_NS):
        want = RC.ODD_STOPS[family].get(n)
        got = (int(B[k].scalar("outer_total")), int(B[k].scalar("pcg_total")))
        if want:
            assert got == want and int(B[k].scalar("stop")) == 1, (n, got)
        else:
            assert got[0] == 60 and int(B[k].scalar("stop")) == 0, (n, got)
        assert not np.isnan(B[k].vec("x")).any()
    B.close()


def test_own_stops():
    cases = sorted(RC.OWN_STOPS)
    B = make_batch([(key, None) for key in cases])
    rets = B.solve_iter(0, 20000)
    for k, key in enumerate(cases):
        snap, g = RC.oracle_solve(key), B[k]
        assert (int(rets[k]), int(g.scalar("stop")), int(g.scalar("plain_iter_p1"))) == (snap["ret"], snap["stop"], snap["plain_iter_p1"]), key
        assert (snap["stop"], snap["plain_iter_p1"], snap["ret"]) == RC.OWN_STOPS[key], key
        assert bits_equal(g.local_x(), snap["x"]) and bits_equal(g.local_x_sol(), snap["x_sol"]), key
        assert g.cal_Obj() == snap["obj"], key
        assert (g.scalar("outer_total"), g.scalar("pcg_total")) == (snap["outer_total"], snap["pcg_total"]), key      # its own count
    assert len({B[k].scalar("outer_total") for k in range(len(cases))}) == len(cases)
    B.close()


def test_resumed_pcg_in_lockstep(monkeypatch):
    """LPBOX_BIG_KMAX=4: every iteration of every member halts in `post`; the chain resumes for all, and a member whose PCG is complete
    falls through the resumes (and their walks) the others still need."""
    monkeypatch.setenv("LPBOX_BIG_KMAX", "4")
    members = [((300, 0), None), ((513, 2), None), ((1100, 4), None), ((300, 0), "set")]
    B = make_batch(members)
    assert int(B.scalar("kmax")) == 4
    rets = B.solve_iter(0, 40)
    windows = ((0, 40),)
    want = []
    for k, (key, fam) in enumerate(members):
        snap = RC.oracle_windows(key, fam, windows)[0]
        assert rets[k] == snap["ret"]
        RC.compare(B[k], snap, f"kmax 4, {key} {fam}", unit=fam is None)
        want.append(expected_resumes(snap["trace"], 4))
        assert B[k].scalar("pcg_resumes") == want[-1] == B.scalar(f"pcg_resumes_{k}"), (key, fam, want)
    assert int(B.scalar("kmax")) == 4 and min(want) >= 40
    B.close()


def test_batch_of_one_equals_the_solo_handle():
    run_windows([(RC.MIXED[2], None)], RC.WINDOWS[:2]).close()
    run_windows([(RC.MIXED[1], "set")], RC.WINDOWS[:2]).close()


def test_more_members_than_compute_units():
    """300 members: more grid rows than CUs, and one walker fits per CU, so the walkers queue."""
    members = [((300, seed), None) for seed in range(300)]
    B = make_batch(members)
    rets = B.solve_iter(0, 20)
    assert B.scalar("count") == 300.0
    windows = ((0, 20),)
    for k, (key, fam) in enumerate(members):
        snap = RC.oracle_windows(key, fam, windows)[0]
        assert rets[k] == snap["ret"]
        RC.compare(B[k], snap, f"member {k}")
    B.close()


def test_interleaved_with_a_window_of_its_own(monkeypatch):
    """A member runs a window alone between two batch windows.  With an even forced launch count a window of a handle's own flips its
    state ping-pong an odd number of times (the walks flip nothing), so the member comes back on the other parity and the batch copies
    its state across first."""
    monkeypatch.setenv("LPBOX_BIG_KMAX", "24")
    members = [(RC.MIXED[0], None), (RC.MIXED[1], "set"), (RC.MIXED[2], None)]
    B = make_batch(members)
    rets = B.solve_iter(0, 7)
    for k, (key, fam) in enumerate(members):
        snap = RC.oracle_windows(key, fam)[0]
        assert rets[k] == snap["ret"]
        RC.compare(B[k], snap, f"first batch window, member {k}", unit=fam is None)
    key1, fam1 = members[1]
    own = RC.oracle_windows(key1, fam1)[1]
    assert B[1].solve_iter(7, 60) == own["ret"]
    RC.compare(B[1], own, "own window", unit=False)                                          # the solo getters answer in between
    assert bits_equal(B[1].local_x_sol(), (own["x"] >= 0.5).astype(float)) and B[1].cal_Obj() == own["cur_obj"]
    RC.compare(B[0], RC.oracle_windows(*members[0])[0], "member 0 untouched")
    rets = B.solve_iter(60, 130)
    assert B.scalar("parity_copies") == 1.0
    for k, (key, fam) in enumerate(members):
        snap = RC.oracle_windows(key, fam)[2] if k == 1 else RC.oracle_windows(key, fam, ((0, 7), (60, 130)))[1]
        assert rets[k] == snap["ret"]
        RC.compare(B[k], snap, f"second batch window, member {k}", unit=fam is None)
    B.close()


def test_refusals():
    from lpbox_hip._lib import LpboxError
    from lpbox_hip.big import BigLp, BigLpBatch
    P0, P1 = RC.problem((300, 0)), RC.problem((300, 1))
    r0, r1, d1 = BigLp(P0, order="reference"), BigLp(P1, order="reference"), BigLp(P1)
    for members, who in (([r0, d1], "default order"), ([d1, r0], "reference summation order")):
        with pytest.raises(LpboxError) as e:
            BigLpBatch(members)
        assert e.value.code == E_UNSUPPORTED and "problem 1" in str(e.value) and who in str(e.value), str(e.value)
        assert "reference summation order" in str(e.value)
    B = BigLpBatch([r0, r1])
    B.solve_init()
    assert list(B.solve_iter(0, 5)) == [0, 0]
    before = [g.vec("x") for g in (r0, r1)]
    launches = B.scalar("launches")
    # the early-fixing calls: refused, nothing changes
    with pytest.raises(LpboxError) as e:
        B.solve_iter_l2f(5, 10, None, np.zeros(2, np.int64))
    assert e.value.code == E_UNSUPPORTED and "reference summation order" in str(e.value)
    with pytest.raises(LpboxError) as e:
        B.solve_iter_l2f_scores(5, 10, None)
    assert e.value.code == E_UNSUPPORTED
    ptr, off = C.c_void_p(), np.zeros(3, np.int64)
    assert B._L.lpbox_big_batch_get_x_iters_device(B._h, 5, C.byref(ptr), off.ctypes.data_as(C.c_void_p)) == E_UNSUPPORTED and not ptr.value
    assert B.scalar("launches") == launches and all(bits_equal(g.vec("x"), x) for g, x in zip((r0, r1), before))
    assert [int(g.scalar("iter")) for g in (r0, r1)] == [5, 5]
    # a member that fixed variables in a window of its own between two batch windows
    vec = -np.ones(P1["n"])
    vec[:3] = (1.0, 0.0, 0.0)
    r1.solve_iter_l2f(5, 10, vec, 3)
    with pytest.raises(LpboxError) as e:
        B.solve_iter(5, 10)
    assert e.value.code == E_UNSUPPORTED and "problem 1" in str(e.value) and "fixed variables" in str(e.value)
    assert int(r0.scalar("iter")) == 5                        # refused: member 0 did not move
    B.close()
    # the batch is gone, the members are usable: member 0 goes on alone to the oracle's bits
    snap = RC.oracle_windows((300, 0), None, ((0, 5), (5, 20)))[1]
    assert r0.solve_iter(5, 20) == snap["ret"]
    RC.compare(r0, snap, "alone after the refusals")
    # and a fresh batch of member 0's twin with a re-initialised member 1 runs
    r1.solve_init()
    t0 = BigLp(P0, order="reference")
    B = BigLpBatch([t0, r1])
    B.solve_init()
    B.solve_iter(0, 20)
    RC.compare(t0, RC.oracle_windows((300, 0), None, ((0, 20),))[0], "fresh batch, member 0")
    RC.compare(r1, RC.oracle_windows((300, 1), None, ((0, 20),))[0], "fresh batch, member 1")
    B.close()
    for g in (r0, r1, d1, t0):
        g.close()


def test_solve_many():
    from lpbox_hip.big import solve_many
    cases = sorted(RC.OWN_STOPS)
    rets, xs, objs = solve_many([RC.problem(key) for key in cases], order="reference")
    for k, key in enumerate(cases):
        snap = RC.oracle_solve(key)
        assert rets[k] == snap["ret"] and bits_equal(xs[k], snap["x_sol"]) and objs[k] == snap["obj"]
