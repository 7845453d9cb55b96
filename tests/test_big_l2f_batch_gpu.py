"""GPU tests of the early-fixing windows of a batch on the large route (lpbox_big_batch_iterate_l2f*, BigLpBatch.solve_iter_l2f*,
l2f.run_l2f_big_batch).  The contract is that a member gets the same bits in the batch as from
lpbox_big_iterate_l2f alone on the same fix vectors, so every comparison is bit for bit -- against the CPU oracle in the kernels'
reduction order (tests/big_l2f_batch_cases.py) and against a solo BigLp twin driven through solve_iter_l2f."""
import ctypes as C

import numpy as np
import pytest

import big_batch_cases as BC
import big_l2f_batch_cases as LC
from chain_cases import expected_resumes
from helpers import bits_equal

pytestmark = pytest.mark.gpu

E_BADARG, E_STATE, E_UNSUPPORTED = -2, -3, -7
WS = LC.WS


def make_batch(cases):
    from lpbox_hip.big import BigLpBatch
    B = BigLpBatch([BC.problem(n, s) for (n, s) in cases])
    assert B.solve_init() == 1
    for g in B.solvers:                                     # the geometry the shared oracle runs were made with
        assert (int(g.scalar("threads")), int(g.scalar("chunk"))) == (BC.T, BC.CHUNK) and g.scalar("folded_reductions") == 1.0
    assert int(B.scalar("compact_chunk")) == LC.COMPACT_CHUNK
    return B


def solo(n, seed):
    from lpbox_hip.big import BigLp
    g = BigLp(BC.problem(n, seed))
    g.solve_init()
    return g


def scripted_scores(X, last=5):
    """The scripted rule as a policy on the packed float64 rows: exactly 1.0, 0.0 or 0.5 per row (float32)."""
    import torch
    tail = X[:, -last:]
    one, zero = (tail > LC.RULE["hi"]).all(dim=1), (tail < LC.RULE["lo"]).all(dim=1)
    return torch.where(one, 1.0, torch.where(zero, 0.0, 0.5)).to(torch.float32)


def scores_from_vecs(vecs, off, device):
    """Scores that make deter_fix_2 decide what the host vectors say: 1.0 / 0.0 / 0.5; vecs[k] None: 0.5 for member k's rows."""
    import torch
    s = np.full(int(off[-1]), 0.5, np.float32)
    for k, v in enumerate(vecs):
        if v is not None:
            assert len(v) == off[k + 1] - off[k]
            s[off[k]:off[k + 1]] = np.where(v == 1, 1.0, np.where(v == 0, 0.0, 0.5))
    return torch.from_numpy(s).to(device)


def live_list(g):
    return np.flatnonzero(g.vec("live") == 1.0)


def test_eight_windows_host_vectors():
    """The five instances in one batch through solve_iter_l2f: after each window every member equals its oracle and its twin.  In windows
    6 and 7 some members fix and others do not."""
    B = make_batch(LC.MIXED)
    twins = [solo(n, s) for (n, s) in LC.MIXED]
    vecs, nums = [None] * len(LC.MIXED), [0] * len(LC.MIXED)
    for w in range(LC.NWIN):
        rets = B.solve_iter_l2f(WS * w, WS * (w + 1), vecs, nums)
        assert rets.dtype == np.int32 and len(rets) == len(LC.MIXED)
        X, off = B.x_iters_torch(WS)
        Xh = X.cpu().numpy()
        for k, (n, s) in enumerate(LC.MIXED):
            tag = f"n={n} seed={s} window {w}"
            snap = LC.oracle_l2f(n, s)[0][w]
            assert nums[k] == snap["num"], tag
            assert rets[k] == snap["ret"] == twins[k].solve_iter_l2f(WS * w, WS * (w + 1), vecs[k], nums[k]), tag
            LC.same_as_snapshot(B[k], snap, tag, x_iters=Xh[off[k]:off[k + 1]])
            LC.same_as_twin(B[k], twins[k], tag)
            assert np.array_equal(live_list(B[k]), snap["left"]), tag
        vecs, nums = map(list, zip(*(LC.guarded(B[k].get_x_iters_2d(WS)) for k in range(len(LC.MIXED)))))
    for k, (n, s) in enumerate(LC.MIXED):
        assert np.array_equal(B[k].local_x_sol(), LC.oracle_l2f(n, s)[1])
    assert B.scalar("fix_launches") == 8 * 7 and B.scalar("packs") == LC.NWIN and B.scalar("parity_copies") == 0
    for t in twins:
        t.close()
    B.close()


def test_device_decided_form():
    """The same batch through solve_iter_l2f_scores with the scripted rule as a three-valued policy on the device: `fixed` and every
    state equal the host-vector run's (the oracle's); the compaction on the device leaves the oracle's row order."""
    B = make_batch(LC.MIXED)
    sig = None
    for w in range(LC.NWIN):
        rets, fx = B.solve_iter_l2f_scores(WS * w, WS * (w + 1), sig, LC.C_HI, LC.MIN_FIX)
        X, off = B.x_iters_torch(WS)
        Xh = X.cpu().numpy()
        for k, (n, s) in enumerate(LC.MIXED):
            tag = f"n={n} seed={s} window {w}"
            snap = LC.oracle_l2f(n, s)[0][w]
            assert (rets[k], fx[k]) == (snap["ret"], snap["num"]), tag
            assert np.array_equal(live_list(B[k]), snap["left"]), tag
            LC.same_as_snapshot(B[k], snap, tag, x_iters=Xh[off[k]:off[k + 1]])
        sig = scripted_scores(X)
        assert set(np.unique(sig.cpu().numpy())) <= {0.0, 0.5, 1.0}
    for k, (n, s) in enumerate(LC.MIXED):
        assert np.array_equal(B[k].local_x_sol(), LC.oracle_l2f(n, s)[1])
    assert B.scalar("fix_launches") == 8 * 7 and B.scalar("packs") == LC.NWIN
    B.close()


def test_guard_nan_and_null_scores_fix_nothing():
    import torch
    cases = LC.MIXED[:2]
    B = make_batch(cases)
    never = [LC.oracle_l2f(n, s, nwin=4, min_fix=10 ** 9)[0] for (n, s) in cases]
    assert all(sn["num"] == 0 for snaps in never for sn in snaps)
    rets, fx = B.solve_iter_l2f_scores(0, WS, None, LC.C_HI, LC.MIN_FIX)
    for w in (1, 2, 3):
        X, off = B.x_iters_torch(WS)
        if w == 1:
            sig, min_fix = scripted_scores(X), 10 ** 9                  # the rule would fix 141 / 227 variables: the guard holds them back
            assert int((sig != 0.5).sum()) == sum(LC.FIXES[c][0] for c in cases)
        elif w == 2:
            sig, min_fix = torch.full((X.shape[0],), float("nan"), dtype=torch.float32, device=X.device), 0
        else:
            sig, min_fix = None, 0
        rets, fx = B.solve_iter_l2f_scores(WS * w, WS * (w + 1), sig, LC.C_HI, min_fix)
        assert not fx.any() and not rets.any()
        for k, (n, s) in enumerate(cases):
            LC.same_as_snapshot(B[k], never[k][w], f"n={n} window {w}: nothing fixed")
            assert B[k].get_n() == n
    assert B.scalar("fix_launches") == 0
    B.close()


def test_shrinking_live_list():
    """n = 2 * chunk + 37 beside two small members, the two forms in turn: the live list shrinks to 4097, 4096, 4095, 1 and 0 entries; the
    member that reaches 0 returns 1 with the all-fixed stop and is deactivated, the others run two more windows."""
    ws = LC.SHRINK_WS
    small = [(300, 0), (513, 2)]
    cases = [LC.SHRINK] + small
    B = make_batch(cases)
    twins = [solo(n, s) for (n, s) in cases]
    big_snaps, big_sol = LC.oracle_shrink()
    never = [LC.oracle_l2f(n, s, nwin=8, ws=ws, min_fix=10 ** 9)[0] for (n, s) in small]
    nwin = len(big_snaps)

    def check(w, members):
        X, off = B.x_iters_torch(ws)
        Xh = X.cpu().numpy()
        for k in members:
            snap = big_snaps[w] if k == 0 else never[k - 1][w]
            tag = f"member {k} window {w}"
            LC.same_as_snapshot(B[k], snap, tag, ws=ws, x_iters=Xh[off[k]:off[k + 1]])
            LC.same_as_twin(B[k], twins[k], tag, ws=ws)
            assert np.array_equal(live_list(B[k]), snap["left"]), tag
        return X, off

    for w in range(nwin):
        vec, num = big_snaps[w]["vec"], big_snaps[w]["num"]
        if w % 2 == 0:
            rets = B.solve_iter_l2f(ws * w, ws * (w + 1), [vec, None, None], [num, 0, 0])
        else:
            rets, fx = B.solve_iter_l2f_scores(ws * w, ws * (w + 1), scores_from_vecs([vec, None, None], off, X.device), LC.C_HI, 0)
            assert list(fx) == [num, 0, 0]
        for k in range(3):
            assert twins[k].solve_iter_l2f(ws * w, ws * (w + 1), vec if k == 0 else None, num if k == 0 else 0) == rets[k]
        assert list(rets) == [big_snaps[w]["ret"], 0, 0]
        X, off = check(w, range(3))
    assert rets[0] == 1 and int(B[0].scalar("stop")) == 4 and B[0].get_n() == 0                  # LP_STOP_ALLFIXED
    assert np.array_equal(B[0].local_x_sol(), big_sol)
    B.set_active([False, True, True])
    before = LC.state_of(B[0], ws)
    for w in (nwin, nwin + 1):
        rets = B.solve_iter_l2f(ws * w, ws * (w + 1), None, [0, 0, 0])
        for k in (1, 2):
            assert twins[k].solve_iter_l2f(ws * w, ws * (w + 1), None, 0) == rets[k] == 0
        X, off = check(w, (1, 2))
        assert off[1] == off[0] == 0
    assert LC.same_state(before, LC.state_of(B[0], ws))
    for t in twins:
        t.close()
    B.close()


def test_resumed_pcg_with_fixes(monkeypatch):
    """LPBOX_BIG_KMAX=4: window 0 needs up to 22 PCG iterations per outer iteration, the later ones 4 to 9 -- the chain resumes for all,
    a member whose PCG is complete falls through, and the fix prologue sits between resumed windows."""
    monkeypatch.setenv("LPBOX_BIG_KMAX", "4")
    cases = [(300, 0), (1100, 4), (2600, 7)]
    B = make_batch(cases)
    assert int(B.scalar("kmax")) == 4
    vecs, nums = [None] * 3, [0] * 3
    for w in range(3):
        rets = B.solve_iter_l2f(WS * w, WS * (w + 1), vecs, nums)
        for k, (n, s) in enumerate(cases):
            snap = LC.oracle_l2f(n, s)[0][w]
            assert rets[k] == snap["ret"] and nums[k] == snap["num"]
            LC.same_as_snapshot(B[k], snap, f"kmax 4, n={n} window {w}")
        vecs, nums = map(list, zip(*(LC.guarded(B[k].get_x_iters_2d(WS)) for k in range(3))))
    for k, (n, s) in enumerate(cases):
        trace = sum((LC.oracle_l2f(n, s)[0][w]["trace"] for w in range(3)), ())
        want = expected_resumes(trace, 4)
        assert want >= 20 and B[k].scalar("pcg_resumes") == want == B.scalar(f"pcg_resumes_{k}"), (n, want)
    assert int(B.scalar("kmax")) == 4
    B.close()


def test_activity_mixing_with_solo_windows_and_parity(monkeypatch):
    """A member inactive for a window is untouched.  A member runs a window of its own between two batch windows, after a fix that was
    decided on the device: its host live list follows on demand, and with an even forced launch count the window without a fix flips its
    state ping-pong an odd number of times, so the batch copies its state across before the next window."""
    monkeypatch.setenv("LPBOX_BIG_KMAX", "24")
    cases = LC.MIXED[:3]
    B = make_batch(cases)
    sched = [((0, 10, False), (10, 20, True), (30, 40, True)),
             ((0, 10, False), (10, 20, True), (20, 30, False), (30, 40, True)),
             ((0, 10, False), (30, 40, True))]
    snaps = [LC.oracle_schedule(n, s, sched[k])[0] for k, (n, s) in enumerate(cases)]
    rets, fx = B.solve_iter_l2f_scores(0, 10, None, LC.C_HI, LC.MIN_FIX)
    for k in range(3):
        LC.same_as_snapshot(B[k], snaps[k][0], f"member {k} window 0")
    B.set_active([True, True, False])
    before, launches2 = LC.state_of(B[2]), B[2].scalar("launches")
    X, off = B.x_iters_torch(WS)
    assert off[3] == off[2] and B.scalar("active") == 2
    rets, fx = B.solve_iter_l2f_scores(10, 20, scripted_scores(X), LC.C_HI, LC.MIN_FIX)
    assert (rets[2], fx[2]) == (0, 0) and list(fx[:2]) == [snaps[0][1]["num"], snaps[1][1]["num"]] and min(fx[:2]) > 0
    assert LC.same_state(before, LC.state_of(B[2])) and B[2].scalar("launches") == launches2
    for k in (0, 1):
        LC.same_as_snapshot(B[k], snaps[k][1], f"member {k} window 1")
    copies = B.scalar("parity_copies")
    assert B[1].solve_iter_l2f(20, 30, None, 0) == snaps[1][2]["ret"]           # alone, on the list the device compacted
    LC.same_as_snapshot(B[1], snaps[1][2], "member 1, window of its own")
    assert B[1].get_n() == cases[1][0] - snaps[1][1]["num"]
    B.set_active(None)
    X, off = B.x_iters_torch(WS)
    assert [int(off[k + 1] - off[k]) for k in range(3)] == [B[k].get_n() for k in range(3)]
    rets, fx = B.solve_iter_l2f_scores(30, 40, scripted_scores(X), LC.C_HI, LC.MIN_FIX)
    assert B.scalar("parity_copies") == copies + 1
    for k in range(3):
        assert (rets[k], fx[k]) == (snaps[k][-1]["ret"], snaps[k][-1]["num"])
        LC.same_as_snapshot(B[k], snaps[k][-1], f"member {k} last window")
    # batched, then solo with a host vector on the list the device compacted
    vec, num = LC.guarded(B[0].get_x_iters_2d(WS))
    o_ret = B[0].solve_iter_l2f(40, 50, vec, num)
    extra = LC.oracle_schedule(*cases[0], sched[0] + ((40, 50, True),))[0][-1]
    assert o_ret == extra["ret"] and num == extra["num"]
    LC.same_as_snapshot(B[0], extra, "member 0 alone after the batch")
    B.close()


def test_batch_of_one_equals_the_solo_handle():
    (n, s) = LC.MIXED[2]
    B, t = make_batch([(n, s)]), solo(n, s)
    sig, vec, num = None, None, 0
    for w in range(3):
        rets, fx = B.solve_iter_l2f_scores(WS * w, WS * (w + 1), sig, LC.C_HI, LC.MIN_FIX)
        assert rets[0] == t.solve_iter_l2f(WS * w, WS * (w + 1), vec, num) and fx[0] == num
        LC.same_as_twin(B[0], t, f"B = 1 window {w}")
        LC.same_as_snapshot(B[0], LC.oracle_l2f(n, s)[0][w], f"B = 1 window {w}")
        X, off = B.x_iters_torch(WS)
        sig = scripted_scores(X)
        vec, num = LC.guarded(t.get_x_iters_2d(WS))
    t.close()
    B.close()


def test_many_small_problems():
    """300 members of n = 300, three windows with fixes decided on the device: the grid's y-extent exceeds the CU count."""
    cases = [(300, seed) for seed in range(300)]
    B = make_batch(cases)
    sig = None
    for w in range(3):
        rets, fx = B.solve_iter_l2f_scores(WS * w, WS * (w + 1), sig, LC.C_HI, LC.MIN_FIX)
        X, off = B.x_iters_torch(WS)
        Xh = X.cpu().numpy()
        for k, (n, s) in enumerate(cases):
            snap = LC.oracle_l2f(n, s, nwin=3)[0][w]
            assert (rets[k], fx[k]) == (snap["ret"], snap["num"]), (k, w)
            assert bits_equal(Xh[off[k]:off[k + 1]], snap["x_iters"]), (k, w)
        sig = scripted_scores(X)
    assert fx.sum() > 0
    for k, (n, s) in enumerate(cases):
        LC.same_as_snapshot(B[k], LC.oracle_l2f(n, s, nwin=3)[0][2], f"member {k}")
    B.close()


def test_refusals_leave_everything_as_it_was():
    import torch
    from lpbox_hip import _lib
    from lpbox_hip._lib import LpboxError
    L = _lib.load()
    cases = [(300, 0), (300, 1), (513, 2)]
    B = make_batch(cases)
    rets_c, fixed_c = (C.c_int * 3)(), (C.c_int * 3)()

    def refused(call, code, *texts):
        states = [LC.state_of(g) for g in B.solvers] if all(g.scalar("iter") > 0 for g in B.solvers) else None
        launches = B.scalar("launches")
        with pytest.raises(LpboxError) as e:
            call()
        assert e.value.code == code and all(t in str(e.value) for t in texts), str(e.value)
        assert B.scalar("launches") == launches
        if states:
            assert all(LC.same_state(st, LC.state_of(g)) for st, g in zip(states, B.solvers))

    def raw_scores(t):
        _lib.check(L.lpbox_big_batch_iterate_l2f_scores(B._h, 10, 20, C.c_void_p(t.data_ptr()), 0.9, 0.1, 10, C.cast(rets_c, C.c_void_p),
                                                        C.cast(fixed_c, C.c_void_p)), "scores")

    some = torch.full((1113,), 0.5, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    refused(lambda: raw_scores(some), E_STATE, "has not been called since the last window")          # scores without a pack
    assert B.solve_iter_l2f(0, 10, None, [0, 0, 0]).tolist() == [0, 0, 0]
    refused(lambda: raw_scores(some), E_STATE, "has not been called since the last window")
    refused(lambda: B.solve_iter_l2f(10, 511, None, [0, 0, 0]), E_BADARG, "501")
    refused(lambda: B.solve_iter_l2f_scores(10, 511, None), E_BADARG, "501")
    vecs, nums = map(list, zip(*(LC.guarded(g.get_x_iters_2d(WS)) for g in B.solvers)))
    assert nums[0] > 10 and nums[2] > 10
    refused(lambda: B.solve_iter_l2f(10, 20, vecs, nums[:2] + [nums[2] + 1]), E_BADARG, "problem 2 of the batch", f"vec fixes {nums[2]}")
    refused(lambda: B.solve_iter_l2f(10, 20, vecs, [nums[0], 301, nums[2]]), E_BADARG, "problem 1 of the batch", "outside")
    refused(lambda: B.solve_iter_l2f(10, 20, None, nums), E_BADARG, "problem 0 of the batch", "fix vector missing")
    B.set_active([True, True, False])
    X, off = B.x_iters_torch(WS)
    B.set_active(None)                                                                              # the active set grew after the pack
    refused(lambda: B.solve_iter_l2f_scores(10, 20, scripted_scores(X)), E_STATE, "problem 2 of the batch", "packed buffer")
    assert L.lpbox_big_set_record(B[1]._h, 1) == 0
    refused(lambda: B.solve_iter_l2f(10, 20, vecs, nums), E_UNSUPPORTED, "problem 1", "recording")
    refused(lambda: B.solve_iter_l2f_scores(10, 20, None), E_UNSUPPORTED, "problem 1", "recording")
    assert L.lpbox_big_set_record(B[1]._h, 0) == 0
    with pytest.raises(LpboxError) as e:
        B.x_iters_torch(501)
    assert e.value.code == E_BADARG
    # after the refusals the next valid call gives the oracle's bits
    rets = B.solve_iter_l2f(10, 20, vecs, nums)
    for k, (n, s) in enumerate(cases):
        snap = LC.oracle_l2f(n, s, nwin=2)[0][1]
        assert rets[k] == snap["ret"] and nums[k] == snap["num"]
        LC.same_as_snapshot(B[k], snap, f"member {k} after the refusals")
    # the plain window keeps refusing a member with fixed variables
    refused(lambda: B.solve_iter(20, 30), E_UNSUPPORTED, "problem 0", "fixed variables")
    B.close()


def test_run_l2f_big_batch_returns_what_run_l2f_big_returns():
    from lpbox_hip import l2f
    from lpbox_hip.big import BigLp
    import torch
    cases = [(300, 0), (1100, 4), (2600, 7)]

    def policy(x):                                   # float32 (rows, 5, 2): the scripted rule on the last five iterates
        tail = x.reshape(x.shape[0], -1)[:, -5:]
        return torch.where((tail > 0.95).all(dim=1), 1.0, torch.where((tail < 0.05).all(dim=1), 0.0, 0.5))

    got = l2f.run_l2f_big_batch([BC.problem(n, s) for (n, s) in cases], policy, ws=WS, max_iter=80, tokens=5)
    assert len(got) == 3
    for k, (n, s) in enumerate(cases):
        g = BigLp(BC.problem(n, s), use_torch_stream=True)
        g.solve_init()
        want = l2f.run_l2f_big(g, policy, ws=WS, max_iter=80, tokens=5)
        g.close()
        assert set(got[k]) == {"objective", "windows", "fixed", "live"} == set(want)
        assert got[k] == want and got[k]["fixed"] > 0 and got[k]["live"] == n - got[k]["fixed"], (k, got[k], want)
