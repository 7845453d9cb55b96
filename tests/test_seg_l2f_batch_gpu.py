"""GPU tests of the batched early-fixing windows of the segmentation flavour (lpbox_seg_batch_*, lpbox_hip.seg.SegBatch,
lpbox_hip.l2f.run_l2f_seg_batch).  Bar: per problem, bit for bit what the single-handle calls give (iterates, state, counters,
return codes, live sets, solution, energy) -- and, for two of the problems, what the CPU oracle in the kernels' order gives.

Every multi-problem test runs five problems cut from the two sample images: 400 nodes (one workgroup), 1 600 and 2 500 (several
workgroups, a ragged last one), 2 500 from the other image and one of 10^4."""
import functools
import os

import numpy as np
import pytest

from helpers import GOLDEN, bits_equal, scripted_fix_vec
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SCALARS = ("rho1", "gamma", "cur_obj", "std_obj", "cvg1", "cvg2", "obj_val", "best_bin_obj")
VECS = ("x", "z1", "z2", "b")
WS = 10


@functools.lru_cache(None)
def gray(name):
    from lpbox_hip.seg import load_gray
    return load_gray(os.path.join(GOLDEN, "seg", name))


def specs():
    # (with the scripted policy of the first test the 400-node problem ends all fixed in window 25, the first 2 500-node one stops in
    #  window 29, the 1 600-node one in 37, the 10^4-node one ends all fixed in 38, the flipped one runs all 40 windows)
    g0, g7 = gray("0.jpg"), gray("7.jpg")
    return [(np.ascontiguousarray(g7[:180, 250:]), 400), (np.ascontiguousarray(g0[150:, 200:]), 1600), (np.ascontiguousarray(g7[:180, 250:]), 2500),
            (np.ascontiguousarray(g0[:, ::-1]), 2500), (np.ascontiguousarray(g0[150:, 200:]), 10000)]


def make(k):
    from lpbox_hip.seg import PyLPboxADMMsolver
    img, nodes = specs()[k]
    s = PyLPboxADMMsolver(0, nodes, k)
    s.write_files = False
    s.set_image(img)
    return s


def make_all():
    return [make(k) for k in range(len(specs()))]


def batch_and_twins():
    """(SegBatch over five solvers after its solve_init, five twin solvers after their own solve_init)"""
    from lpbox_hip.seg import SegBatch
    ss, tw = make_all(), make_all()
    B = SegBatch(ss)
    assert B.solve_init() == 1
    for t in tw:
        t.solve_init()
    groups = [s.config()["groups"] for s in ss]
    assert min(groups) == 1 and max(groups) > 4 and ss[1].get_org_n() % (ss[1].config()["threads"] * ss[1].config()["elems_per_thread"])
    return B, ss, tw


def same_state(s, t, tag, live=None):
    """solver s (of the batch) against its twin t: return-code independent state, counters, live count"""
    assert s.get_n() == t.get_n(), tag
    assert s.counters() == t.counters(), tag
    for name in SCALARS + ("iter", "last_pcg"):
        a, b = s.debug_scalar(name), t.debug_scalar(name)
        assert a == b or (a != a and b != b), f"{tag}: {name} {a} {b}"
    for name in VECS:
        a, b = s.debug_vec(name), t.debug_vec(name)
        if live is not None:
            a, b = a[live], b[live]
        assert bits_equal(a, b), f"{tag}: {name}"


def same_window(s, t, tag, ws=WS):
    xs, xt = s.get_x_iters_2d(ws), t.get_x_iters_2d(ws)
    assert bits_equal(xs, xt), f"{tag}: x_iters {xs.shape} {xt.shape}"
    return xt


def same_end(s, t, tag):
    assert np.array_equal(s.get_x_sol(), t.get_x_sol()), tag
    assert s.get_obj() == t.get_obj() and s.stop() == t.stop(), tag


def steep_policy(x):
    """Row-wise scripted policy on the (rows, 5, 5) float32 windows: the sigmoid of a steep affine function of the mean of the last
    token's five iterates, written as element-wise float32 operations (the same bits whatever the number of rows)."""
    import torch
    t = x[:, -1, :].to(torch.float32)
    m = ((((t[:, 0] + t[:, 1]) + t[:, 2]) + t[:, 3]) + t[:, 4]) * 0.2
    return torch.sigmoid((m - 0.5) * 5.0)


def steep_scores_of(xiters):
    """steep_policy on a packed (rows, ws) float64 window (device tensor or numpy) -> float32 CUDA scores"""
    import torch
    X = torch.as_tensor(xiters, device="cuda")
    if X.shape[0] == 0:
        return torch.zeros(0, dtype=torch.float32, device="cuda")
    return steep_policy(X.unfold(1, 5, 1)[:, :5].to(torch.float32)).reshape(-1)


def guarded(scores, min_fix=10):
    from lpbox_hip.l2f import fix_vector_from_scores
    vec, f1, f0 = fix_vector_from_scores(scores)
    n = f1 + f0
    return vec, (n if n > min_fix else 0)


def test_batch_equals_single_handles_with_host_vectors():
    B, ss, tw = batch_and_twins()
    K = len(ss)
    nmax = max(s.get_org_n() for s in ss)
    vecs, nums = -np.ones((K, nmax)), np.zeros(K, np.int32)
    live = [np.arange(s.get_org_n()) for s in ss]
    done, stop_window, fixed_total = np.zeros(K, bool), [None] * K, np.zeros(K, int)
    for w in range(40):
        act = ~done
        B.set_active(act)
        rets = B.solve_iter_l2f(w * WS, (w + 1) * WS, vecs, nums)
        for k in range(K):
            tag = f"window {w}, problem {k}"
            if act[k]:
                if nums[k]:
                    live[k] = live[k][vecs[k, :len(live[k])] == -1]
                    fixed_total[k] += nums[k]
                rt = tw[k].solve_iter_l2f(w * WS, (w + 1) * WS, vecs[k], int(nums[k]))
                assert rets[k] == rt, tag
                if rt:
                    done[k], stop_window[k] = True, w
            else:
                assert rets[k] == 0, tag                       # an inactive problem's entry is not written
            same_state(ss[k], tw[k], tag, live[k])             # also for the problems that left many windows ago
            x = same_window(ss[k], tw[k], tag)
            nums[k] = 0
            if not done[k]:
                v, n = scripted_fix_vec(x, last=5)
                if n > 10:
                    vecs[k, :len(v)], nums[k] = v, n
        if done.all():
            break
    print("stop windows", stop_window, "fixed", fixed_total.tolist())
    assert np.count_nonzero(fixed_total) >= 2
    assert len(set(stop_window)) > 1
    for k in range(K):
        same_end(ss[k], tw[k], f"end, problem {k}")
    B.close()


def test_batch_equals_the_oracle():
    """Not against product code only: the 400- and one 2 500-node problem against the CPU oracle with its real compaction."""
    from lpbox_hip.seg import SegBatch
    ss = [make(0), make(2)]
    B = SegBatch(ss)
    B.solve_init()
    os_ = []
    for s in ss:
        cfg = s.config()
        o = O.SegOracle(0, s.numNodes, 0, order=O.ORDER_GPU, T=cfg["threads"], chunk=cfg["threads"] * cfg["elems_per_thread"])
        o.set_problem(s.get_problem())
        o.solve_init()
        os_.append(o)
    nmax = max(s.get_org_n() for s in ss)
    vecs, nums, done, fixed_any = -np.ones((2, nmax)), np.zeros(2, np.int32), np.zeros(2, bool), False
    for w in range(40):
        act = ~done
        B.set_active(act)
        rets = B.solve_iter_l2f(w * WS, (w + 1) * WS, vecs, nums)
        for k in np.flatnonzero(act):
            tag = f"window {w}, problem {k}"
            ro = os_[k].solve_iter_l2f(w * WS, (w + 1) * WS, vecs[k], int(nums[k]))
            assert rets[k] == ro and ss[k].get_n() == os_[k].get_n(), tag
            assert ss[k].counters() == (os_[k].total_outer_iters, os_[k].total_pcg_iters), tag
            nums[k] = 0
            if ro:
                done[k] = True
                continue
            xo = os_[k].get_x_iters_2d(WS)
            assert bits_equal(ss[k].get_x_iters_2d(WS), xo), tag
            left = os_[k].vec("left_idx").astype(int)
            for name in VECS:
                assert bits_equal(ss[k].debug_vec(name)[left], os_[k].vec(name)), f"{tag}: {name}"
            for name in SCALARS:
                assert ss[k].debug_scalar(name) == os_[k].scalar(name), f"{tag}: {name}"
            v, n = scripted_fix_vec(xo, last=5)
            if n > 10:
                vecs[k, :len(v)], nums[k], fixed_any = v, n, True
        if done.all():
            break
    assert fixed_any
    for k in range(2):
        assert np.array_equal(ss[k].get_x_sol(), os_[k].get_x_sol()) and ss[k].get_obj() == os_[k].get_obj(), k
    B.close()


def test_decisions_on_the_device():
    import torch
    B, ss, tw = batch_and_twins()
    K = len(ss)
    n0 = [s.get_org_n() for s in ss]
    rets, fixed = B.solve_iter_l2f_scores(0, WS, None)                  # scores = None fixes nothing
    assert not rets.any() and not fixed.any() and [s.get_n() for s in ss] == n0
    zero = np.zeros(max(n0))
    for k in range(K):
        assert tw[k].solve_iter_l2f(0, WS, zero, 0) == 0
        same_window(ss[k], tw[k], f"window 0, problem {k}")
    X, ro = B.x_iters_torch(WS)
    assert list(np.diff(ro)) == n0 and X.shape == (sum(n0), WS)
    f = np.float32
    sc = np.full(sum(n0), 0.5, f)
    rs = np.random.RandomState(5)

    def put(k, values):
        pos = rs.choice(n0[k], len(values), replace=False)
        sc[ro[k] + pos] = np.asarray(values, f)
    put(0, [0.95] * 6 + [0.05] * 4)                                     # exactly min_fix confident scores: nothing is fixed
    put(1, [0.95] * 5 + [0.05] * 6)                                     # min_fix + 1: all eleven are
    hi, lo, up, dn = f(0.9), f(0.1), f(np.inf), f(-np.inf)
    edge = [hi, np.nextafter(hi, up), np.nextafter(hi, dn), lo, np.nextafter(lo, up), np.nextafter(lo, dn), f(0), f(1), f(np.nan)]
    put(2, edge + [0.97] * 7 + [0.02] * 6)
    put(4, list(rs.choice(np.array([0.93, 0.07, 0.5, 0.91, 0.099], f), 3000)))
    rets, fixed = B.solve_iter_l2f_scores(WS, 2 * WS, torch.from_numpy(sc).cuda())
    expect = []
    for k in range(K):
        tag = f"window 1, problem {k}"
        vec, n = guarded(sc[ro[k]:ro[k + 1]])
        expect.append(n)
        assert tw[k].solve_iter_l2f(WS, 2 * WS, vec, n) == rets[k], tag
        assert fixed[k] == n and ss[k].get_n() == n0[k] - n, tag
        same_window(ss[k], tw[k], tag)                                  # the rows are the live variables in ascending order
        same_state(ss[k], tw[k], tag)
    # nextafter(0.9f, up) -> 1, nextafter(0.1f, down) -> 0, 0 -> 0, 1 -> 1; 0.9f, 0.1f themselves, their other neighbours and NaN: nothing
    assert expect[0] == 0 and expect[1] == 11 and expect[2] == 4 + 13 and expect[3] == 0 and expect[4] > 1000
    # one more window on the compacted problems, scores None again
    rets, fixed = B.solve_iter_l2f_scores(2 * WS, 3 * WS, None)
    assert not fixed.any()
    for k in range(K):
        assert tw[k].solve_iter_l2f(2 * WS, 3 * WS, zero, 0) == rets[k]
        same_window(ss[k], tw[k], f"window 2, problem {k}")
        same_state(ss[k], tw[k], f"window 2, problem {k}")
        same_end(ss[k], tw[k], f"end, problem {k}")
    B.close()


def test_all_fixed_problem_leaves_and_the_others_go_on():
    import torch
    B, ss, tw = batch_and_twins()
    K = len(ss)
    zero = np.zeros(max(s.get_org_n() for s in ss))
    B.solve_iter_l2f_scores(0, WS, None)
    for t in tw:
        t.solve_iter_l2f(0, WS, zero, 0)
    X, ro = B.x_iters_torch(WS)
    sc = np.full(int(ro[-1]), 0.5, np.float32)
    sc[ro[0]:ro[1]] = np.where(np.arange(ro[1] - ro[0]) % 3 == 0, 0.02, 0.97)      # every score of the 400-node problem says "fix"
    rets, fixed = B.solve_iter_l2f_scores(WS, 2 * WS, torch.from_numpy(sc).cuda())
    n400 = ss[0].get_org_n()
    vec, n = guarded(sc[ro[0]:ro[1]])
    assert n == n400 and fixed[0] == n400
    assert tw[0].solve_iter_l2f(WS, 2 * WS, vec, n) == rets[0] == 1
    assert ss[0].get_n() == tw[0].get_n() == 0 and ss[0].stop() == tw[0].stop() and ss[0].stop()[0] == 4     # SEG_STOP_ALLFIXED
    assert ss[0].get_x_iters_2d(WS).shape == tw[0].get_x_iters_2d(WS).shape == (0, WS)
    same_end(ss[0], tw[0], "all fixed")
    assert np.array_equal(ss[0].get_x_sol().ravel(), (vec == 1).astype(float))
    for k in range(1, K):
        assert tw[k].solve_iter_l2f(WS, 2 * WS, zero, 0) == rets[k] == 0 and fixed[k] == 0
        same_window(ss[k], tw[k], f"window 1, problem {k}")
    B.set_active(rets == 0)
    X, ro = B.x_iters_torch(WS)
    assert ro[1] == 0
    rets, fixed = B.solve_iter_l2f_scores(2 * WS, 3 * WS, steep_scores_of(X))
    for k in range(1, K):
        vec, n = guarded(steep_scores_of(tw[k].get_x_iters_2d(WS)).cpu().numpy())
        assert tw[k].solve_iter_l2f(2 * WS, 3 * WS, vec, n) == rets[k] and fixed[k] == n
        same_window(ss[k], tw[k], f"window 2, problem {k}")
        same_state(ss[k], tw[k], f"window 2, problem {k}")
    same_state(ss[0], tw[0], "all fixed, a window later")
    B.close()


def test_packed_buffer_rows_and_contents():
    B, ss, tw = batch_and_twins()
    K, mid = len(ss), 2
    n0 = [s.get_org_n() for s in ss]
    B.solve_iter_l2f_scores(0, WS, None)
    before = ss[mid].get_x_iters_2d(WS).copy()
    act = np.ones(K, bool)
    act[mid] = False
    B.set_active(act)
    rets, _ = B.solve_iter_l2f_scores(WS, 2 * WS, None)
    assert not rets.any()
    for ws in (WS, 4):
        X, ro = B.x_iters_torch(ws)
        rows = [n0[k] if act[k] else 0 for k in range(K)]
        assert list(ro) == [0] + list(np.cumsum(rows)) and X.shape == (sum(rows), ws)
        Xh = X.cpu().numpy()
        for k in range(K):
            if act[k]:
                assert bits_equal(Xh[ro[k]:ro[k + 1]], ss[k].get_x_iters_2d(ws)), (ws, k)
    assert bits_equal(ss[mid].get_x_iters_2d(WS), before) and ss[mid].debug_scalar("iter") == WS     # the inactive handle: untouched
    zero = np.zeros(max(n0))
    for k in range(K):
        for w in range(2 if act[k] else 1):
            tw[k].solve_iter_l2f(w * WS, (w + 1) * WS, zero, 0)
        same_window(ss[k], tw[k], f"problem {k}")
        same_state(ss[k], tw[k], f"problem {k}")
    B.close()


def _single_window(t, w, scores):
    vec, n = (np.zeros(t.get_org_n()), 0) if scores is None else guarded(scores.cpu().numpy())
    ret = t.solve_iter_l2f(w * WS, (w + 1) * WS, vec, n)
    return ret, (None if ret else steep_scores_of(t.get_x_iters_2d(WS)))


def test_mixing_batched_and_single_windows():
    import torch
    # all-single twins: five windows with the steep policy
    B, ss, tw = batch_and_twins()
    K = len(ss)
    ref = []
    for t in tw:
        sc, rec = None, []
        for w in range(5):
            ret, sc = _single_window(t, w, sc)
            rec.append((ret, t.get_n(), t.get_x_iters_2d(WS).copy()))
            if ret:
                break
        ref.append(rec)
    # (a) two batched windows with device-side fixes, then handles 1 and 4 alone
    sig = None
    for w in range(2):
        rets, fixed = B.solve_iter_l2f_scores(w * WS, (w + 1) * WS, sig)
        assert not rets.any()
        X, ro = B.x_iters_torch(WS)
        sig = steep_scores_of(X)
    assert ref[1][1][1] < ss[1].get_org_n() or ref[4][1][1] < ss[4].get_org_n(), "the policy fixed nothing in window 1"
    for k in (1, 4):
        assert ss[k].get_n() == ref[k][1][1]
        sc = sig[ro[k]:ro[k + 1]]
        for w in range(2, len(ref[k])):
            ret, sc = _single_window(ss[k], w, sc)
            assert (ret, ss[k].get_n()) == ref[k][w][:2] and bits_equal(ss[k].get_x_iters_2d(WS), ref[k][w][2]), (k, w)
        same_state(ss[k], tw[k], f"batched then single, problem {k}")
        same_end(ss[k], tw[k], f"batched then single, problem {k}")
    B.close()
    # (b) the reverse: two single windows per handle (the handles end on whatever ping-pong parity), then batched ones
    from lpbox_hip.seg import SegBatch
    ss = make_all()
    B = SegBatch(ss)
    B.solve_init()
    scs = []
    for k, s in enumerate(ss):
        sc = None
        for w in range(2):
            ret, sc = _single_window(s, w, sc)
            assert ret == 0 and bits_equal(s.get_x_iters_2d(WS), ref[k][w][2])
        scs.append(sc)
    X, ro = B.x_iters_torch(WS)
    assert bits_equal(steep_scores_of(X).cpu().numpy().astype(np.float64), torch.cat(scs).cpu().numpy().astype(np.float64))
    sig, done = steep_scores_of(X), np.zeros(K, bool)
    for w in range(2, 5):
        B.set_active(~done)
        rets, fixed = B.solve_iter_l2f_scores(w * WS, (w + 1) * WS, sig)
        for k in np.flatnonzero(~done):
            assert (rets[k], ss[k].get_n()) == ref[k][w][:2] and bits_equal(ss[k].get_x_iters_2d(WS), ref[k][w][2]), (k, w)
        done |= rets != 0
        if done.all():
            break
        B.set_active(~done)
        X, ro = B.x_iters_torch(WS)
        sig = steep_scores_of(X)
    for k in range(K):
        same_state(ss[k], tw[k], f"single then batched, problem {k}")
        same_end(ss[k], tw[k], f"single then batched, problem {k}")
    B.close()


def test_window_lengths_10_4_10_leave_no_stale_columns():
    """x_iters = Zero(n, 10) on every l2f call (SEGcpp:924), in the batch: a 4-iteration window after a 10-iteration one shows zeros in
    columns 4..9, in every handle's own getter and in the packed buffer."""
    B, ss, tw = batch_and_twins()
    zero = np.zeros(max(s.get_org_n() for s in ss))
    for (a, b) in ((0, 10), (10, 14), (14, 24)):
        rets = B.solve_iter_l2f(a, b, None, np.zeros(len(ss), np.int32))
        X, ro = B.x_iters_torch(WS)
        Xh = X.cpu().numpy()
        for k, (s, t) in enumerate(zip(ss, tw)):
            assert t.solve_iter_l2f(a, b, zero, 0) == rets[k]
            x = same_window(s, t, f"[{a},{b}) problem {k}")
            assert bits_equal(Xh[ro[k]:ro[k + 1]], x)
            assert x[:, :b - a].any() and not x[:, b - a:].any()
            same_state(s, t, f"[{a},{b}) problem {k}")
    B.close()


def test_the_loop_with_a_scripted_and_with_the_fused_policy():
    import torch

    from lpbox_hip.l2f import run_l2f_seg, run_l2f_seg_batch, run_l2f_seg_device
    from lpbox_hip.policy import FusedEarlyFixPolicy

    def numpy_policy(x):
        return steep_policy(torch.from_numpy(x).cuda()).cpu().numpy()
    got = run_l2f_seg_batch(make_all(), steep_policy, max_iter=80)
    ref = []
    for t in make_all():
        t.solve_init()
        ref.append(run_l2f_seg(t, numpy_policy, max_iter=80))
    print("scripted", got)
    assert got == ref
    assert max(r["fixed"] for r in got) > 10
    policy = FusedEarlyFixPolicy.random(tokens=5)
    got = run_l2f_seg_batch(make_all(), policy)
    ref = []
    for t in make_all():
        t.solve_init()
        ref.append(run_l2f_seg_device(t, policy))
    print("fused", got)
    assert got == ref
