"""The LP batch's early-fixing window with the fix decided on the device (lpbox_iterate_l2f_scores, lp_decide_fix_kernel) and the row
table a device policy reads the iterates through (lpbox_get_x_iters_rows_device, lp_row_offsets_kernel): against the CPU oracle
through the whole loop, against the vector form window by window, the rule's edges, isolation between instances, the other kernel
modes, and the loop with the fused policy.  Everything is compared bit for bit."""
import functools
import os

import numpy as np
import pytest

from helpers import GOLDEN, bits_equal, oracle_for
from lpbox_hip import l2f
from lpbox_hip.lp import LpBatch, LpboxError

pytestmark = pytest.mark.gpu

E_STATE = -3
WS = 100


def _last_iterate(x):                 # the scripted policy of tests/test_l2f_loop_gpu.py: score = newest iterate (exact in float32)
    return x[:, -1, -1]


@functools.lru_cache(maxsize=None)
def first_instances(name, k=8):
    """The first k instances of a tests/golden/lp_*.npz fixture, as oracle.load_lp_batch splits them (every array is read once)."""
    d = {key: v for key, v in np.load(os.path.join(GOLDEN, name)).items()}
    out, cp, ri, pr = [], 0, 0, 0
    for n, l, nnz in zip(d["n"][:k].tolist(), d["l"][:k].tolist(), d["nnz"][:k].tolist()):
        out.append(dict(n=n, l=l, colptr=d["colptr"][cp:cp + n + 1].astype(np.int32), rowidx=d["rowidx"][ri:ri + nnz].astype(np.int32),
                        b=-1.0 * d["price"][pr:pr + n]))
        cp, ri, pr = cp + n + 1, ri + nnz, pr + n
    return out


def s60():
    return first_instances("lp_20_60_seed0.npz")


def s500():
    return first_instances("lp_100_500_seed0.npz")


def state(b, i):
    return dict(n=b.get_n(i), counters=b.counters(i), stop=b.stop(i), **{v: b.debug_vec(v, i) for v in ("x", "z1", "z2", "live")})


def same_state(a, b, tag):
    assert a["n"] == b["n"] and a["counters"] == b["counters"] and a["stop"] == b["stop"], tag
    for v in ("x", "z1", "z2", "live"):
        assert bits_equal(a[v], b[v]), (tag, v)


def last_scores(b, i, ws=WS):
    """float32 score per live variable of instance i: its newest iterate."""
    return b.get_x_iters_2d(ws, i)[:, -1].astype(np.float32)


def upload(per_instance):
    import torch
    return torch.from_numpy(np.concatenate(per_instance).astype(np.float32)).cuda()


def vec_request(B, nmax, scores, min_fix, C=0.9):
    """What run_l2f_batch hands the vector form: fix_vector_from_scores per instance with the `<= min_fix -> none` guard."""
    vecs, nums = np.zeros((B, nmax)), np.zeros(B, np.int32)
    for i, s in scores.items():
        v, f1, f0 = l2f.fix_vector_from_scores(s, C)
        if f1 + f0 > min_fix:
            vecs[i, :len(v)] = v
            nums[i] = f1 + f0
    return vecs, nums


# ---- 1. the loop against the oracle ----
@pytest.mark.parametrize("case", ["mixed_60_500", "one_2000"])
def test_device_loop_matches_per_instance_oracle(case):
    if case == "mixed_60_500":       # one slot per thread; min_fix 3: the n = 60 instances rarely have more than 10 confident variables at once
        insts, kw = [s60()[0], s500()[0], s60()[1], s500()[1]], dict(min_fix=3, max_iter=1000)
    else:                            # four slots per thread: a storage position is not the thread index
        insts, kw = first_instances("lp_500_2000_seed0.npz", 1), dict(min_fix=10, max_iter=400)
    b = LpBatch(insts)
    b.solve_init()
    assert b.config()["elems_per_thread"] == (1 if case == "mixed_60_500" else 4)
    res = l2f.run_l2f_batch_device(b, _last_iterate, ws=WS, **kw)
    for i, I in enumerate(insts):
        o = oracle_for(b, i, I)
        ro = l2f.run_l2f(o, _last_iterate, ws=WS, **kw)
        assert ro["fixed"] > 0, "the oracle run fixed nothing: the case shows nothing"
        assert res["objective"][i] == ro["objective"] and res["infeasible"][i] == ro["infeasible"], i
        assert res["instance_windows"][i] == ro["windows"] and res["fixed"][i] == ro["fixed"], i
        assert bits_equal(b.get_x_sol(i).ravel(), o.get_x_sol().ravel()), i
    assert res["windows"] == res["instance_windows"].max()


# ---- 2. the vector form, window by window ----
def test_same_as_the_vector_form_window_by_window():
    insts = s500()[:6]
    a, b = LpBatch(insts), LpBatch(insts)
    a.solve_init(); b.solve_init()
    B, done, sig, applied = len(insts), np.zeros(6, bool), None, 0
    vecs, nums = np.zeros((B, 500)), np.zeros(B, np.int32)
    for w in range(8):
        a.set_active(~done); b.set_active(~done)
        ra = a.solve_iter_l2f(WS * w, WS * (w + 1), vecs, nums)
        rb, fixed = b.solve_iter_l2f_scores(WS * w, WS * (w + 1), sig, 0.9, 10)
        assert np.array_equal(ra, rb) and np.array_equal(fixed, nums), w
        applied += int(fixed.sum())
        for i in range(B):
            same_state(state(a, i), state(b, i), (w, i))
            assert bits_equal(a.get_x_iters_2d(WS, i), b.get_x_iters_2d(WS, i)), (w, i)
        done |= ra != 0
        if done.all():
            break
        a.set_active(~done); b.set_active(~done)
        scores = {int(i): last_scores(a, int(i)) for i in np.flatnonzero(~done)}
        vecs, nums = vec_request(B, 500, scores, 10)
        _, _, first = b.x_iters_rows_torch(WS)
        assert np.array_equal(np.diff(first), [0 if done[i] else a.get_n(i) for i in range(B)])
        sig = upload([scores[i] for i in sorted(scores)])
    assert applied > 0 and w >= 2


# ---- 3. the rule's edges ----
def test_rule_edges_in_one_batch():
    insts = s60()[:4]
    b = LpBatch(insts)
    b.solve_init()
    b.solve_iter_l2f_scores(0, 10)
    _, row_off, first = b.x_iters_rows_torch(10)
    assert first.tolist() == [0, 60, 120, 180, 240] and row_off.numel() == 240
    hi, lo = np.float32(0.9), np.float32(0.1)
    up, dn = np.nextafter(hi, np.float32(1)), np.nextafter(lo, np.float32(0))
    assert up > hi and dn < lo and up.dtype == np.float32
    S = np.full((4, 60), 0.5, np.float32)
    S[0, 3:13:2], S[0, 20:25] = 0.95, 0.05                 # exactly min_fix = 10 confident scores: nothing is fixed
    S[1, 3:13:2], S[1, 20:26] = 0.95, 0.05                 # min_fix + 1: fixed
    S[2, :15], S[2, 30:45] = hi, lo                        # equal to the thresholds (as float32): not confident
    S[3, 1:7], S[3, 10:16] = up, dn                        # the neighbouring float32 values: confident
    S[3, 20:25], S[3, 30:33], S[3, 40:43] = np.nan, np.inf, -np.inf
    rets, fixed = b.solve_iter_l2f_scores(10, 20, upload(list(S)), 0.9, 10)
    for i in range(4):
        vec, f1, f0 = l2f.fix_vector_from_scores(S[i])
        k = f1 + f0
        assert k == (10, 11, 0, 18)[i]
        want = k if k > 10 else 0
        assert fixed[i] == want and b.get_n(i) == 60 - want, i
        live, x = b.debug_vec("live", i), b.debug_vec("x", i)
        if want:
            assert np.array_equal(live != 0, vec == -1), i
            assert np.all(x[vec == 1] == 1.0) and np.all(x[vec == 0] == 0.0), i
        else:
            assert np.all(live != 0), i
    vec3 = l2f.fix_vector_from_scores(S[3])[0]
    assert np.all(vec3[20:25] == -1) and np.all(vec3[30:33] == 1) and np.all(vec3[40:43] == 0)      # NaN, +inf, -inf


# ---- 4. isolation ----
def test_guarded_and_parked_instances_are_left_alone():
    insts = [s60()[0], s60()[1], s500()[0], s60()[2]]
    b = LpBatch(insts)
    b.solve_init()
    b.solve_iter_l2f_scores(0, WS)
    b.set_active([True, True, False, True])
    parked = state(b, 2)
    _, row_off, first = b.x_iters_rows_torch(WS)
    assert first.tolist() == [0, 60, 120, 120, 180]          # the parked instance owns no rows
    S = np.full((3, 60), 0.5, np.float32)
    S[0, 50:60] = 0.95                                        # 10 confident: under the guard
    S[1, :12], S[1, 48:60] = 0.05, 0.95                       # 24: fixes, first and last rows next to its neighbours' ranges
    S[2, 0:10] = 0.05                                         # under the guard too
    rets, fixed = b.solve_iter_l2f_scores(WS, 2 * WS, upload(list(S)), 0.9, 10)
    assert fixed.tolist() == [0, 24, 0, 0]
    assert [b.get_n(i) for i in range(4)] == [60, 36, 500, 60]
    live1 = b.debug_vec("live", 1)
    assert not live1[:12].any() and not live1[48:].any() and live1[12:48].all()
    # the codes of the guarded instances were written but never applied -- not in the next window either
    rets, fixed = b.solve_iter_l2f_scores(2 * WS, 3 * WS)
    assert not fixed.any() and [b.get_n(i) for i in range(4)] == [60, 36, 500, 60]
    assert b.debug_vec("live", 0).all() and b.debug_vec("live", 3).all()
    same_state(parked, state(b, 2), "parked instance")
    # ... and a guarded instance ran exactly the windows of a batch that never saw a score
    c = LpBatch(insts)
    c.solve_init()
    c.solve_iter_l2f(0, WS)
    c.set_active([True, True, False, True])
    for w in (1, 2):
        c.solve_iter_l2f(WS * w, WS * (w + 1))
    for i in (0, 3):
        same_state(state(c, i), state(b, i), ("guarded", i))


def test_mask_change_after_the_table_is_refused_and_touches_nothing():
    insts = s60()[:3]
    b = LpBatch(insts)
    b.solve_init()
    b.solve_iter_l2f_scores(0, WS)
    b.x_iters_rows_torch(WS)
    sig = upload([np.full(180, 0.95, np.float32)])
    b.set_active([True, True, True])                          # repeats the mask: the table stays valid
    before = [state(b, i) for i in range(3)]
    b.set_active([True, False, True])
    b._table_rows = 180                                       # (get past the Python-side length check: the library must refuse)
    with pytest.raises(LpboxError, match="lpbox_set_active changed the active instances") as e:
        b.solve_iter_l2f_scores(WS, 2 * WS, sig, 0.9, 10)
    assert e.value.code == E_STATE
    for i in range(3):
        same_state(before[i], state(b, i), i)
        assert b.get_x_iters_2d(WS, i).shape == (60, WS)
    # a new table for the new mask, and the loop goes on
    _, row_off, first = b.x_iters_rows_torch(WS)
    assert first.tolist() == [0, 60, 60, 120]
    rets, fixed = b.solve_iter_l2f_scores(WS, 2 * WS, upload([np.full(120, 0.95, np.float32)]), 0.9, 10)
    assert fixed.tolist() == [60, 0, 60] and rets.tolist()[0] == 1 and rets.tolist()[2] == 1
    same_state(before[1], state(b, 1), "parked")
    # without a table since the last window the scores are refused as well
    b._table_rows = 120
    with pytest.raises(LpboxError, match="has not been called since the last window") as e:
        b.solve_iter_l2f_scores(2 * WS, 3 * WS, sig[:120], 0.9, 10)
    assert e.value.code == E_STATE
    _, row_off, first = b.x_iters_rows_torch(WS)              # two instances have no live variable left, one is parked
    assert first.tolist() == [0, 0, 0, 0] and row_off.numel() == 0
    with pytest.raises(ValueError):                           # Python refuses a wrong length before the library is asked
        b.solve_iter_l2f_scores(2 * WS, 3 * WS, sig[:7], 0.9, 10)


# ---- 5. everything fixed ----
def test_all_fixed_matches_the_vector_form():
    insts = s60()[:2]
    a, b = LpBatch(insts), LpBatch(insts)
    a.solve_init(); b.solve_init()
    a.solve_iter_l2f(0, WS); b.solve_iter_l2f_scores(0, WS)
    S = np.full((2, 60), 0.5, np.float32)
    S[0] = np.where(last_scores(a, 0) >= 0.5, 0.95, 0.05)
    vecs, nums = vec_request(2, 60, {0: S[0], 1: S[1]}, 10)
    assert nums.tolist() == [60, 0]
    b.x_iters_rows_torch(WS)
    ra = a.solve_iter_l2f(WS, 2 * WS, vecs, nums)
    rb, fixed = b.solve_iter_l2f_scores(WS, 2 * WS, upload(list(S)), 0.9, 10)
    assert ra.tolist() == rb.tolist() and rb[0] == 1 and fixed.tolist() == [60, 0]
    assert a.stop(0) == b.stop(0) and b.stop(0)[0] == 4
    for i in range(2):
        same_state(state(a, i), state(b, i), i)
        assert bits_equal(a.get_x_sol(i), b.get_x_sol(i)), i


# ---- 6. the other kernel modes ----
def _mode_batch(mode):
    if mode == "reference_500":
        return LpBatch(s500()[:1], order="reference"), 10
    if mode == "direct_500":
        b = LpBatch(s500()[1:2])
        b.set_x_update("direct")
        return b, 10
    b = LpBatch(batch=2, order="reference")                   # the valued fixture files <k>_7 (40 variables), with min_fix 0
    for i, k in enumerate((2, 3)):
        b.read_file(i, 1, k, 7, root=GOLDEN)
    return b, 0


@pytest.mark.parametrize("mode", ["reference_500", "valued_7", "direct_500"])
def test_other_modes_two_windows_against_the_vector_form(mode):
    (a, min_fix), (b, _) = _mode_batch(mode), _mode_batch(mode)
    a.solve_init(); b.solve_init()
    if mode == "valued_7":
        assert "vals" in b.get_problem(0) and "vals" in b.get_problem(1)
    B = a.B
    ra, (rb, fixed) = a.solve_iter_l2f(0, WS), b.solve_iter_l2f_scores(0, WS)
    assert ra.tolist() == rb.tolist() and not fixed.any()
    scores = {}
    for i in range(B):                                        # confident about the first half of the live variables, undecided about the rest
        x = last_scores(a, i)
        s = np.full(len(x), 0.5, np.float32)
        h = (len(x) + 1) // 2
        s[:h] = np.where(x[:h] >= 0.5, 0.95, 0.05)
        scores[i] = s
        same_state(state(a, i), state(b, i), ("window 0", i))
    nmax = max(a.get_org_n(i) for i in range(B))
    vecs, nums = vec_request(B, nmax, scores, min_fix)
    assert nums.all()
    b.x_iters_rows_torch(WS)
    ra = a.solve_iter_l2f(WS, 2 * WS, vecs, nums)
    rb, fixed = b.solve_iter_l2f_scores(WS, 2 * WS, upload([scores[i] for i in range(B)]), 0.9, min_fix)
    assert ra.tolist() == rb.tolist() and fixed.tolist() == nums.tolist()
    for i in range(B):
        same_state(state(a, i), state(b, i), ("window 1", i))
        assert bits_equal(a.get_x_iters_2d(WS, i), b.get_x_iters_2d(WS, i)), i
        assert bits_equal(a.get_x_sol(i), b.get_x_sol(i)) and a.cal_obj(i) == b.cal_obj(i), i


# ---- 7. the row table ----
def test_row_table_equals_the_host_expression_and_addresses_the_packed_rows():
    import torch
    insts = [s60()[0], s500()[0], s60()[1], s500()[1]]
    b = LpBatch(insts)
    b.solve_init()
    b.solve_iter_l2f_scores(0, WS)
    b.x_iters_rows_torch(WS)
    S = [np.full(I["n"], 0.5, np.float32) for I in insts]
    S[1][5:300:3] = 0.95                                      # instance 1 is partly fixed ...
    b.solve_iter_l2f_scores(WS, 2 * WS, upload(S), 0.9, 10)
    done = np.array([False, False, True, False])              # ... and instance 2 parked
    b.set_active(~done)
    flat, row_off, first = b.x_iters_rows_torch(WS)
    _, stride = b.x_iters_torch(WS)
    act = np.flatnonzero(~done)
    rows = [b.get_n(int(i)) for i in act]
    assert rows == [60, 500 - len(range(5, 300, 3)), 500]
    r = np.asarray(rows, np.int64)                            # lpbox_hip.l2f.run_l2f_batch, the fused branch
    first_h = np.repeat(np.cumsum(r) - r, r)
    off = np.repeat(act.astype(np.int64) * stride, r) + (np.arange(int(r.sum()), dtype=np.int64) - first_h) * WS
    assert row_off.dtype == torch.int64 and row_off.is_cuda and np.array_equal(row_off.cpu().numpy(), off)
    assert first.tolist() == [0, 60, 60 + rows[1], 60 + rows[1], 60 + rows[1] + 500]
    X = flat[row_off[:, None] + torch.arange(WS, device=flat.device)].cpu().numpy()
    for i in act:
        assert bits_equal(X[first[i]:first[i + 1]], b.get_x_iters_2d(WS, int(i))), i
    # the same table is handed out again while nothing has changed
    _, again, _ = b.x_iters_rows_torch(WS)
    assert again.data_ptr() == row_off.data_ptr() and np.array_equal(again.cpu().numpy(), off)


# ---- 8. the fused policy ----
def test_device_loop_with_the_fused_policy_equals_the_host_loop():
    from lpbox_hip.policy import FusedEarlyFixPolicy
    insts = s500()[:4]
    res = []
    for run in (l2f.run_l2f_batch_device, l2f.run_l2f_batch):
        pol = FusedEarlyFixPolicy.random(tokens=20, seed=0)
        b = LpBatch(insts)
        b.solve_init()
        res.append(run(b, pol, ws=WS, max_iter=1000))
        res[-1]["x_sol"] = [b.get_x_sol(i) for i in range(4)]
    assert res[0]["windows"] == res[1]["windows"] and np.array_equal(res[0]["objective"], res[1]["objective"])
    assert np.array_equal(res[0]["infeasible"], res[1]["infeasible"])
    for i in range(4):
        assert bits_equal(res[0]["x_sol"][i], res[1]["x_sol"][i]), i
