"""The LP kernels on objective vectors outside the auction range, and the return after a fix that leaves a remainder of almost zero norm
(tests/objective_cases.py).  Every kernel family is compared bit for bit with the C oracle in its own summation
order: return codes, counters, stop reason, x, z1, z2, z4, the objective scalars and cal_obj.  std_obj, which is 0 / 0 on `all_zero`, is
compared as "both NaN or equal" (the sign bit of a NaN is not compared).  tests/test_lp_objective_cases.py holds, on the CPU, what these
tests lean on: where the oracle stops on every variant, that it agrees with the numpy restatement step by step, and the k values of
the remainder procedure.  The last two tests hold the kernels to the restatement directly, with no oracle in between."""
import numpy as np
import pytest

import lp_steplock as S
from helpers import bits_equal, make_oracle, oracle_for, scripted_fix_vec
from lpbox_hip.big import BigLp
from lpbox_hip.lp import LpBatch
from objective_cases import (ABOVE, BELOW, REMAINDER_AT, REMAINDER_MORE, SHORT_LIST, VARIANTS, keep_smallest_fix, objective_variant,
                             remainder_instance, remainder_ks)
from oracle import oracle as O
from test_lp_steplock_gpu import run_batch
from valued_cases import valued, valued_oracle

pytestmark = pytest.mark.gpu

WINDOWS = ((0, 40), (40, 400), (400, 3000))
SCALARS = ("obj_val", "cur_obj", "best_bin_obj", "cvg1", "cvg2", "rho1", "gamma")


def nan_or_equal(got, want):
    return bool(np.isnan(got) and np.isnan(want)) or bits_equal([got], [want])


def std_obj_agrees(got, o, reference_order):
    """Reference order: the kernels take sqrt where the oracle's Eigen model calls pow(v, 1/2); where the oracle
    counted a disagreement of the two, std_obj may differ by 2 ulp.  Everywhere else: both NaN, or the same bits."""
    want = o.scalar("std_obj")
    if reference_order and o.scalar("pow_sqrt_mismatch") > 0 and not np.isnan(want):
        return abs(got - want) <= 2 * np.spacing(abs(want))
    return nan_or_equal(got, want)


def compare_batch(b, i, o, tag, reference_order=False):
    left = o.vec("left_idx").astype(int)                  # the kernels never compact: fixed variables stay in place, masked
    assert b.get_n(i) == o.get_n() == len(left), tag
    for name in ("x", "z1", "z2"):
        gv, ov = b.debug_vec(name, i)[left], o.vec(name)
        assert np.all(np.isfinite(gv)) and bits_equal(gv, ov), f"{tag}: {name} differs (max abs {np.abs(gv - ov).max():.3e})"
    assert bits_equal(b.debug_vec("z4", i), o.vec("z4")), f"{tag}: z4"
    assert b.counters(i) == (o.total_outer_iters, o.total_pcg_iters), tag
    assert b.stop(i)[0] == o.last_stop_reason, tag
    for name in SCALARS:
        assert nan_or_equal(b.debug_scalar(name, i), o.scalar(name)), f"{tag}: {name} {b.debug_scalar(name, i)!r} vs {o.scalar(name)!r}"
    assert std_obj_agrees(b.debug_scalar("std_obj", i), o, reference_order), f"{tag}: std_obj {b.debug_scalar('std_obj', i)!r} vs {o.scalar('std_obj')!r}"
    assert bits_equal([b.cal_obj(i)], [o.cal_Obj()]), tag


def plain_windows(b, oracles, tags, windows, reference_order=False, ended=None):
    """solve_iter windows on the batch and on one oracle per instance; an instance that stopped is parked.  Returns, per instance, the
    (return, outer iterations, stop reason) of the window in which it stopped, or None.  `ended`: what stopped before these windows."""
    ended = [None] * b.B if ended is None else ended
    for (a, e) in windows:
        b.set_active(np.array([r is None for r in ended], np.int32))
        rets = b.solve_iter(a, e)
        for i, o in enumerate(oracles):
            if ended[i] is not None:
                continue
            t = f"{tags[i]} [{a},{e})"
            assert int(rets[i]) == o.solve_iter(a, e), t
            compare_batch(b, i, o, t, reference_order)
            if o.last_stop_reason != 0:
                ended[i] = (int(rets[i]), b.counters(i)[0], b.stop(i)[0])
    return ended


def variants_of(cases, names):
    insts, tags = [], []
    for case, I in cases:
        for name in names:
            insts.append(objective_variant(I, name))
            tags.append(f"{case} {name}")
    return insts, tags


# ------------------------------------------------------------------------------------------------
# a. on chip, default order, one slot: every variant of three instances in one ragged batch
# ------------------------------------------------------------------------------------------------
def test_onchip_default_order_every_variant():
    cases = [("gen20_1", remainder_instance("gen20_1")), ("heavy_row_3", S.fuzz_instance("heavy_row_3")), ("empty_rows_65", S.fuzz_instance("empty_rows_65"))]
    insts, tags = variants_of(cases, VARIANTS)
    b = LpBatch(insts)
    b.solve_init()
    assert b.config()["elems_per_thread"] == 1 and b.B == 33
    ended = plain_windows(b, [oracle_for(b, i, I) for i, I in enumerate(insts)], tags, WINDOWS)
    by_tag = dict(zip(tags, ended))
    print(by_tag)
    for case, _ in cases:
        assert by_tag[f"{case} subnormal"] == (1, 10, 2)          # variance 0 at the first test of the std rule: the squares underflow
        assert by_tag[f"{case} scale1e6"] is None                 # still running at 3000
    # dev == 0 with an objective that is no zero (on gen20_1 the two stop rules race near iteration 850 and the batch's layout decides)
    assert by_tag["heavy_row_3 scale1e-160"] == (1, 31, 2) and by_tag["empty_rows_65 scale1e-160"] == (1, 537, 2)
    assert {r[2] for r in ended if r is not None} == {1, 2}       # both stop rules among the GPU results
    b.close()


# ------------------------------------------------------------------------------------------------
# b. two and four slots
# ------------------------------------------------------------------------------------------------
def l2f_fix_then_plain(b, oracles, tags, n0, reference_order=False):
    """l2f windows (0, 60) and (60, 120) with the scripted fix between them, then solve_iter(120, 200)."""
    B = b.B
    ended = [None] * B
    vecs, nums = [np.zeros(0)] * B, np.zeros(B, np.int32)
    fixed = 0
    for (a, e) in ((0, 60), (60, 120)):
        b.set_active(np.array([r is None for r in ended], np.int32))
        V = -np.ones((B, n0))
        for i in range(B):
            V[i, :len(vecs[i])] = vecs[i]
        rets = b.solve_iter_l2f(a, e, V, nums)
        for i, o in enumerate(oracles):
            if ended[i] is not None:
                continue
            t = f"{tags[i]} l2f [{a},{e})"
            assert int(rets[i]) == o.solve_iter_l2f(a, e, vecs[i] if nums[i] else np.zeros(o.get_n()), int(nums[i])), t
            compare_batch(b, i, o, t, reference_order)
            vecs[i], nums[i] = np.zeros(0), 0
            if rets[i]:
                ended[i] = (int(rets[i]), b.counters(i)[0], b.stop(i)[0])
                continue
            xg, xo = b.get_x_iters_2d(e - a, i), o.get_x_iters_2d(e - a)
            assert bits_equal(xg, xo), f"{t}: x_iters"
            if a == 0:
                vecs[i], nums[i] = scripted_fix_vec(xo, lo=0.05, hi=0.95, last=20)
                fixed += int(nums[i])
    assert fixed > 0, "the scripted fix never fired"
    return plain_windows(b, oracles, tags, ((120, 200),), reference_order, ended)


@pytest.mark.parametrize("case,slots", [("dup_cols_700", 2), ("dup_cols_1200", 4)])
def test_onchip_default_order_two_and_four_slots(case, slots):
    I = S.fuzz_instance(case)
    insts, tags = variants_of([(case, I)], SHORT_LIST)
    b = LpBatch(insts)
    b.solve_init()
    assert b.config()["elems_per_thread"] == slots, b.config()
    ended = l2f_fix_then_plain(b, [oracle_for(b, i, J) for i, J in enumerate(insts)], tags, I["n"])
    assert ended[SHORT_LIST.index("subnormal")] == (1, 10, 2) and sum(r is None for r in ended) >= 4
    b.close()


# ------------------------------------------------------------------------------------------------
# c. reference order (unit and stored values) and the direct x-update
# ------------------------------------------------------------------------------------------------
def test_onchip_reference_order_unit():
    insts, tags = variants_of([("gen20_1", remainder_instance("gen20_1")), ("empty_rows_65", S.fuzz_instance("empty_rows_65"))], SHORT_LIST)
    b = LpBatch(insts, order="reference")
    b.solve_init()
    ended = plain_windows(b, [make_oracle(I, O.ORDER_EIGEN) for I in insts], tags, WINDOWS[:2], reference_order=True)
    assert ended[0] == ended[len(SHORT_LIST)] == (1, 10, 2)
    b.close()


def test_onchip_reference_order_stored_values():
    insts, tags = variants_of([("signed empty_rows_65", valued(S.fuzz_instance("empty_rows_65"), "signed", 0))], SHORT_LIST)
    assert all(np.any(I["vals"] < 0) for I in insts)
    b = LpBatch(insts, order="reference")
    b.solve_init()
    ended = plain_windows(b, [valued_oracle(I) for I in insts], tags, WINDOWS[:2], reference_order=True)
    assert ended[0] == (1, 10, 2)
    b.close()


def test_onchip_direct_x_update():
    insts, tags = variants_of([("gen20_1", remainder_instance("gen20_1")), ("empty_rows_65", S.fuzz_instance("empty_rows_65"))], SHORT_LIST)
    b = LpBatch(insts)
    b.set_x_update("direct")
    b.solve_init()
    oracles = [oracle_for(b, i, I, x_update="direct", direct_rows=b.direct_rows(i)) for i, I in enumerate(insts)]
    ended = plain_windows(b, oracles, tags, WINDOWS[:2])
    assert ended[0] == ended[len(SHORT_LIST)] == (1, 10, 2)
    assert all(b.counters(i)[1] == 0 for i in range(b.B))
    b.close()


# ------------------------------------------------------------------------------------------------
# d. the large route
# ------------------------------------------------------------------------------------------------
BIG_MODES = {"reference_pcg": dict(pcg_mode="reference"), "lean": dict(pcg_mode="lean"), "reference_order": dict(order="reference")}
BIG_SCALARS = ("obj_val", "cur_obj", "best_bin_obj", "cvg1", "cvg2", "rho1", "gamma", "sum_fix_obj")


def big_pair(P, mode):
    g = BigLp(P, **BIG_MODES[mode])
    g.solve_init()
    if mode == "reference_order":
        o = O.LpOracle(0, order=O.ORDER_EIGEN)
    else:
        o = O.LpOracle(0, order=O.ORDER_GPU, T=int(g.scalar("threads")), chunk=int(g.scalar("chunk")))
        if mode == "lean":
            o.set_pcg_lean(True, int(g.scalar("row_chunk")))
    o.set_problem(P["n"], P["l"], P["colptr"], P["rowidx"], P["b"])
    o.solve_init()
    return g, o


def compare_big(g, o, tag, reference_order):
    left = o.vec("left_idx").astype(int)
    assert g.get_n() == o.get_n() == len(left), tag
    for name in ("x", "z1", "z2"):
        gv, ov = g.vec(name)[left], o.vec(name)
        assert np.all(np.isfinite(gv)) and bits_equal(gv, ov), f"{tag}: {name} differs (max abs {np.abs(gv - ov).max():.3e})"
    assert bits_equal(g.vec("z4"), o.vec("z4")), f"{tag}: z4"
    assert (g.scalar("outer_total"), g.scalar("pcg_total")) == (o.total_outer_iters, o.total_pcg_iters), tag
    assert int(g.scalar("stop")) == o.last_stop_reason, tag
    for name in BIG_SCALARS:
        assert nan_or_equal(g.scalar(name), o.scalar(name)), f"{tag}: {name} {g.scalar(name)!r} vs {o.scalar(name)!r}"
    assert std_obj_agrees(g.scalar("std_obj"), o, reference_order), f"{tag}: std_obj {g.scalar('std_obj')!r} vs {o.scalar('std_obj')!r}"
    assert bits_equal([g.cal_Obj()], [o.cal_Obj()]), tag


@pytest.mark.parametrize("mode", list(BIG_MODES))
def test_large_route(mode):
    """l2f windows (0, 30), (30, 60) with the scripted fix between them, (60, 90); `subnormal` stops at iteration 10."""
    P0 = remainder_instance("auction3000")
    for name in ("subnormal", "mixed_sign", "all_zero"):
        P = objective_variant(P0, name)
        g, o = big_pair(P, mode)
        vec, num = np.zeros(P["n"]), 0
        for w in range(3):
            t = f"big {mode} {name} window {w}"
            rg = g.solve_iter_l2f(30 * w, 30 * w + 30, vec, num)
            assert rg == o.solve_iter_l2f(30 * w, 30 * w + 30, vec, num), t
            compare_big(g, o, t, mode == "reference_order")
            if rg:
                break
            xg, xo = g.get_x_iters_2d(30), o.get_x_iters_2d(30)
            assert bits_equal(xg, xo), f"{t}: x_iters"
            vec, num = scripted_fix_vec(xo, lo=0.05, hi=0.95, last=20) if w == 0 else (np.zeros(o.get_n()), 0)
            assert w or num > 0, f"{t}: the scripted fix did not fire"
        if name == "subnormal":
            assert (rg, w, int(g.scalar("outer_total")), int(g.scalar("stop"))) == (1, 0, 10, 2)
        else:
            assert (rg, w, int(g.scalar("outer_total"))) == (0, 2, 90)
        if name == "all_zero":
            assert np.isnan(g.scalar("std_obj")) and g.scalar("obj_val") == 0.0
        g.close()


# ------------------------------------------------------------------------------------------------
# e. the return after a fix that leaves a remainder of almost zero norm, on every family
# ------------------------------------------------------------------------------------------------
def remainder_on_batch(names, slots=None, order=None, x_update="pcg"):
    """Every instance twice in one batch: after 75 l2f iterations the first copy keeps the largest k whose kept norm is below 0.9e-3 (the
    call returns 1), the second the smallest k above 1.1e-3 (returns 0); the iteration of the call and five more are bit-equal to the
    oracle's, the stop reason stays 0.  k comes from the oracle's x in the kernels' own order."""
    insts = [remainder_instance(n) for n in names for _ in (0, 1)]
    tags = [f"{n} {w}" for n in names for w in ("below", "above")]
    b = LpBatch(insts, order=order)
    if x_update == "direct":
        b.set_x_update("direct")
    b.solve_init()
    if slots is not None:
        assert b.config()["elems_per_thread"] == slots, b.config()
    ref = order == "reference"
    if ref:
        oracles = [make_oracle(I, O.ORDER_EIGEN) for I in insts]
    elif x_update == "direct":
        oracles = [oracle_for(b, i, I, x_update="direct", direct_rows=b.direct_rows(i)) for i, I in enumerate(insts)]
    else:
        oracles = [oracle_for(b, i, I) for i, I in enumerate(insts)]
    stride = max(I["n"] for I in insts)
    rets = b.solve_iter_l2f(0, REMAINDER_AT, -np.ones((b.B, stride)), np.zeros(b.B, np.int32))
    V, nums, want = -np.ones((b.B, stride)), np.zeros(b.B, np.int32), []
    for i, o in enumerate(oracles):
        assert int(rets[i]) == o.solve_iter_l2f(0, REMAINDER_AT, np.zeros(insts[i]["n"]), 0) == 0, tags[i]
        compare_batch(b, i, o, f"{tags[i]} [0,75)", ref)
        x = o.vec("x")
        ks = remainder_ks(x)
        assert None not in ks, f"{tags[i]}: no k either side of 1e-3: {ks}"
        k = ks[i % 2]
        vec, num = keep_smallest_fix(x, k)
        kept = np.sqrt(np.sum(x[vec == -1.0] ** 2))
        assert kept < BELOW if i % 2 == 0 else kept > ABOVE
        V[i, :len(vec)], nums[i] = vec, num
        want.append((1 - i % 2, k, vec, num))
        print(tags[i], "k =", k, "kept norm %.3e" % kept)
    rets = b.solve_iter_l2f(REMAINDER_AT, REMAINDER_AT + 1, V, nums)
    for i, (o, (ret, k, vec, num)) in enumerate(zip(oracles, want)):
        assert o.solve_iter_l2f(REMAINDER_AT, REMAINDER_AT + 1, vec, num) == ret, tags[i]      # the oracle, as pinned on the CPU
        assert int(rets[i]) == ret, f"{tags[i]}: the kernel returned {int(rets[i])} with a kept norm {'below' if ret else 'above'} 1e-3"
        assert b.get_n(i) == k and b.stop(i)[0] == 0 and b.counters(i)[0] == REMAINDER_AT + 1, tags[i]
        compare_batch(b, i, o, f"{tags[i]} the fix", ref)
    end = REMAINDER_AT + 1 + REMAINDER_MORE
    rets = b.solve_iter_l2f(REMAINDER_AT + 1, end, None, None)
    for i, (o, (ret, k, vec, num)) in enumerate(zip(oracles, want)):
        assert int(rets[i]) == o.solve_iter_l2f(REMAINDER_AT + 1, end, np.zeros(k), 0) == 0, tags[i]
        assert bits_equal(b.get_x_iters_2d(REMAINDER_MORE, i), o.get_x_iters_2d(REMAINDER_MORE)), f"{tags[i]}: the five iterations after the fix"
        assert b.get_n(i) == k and b.stop(i)[0] == 0 and b.counters(i)[0] == end, tags[i]
        compare_batch(b, i, o, f"{tags[i]} five more", ref)
    b.close()


def test_remainder_one_slot():
    remainder_on_batch(["gen100_0", "gen100_2"], slots=1)


def test_remainder_two_slots():
    remainder_on_batch(["dup_cols_700"], slots=2)


def test_remainder_four_slots():
    remainder_on_batch(["dup_cols_1200", "heavy_row_2048"], slots=4)


def test_remainder_reference_order():
    remainder_on_batch(["gen100_2", "dup_cols_700"], order="reference")


def test_remainder_direct_x_update():
    remainder_on_batch(["gen100_0", "gen100_2"], x_update="direct")


@pytest.mark.parametrize("mode", ["reference_pcg", "reference_order"])
def test_remainder_large_route(mode):
    P = remainder_instance("auction3000")
    ref = mode == "reference_order"
    end = REMAINDER_AT + 1 + REMAINDER_MORE
    for which, ret in ((0, 1), (1, 0)):
        g, o = big_pair(P, mode)
        t = f"big {mode} {'below' if ret else 'above'}"
        assert g.solve_iter_l2f(0, REMAINDER_AT, np.zeros(P["n"]), 0) == o.solve_iter_l2f(0, REMAINDER_AT, np.zeros(P["n"]), 0) == 0
        compare_big(g, o, f"{t} [0,75)", ref)
        x = o.vec("x")
        ks = remainder_ks(x)
        assert None not in ks, ks
        vec, num = keep_smallest_fix(x, ks[which])
        assert o.solve_iter_l2f(REMAINDER_AT, REMAINDER_AT + 1, vec, num) == ret
        rg = g.solve_iter_l2f(REMAINDER_AT, REMAINDER_AT + 1, vec, num)
        assert rg == ret, f"{t}: the kernel returned {rg}"
        assert g.get_n() == ks[which] and int(g.scalar("stop")) == 0 and int(g.scalar("outer_total")) == REMAINDER_AT + 1
        compare_big(g, o, f"{t} the fix", ref)
        assert g.solve_iter_l2f(REMAINDER_AT + 1, end, np.zeros(ks[which]), 0) == o.solve_iter_l2f(REMAINDER_AT + 1, end, np.zeros(ks[which]), 0) == 0
        assert bits_equal(g.get_x_iters_2d(REMAINDER_MORE), o.get_x_iters_2d(REMAINDER_MORE)), f"{t}: the five iterations after the fix"
        assert int(g.scalar("stop")) == 0 and int(g.scalar("outer_total")) == end
        compare_big(g, o, f"{t} five more", ref)
        g.close()


# ------------------------------------------------------------------------------------------------
# f. step-locked on the device: the kernels against the restatement, no oracle in between
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [None, "reference"])
def test_steplocked_every_variant_of_empty_rows_65(order):
    insts, tags = variants_of([(order or "default", S.fuzz_instance("empty_rows_65"))], VARIANTS)
    cases = run_batch(insts, tags, order=order)
    by_name = dict(zip(VARIANTS, cases))
    assert by_name["subnormal"].stop_at == (9, "obj_std")
    assert by_name["all_zero"].nan_agreed == by_name["all_zero"].checked - 9 > 0      # std_obj 0 / 0 from iteration 9 on, on both sides
    assert all(c.nan_agreed == 0 for n, c in by_name.items() if n != "all_zero")
