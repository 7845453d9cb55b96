"""CPU side of the objective-vector tests (tests/objective_cases.py): what tests/test_lp_objective_gpu.py relies
on, held on the C oracle alone, and the oracle held to the numpy restatement one iteration at a time on the same vectors.

Every LP instance of the suite so far had b = -price with price in about [1, 5500].  Here b is scaled down to subnormals and up by
1e6, made positive, of mixed sign, partly and wholly zero, constant, and spread over twelve decades.  The GPU tests lean on these facts:
  * the oracle's full solve of every variant ends as FULL_SOLVE says, in both orders: both stop rules and the cap are met, `subnormal`
    stops at iteration 10 by the std rule (variance 0: the squares underflow), `scale1e-160` by dev == 0, `all_zero` never by it
    (std_obj is NaN from iteration 9 on: 0 / 0) -- so a kernel that treats dev == 0, 0 / 0 or subnormals otherwise ends elsewhere;
  * all iterates stay finite;
  * the return after a fix that leaves a remainder of almost zero norm is reachable: REMAINDER_K gives, per instance, the k whose kept
    norm is safely either side of 1e-3."""
import functools

import numpy as np
import pytest

import lp_steplock as S
from helpers import STEPLOCK_C
from objective_cases import (ABOVE, BELOW, FULL_SOLVE, REMAINDER_AT, REMAINDER_K, REMAINDER_K_EIGEN, REMAINDER_MORE, VARIANTS, keep_smallest_fix,
                             objective_variant, remainder_instance, remainder_ks)
from oracle import oracle as O
from test_lp_steplock import check, instance, oracle, run_all_windows

TINY = np.finfo(np.float64).tiny                             # the smallest normal double
ORDERS = (dict(order=O.ORDER_EIGEN), dict(order=O.ORDER_GPU, T=512))


def full_solve(I, cfg):
    o = O.LpOracle(0, **cfg)
    o.set_problem(I["n"], I["l"], I["colptr"], I["rowidx"], I["b"])
    o.solve_init()
    ret = o.solve_iter(0, 20000)
    return o, (ret, o.total_outer_iters, o.last_stop_reason)


def test_variants_are_deterministic_and_independent():
    I = instance("gen20_1")
    b = I["b"]
    for name in VARIANTS:
        assert np.array_equal(objective_variant(I, name)["b"], objective_variant(dict(I), name)["b"])
    assert objective_variant(I, "base")["b"] is not b and np.array_equal(objective_variant(I, "base")["b"], b)
    s = objective_variant(I, "mixed_sign")["b"] != b
    z = objective_variant(I, "some_zero")["b"] == 0
    w = objective_variant(I, "wide")["b"]
    rs = np.random.RandomState(5)
    assert np.array_equal(s, rs.rand(I["n"]) < 0.5) and np.array_equal(z, rs.rand(I["n"]) < 0.3)
    assert np.array_equal(w, -10.0 ** rs.uniform(-6, 6, I["n"]))
    assert 0 < s.sum() < I["n"] and 0 < z.sum() < I["n"] and w.min() < -1e5 and w.max() > -1e-5
    sub = objective_variant(I, "subnormal")["b"]
    assert np.all(sub != 0) and np.any(np.abs(sub) < TINY)
    assert np.all(objective_variant(I, "positive")["b"] > 0) and not np.any(objective_variant(I, "all_zero")["b"])
    assert np.all(objective_variant(I, "all_equal")["b"] == -7.0)


@pytest.mark.parametrize("case", list(FULL_SOLVE))
def test_full_solves_end_as_pinned(case):
    """Return, outer iterations and stop reason of solve_iter(0, 20000) per variant and order; every iterate finite."""
    I = instance(case)
    for name in ("base",) + VARIANTS:
        J = objective_variant(I, name)
        got = []
        for cfg in ORDERS:
            o, res = full_solve(J, cfg)
            got.append(res)
            for v in ("x", "z1", "z2", "z4", "y3"):
                assert np.all(np.isfinite(o.vec(v))), (case, name, v)
            if name == "all_zero":                           # 0 / 0 in the std stop test: NaN never satisfies `<= 1e-12`
                assert np.isnan(o.scalar("std_obj")) and o.scalar("obj_val") == 0.0 and res[2] != 2
            else:
                assert np.isfinite(o.scalar("std_obj")), (case, name)
        print(case, name, got)
        assert tuple(got) == FULL_SOLVE[case][name], (case, name)
    reasons = {r[2] for v in FULL_SOLVE[case].values() for r in v}
    assert reasons == {0, 1, 2}                              # the cap, the residual rule and the std rule, per instance


def test_what_the_gpu_windows_meet_inside_3000_iterations():
    """The on-chip GPU test stops at iteration 3000: both stop rules are met before it in the kernels' order, among them the
    iteration-10 stop of `subnormal` and the dev == 0 stop of `scale1e-160`."""
    inside = {(c, v): r[1] for c, t in FULL_SOLVE.items() for v, r in t.items() if r[1][1] < 3000}
    assert {r[2] for r in inside.values()} == {1, 2}
    for c in FULL_SOLVE:
        assert inside[(c, "subnormal")] == (1, 10, 2) and inside[(c, "scale1e-160")][2] == 2


def test_subnormal_objective_of_heavy_row_3():
    """The objective of the `subnormal` variant lives on the subnormal grid.  Two of the three costs are just above the smallest normal
    double (price * 1e-310 with a price above 222), one is subnormal, and every term b_j x_j with x_j < 1 is subnormal or within a
    factor two of it, where the spacing is still 2^-1074: the sums are exact in any order, and a device that flushed subnormal inputs
    or results to zero would return another objective.  The final obj_val is -4.29e-308 (|.| < 2 * 2.2251e-308, not itself subnormal --
    the issue behind these tests called it one); cur_obj and cal_Obj are one cost, -4.2051e-308."""
    J = objective_variant(instance("heavy_row_3"), "subnormal")
    b = J["b"]
    assert np.sum(np.abs(b) < TINY) == 1 and np.all(b != 0) and np.all(np.abs(b) < 2 * TINY)
    for cfg in ORDERS:
        o, res = full_solve(J, cfg)
        assert res == (1, 10, 2)
        x, obj = o.vec("x"), o.scalar("obj_val")
        terms = b * x
        assert np.all(terms != 0) and np.sum(np.abs(terms) < TINY) >= 2        # nonzero subnormal terms
        assert obj != 0 and abs(obj) < 2 * TINY and obj == terms.sum() == terms[::-1].sum()
        flushed = np.where(np.abs(terms) < TINY, 0.0, terms).sum()
        assert flushed != obj                                                  # flush-to-zero would show
        assert o.scalar("std_obj") == 0.0                                      # the squared deviations underflow: dev == 0, no 0 / 0
        assert o.scalar("cur_obj") == o.cal_Obj() == b[x >= 0.5].sum() != 0


# ------------------------------------------------------------------------------------------------
# step-locked against the restatement
# ------------------------------------------------------------------------------------------------
STEPLOCKED = [("empty_rows_65", v) for v in VARIANTS] + [("gen20_1", v) for v in ("scale1e-6", "scale1e-150", "positive", "some_zero", "all_equal", "wide")]
# iterations of 0..74 with B(x) > 1e-4 in the Eigen-order run (gen20_1; the quarter cap, 18 of 75, holds for all of them)
WEAK_GEN20 = {"scale1e-6": 1, "scale1e-150": 1, "positive": 2, "some_zero": 5, "all_equal": 0, "wide": 18}


@functools.lru_cache(maxsize=None)
def variant_run(case, name, cfg):
    return run_all_windows(objective_variant(instance(case), name), cfg, f"{cfg} {case} {name}")


def check_variant(cases, name):
    check(cases)                                             # no violation, the quarter cap on weak iterations
    if name == "subnormal":
        # the restatement's own decision: the std rule at iteration 9 (the tenth), and the harness saw the subject stop there too
        (c,) = cases
        assert c.done and c.stop_at == (9, "obj_std") and c.view.stop() == 2 and c.view.totals()[0] == 10
    else:
        assert len(cases) == 4 and all(c.checked > 0 for c in cases[:3])
    for c in cases:
        if name == "all_zero" and not c.tag.endswith(" all"):
            # std_obj is 0 / 0 from iteration 9 on, in the restatement and in the subject alike: counted, not a violation
            assert c.nan_agreed > 0, c.tag
            assert c.nan_agreed == (c.checked - 9 if c is cases[0] else c.checked), (c.tag, c.nan_agreed, c.checked)
        else:
            assert c.nan_agreed == 0, c.tag


@pytest.mark.parametrize("case,name", STEPLOCKED)
@pytest.mark.parametrize("cfg", ["eigen", "gpu512"])
def test_oracle_every_window_against_the_restatement(cfg, case, name):
    cases = variant_run(case, name, cfg)
    check_variant(cases, name)
    if cfg == "eigen" and case == "gen20_1":
        assert cases[0].weak == WEAK_GEN20[name], (name, cases[0].weak)
    if cfg == "eigen" and case == "empty_rows_65":
        assert cases[0].weak <= 16 and all(c.post[1] == 0 for c in cases)


def test_a_nan_on_one_side_alone_stays_a_violation():
    """The NaN rule of lp_steplock.Case.compare: agreement only when the restatement's natural float64 member and the subject are both
    NaN.  A subject that reports a number where the restatement has NaN, or NaN where it has a number, is flagged."""
    class Reporting(S.OracleSubject):
        def __init__(self, o, report):
            super().__init__(o)
            self.report = report

        def scalar(self, name):
            true = super().scalar(name)
            return self.report(true) if name == "std_obj" else true

    nan = float("nan")
    for variant, report, want, count in (("all_zero", lambda t: t, None, 0),                                   # NaN where the restatement has NaN
                                         ("all_zero", lambda t: 0.0 if np.isnan(t) else t, "restatement nan", 3),   # a number there instead
                                         ("some_zero", lambda t: nan, "subject nan", 12)):                     # NaN where it has a number
        I = objective_variant(instance("empty_rows_65"), variant)
        o = oracle(I, "eigen")
        c = S.Case(I, Reporting(o, report), "reporting", calibrate=False)
        S.run_cases(S.OracleGroup([o]), [c], S.l2f_steps(0, 12))
        msgs = [m for m in c.violations if "std_obj" in m]
        assert msgs == c.violations and len(msgs) == count, (variant, c.violations[:3])
        for m in msgs:
            subject, restatement = m.split("subject ")[1].split(", restatement ")
            assert ("nan" in subject, "nan" in restatement.split(",")[0]) == (want == "subject nan", want == "restatement nan"), m
        assert c.nan_agreed == (3 if want is None else 0)                      # iterations 9, 10, 11


def test_calibration_of_c_objective_variants():
    """The calibration of test_lp_steplock.py::test_calibration_of_c on the new cases, on the restatement alone: the distance of every
    float64 permuted member from the natural member over the spread of the other eleven stays below c / 2, so c stays 10."""
    worst = {(case, name): max(c.loo for c in variant_run(case, name, "eigen")) for case, name in STEPLOCKED}
    print({k: round(v, 2) for k, v in worst.items()})
    assert max(worst.values()) <= STEPLOCK_C / 2


# ------------------------------------------------------------------------------------------------
# the return after a fix that leaves a remainder of almost zero norm
# ------------------------------------------------------------------------------------------------
REMAINDER_CFG = {"auction3000": "gpu256c512"}                # the large route's tree; the on-chip instances: T = 512


def oracle_at_75(I, cfg):
    o = oracle(I, cfg)
    for it in range(REMAINDER_AT):
        assert o.solve_iter_l2f(it, it + 1, np.zeros(I["n"]), 0) == 0
    return o


def test_remainder_ks_helper():
    x = np.array([0.9, -3e-4, 1.0, 4e-4, 0.0, 8e-4, 2e-3])
    assert remainder_ks(x) == (3, 5)                         # kept norms 0, 3e-4, 5e-4, 9.43e-4 (between the margins), 2.2e-3, 0.9
    assert remainder_ks(x, 1e-5, 0.5) == (1, 6) and remainder_ks(np.ones(4)) == (None, 1) and remainder_ks(np.zeros(4)) == (3, None)
    vec, num = keep_smallest_fix(x, 3)
    assert num == 4 and list(vec) == [1.0, -1.0, 1.0, -1.0, -1.0, 0.0, 0.0]


@pytest.mark.parametrize("case", list(REMAINDER_K))
@pytest.mark.parametrize("order", ["kernels", "eigen"])
def test_near_zero_remainder_on_the_oracle(order, case):
    """75 l2f iterations of length 1, then every variable but the k of smallest |x| is fixed to x >= 0.5.  With the kept norm below 1e-3
    the call returns 1 although nothing stopped: the iteration of the call and five more run, the stop reason stays 0.  With the kept
    norm above it the same call returns 0.  Only the return code tells the two apart."""
    I = remainder_instance(case)
    cfg = "eigen" if order == "eigen" else REMAINDER_CFG.get(case, "gpu512")
    x = oracle_at_75(I, cfg).vec("x")
    ks = remainder_ks(x)
    print(case, order, ks)
    assert ks == (REMAINDER_K_EIGEN if order == "eigen" else REMAINDER_K)[case]
    assert None not in ks
    for k, want in zip(ks, (1, 0)):
        o = oracle_at_75(I, cfg)
        vec, num = keep_smallest_fix(x, k)
        kept = np.sqrt(np.sum(x[vec == -1.0] ** 2))
        assert (kept < BELOW) if want else (kept > ABOVE)
        assert o.solve_iter_l2f(REMAINDER_AT, REMAINDER_AT + 1, vec, num) == want
        assert o.get_n() == k and o.last_stop_reason == 0 and o.total_outer_iters == REMAINDER_AT + 1
        for it in range(REMAINDER_AT + 1, REMAINDER_AT + 1 + REMAINDER_MORE):
            assert o.solve_iter_l2f(it, it + 1, np.zeros(k), 0) == 0 and o.last_stop_reason == 0
        assert o.total_outer_iters == REMAINDER_AT + 1 + REMAINDER_MORE and o.get_n() == k
        assert np.all(np.isfinite(o.vec("x")))


def test_one_live_variable_of_gen20_1_stays_above():
    """On lp_20_60_seed0[1] even the single smallest variable has |x| above 1e-3 at iteration 75: the call returns 0 with one live
    variable."""
    I = instance("gen20_1")
    for cfg in ("gpu512", "eigen"):
        x = oracle_at_75(I, cfg).vec("x")
        assert remainder_ks(x) == (None, 1) and 1.4e-3 < np.abs(x).min() < 1.9e-3
        o = oracle_at_75(I, cfg)
        assert o.solve_iter_l2f(75, 76, *keep_smallest_fix(x, 1)) == 0 and o.get_n() == 1 and o.last_stop_reason == 0


@pytest.mark.parametrize("case", ["gen100_0", "gen100_2", "gen20_1"])
@pytest.mark.parametrize("cfg", ["eigen", "gpu512"])
def test_near_zero_remainder_against_the_restatement(cfg, case):
    """The same procedure through the step-locked harness with an explicit fix vector: the restatement's own
    `np.sqrt(self.x @ self.x) < 1e-3` decides the same return (the harness compares it exactly), and the iteration of the call and the
    five that follow are held to the bound like any other."""
    I = remainder_instance(case)
    o = oracle(I, cfg)
    main = S.Case(I, S.OracleSubject(o), f"{cfg} {case}")
    S.run_cases(S.OracleGroup([o]), [main], S.l2f_steps(0, REMAINDER_AT))
    assert not main.done
    x = o.vec("x")
    for k, want in zip(remainder_ks(x), (1, 0)):
        if k is None:
            assert case == "gen20_1" and want == 1
            continue
        o2 = oracle_at_75(I, cfg)
        c = main.fork(S.OracleSubject(o2), f"{cfg} {case} keep {k}")
        steps = S.l2f_steps(REMAINDER_AT, REMAINDER_AT + 1, keep_smallest_fix(x, k)) + S.l2f_steps(REMAINDER_AT + 1, REMAINDER_AT + 1 + REMAINDER_MORE)
        rets, group = [], S.OracleGroup([o2])
        for st in steps:                                     # one step at a time: the restatement's own return of every call
            S.run_cases(group, [c], [st])
            rets.append(c.members[0].ret)
        check([c])                                           # no violation: the subject's return equalled it every time
        assert rets == [want] + [0] * REMAINDER_MORE and c.members[0].n == k == o2.get_n()
        assert c.checked == 1 + REMAINDER_MORE and c.fixed == I["n"] - k and c.stop_at is None and not c.done
    check([main])
