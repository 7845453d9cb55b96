"""CPU pins of the cases behind tests/test_chain_resume_gpu.py, on the oracles alone.

The GPU tests reach the halt-and-resume path of the segmentation and BQP launch chains only because the PCG of these problems needs
more (matvec, update) pairs than a chain enqueues.  Every property they lean on is a condition on an oracle's PCG trace and is held
here, so that a later change to a helper cannot quietly turn them into tests of a chain that never halts."""
import numpy as np
import pytest

from chain_cases import (BQP_KMAX_START, PAIRS_PER_RESUME, PCG_MAXITERS, SEG_FIX_AFTER, SEG_FIXED, SEG_KMAX_LIMIT, SEG_KMAX_START, SEG_LEGACY,
                         bqp_case, bqp_case_params, expected_resumes, oracle_windows, seg_case, seg_oracle)
from helpers import scripted_fix_vec, spread_bound
from oracle import oracle as O
from oracle.bqp_numpy import NumpyBqp, NumpySeg


def seg_trace(name, fix_after=None, order=O.ORDER_GPU):
    trace, fixed, _ = oracle_windows(seg_oracle(seg_case(name), order=order), [10, 10, 10], fix_after)
    return [int(k) for k in trace], fixed


def test_expected_resumes_rule():
    assert expected_resumes([10, 9, 1], 10) == 0
    assert expected_resumes([11, 26, 27, 42, 43], 10) == 1 + 1 + 2 + 2 + 3
    assert expected_resumes([1000], 1) == 63 and expected_resumes([1000], 24) == 61 and expected_resumes([1000], 10) == 62
    assert PCG_MAXITERS // PAIRS_PER_RESUME + 2 >= expected_resumes([PCG_MAXITERS], 1)         # the bound of the host loops admits the cap


def test_s2_needs_two_resumes_even_at_the_clamp():
    for fix_after in (None, SEG_FIX_AFTER["S2"]):
        trace, _ = seg_trace("S2", fix_after)
        assert len(trace) == 30
        assert max(trace[:10]) > SEG_KMAX_LIMIT + PAIRS_PER_RESUME == 40                       # 24 + 16 pairs do not reach it
        assert trace[0] > SEG_KMAX_START + 2 * PAIRS_PER_RESUME                                # iteration 0 from kmax = 10: three resumes
        assert min(trace) >= 20
        assert trace[0] == max(trace) == 44 and min(trace[:10]) == 35 and trace[-1] == (29 if fix_after is None else 20)


def test_s3_resumes_once_from_the_starting_kmax():
    trace, _ = seg_trace("S3")
    assert SEG_KMAX_START < trace[0] <= SEG_KMAX_START + PAIRS_PER_RESUME == 26
    assert trace[0] == 18 and trace[-1] == 11 and min(trace) > 4


def test_s1_and_s4_stay_below_the_starting_kmax():
    s1, _ = seg_trace("S1")
    s4, _ = seg_trace("S4")
    assert max(s1) == s1[0] == 9 and min(s1) == 5 and max(s4) == 4 and min(s4) == 3
    assert max(s1) < SEG_KMAX_START and min(s1) > 4                                            # kmax 1, 2, 4: every iteration resumes


def test_s5_runs_into_the_pcg_cap():
    for order in (O.ORDER_GPU, O.ORDER_EIGEN):
        o = seg_oracle(seg_case("S5"), order=order)
        assert o.solve_iter_l2f(0, 3, np.zeros(o.get_org_n()), 0) == 0
        assert list(o.pcg_trace()) == [PCG_MAXITERS] * 3 and (o.total_outer_iters, o.total_pcg_iters) == (3, 3000)
    # from kmax = 10 the cap is met inside a resume's pairs (10 + 61 * 16 = 986, then 14 of 16); from the clamp, 24 + 61 * 16 = 1000: the
    # pending exit test of `post` sees k = 1000
    assert (PCG_MAXITERS - SEG_KMAX_LIMIT) % PAIRS_PER_RESUME == 0 and (PCG_MAXITERS - SEG_KMAX_START) % PAIRS_PER_RESUME != 0


@pytest.mark.parametrize("name", ["S1", "S2", "S3"])
def test_three_traces_agree_with_and_without_the_fix(name):
    """Oracle in the kernels' order, oracle in Eigen order and the numpy restatement: the same PCG counts over 30 iterations, the same
    fix, and the oracle within B (helpers.spread_bound) of the restatement on every recorded column."""
    P = seg_case(name)
    for fix_after in (None, SEG_FIX_AFTER[name]):
        trace, fixed = seg_trace(name, fix_after)
        assert seg_trace(name, fix_after, O.ORDER_EIGEN) == (trace, fixed)
        assert fixed == (SEG_FIXED[name] if fix_after is not None else 0)
        o, e, r = seg_oracle(P), seg_oracle(P, order=O.ORDER_EIGEN), NumpySeg(P)
        r.solve_init()
        vec, num = np.zeros(P["n"]), 0
        for w in range(3):
            rets = [s.solve_iter_l2f(10 * w, 10 * w + 10, vec, num) for s in (o, e, r)]
            assert rets == [0, 0, 0]
            xo, xe, xr = o.get_x_iters_2d(10), e.get_x_iters_2d(10), r.get_x_iters_2d(10)
            for c in range(10):
                d, B = np.abs(xo[:, c] - xr[:, c]).max(), spread_bound(xe[:, c], xo[:, c])
                assert d <= 0.05 * B, f"{name} window {w} column {c}: {d:.3e} vs B = {B:.3e}"
            vec, num = scripted_fix_vec(xo, lo=0.05, hi=0.95, last=5) if fix_after == w else (np.zeros(o.get_n()), 0)
        assert [int(k) for k in r.pcg] == trace


@pytest.mark.parametrize("name", ["S1", "S2", "S3", "S4"])
def test_legacy_solve_figures(name):
    for order in (O.ORDER_GPU, O.ORDER_EIGEN):
        o = seg_oracle(seg_case(name), order=order)
        assert (o.solve_iter(), o.total_outer_iters, o.total_pcg_iters) == SEG_LEGACY[name]
        assert o.last_stop == 1 and len(o.pcg_trace()) == SEG_LEGACY[name][1]
    if name == "S2":
        assert max(o.pcg_trace()) == 44
    if name == "S4":
        assert max(o.pcg_trace()) == 4


BQP_TRACE_ENDS = {"G0": (4, 2), "G1": (8, 6), "G2": (10, 7), "G3": (11, 8)}


@pytest.mark.parametrize("name", ["G0", "G1", "G2", "G3"])
def test_bqp_presets_stay_below_the_starting_kmax(name):
    P, _ = bqp_case(name)
    traces = []
    for order in (O.ORDER_GPU, O.ORDER_EIGEN):
        o = O.BqpOracle(P, params=bqp_case_params(name), order=order)
        assert o.solve() == 30
        traces.append([int(k) for k in o.pcg_trace()])
    r = NumpyBqp(P, params=bqp_case_params(name))
    r.solve(record=True)
    assert traces[0] == traces[1] == [int(k) for k in r.pcg]
    t = traces[0]
    assert (t[0], t[-1]) == BQP_TRACE_ENDS[name] and max(t) == t[0] < BQP_KMAX_START
    assert min(t) > 1                                                                          # kmax = 1: every iteration resumes
    if name != "G0":
        assert min(t) > 3                                                                      # kmax = 3 as well


@pytest.mark.parametrize("name", ["G1", "G2", "G3"])
def test_bqp_with_five_pcg_iterations_caps_every_time(name):
    P, _ = bqp_case(name)
    for order in (O.ORDER_GPU, O.ORDER_EIGEN):
        o = O.BqpOracle(P, params=bqp_case_params(name, pcg_maxiters=5), order=order)
        assert o.solve() == 30 and list(o.pcg_trace()) == [5] * 30
    assert expected_resumes([5] * 30, 2) == 30


def test_g4_needs_two_resumes_in_iteration_0():
    P, _ = bqp_case("G4")
    traces = []
    for order in (O.ORDER_GPU, O.ORDER_EIGEN):
        o = O.BqpOracle(P, params=bqp_case_params("G4"), order=order)
        assert o.solve() == 30
        traces.append([int(k) for k in o.pcg_trace()])
    r = NumpyBqp(P, params=bqp_case_params("G4"))
    r.solve(record=True)
    assert traces[0] == traces[1] == [int(k) for k in r.pcg]
    t = traces[0]
    assert t[0] > BQP_KMAX_START + PAIRS_PER_RESUME == 28                                      # 12 + 16 pairs do not reach it
    assert t[:3] == [31, 30, 31] and t[-1] == 18 and len(set(t)) > 8                           # the graph cache sees several kmax values
