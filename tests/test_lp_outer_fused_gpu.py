"""The fused outer iteration of the 512 x 1 LP window kernel: the PCG start vector y1 of iteration k + 1 is formed at the end of
iteration k from the rho that iteration k + 1 will see, E y1 comes out of the row pass that gathers E x, rho4_E_transpose * (E y1) is
published with the other l-vectors -- scaled by what the NEXT refresh will make of rho4_E_transpose -- and one column pass brings the
three products in front of the PCG.  The work that moved depends on where a launch starts (the pre-loop path prepares the first
iteration of a launch), on whether a rho update is pending there, on a fix in that launch, and on the PCG that consumes it.  Every case
below puts a launch boundary, a fix or a short PCG at one of those places and compares every window with the CPU oracle in the kernel's
summation order bit for bit: return code, iterates, state vectors, scalars and counters.

The rho step falls at the end of the iterations with (it + 1) % 25 == 0: a launch that starts at it = 25, 50, 75 finds the update
pending, one that starts anywhere else does not."""
import numpy as np
import pytest

from helpers import bits_equal, oracle_like, scripted_fix_vec
from test_lp_gpu_parity import compare_state, gpu_solver
from test_lp_pcg_loop_gpu import SHAPES, Snapshot, generated

pytestmark = pytest.mark.gpu

# launch boundaries per scenario; "fix" = index of the window that applies a scripted fix made from the window before it
SCENARIOS = {
    # lengths 24, 1, 1, 24, 25, 26: launches start at it = 0, at 24 (nothing pending, the step falls at the end of this one-iteration
    # launch), at 25, 50 and 75 (update pending) and at 26 (not pending)
    "straddle": dict(bounds=[0, 24, 25, 26, 50, 75, 101], fix=None),
    # every iteration is the first of its launch: all of the moved work runs in the pre-loop path (it = 0, pending at 25, neither)
    "ones": dict(bounds=list(range(0, 31)), fix=None),
    # a fix in a launch that starts right behind a rho step: the refresh scales the rho4_E_transpose the fix has just reset (double count)
    "fix_pending": dict(bounds=[0, 50, 75, 101], fix=1),
    # a fix with no update pending
    "fix_plain": dict(bounds=[0, 40, 60, 101], fix=1),
}
# "pcg01" stops after 75 iterations; its PCG of iteration 57 runs once and that of iteration 63 not at all, so one-iteration launches up
# to the stop put both behind a pre-loop path, and the straddling windows put both inside a loop
ONES_PCG01 = dict(bounds=list(range(0, 81)), fix=None)

_ORACLE = {}


def solver(I):
    g = gpu_solver(I)
    cfg = g.batch.config()
    assert (cfg["threads"], cfg["elems_per_thread"]) == (512, 1), "these instances run on the 512 x 1 kernel"
    return g


def oracle_run(name, scen, g, I):
    """The scenario on the CPU oracle, once per (shape, scenario): per window the call's arguments and everything compared afterwards."""
    key = (name, scen)
    if key not in _ORACLE:
        S = ONES_PCG01 if (name, scen) == ("pcg01", "ones") else SCENARIOS[scen]
        o = oracle_like(g, I)
        vec, num, out, x = np.zeros(I["n"]), 0, [], None
        for w, (a, b) in enumerate(zip(S["bounds"][:-1], S["bounds"][1:])):
            if S["fix"] == w:
                vec, num = scripted_fix_vec(x, lo=0.02, hi=0.98, last=20)
                assert 0 < num < o.get_n(), "the scripted vector must fix some variables and leave some"
            else:
                vec, num = np.zeros(o.get_n()), 0
            ret = o.solve_iter_l2f(a, b, vec, num)
            x = o.get_x_iters_2d(b - a)
            out.append(dict(a=a, b=b, vec=vec, num=num, ret=ret, x=x, state=Snapshot(o), counters=(o.total_outer_iters, o.total_pcg_iters),
                            n=o.get_n(), trace=o.pcg_trace(), rho1=o.scalar("rho1")))
            if ret:
                break
        _ORACLE[key] = out
    return _ORACLE[key]


def replay(g, want, tag):
    for ow in want:
        t = f"{tag}, window [{ow['a']}, {ow['b']})"
        rg = g.solve_iter_l2f(ow["a"], ow["b"], ow["vec"], ow["num"])
        assert rg == ow["ret"], t
        assert bits_equal(g.get_x_iters_2d(ow["b"] - ow["a"]), ow["x"]), f"{t}: iterates differ"
        compare_state(g, ow["state"], t)
        assert g.batch.counters() == ow["counters"], t
        assert g.get_n() == ow["n"], t


@pytest.mark.parametrize("scen", list(SCENARIOS))
@pytest.mark.parametrize("name", list(SHAPES))
def test_windows_bit_exact(name, scen):
    I = SHAPES[name]()
    g = solver(I)
    want = oracle_run(name, scen, g, I)
    replay(g, want, f"{name}/{scen}")
    S = SCENARIOS[scen]
    if name == "pcg01":
        assert want[-1]["ret"] == 1, "this instance stops inside the scenario"
        if S["fix"] is None:
            trace = want[-1]["trace"] if scen == "straddle" else np.concatenate([w["trace"] for w in want])
            assert 0 in trace and 1 in trace, f"the instance was picked for a PCG of 0 and one of 1 iteration: {sorted(set(trace.tolist()))}"
            assert want[-1]["counters"][0] == 75
    else:
        assert len(want) == len(S["bounds"]) - 1 and not want[-1]["ret"], "the solve runs through every window"
        # the schedule stepped where the scenario says it does: rho1 grows from one window to the next exactly when a step lies in between
        steps, rhos = [w["b"] // 25 for w in want], [w["rho1"] for w in want]
        assert all((rhos[k] < rhos[k + 1]) == (steps[k] < steps[k + 1]) for k in range(len(want) - 1)), (steps, rhos)
    if S["fix"] is not None:
        assert want[S["fix"]]["n"] < I["n"], "fewer variables after the fix"
        assert want[S["fix"]]["a"] % 25 == (0 if scen == "fix_pending" else 15)


WHOLE = {
    # (instance, stop reason of the plain loop: 1 = y1 / y2 test, 2 = objective-std test)
    "y1y2": (lambda: generated(65, 12), 1),
    "objstd": (lambda: generated(60, 0), 2),
}


@pytest.mark.parametrize("case", list(WHOLE))
def test_whole_solve_stops_where_the_oracle_stops(case):
    mk, reason = WHOLE[case]
    I = mk()
    g = solver(I)
    o = oracle_like(g, I)
    ro, rg = o.solve_iter(0, 20000), g.solve_iter(0, 20000)
    assert o.last_stop_reason == reason, "the instance was picked for this stop test"
    assert rg == ro and g.batch.stop(0)[0] == o.last_stop_reason
    assert g.batch.counters() == (o.total_outer_iters, o.total_pcg_iters)
    compare_state(g, o, case)
    assert np.array_equal(g.get_x_sol().ravel(), o.get_x_sol().ravel()) and g.cal_Obj() == o.cal_Obj()
