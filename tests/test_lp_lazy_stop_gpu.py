"""The leaner instruction stream of the 512 x 1 LP window kernel: stop-test quotients that are formed only where
a filter cannot decide the test and otherwise stay pending until the state is written back, fixed variables that run through the PCG
as +0.0 instead of being masked, wide butterfly steps without register copies.  None of it may change a bit, so every case compares
with the CPU oracle in the kernel's summation order bit for bit after EVERY launch -- iterates, state vectors, counters and in
particular the scalars cvg1, cvg2 and std_obj, which a launch now has to materialise at whatever exit it takes.

Instances: n = 40 (the layout deals 16, 16 and 8 variables to three wavefronts, five stay empty) and n = 70 (four wavefronts with 16
variables, one with 6, three empty)."""
import numpy as np
import pytest

from helpers import bits_equal, oracle_like, scalar_bits_equal
from test_lp_gpu_parity import compare_state, gpu_solver
from test_lp_pcg_loop_gpu import Snapshot, generated

pytestmark = pytest.mark.gpu

LAZY_SCALARS = ("cvg1", "cvg2", "std_obj")
SHAPES = {"n40": lambda: generated(40, 1), "n70": lambda: generated(70, 2)}
BOUNDS = {
    # every iteration is the last of its launch: the pending values are materialised at every exit; launches 1..9 take the
    # std test with a window that is not full yet (the stale value of the state), launch 10 fills it
    "ones": list(range(0, 31)),
    # 9 + 1: the window fills in a one-iteration launch; + 1: full window from the first iteration of a launch; + 10: full throughout
    "9_1_1_10": [0, 9, 10, 11, 21],
}
_ORACLE = {}


def solver(I):
    g = gpu_solver(I)
    cfg = g.batch.config()
    assert (cfg["threads"], cfg["elems_per_thread"]) == (512, 1), "these instances run on the 512 x 1 kernel"
    return g


def check_window(g, ow, tag):
    assert bits_equal(g.get_x_iters_2d(ow["b"] - ow["a"]), ow["x"]), f"{tag}: iterates differ"
    compare_state(g, ow["state"], tag)
    for k in LAZY_SCALARS:
        assert scalar_bits_equal(g.batch.debug_scalar(k), ow["state"].scalar(k)), f"{tag}: {k} {g.batch.debug_scalar(k)!r} vs {ow['state'].scalar(k)!r}"
    assert g.batch.counters() == ow["counters"], tag
    assert g.get_n() == ow["n"], tag


def oracle_windows(key, o, windows):
    """windows: (a, b, vec, num) or a callable (previous iterates -> that tuple).  Cached per key: the oracle runs once."""
    if key not in _ORACLE:
        out, x = [], None
        for w in windows:
            a, b, vec, num = w(x, o) if callable(w) else w
            ret = o.solve_iter_l2f(a, b, vec, num)
            x = o.get_x_iters_2d(b - a)
            out.append(dict(a=a, b=b, vec=vec, num=num, ret=ret, x=x, state=Snapshot(o), counters=(o.total_outer_iters, o.total_pcg_iters),
                            n=o.get_n(), trace=o.pcg_trace()))
            if ret:
                break
        _ORACLE[key] = out
    return _ORACLE[key]


@pytest.mark.parametrize("scen", list(BOUNDS))
@pytest.mark.parametrize("name", list(SHAPES))
def test_launch_boundaries_bit_exact(name, scen):
    I = SHAPES[name]()
    if name == "n70":
        assert I["n"] == 70
    g = solver(I)
    bounds = BOUNDS[scen]
    free = np.zeros(I["n"])
    want = oracle_windows((name, scen), oracle_like(g, I), [(a, b, free, 0) for a, b in zip(bounds[:-1], bounds[1:])])
    assert len(want) == len(bounds) - 1 and not want[-1]["ret"], "the solve runs through every window"
    for ow in want:
        tag = f"{name}/{scen}, window [{ow['a']}, {ow['b']})"
        assert g.solve_iter_l2f(ow["a"], ow["b"], ow["vec"], ow["num"]) == ow["ret"], tag
        check_window(g, ow, tag)
    # the scenario does what it was written for: the objective window fills at iteration 10, std_obj moves from then on
    stds = [w["state"].scalar("std_obj") for w in want]
    before = [s for w, s in zip(want, stds) if w["b"] < 10]
    assert all(scalar_bits_equal(s, before[0]) for s in before), "std_obj keeps the value of solve_init while the window fills"
    assert not scalar_bits_equal(stds[-1], before[0])


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
    for k in LAZY_SCALARS:
        assert scalar_bits_equal(g.batch.debug_scalar(k), o.scalar(k)), k
    if reason == 2:
        assert o.scalar("std_obj") <= 1e-12
    else:
        assert o.scalar("cvg1") <= 1e-4 and o.scalar("cvg2") <= 1e-4
    assert np.array_equal(g.get_x_sol().ravel(), o.get_x_sol().ravel()) and g.cal_Obj() == o.cal_Obj()


def test_constant_objective_takes_the_exact_path():
    """b = 0: the objective is 0 in every iteration, so the deviation AND the last value of the window are 0 -- both guards of the
    std filter -- and std_obj = 0 / 0 is a NaN, which stops nothing.  Same on both sides, NaN for NaN."""
    I = dict(generated(40, 1))
    I["b"] = np.zeros(I["n"])
    g = solver(I)
    free = np.zeros(I["n"])
    want = oracle_windows("b0", oracle_like(g, I), [(0, 9, free, 0), (9, 12, free, 0), (12, 30, free, 0)])
    for ow in want:
        tag = f"b = 0, window [{ow['a']}, {ow['b']})"
        assert g.solve_iter_l2f(ow["a"], ow["b"], ow["vec"], ow["num"]) == ow["ret"], tag
        assert bits_equal(g.get_x_iters_2d(ow["b"] - ow["a"]), ow["x"]), tag
        for k in LAZY_SCALARS + ("obj_val",):
            assert scalar_bits_equal(g.batch.debug_scalar(k), ow["state"].scalar(k)), f"{tag}: {k}"
        assert g.batch.counters() == ow["counters"], tag
    assert np.isnan(want[-1]["state"].scalar("std_obj")) and want[-1]["state"].scalar("obj_val") == 0.0


def kill_wave(wave):
    """Window maker: fix EVERY live variable stored in wavefront `wave` (to the rounding of its last iterate), leave the others free."""
    def make(x, o, a=40, b=80):
        pos = kill_wave.pos
        vec = -np.ones(x.shape[0])
        hit = (pos >> 6) == wave
        vec[hit] = (x[hit, -1] >= 0.5).astype(np.float64)
        return a, b, vec, int(hit.sum())
    return make


@pytest.mark.parametrize("wave", [0, 4])
def test_a_fix_that_empties_a_wavefront(wave):
    """n = 70: wavefronts 0..3 hold 16 variables each, wavefront 4 six.  An l2f window with a fix that kills all variables of one of
    them -- its lanes then carry zeros through the PCG, next to wavefronts that have live and unused lanes -- followed by a plain window."""
    I = SHAPES["n70"]()
    g = solver(I)
    pos = np.asarray(g.batch.layout(0))
    assert np.bincount(pos >> 6, minlength=8).tolist() == [16, 16, 16, 16, 6, 0, 0, 0]
    kill_wave.pos = pos
    free = lambda n: np.zeros(n)
    want = oracle_windows(("kill", wave), oracle_like(g, I),
                          [(0, 40, free(70), 0), kill_wave(wave), lambda x, o: (80, 120, free(o.get_n()), 0)])
    assert len(want) == 3 and not want[-1]["ret"]
    assert want[1]["n"] == 70 - (16 if wave == 0 else 6), "the whole wavefront is gone"
    for ow in want:
        tag = f"kill wave {wave}, window [{ow['a']}, {ow['b']})"
        assert g.solve_iter_l2f(ow["a"], ow["b"], ow["vec"], ow["num"]) == ow["ret"], tag
        check_window(g, ow, tag)


def test_pcg_of_zero_and_one_iteration_with_dead_lanes():
    """The instance whose PCG runs once at iteration 57 and not at all at iteration 63 (tests/test_lp_pcg_loop_gpu.py), here behind a
    fix at iteration 40 that leaves dead lanes in its one busy wavefront."""
    I = generated(60, 0)
    g = solver(I)

    def fix_some(x, o):
        vec = -np.ones(x.shape[0])
        vec[np.all(x[:, -5:] < 0.02, axis=1)] = 0.0
        return 40, 70, vec, int((vec != -1).sum())
    want = oracle_windows("pcg01fix", oracle_like(g, I), [(0, 40, np.zeros(I["n"]), 0), fix_some, lambda x, o: (70, 100, np.zeros(o.get_n()), 0)])
    assert 0 < want[1]["num"] < I["n"]
    for ow in want:
        tag = f"pcg01 with a fix, window [{ow['a']}, {ow['b']})"
        assert g.solve_iter_l2f(ow["a"], ow["b"], ow["vec"], ow["num"]) == ow["ret"], tag
        check_window(g, ow, tag)
    lens = set(np.concatenate([w["trace"] for w in want]).tolist())
    assert min(lens) <= 1, f"a PCG of at most one iteration runs behind the fix: {sorted(lens)}"
