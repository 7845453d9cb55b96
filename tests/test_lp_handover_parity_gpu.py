"""The 512 x 1 LP window kernel with its LDS hand-overs (lds_handover(), no drain of the LDS counter in front of the barrier) against the
same library built with the step macro at 0 (make variant: the parent's text, __syncthreads() everywhere) and against the CPU oracle.

Both builds run, each in a process of its own library, on the j = 20 / k = 60 fixture, on four instances of the j = 100 / k = 500 fixture and
on the wave shapes of tests/test_lp_pcg_loop_gpu.py (an empty wave, every lane in use, a wave with a list tail, a PCG of 0 and of 1
iteration): three windows with a scripted fix, and whole solves that stop on either stop test.  Iterates, counters and state scalars must
be identical on their uint64 views, and equal to the oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "accelerated-lpbox-admm_amd")
if __name__ == "__main__":
    for p in (HERE, ROOT, PKG):
        if p not in sys.path:
            sys.path.insert(0, p)

from helpers import bits_equal, lp_instances, oracle_for, oracle_full_solve, scripted_fix_vec
from test_lp_pcg_loop_gpu import SHAPES

pytestmark = pytest.mark.gpu

VARIANT = "handover_off"
VARIANT_FLAGS = "-DLPBOX_LP_HANDOVER_PCG=0"
WS = 40
BIG = (0, 2, 5, 7)                             # instances of the 100 / 500 fixture
VECS = ("x", "z1", "z2", "z4", "f")
SCALARS = ("rho1", "rho4", "gamma", "dI", "rho4Et", "std_obj", "cur_obj", "sum_fix_obj", "best_bin_obj", "cvg1", "cvg2", "obj_val")
STOP_Y1Y2, STOP_OBJSTD = 1, 2                  # LP_STOP_* of csrc/lpbox_lp.h


def window_cases():
    cases = {name: make() for name, make in SHAPES.items()}
    big = lp_instances("lp_100_500_seed0.npz")
    for i in BIG:
        cases[f"lp100_500_{i}"] = big[i]
    return cases


def solve_batches():
    small, big = lp_instances("lp_20_60_seed0.npz"), lp_instances("lp_100_500_seed0.npz")
    return {"lp20_60": small[:4], "lp100_500": [big[i] for i in BIG]}


def run_windows(I, fix=True):
    """Three windows of WS iterations; the fix of the second comes from the iterates of the first (fix = False: none, the instance picked
    for its short PCGs keeps the course it was found on).  -> flat list of float64 arrays."""
    from test_lp_gpu_parity import gpu_solver
    g = gpu_solver(I)
    cfg = g.batch.config()
    assert (cfg["threads"], cfg["elems_per_thread"], cfg["pcg_loop"]) == (512, 1, "specialised")
    out, vec, num = [], np.zeros(I["n"]), 0
    for w in range(3):
        ret = g.solve_iter_l2f(w * WS, (w + 1) * WS, vec, num)
        x = g.get_x_iters_2d(WS)
        out += [np.array([ret, g.get_n(), *g.batch.counters()], np.float64), x.ravel()]
        out += [g.batch.debug_vec(k) for k in VECS] + [np.array([g.batch.debug_scalar(k) for k in SCALARS])]
        if w == 0 and fix:
            vec, num = scripted_fix_vec(x, lo=0.02, hi=0.98, last=20)
        else:
            vec, num = np.zeros(g.get_n()), 0
        if ret:
            break
    return out, g


def run_solves(insts):
    from lpbox_hip.lp import LpBatch
    B = LpBatch(insts)
    cfg = B.config()
    assert (cfg["threads"], cfg["elems_per_thread"]) == (512, 1)
    B.solve_init()
    rets = B.solve_iter(0, 20000)
    out = []
    for i in range(len(insts)):
        out += [np.array([rets[i], *B.counters(i), B.stop(i)[0], B.cal_obj(i)], np.float64), B.debug_vec("x", i), B.get_x_sol(i).ravel().astype(np.float64)]
    return out, B


def payload():
    arrs = {}
    for name, I in window_cases().items():
        for k, a in enumerate(run_windows(I, fix=name != "pcg01")[0]):
            arrs[f"w/{name}/{k}"] = np.ascontiguousarray(a, np.float64)
    for name, insts in solve_batches().items():
        for k, a in enumerate(run_solves(insts)[0]):
            arrs[f"s/{name}/{k}"] = np.ascontiguousarray(a, np.float64)
    return arrs


def same_bits(a, b):
    """uint64 views; a NaN state scalar must meet a NaN."""
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    a, b = np.where(np.isnan(a), 0.0, a), np.where(np.isnan(b), 0.0, b)
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.fixture(scope="module")
def variant_library():
    """liblpbox_hip_handover_off.so: built here unless it is already newer than its sources."""
    csrc = os.path.join(PKG, "csrc")
    lib = os.path.join(PKG, "lpbox_hip", f"liblpbox_hip_{VARIANT}.so")
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hip", ".h", ".cpp"))] + [os.path.join(ROOT, "include", "lpbox_hip.h")]
    if not os.path.exists(lib) or any(os.path.getmtime(s) > os.path.getmtime(lib) for s in srcs):
        subprocess.check_call(["make", "-s", "-C", csrc, "variant", f"NAME={VARIANT}", f"EXTRA={VARIANT_FLAGS}"])
    return lib


@pytest.fixture(scope="module")
def shipped():
    assert not os.environ.get("LPBOX_LIB_VARIANT"), "this process must run the shipped library"
    return payload()


def test_same_bits_as_the_build_without_the_handovers(tmp_path, variant_library, shipped):
    out = str(tmp_path / "variant.npz")
    env = dict(os.environ, LPBOX_LIB_VARIANT=VARIANT)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.load(out)
    assert sorted(got.files) == sorted(shipped), "both builds ran the same cases through the same windows"
    for k in shipped:
        assert same_bits(shipped[k], got[k]), f"{k}: the two builds differ"


@pytest.mark.parametrize("name", list(SHAPES) + [f"lp100_500_{i}" for i in BIG])
def test_windows_equal_the_oracle(shipped, name):
    I = window_cases()[name]
    from test_lp_gpu_parity import gpu_solver
    g = gpu_solver(I)
    o = oracle_for(g.batch, 0, I)
    got = [shipped[f"w/{name}/{k}"] for k in range(sum(1 for f in shipped if f.startswith(f"w/{name}/")))]
    per = 2 + len(VECS) + 1
    vec, num = np.zeros(I["n"]), 0
    for w in range(len(got) // per):
        head, x, *rest = got[w * per:(w + 1) * per]
        ret = o.solve_iter_l2f(w * WS, (w + 1) * WS, vec, num)
        xo = o.get_x_iters_2d(WS)
        assert list(head) == [ret, o.get_n(), o.total_outer_iters, o.total_pcg_iters], f"window {w}"
        assert bits_equal(x, xo.ravel()), f"window {w}: iterates differ from the oracle"
        left = o.vec("left_idx").astype(int)
        for k, gv in zip(VECS, rest):
            assert bits_equal(gv[left] if k in ("x", "z1", "z2") else gv, o.vec(k)), f"window {w}: {k}"
        assert same_bits(rest[-1], np.array([o.scalar(k) for k in SCALARS])), f"window {w}: state scalars"
        vec, num = scripted_fix_vec(xo, lo=0.02, hi=0.98, last=20) if w == 0 and name != "pcg01" else (np.zeros(o.get_n()), 0)
        assert w > 0 or name == "pcg01" or 0 < num < I["n"], "the scripted vector must fix some variables and leave some"
    if name == "pcg01":
        trace = o.pcg_trace()
        assert len(got) // per == 2 and ret == 1 and 0 in trace and 1 in trace, "it stops in the second window, behind a PCG of 0 and one of 1 iteration"
    else:
        assert len(got) // per == 3 and o.get_n() < I["n"], "the solve runs through all three windows, with fewer variables after the fix"


@pytest.mark.parametrize("name", ["lp20_60", "lp100_500"])
def test_whole_solves_equal_the_oracle(shipped, name):
    from lpbox_hip.lp import LpBatch
    insts = solve_batches()[name]
    B = LpBatch(insts)
    stops = set()
    for i, I in enumerate(insts):
        ret, outer, pcg, obj, x, xs = oracle_full_solve((I, 512, 512, B.layout(i), B.row_split(i), B.col_split(i)))
        head, gx, gxs = (shipped[f"s/{name}/{3 * i + k}"] for k in range(3))
        assert list(head[:3]) == [ret, outer, pcg] and head[4] == obj, (name, i)
        assert bits_equal(gx, x) and np.array_equal(gxs, xs), (name, i)
        stops.add(int(head[3]))
    print(f"{name}: stop reasons {sorted(stops)}")
    assert stops <= {STOP_OBJSTD, STOP_Y1Y2}


def test_the_solves_stop_on_either_test(shipped):
    stops = set()
    for name, insts in solve_batches().items():
        stops |= {int(shipped[f"s/{name}/{3 * i}"][3]) for i in range(len(insts))}
    assert stops == {STOP_OBJSTD, STOP_Y1Y2}, f"one whole solve per stop test: {sorted(stops)}"


if __name__ == "__main__":
    np.savez(sys.argv[1], **payload())
