"""The cases of the reference-order segmentation tests (tests/test_seg_ref_order_api.py on the CPU, tests/test_seg_ref_order_gpu.py and
tests/test_cxx_seg_ref_order_gpu.py on the GPU) and their runs on the CPU oracle in its Eigen order -- oracle.SegOracle(order=
ORDER_EIGEN): redux_sum_eigen over the compacted live vector, pow(v, 1/2) -- which is what lpbox_seg_set_order(LPBOX_ORDER_REFERENCE)
has to return bit for bit.  Every oracle run is made once and shared: do not modify what these functions return."""
import functools
import math

import numpy as np

import degenerate_cases as D
from helpers import (banded_seg_problem, laplacian_seg_problem, scaled_seg_problem, scripted_fix_vec, synthetic_gray,
                     synthetic_seg_problem)
from oracle import oracle as O
from seg_harness import SCALARS

VECS = ("x", "z1", "z2", "b")
WINDOWS, FIX_AFTER = 5, (1, 3)

# ---- the seven l2f cases and the live counts their scripted fixes (after windows 1 and 3) leave ----
_CASES = {
    "syn0": lambda: synthetic_seg_problem(0),                      # an image, 480: diagonal storage
    "syn1-7x5": lambda: synthetic_seg_problem(1, 7, 5),            # 35
    "lap600": lambda: laplacian_seg_problem(600, 9),               # ELL, non-integer weights and costs
    "lap1029": lambda: laplacian_seg_problem(1029, 64, 1),         # ELL, rows of up to 64: three workgroups
    "band1025": lambda: banded_seg_problem(1025),                  # diagonal storage, one past two workgroups' chunk
    "band9": lambda: banded_seg_problem(9),
    "lap9": lambda: laplacian_seg_problem(9, 4),
}
L2F_CASES = tuple(_CASES)
LIVE = {"syn0": (480, 465, 213), "syn1-7x5": (35, 13, 12), "lap600": (600, 323, 223), "lap1029": (1029, 640, 434),
        "band1025": (1025, 388, 311), "band9": (9, 3), "lap9": (9, 1)}
LAP9_RET = 1                                                       # lap9 returns 1 in the window after its fix

# sizes either side of the short branches of the redux, of one workgroup's chunk (T * EPT = 512) and of the walker's tile (1024), and
# one with G >= 3 at every EPT of the tests
EDGE_N = (1, 2, 3, 4, 5, 6, 7, 511, 512, 513, 1023, 1024, 1025, 1027, 2049)
EPT_FORCED = (1, 4, 8)
EPT_N = 2049 + 2048 * 2 + 3                                        # 6148: G = 25 / 7 / 4 at EPT 1 / 4 / 8


@functools.lru_cache(None)
def problem(name):
    if name in _CASES:
        return _CASES[name]()
    if name.startswith("edge"):                                    # "edge<n>": a banded problem (diagonal storage from n = 2 on)
        n = int(name[4:])
        if n == 1:
            return D.seg_case("boundary-n1")
        return banded_seg_problem(n, 3)
    if name == "c1":
        return laplacian_seg_problem(3000, 9)
    if name == "resume":
        return scaled_seg_problem(laplacian_seg_problem(700, 5, 1), 30)     # S3 of tests/chain_cases.py: 18 PCG iterations in iteration 0
    if name.startswith("deg:"):
        return D.seg_case(name[4:])
    raise KeyError(name)


def oracle(P, order=O.ORDER_EIGEN, T=256, chunk=512):
    o = O.SegOracle(0, P["n"], 0, order=order, T=T, chunk=chunk)
    o.set_problem(P)
    o.solve_init()
    return o


def snapshot(o, ret, ws):
    """What a window leaves on the oracle, by value."""
    return dict(ret=ret, n=o.get_n(), x_iters=o.get_x_iters_2d(ws), left=o.vec("left_idx").astype(int),
                vecs={v: o.vec(v) for v in VECS}, scalars={s: o.scalar(s) for s in SCALARS},
                counters=(o.total_outer_iters, o.total_pcg_iters), trace=tuple(int(k) for k in o.pcg_trace()))


def run_windows(o, windows=WINDOWS, fix_after=FIX_AFTER, ws=10, first_fix=None):
    """`windows` l2f windows of `ws` on the oracle `o`, a scripted fix (scripted_fix_vec(lo=0.05, hi=0.95, last=5) of the window's
    columns) after the windows in fix_after; first_fix = (vec, num) applies before window 0 instead.  Ends behind a window that returns
    1.  Per window: dict(vec, num: what the window was called with; the snapshot behind it)."""
    out = []
    vec, num = first_fix if first_fix is not None else (np.zeros(o.get_org_n()), 0)
    for w in range(windows):
        ret = o.solve_iter_l2f(ws * w, ws * w + ws, vec, num)
        out.append(dict(snapshot(o, ret, ws), vec=vec, num=num))
        if ret:
            break
        vec, num = scripted_fix_vec(out[-1]["x_iters"], lo=0.05, hi=0.95, last=5) if w in fix_after else (np.zeros(o.get_n()), 0)
    return out


@functools.lru_cache(None)
def l2f_reference(name, order=O.ORDER_EIGEN):
    return run_windows(oracle(problem(name), order))


def live_counts(rec):
    """The distinct live counts a run went through, in order."""
    out = []
    for r in rec:
        if not out or out[-1] != r["n"]:
            out.append(r["n"])
    return tuple(out)


@functools.lru_cache(None)
def two_live_reference():
    """band9 fixed down to two live variables: after window 0 everything but the two variables closest to 1/2 goes to its rounded value."""
    o = oracle(problem("band9"))
    first = run_windows(o, windows=1)
    x = first[0]["x_iters"][:, -1]
    keep = np.argsort(np.abs(x - 0.5), kind="stable")[:2]
    vec = (x >= 0.5).astype(np.float64)
    vec[keep] = -1.0
    ret = o.solve_iter_l2f(10, 20, vec, 7)
    return first + [dict(snapshot(o, ret, 10), vec=vec, num=7)]


# ---- c1 = pow(n_live, 1/2): glibc's pow is one ulp away from sqrt at 2921 ----
C1_N, C1_LIVE = 3000, 2921


def pow_differs_from_sqrt(n=C1_LIVE):
    return math.pow(float(n), 0.5) != math.sqrt(float(n))


@functools.lru_cache(None)
def c1_reference():
    """laplacian_seg_problem(3000, 9): window 0, then exactly 79 variables (the ones farthest from 1/2) fixed to their rounded values, so
    that 2921 stay live, and the window after the fix."""
    o = oracle(problem("c1"))
    first = run_windows(o, windows=1)
    x = first[0]["x_iters"][:, -1]
    fix = np.argsort(-np.abs(x - 0.5), kind="stable")[:C1_N - C1_LIVE]
    vec = -np.ones(C1_N)
    vec[fix] = (x[fix] >= 0.5).astype(np.float64)
    ret = o.solve_iter_l2f(10, 20, vec, C1_N - C1_LIVE)
    return first + [dict(snapshot(o, ret, 10), vec=vec, num=C1_N - C1_LIVE)]


# ---- legacy solves ----
def legacy_snapshot(o, energy):
    return dict(energy=energy, stop=(o.last_stop, o.legacy_iter_plus1), counters=(o.total_outer_iters, o.total_pcg_iters),
                x_sol=o.get_x_sol(), obj=o.get_obj(), left=o.vec("left_idx").astype(int), vecs={v: o.vec(v) for v in VECS},
                scalars={s: o.scalar(s) for s in SCALARS}, trace=tuple(int(k) for k in o.pcg_trace()))


@functools.lru_cache(None)
def legacy_reference(name, order=O.ORDER_EIGEN):
    o = oracle(problem(name), order)
    return legacy_snapshot(o, o.solve_iter())


IMAGE_SHAPE, IMAGE_NODES = (60, 50), 3000


def image_gray():
    return synthetic_gray(*IMAGE_SHAPE, seed=5)


# ---- PCG halt and resume: the PCG counts of the resume case in the Eigen order (two windows of 10, no fix) ----
RESUME_TRACE_HEAD = (18, 17, 17)          # iterations 0-2; every one of the 20 iterations needs more pairs than kmax = 1 or 4 enqueues
RESUME_COUNTS = (21, 20)                  # chain_cases.expected_resumes of the 20 counts at kmax = 1 and at kmax = 4


@functools.lru_cache(None)
def resume_reference():
    return run_windows(oracle(problem("resume")), windows=2, fix_after=())


# ---- degenerate branches (tests/degenerate_cases.py): zero right-hand side, DBL_MIN clamp, first residual below the threshold, a zero
# preconditioner diagonal; one window (0, 3) each ----
DEGENERATE = ("b-x0", "b-x1e-155", "b-x1e-160", "zero_td")


@functools.lru_cache(None)
def degenerate_reference(name):
    return run_windows(oracle(problem("deg:" + name)), windows=1, fix_after=(), ws=3)


# ---- batches ----
BATCH_LEGACY = ("syn0", "lap600", "band9", "lap1029", "syn1-7x5", "band1025")      # diagonal and ELL storage, six different n
