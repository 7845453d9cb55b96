"""The problems of the halt-and-resume tests (tests/test_chain_resume_cases.py on the CPU, tests/test_chain_resume_gpu.py on the GPU)
and the rule that turns an oracle's PCG trace into the number of resumes a launch chain with a fixed kmax must make.

Segmentation (S1..S5) and generic BQP (G0..G4) problems whose PCG needs more (matvec, update) pairs than the chains enqueue: the
chains start at kmax = 10 (segmentation) and 12 (BQP), a resume adds 16 pairs, the segmentation chain never enqueues more than 24."""
import functools

import numpy as np

from helpers import banded_seg_problem, bqp_params, bqp_problem, laplacian_seg_problem, scaled_seg_problem, scripted_fix_vec, synthetic_seg_problem
from oracle import oracle as O

PAIRS_PER_RESUME = 16
SEG_KMAX_START, SEG_KMAX_LIMIT, BQP_KMAX_START = 10, 24, 12
PCG_MAXITERS = 1000


@functools.lru_cache(None)
def seg_case(name):
    if name == "S1":
        return synthetic_seg_problem(4)                                        # an image: diagonal storage, n = 480
    if name == "S2":
        return scaled_seg_problem(banded_seg_problem(1500, 5), 30)              # integer weights <= 150: diagonal storage
    if name == "S3":
        return scaled_seg_problem(laplacian_seg_problem(700, 5, 1), 30)         # ELL, rows of <= 5
    if name == "S4":
        return laplacian_seg_problem(700, 5, 1)
    if name == "S5":
        return scaled_seg_problem(laplacian_seg_problem(3000, 9, 9), 1e7)       # ELL, rows of <= 9: the PCG runs into its cap
    raise KeyError(name)


# the window after which the scripted fix of a case is applied, and how many variables it fixes there (pinned by the CPU file)
SEG_FIX_AFTER = {"S1": 0, "S2": 1, "S3": 1, "S4": None}
SEG_FIXED = {"S1": 268, "S2": 29, "S3": 618}
# legacy solve on the oracle: (energy, outer iterations, PCG iterations)
SEG_LEGACY = {"S1": (182, 548, 1703), "S2": (2510, 1087, 8050), "S3": (17, 844, 2865), "S4": (-282, 156, 290)}

BQP_ML = {0: (0, 0), 1: (25, 0), 2: (0, 25), 3: (25, 20)}


@functools.lru_cache(None)
def bqp_case(name):
    """(problem, type)"""
    if name in ("G0", "G1", "G2", "G3"):
        t = int(name[1])
        m, l = BQP_ML[t]
        return bqp_problem(400, m, l, seed=90 + t), t
    if name == "G4":                                                            # the S3 matrix, scaled by 100, as an unconstrained BQP
        L = scaled_seg_problem(laplacian_seg_problem(700, 5, 1), 100)
        return dict(n=700, A=(L["rowptr"], L["colidx"], L["vals"]), b=L["b"], x0=np.random.RandomState(0).uniform(0.2, 0.8, 700)), 0
    raise KeyError(name)


def bqp_case_params(name, K=30, pcg_maxiters=None):
    p = bqp_params(bqp_case(name)[1], K)
    if pcg_maxiters is not None:
        p[10] = pcg_maxiters
    return p


def expected_resumes(trace, kmax):
    """Resumes of a chain that enqueues `kmax` pairs per outer iteration and 16 more per resume, over the PCG counts `trace`:
    an iteration of K > kmax PCG iterations halts ceil((K - kmax) / 16) times."""
    return int(sum(-(-(int(K) - kmax) // PAIRS_PER_RESUME) for K in trace if K > kmax))


def seg_oracle(P, order=O.ORDER_GPU, T=256, chunk=512):
    o = O.SegOracle(0, P["n"], 0, order=order, T=T, chunk=chunk)
    o.set_problem(P)
    o.solve_init()
    return o


def oracle_windows(o, lengths, fix_after=None):
    """Consecutive l2f windows of the given lengths on the oracle `o`, a scripted fix (helpers.scripted_fix_vec(lo=0.05, hi=0.95,
    last=5) on the window's columns) before the window that follows window `fix_after`.
    Returns (the PCG counts of every iteration, the variables fixed, per window (ret, x_iters))."""
    trace, fixed, out = [], 0, []
    vec, num, it = np.zeros(o.get_org_n()), 0, 0
    for w, ws in enumerate(lengths):
        ret = o.solve_iter_l2f(it, it + ws, vec, num)
        fixed += num
        it += ws
        trace += list(o.pcg_trace())
        x = o.get_x_iters_2d(ws)
        out.append((ret, x))
        vec, num = scripted_fix_vec(x, lo=0.05, hi=0.95, last=min(5, ws)) if fix_after == w else (np.zeros(o.get_n()), 0)
    return trace, fixed, out
