"""The problems of the lockstep-batch tests of the generic BQP (tests/test_bqp_lockstep_api.py on the CPU, tests/test_bqp_lockstep_gpu.py
on the GPU), and their oracle runs: every member is solved once by oracle/bqp_oracle.c in the kernels' order (T = 256 threads, 512
variables per workgroup: what `BqpSolver.scalar("threads")` / `("chunk")` report below 2^21 variables) and the result is shared by all
tests that need it.

A member is (problem, params).  EXTENTS: one batch whose members have 1, 1, 1, 2, 3, 4 column workgroups, all four types, single rows
and more rows than variables.  STOPS: members that end at pairwise different iterations by all three ends.  RESUME: the halt-and-resume
problems of tests/chain_cases.py side by side.  MANY: 300 small members.  WIDE: a member above BqpBatch's limit beside a 2-variable one."""
import functools

import numpy as np

from chain_cases import bqp_case, bqp_case_params
from helpers import BQP_SCALARS, BQP_VECS, bqp_params, bqp_problem
from oracle import oracle as O

T, CHUNK = 256, 512
INT_SCALARS = ("stop", "total_pcg")


def ptype_of(P):
    return (1 if P.get("C") is not None else 0) | (2 if P.get("E") is not None else 0)


def names(P):
    return [v for v in BQP_VECS if v not in ("z3",) or P.get("C") is not None
            if v not in ("z4", "y3") or P.get("E") is not None]


def groups(P):
    """(G, Gm, Gl): the workgroups over the variables, the rows of C and the rows of E."""
    m = len(P["d"]) if P.get("C") is not None else 0
    l = len(P["f"]) if P.get("E") is not None else 0
    return tuple(-(-v // CHUNK) for v in (P["n"], m, l))


# (n, m, l, seed): G = 1, 1, 1, 2, 3, 4; types 0, 1, 2, 2, 3, 1; m = 1, l = 1; l > n with Gl = 3 > G = 2; Gm = 2 beside Gl = 0
EXTENTS_SHAPES = [(2, 0, 0, 11), (255, 1, 0, 12), (512, 0, 1, 13), (513, 0, 1100, 14), (1025, 30, 20, 15), (1537, 600, 0, 16)]
EXTENTS_K = 12

# (n, m, l, seed, changes to the type's preset by index of bqp.PARAM_NAMES): the ends are pinned in tests/test_bqp_lockstep_api.py
STOPS_SHAPES = [
    (300, 0, 0, 21, {0: 5e-2}),              # x / y1 / y2 stop (stop_threshold raised)
    (600, 20, 0, 22, {0: 5e-2}),             # the same stop, later, two workgroups
    (300, 0, 20, 23, {1: 2e-2}),             # objective-std stop (std_threshold raised)
    (520, 20, 20, 24, {1: 2e-2}),            # the same stop at another iteration
    (300, 25, 20, 25, {5: 7}),               # its own max_iters
    (513, 0, 0, 26, {5: 19}),                # another max_iters
    (40, 5, 5, 27, {5: 40}),                 # a third max_iters, below one workgroup
]
BEST_MEMBER = 4                               # of STOPS: its last iteration improves the binary objective (pinned in the CPU file)

RESUME_NAMES = ["G4", "G1", "G3"]
MANY_COUNT, MANY_K = 300, 20
WIDE_K = 30


@functools.lru_cache(None)
def extents():
    return [(bqp_problem(n, m, l, seed=s), bqp_params((1 if m else 0) | (2 if l else 0), EXTENTS_K)) for (n, m, l, s) in EXTENTS_SHAPES]


@functools.lru_cache(None)
def stops():
    out = []
    for (n, m, l, s, change) in STOPS_SHAPES:
        from oracle.bqp_numpy import PRESETS
        p = list(PRESETS[(1 if m else 0) | (2 if l else 0)])
        p[4] = 3
        for k, v in change.items():
            p[k] = v
        out.append((bqp_problem(n, m, l, seed=s), p))
    return out


@functools.lru_cache(None)
def resume():
    return [(bqp_case(name)[0], bqp_case_params(name)) for name in RESUME_NAMES]


@functools.lru_cache(None)
def many():
    out = []
    for i in range(MANY_COUNT):
        t = i % 4
        n = 2 + (i * 7) % 63                                     # 2 ... 64
        m, l = (1 + i % 5 if t & 1 else 0), (1 + i % 6 if t & 2 else 0)
        out.append((bqp_problem(n, m, l, seed=1000 + i), bqp_params(t, MANY_K)))
    return out


@functools.lru_cache(None)
def wide():
    return [(bqp_problem(2100, 64, 64, seed=1), bqp_params(3, WIDE_K)), (bqp_problem(2, 0, 0, seed=2), bqp_params(0, WIDE_K))]


@functools.lru_cache(None)
def doors():
    """solve_any's list: n = 40 and 400 for BqpBatch, 2100 for BqpLockstep, the large one in the middle."""
    return [(bqp_problem(40, 4, 3, seed=31), bqp_params(3, 15)), wide()[0], (bqp_problem(400, 0, 10, seed=32), bqp_params(2, 15))]


SETS = dict(extents=extents, stops=stops, resume=resume, many=many, wide=wide, doors=doors)


def oracle_result(P, params):
    o = O.BqpOracle(P, params=params, order=O.ORDER_GPU, T=T, chunk=CHUNK)
    it = o.solve()
    r = dict(iterations=it, trace=[int(k) for k in o.pcg_trace()])
    for name in names(P):
        r[name] = o.vec(name)
    for name in BQP_SCALARS + INT_SCALARS:
        r[name] = o.scalar(name)
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


@functools.lru_cache(None)
def oracle_runs(set_name):
    """The oracle's result for every member of a set, computed once."""
    return [oracle_result(P, params) for (P, params) in SETS[set_name]()]


@functools.lru_cache(None)
def oracle_run_with(set_name, i, max_iters):
    """Member i of a set with another max_iters."""
    P, params = SETS[set_name]()[i]
    p = list(params)
    p[5] = max_iters
    return oracle_result(P, p)
