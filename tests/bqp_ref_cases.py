"""The problems of the reference-order tests of the BQP batch (tests/test_bqp_batch_ref_order_api.py on the CPU,
tests/test_bqp_batch_ref_order_gpu.py on the GPU) and their solves by oracle/bqp_oracle.c, each computed once.

A case is (problem, preset, params).  `eigen(group, i)` is the case solved by BqpOracle in ORDER_EIGEN -- the reference's association,
what the reference-order kernels must reproduce -- and `kernel_order(group, i)` the same in ORDER_GPU with T = 256, chunk = 512, the
association of the default kernels."""
import functools

from helpers import bqp_params, bqp_problem
from oracle import oracle as O

VECS = ("x", "y1", "y2", "z1", "z2", "z3", "z4", "y3", "best_sol")
EXACT_SCALARS = ("rho1", "rho3", "rho4", "gamma", "cvg1", "cvg2", "cur_obj", "best_bin_obj", "obj_val", "iters", "stop", "total_pcg", "last_pcg")
STD_OBJ_ULPS = 2          # the std stop test takes sqrt where the reference calls pow(v, 1/2): DESIGN.md section 18

# ---- 1. the branches of the redux (n = 1, 2, 3 short; the chains; the left-over pair; the odd last element), in each slot count ------
SMALL = tuple(range(2, 12))
REDUX_SIZES = {"slots2": SMALL + (255, 256, 257, 511, 512),
               "slots4": SMALL + (1021, 1022, 1023, 1024),
               "slots8": SMALL + (1026, 2045, 2046, 2047, 2048)}
REDUX_SLOTS = {"slots2": 2, "slots4": 4, "slots8": 8}
REDUX_K = 60
# sizes at which the oracle's two orders end on different bits of x after REDUX_K iterations (pinned by the CPU file): every size
# of the three batches except 2, 3, 4, 10 and 11, and 513.  At those five a test cannot tell the orders apart by x; they stay in as
# coverage of the short branches.
ORDERS_DIFFER = (5, 6, 7, 8, 9, 255, 256, 257, 511, 512, 513, 1021, 1022, 1023, 1024, 1026, 2045, 2046, 2047, 2048)
ORDERS_AGREE = (2, 3, 4, 10, 11)
PIN_SIZES = tuple(sorted(set(ORDERS_DIFFER + ORDERS_AGREE)))


@functools.lru_cache(None)
def redux_case(n):
    ml = 1 if n < 16 else 8
    return bqp_problem(n, ml, ml, seed=n), 3, tuple(bqp_params(3, REDUX_K))


# ---- 2. all four types, the edge shapes of test_bqp_edges_gpu.py ---------------------------------------------------------------------
@functools.lru_cache(None)
def mixed_cases():
    out = []
    for ptype in (0, 1, 2, 3):
        for offdiag in (False, True):
            m, l = (0, 25, 0, 15)[ptype], (0, 0, 25, 20)[ptype]
            out.append((bqp_problem(400, m, l, seed=90 + ptype, offdiag=offdiag), ptype, tuple(bqp_params(ptype, 8))))
    for n, m, l in [(257, 1, 0), (257, 0, 1), (257, 1, 1), (256, 0, 300), (200, 20, 260)]:     # single rows, more rows than variables
        t = (1 if m else 0) | (2 if l else 0)
        out.append((bqp_problem(n, m, l, seed=7 * n + m + l), t, tuple(bqp_params(t, 8))))
    out.append((bqp_problem(300, 40, 50, seed=5), 3, tuple(bqp_params(3, 8))))                 # empty rows and columns
    out.append((bqp_problem(150, 15, 0, 60, indefinite=True), 1, tuple(bqp_params(1, 3))))
    return tuple(out)


RESTATEMENT_PICK = 13       # index into mixed_cases(): the problem held within B of oracle/bqp_numpy.py

# ---- 3. problems to their own stops: (n, m, l, seed, max_iters or None for the preset's 10^4) ------------------------------------------
STOPPING = ((120, 0, 0, 1000, None), (160, 12, 0, 1000, None), (200, 0, 15, 1001, None), (200, 0, 15, 1000, 8),
            (400, 25, 20, 0, None), (400, 25, 20, 1, None))
SEED1_INDEX = 5
SEED1_BEST_BIN_OBJ = {O.ORDER_EIGEN: 39.044531052280874, O.ORDER_GPU: 40.076849524109555}


@functools.lru_cache(None)
def stopping_cases():
    from oracle.bqp_numpy import PRESETS
    out = []
    for n, m, l, seed, cap in STOPPING:
        t = (1 if m else 0) | (2 if l else 0)
        prm = list(PRESETS[t])
        if cap is not None:
            prm[5] = cap
        out.append((bqp_problem(n, m, l, seed=seed), t, tuple(prm)))
    return tuple(out)


# ---- 6. more problems than compute units ---------------------------------------------------------------------------------------------
MANY = 300
MANY_CHECKED = tuple(range(0, MANY, 10))


@functools.lru_cache(None)
def many_cases():
    out = []
    for i in range(MANY):
        n, t = 5 + i % 36, i % 4
        P = bqp_problem(n, max(1, n // 6) if t & 1 else 0, max(1, n // 5) if t & 2 else 0, seed=3000 + i, offdiag=bool(i % 5))
        out.append((P, t, tuple(bqp_params(t, 8))))
    return tuple(out)


def cases(group):
    if group in REDUX_SIZES:
        return tuple(redux_case(n) for n in REDUX_SIZES[group])
    if group == "pin":
        return tuple(redux_case(n) for n in PIN_SIZES)
    return {"mixed": mixed_cases, "stopping": stopping_cases, "many": many_cases}[group]()


def solve_oracle(case, order):
    P, preset, params = case
    o = O.BqpOracle(P, preset=preset, params=list(params), order=order, T=256, chunk=512)
    return o, o.solve()


@functools.lru_cache(None)
def eigen(group, i):
    """(solved oracle, iterations) of case i of the group in the reference's order"""
    return solve_oracle(cases(group)[i], O.ORDER_EIGEN)


@functools.lru_cache(None)
def kernel_order(group, i):
    return solve_oracle(cases(group)[i], O.ORDER_GPU)


def vec_names(P):
    return [v for v in VECS if (v != "z3" or P.get("C") is not None) and (v not in ("z4", "y3") or P.get("E") is not None)]
