"""The problems of the reference-order tests of the one-problem BQP chain (tests/test_bqp_ref_order_api.py on the CPU,
tests/test_bqp_ref_order_gpu.py on the GPU) and their solves by oracle/bqp_oracle.c, each computed once.

The size cases are those of tests/bqp_ref_cases.py (`redux_case`: bqp_problem(n, ml, ml, seed=n), ml = 1 below n = 16 and 8 from
there, preset 3, 60 iterations); the chain has no 2048 limit, so the list goes on past it, around the walker's tiles of 1024."""
import functools

import numpy as np

import bqp_ref_cases as K
from helpers import bqp_params, bqp_problem
from oracle import oracle as O

WALK_TILE = 1024                 # WTILE of csrc/lpbox_gen_ref_kernels.hip
SIZES = (tuple(range(2, 12))                                                                  # the short branches, the left-over pair, the odd last element
         + (255, 256, 257, 511, 512, 513)                                                     # around the producers' workgroup and chunk
         + (1023, 1024, 1025, 1027, 2047, 2048, 2049, 2050, 2051, 3073, 4097))                # -1, 0, +1, +2, +3 around one, two, three and four tiles
# sizes at which the oracle's two orders end on the same bits of x after the 60 iterations (pinned by the CPU file): there a test cannot
# tell the orders apart by x, they stay in as coverage of the short branches.  2 and 3 have a single association; 4, 10 and 11 are
# the sizes tests/bqp_ref_cases.py already lists as agreeing.
ORDERS_AGREE = (2, 3, 4, 10, 11)

# above the batch limit: the association decides the binary answer (preset 3 to the 10^4-iteration cap in both orders)
BIG = (2100, 64, 64, 1)
BIG_BEST_BIN_OBJ = {O.ORDER_EIGEN: 147.6795702348325, O.ORDER_GPU: 148.33867126179442}
BIG_PCG_STEPS = {O.ORDER_EIGEN: 92455, O.ORDER_GPU: 92163}
BIG_BINARY_DIFFERENCES = 7


def size_case(n):
    return K.redux_case(n)


@functools.lru_cache(None)
def big_case(max_iters=None):
    from oracle.bqp_numpy import PRESETS
    n, m, l, seed = BIG
    prm = list(PRESETS[3])
    if max_iters is not None:
        prm[5] = max_iters
    return bqp_problem(n, m, l, seed=seed), 3, tuple(prm)


@functools.lru_cache(None)
def big_oracle(order, max_iters=None):
    return K.solve_oracle(big_case(max_iters), order)


@functools.lru_cache(None)
def size_oracle(n, order):
    """(solved oracle, iterations) of the size case; ORDER_GPU with T = 256, chunk = 512"""
    return K.solve_oracle(size_case(n), order)


@functools.lru_cache(None)
def two_pow_21_case():
    """The tridiagonal unconstrained problem of tests/test_bqp_edges_gpu.py::test_above_2_pow_21_variables_takes_four_slots, restated:
    n just above 2,097,152, where the chain kernels take four slots per thread (chunk 1024); two iterations."""
    n = 2097152 + 300
    rs = np.random.RandomState(8)
    off = -rs.uniform(0.1, 1.0, n - 1)
    dg = np.concatenate([[0.0], -off]) + np.concatenate([-off, [0.0]]) + rs.uniform(0.5, 1.5, n)
    rp = np.concatenate([[0], np.cumsum(np.r_[2, np.full(n - 2, 3), 2])]).astype(np.int32)
    ci = np.empty(rp[-1], np.int32)
    va = np.empty(rp[-1])
    i = np.arange(n)
    pos = rp[:-1].copy()
    has_lo = i > 0
    ci[pos[has_lo]] = i[has_lo] - 1; va[pos[has_lo]] = off[i[has_lo] - 1]; pos[has_lo] += 1
    ci[pos] = i; va[pos] = dg; pos += 1
    has_hi = i < n - 1
    ci[pos[has_hi]] = i[has_hi] + 1; va[pos[has_hi]] = off[i[has_hi]]
    P = dict(n=n, A=(rp, ci, va), b=rs.uniform(-3, 1, n), x0=np.zeros(n))
    return P, 0, tuple(bqp_params(0, 2))
