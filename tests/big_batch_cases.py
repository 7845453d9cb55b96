"""The instances of the batched large-route tests (tests/test_big_batch_api.py on the CPU, tests/test_big_batch_gpu.py on the GPU) and
their oracle runs.  The large route's geometry at these sizes is fixed: 256 threads, 2 slots per thread, so the oracle runs with
T = 256 and chunk = 512 (the GPU file checks that against the handles); an oracle run is made once and its snapshots are shared."""
import functools

import numpy as np

from oracle import oracle as O

T, CHUNK = 256, 512
# (n, seed) -> (stop reason, plain_iter_p1, ret) of ADMM_lp_iters(0, 20000) on the oracle: both stop rules (1: y1/y2 convergence, ret 0;
# 2: the objective's standard deviation, ret 1), four different stopping points, G = 1 (n = 300) and G = 2 (n = 513, 700)
OWN_STOPS = {(300, 0): (2, 7576, 1), (300, 1): (2, 2982, 1), (513, 2): (2, 5251, 1), (700, 3): (1, 5864, 0)}
# G = 1, 2, 3, 5, 6 column workgroups and Gl = 1 ... 3 row workgroups
MIXED = [(300, 0), (513, 2), (1100, 4), (2100, 6), (2600, 7)]
WINDOWS = ((0, 7), (7, 60), (60, 130))
SCALARS = ("rho1", "rho4", "gamma", "dI", "rho4Et", "std_obj", "cur_obj", "cvg1", "cvg2", "obj_val")
VECS = ("x", "z1", "z2", "z4")


@functools.lru_cache(None)
def problem(n, seed):
    from lpbox_hip.synth import make_auction_like
    return make_auction_like(n, seed)


def fresh_oracle(n, seed):
    P = problem(n, seed)
    o = O.LpOracle(0, order=O.ORDER_GPU, T=T, chunk=CHUNK)
    o.set_problem(P["n"], P["l"], P["colptr"], P["rowidx"], P["b"])
    o.solve_init()
    return o


def snapshot(o, ret):
    s = dict(ret=ret, outer_total=o.total_outer_iters, pcg_total=o.total_pcg_iters, trace=tuple(int(k) for k in o.pcg_trace()),
             stop=o.last_stop_reason, plain_iter_p1=o.last_plain_iter_plus1)
    for name in VECS:
        v = o.vec(name)
        v.setflags(write=False)
        s[name] = v
    for name in SCALARS:
        s[name] = o.scalar(name)
    return s


@functools.lru_cache(None)
def oracle_windows(n, seed, windows=WINDOWS):
    """One snapshot per window of consecutive plain windows on a fresh oracle."""
    o = fresh_oracle(n, seed)
    return tuple(snapshot(o, o.solve_iter(a, b)) for (a, b) in windows)


@functools.lru_cache(None)
def oracle_solve(n, seed):
    """ADMM_lp_iters(0, 20000): the snapshot plus the binary solution and the objective."""
    o = fresh_oracle(n, seed)
    s = snapshot(o, o.solve_iter(0, 20000))
    s["x_sol"] = o.get_x_sol().ravel()
    s["obj"] = o.cal_Obj()
    return s


def same_as_snapshot(g, s, tag):
    """Handle `g` (a BigLp) against an oracle snapshot, bit for bit."""
    from helpers import bits_equal
    for name in VECS:
        assert bits_equal(g.vec(name), s[name]), f"{tag}: {name}"
    assert (g.scalar("outer_total"), g.scalar("pcg_total")) == (s["outer_total"], s["pcg_total"]), tag
    for name in SCALARS:
        assert g.scalar(name) == s[name], f"{tag}: {name}"


def same_as_twin(g, t, tag):
    """Handle `g` against a handle that ran the same windows alone."""
    from helpers import bits_equal
    for name in VECS:
        assert bits_equal(g.vec(name), t.vec(name)), f"{tag}: {name} (twin)"
    for name in SCALARS + ("outer_total", "pcg_total", "iter", "stop", "ret", "plain_iter_p1", "last_pcg"):
        assert g.scalar(name) == t.scalar(name), f"{tag}: {name} (twin)"
