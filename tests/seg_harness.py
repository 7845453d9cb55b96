"""The harness the segmentation GPU tests share (tests/test_seg_branches_gpu.py, tests/test_chain_resume_gpu.py): a HIP solver, the
three references of its problem, and the window loop that holds the four against each other."""
import numpy as np

from helpers import assert_within_bound, bits_equal, common_prefix, scripted_fix_vec
from oracle import oracle as O
from oracle.bqp_numpy import NumpySeg

SCALARS = ("rho1", "gamma", "cur_obj", "std_obj", "cvg1", "cvg2", "obj_val", "best_bin_obj")


def solver(P=None, gray=None, nodes=None):
    from lpbox_hip.seg import PyLPboxADMMsolver
    g = PyLPboxADMMsolver(0, nodes or P["n"], 0)
    g.write_files = False
    if gray is not None:
        g.set_image(gray, nodes)
    else:
        g.set_problem(P)
    g.solve_init()
    return g


def trio(g):
    """The HIP solver's problem on the oracle in its order (T, chunk from the handle), in Eigen order, and on the restatement."""
    P = g.get_problem()
    cfg = g.config()
    o = O.SegOracle(0, P["n"], 0, order=O.ORDER_GPU, T=cfg["threads"], chunk=cfg["threads"] * cfg["elems_per_thread"])
    e = O.SegOracle(0, P["n"], 0)
    for s in (o, e):
        s.set_problem(P)
        s.solve_init()
    r = NumpySeg(P)
    r.solve_init()
    return o, e, r


def windows(g, o, e, r, count, fix_after=None, tag=""):
    """`count` l2f windows of 10 on all four; fix_after = w: a scripted fix (from the oracle's iterates) before window w + 1."""
    vec, num = np.zeros(g.get_org_n()), 0
    fixed = 0
    for w in range(count):
        rets = [s.solve_iter_l2f(10 * w, 10 * w + 10, vec, num) for s in (g, o, e, r)]
        assert len(set(rets)) == 1 and g.get_n() == o.get_n() == r.n, f"{tag} window {w}: {rets}"
        fixed += num
        xg, xo, xe, xr = g.get_x_iters_2d(10), o.get_x_iters_2d(10), e.get_x_iters_2d(10), r.get_x_iters_2d(10)
        assert bits_equal(xg, xo), f"{tag} window {w}: HIP != oracle, max diff {np.abs(xg - xo).max():.3e}"
        assert g.counters() == (o.total_outer_iters, o.total_pcg_iters)
        left = o.vec("left_idx").astype(int)
        for name in ("x", "z1", "z2", "b"):
            assert bits_equal(g.debug_vec(name)[left], o.vec(name)), f"{tag} window {w}: {name}"
        for name in SCALARS:
            assert g.debug_scalar(name) == o.scalar(name), f"{tag} window {w}: {name}"
        # against the restatement while the PCG counts agree
        assert common_prefix(o.pcg_trace(), e.pcg_trace(), r.pcg[-10:]) == 10, f"{tag} window {w}: PCG counts differ"
        for c in range(10):
            assert_within_bound(xg[:, c], xr[:, c], xe[:, c], xo[:, c], f"{tag} window {w} x_iters[{c}]")
        for name in ("x", "z1", "z2", "b"):
            assert_within_bound(o.vec(name), getattr(r, name), e.vec(name), o.vec(name), f"{tag} window {w} {name}")
        for name in SCALARS:
            assert_within_bound(g.debug_scalar(name), getattr(r, "std" if name == "std_obj" else name), e.scalar(name), o.scalar(name),
                                f"{tag} window {w} {name}")
        vec, num = (scripted_fix_vec(xo, lo=0.05, hi=0.95, last=5) if fix_after == w else (np.zeros(g.get_n()), 0))
        if fix_after == w:
            assert num > 0, f"{tag}: nothing to fix after window {w}"
    return fixed
