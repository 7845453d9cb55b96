"""The instances of the batched large route in the reference summation order (tests/test_big_ref_batch_api.py on the CPU,
tests/test_big_ref_batch_gpu.py on the GPU) and their runs on the oracle in ORDER_EIGEN.  An oracle run is made
once per (instance, family of stored values, windows); its snapshots are read-only and shared by the tests.  `with_vals`,
`eigen_oracle`, `odd_instance` and the comparison rule are those of tests/test_big_ref_order_gpu.py, restated."""
import functools

import numpy as np

from oracle import oracle as O

T, CHUNK = 256, 512                                   # the large route's geometry at these sizes (the default order's oracle needs it)
FAMILY = np.array([0.25, 0.5, 1.0, 2.0, -1.0, 3.5])
LEARNING_FACT = 1 + 1.0 / 100
# G = 1, 2, 3, 5, 6 column workgroups and Gl = 1 ... 3 row workgroups
MIXED = [(300, 0), (513, 2), (1100, 4), (2100, 6), (2600, 7)]
WINDOWS = ((0, 7), (7, 60), (60, 130))
# (n, seed) -> (stop reason, plain_iter_p1, ret) of ADMM_lp_iters(0, 20000) on the oracle in ORDER_EIGEN, unit values: both stop rules
# (1: y1/y2 convergence, ret 0; 2: the objective's standard deviation, ret 1), three stopping points, G = 1 and 2
OWN_STOPS = {(300, 0): (1, 4818, 0), (300, 1): (2, 3190, 1), (513, 2): (2, 4658, 1)}
# odd_instance(n, RandomState(11)) drawn in this order: live counts 2 ... 9 take every short branch of the redux, the left-over pair and
# the odd element; 511 / 513 sit beside the rank chunk, 1025 / 1027 beside the walker's tile of 1024, 2049 needs three tiles
ODD_NS = (2, 3, 4, 5, 6, 7, 9, 511, 513, 1025, 1027, 2049)
ODD_WINDOWS = ((0, 7), (7, 60))
# n -> (outer_total, pcg_total) of the odd members that stop by rule 1 inside the second window; every other member runs all 60
ODD_STOPS = {None: {2: (41, 45), 3: (33, 72)}, "set": {2: (50, 80)}}
SCALARS = ("rho1", "rho4", "gamma", "dI", "cur_obj", "cvg1", "cvg2", "obj_val", "sum_fix_obj", "best_bin_obj")
VECS = ("x", "z1", "z2", "z4", "pd")
TWIN_SCALARS = SCALARS + ("std_obj", "outer_total", "pcg_total", "iter", "stop", "ret", "plain_iter_p1", "last_pcg")


def with_vals(P, family):
    """A copy of P with stored values: "set" draws from {0.25, 0.5, 1, 2, -1, 3.5}, "uniform" from [0.25, 4] (RandomState(7))."""
    if family is None:
        return P
    rs = np.random.RandomState(7)
    nnz = len(P["rowidx"])
    vals = FAMILY[rs.randint(0, len(FAMILY), nnz)] if family == "set" else rs.uniform(0.25, 4.0, nnz)
    return dict(P, vals=vals)


def odd_instance(n, rs):
    """Empty rows in the middle, one-entry columns, l != n."""
    l = max(2, int(n * rs.uniform(0.3, 0.9)))
    if l == n:
        l = n + 1
    cols = []
    for j in range(n):
        k = 1 if j % 3 == 0 else int(rs.randint(1, min(l, 5) + 1))
        cols.append(sorted(set(rs.choice(l, size=k, replace=False).tolist())))
    dead = set(rs.choice(l, size=max(1, l // 5), replace=False).tolist()) - {l - 1}
    cols = [[r for r in c if r not in dead] or [l - 1] for c in cols]
    colptr = np.zeros(n + 1, np.int32)
    colptr[1:] = np.cumsum([len(c) for c in cols])
    rowidx = np.array([r for c in cols for r in c], np.int32)
    return dict(n=n, l=l, colptr=colptr, rowidx=rowidx, b=-rs.uniform(1, 500, n))


@functools.lru_cache(None)
def _odd_units():
    rs = np.random.RandomState(11)
    return {n: odd_instance(n, rs) for n in ODD_NS}


@functools.lru_cache(None)
def problem(key, family=None):
    """key: (n, seed) -> make_auction_like(n, seed); ("odd", n) -> the odd instance of n variables.  family: see with_vals."""
    if key[0] == "odd":
        return with_vals(_odd_units()[key[1]], family)
    from lpbox_hip.synth import make_auction_like
    return with_vals(make_auction_like(*key), family)


def eigen_oracle(P):
    o = O.LpOracle(0, order=O.ORDER_EIGEN)
    o.set_problem(P["n"], P["l"], P["colptr"], P["rowidx"], P["b"], P.get("f"), P.get("vals"))
    o.solve_init()
    return o


def snapshot(o, ret):
    s = dict(ret=ret, outer_total=o.total_outer_iters, pcg_total=o.total_pcg_iters, trace=tuple(int(k) for k in o.pcg_trace()),
             stop=o.last_stop_reason, plain_iter_p1=o.last_plain_iter_plus1, std_obj=o.scalar("std_obj"),
             pow_sqrt_mismatch=o.scalar("pow_sqrt_mismatch"), rho4Et=o.scalar("rho4Et"))
    for name in VECS:
        v = o.vec(name)
        v.setflags(write=False)
        s[name] = v
    for name in SCALARS:
        s[name] = o.scalar(name)
    return s


@functools.lru_cache(None)
def oracle_windows(key, family=None, windows=WINDOWS):
    """One snapshot per window of consecutive plain windows on a fresh oracle in ORDER_EIGEN."""
    o = eigen_oracle(problem(key, family))
    return tuple(snapshot(o, o.solve_iter(a, b)) for (a, b) in windows)


@functools.lru_cache(None)
def oracle_solve(key, family=None):
    """ADMM_lp_iters(0, 20000): the snapshot plus the binary solution and the objective."""
    o = eigen_oracle(problem(key, family))
    s = snapshot(o, o.solve_iter(0, 20000))
    s["x_sol"] = o.get_x_sol().ravel()
    s["obj"] = o.cal_Obj()
    return s


@functools.lru_cache(None)
def default_order_x(key, windows=WINDOWS):
    """x after every window on the oracle in the kernels' own order: what a batch that silently ran the default order would give."""
    P = problem(key)
    o = O.LpOracle(0, order=O.ORDER_GPU, T=T, chunk=CHUNK)
    o.set_problem(P["n"], P["l"], P["colptr"], P["rowidx"], P["b"])
    o.solve_init()
    out = []
    for (a, b) in windows:
        o.solve_iter(a, b)
        out.append(o.vec("x"))
    return tuple(out)


def compare(g, s, tag, unit=True):
    """Handle `g` (a BigLp; plain windows: every variable is live) against an oracle snapshot: bit for bit, except std_obj within 2 ulp
    where the oracle's pow_sqrt_mismatch counter moved (the kernel takes sqrt where the reference calls pow(v, 1/2))."""
    from helpers import bits_equal
    for name in VECS:
        gv = g.vec(name)
        assert bits_equal(gv, s[name]), f"{tag}: {name} differs (max abs {np.abs(gv - s[name]).max():.3e})"
    assert (g.scalar("outer_total"), g.scalar("pcg_total")) == (s["outer_total"], s["pcg_total"]), tag
    for name in SCALARS + (("rho4Et",) if unit else ()):
        assert bits_equal([g.scalar(name)], [s[name]]), f"{tag}: scalar {name}"
    a, e = g.scalar("std_obj"), s["std_obj"]
    if s["pow_sqrt_mismatch"] > 0:
        assert abs(a - e) <= 2 * np.spacing(abs(e)), f"{tag}: std_obj {a!r} vs {e!r}"
    else:
        assert bits_equal([a], [e]), f"{tag}: std_obj"


def same_as_twin(g, t, tag, valued=False):
    """Handle `g` against a handle that ran the same windows alone: everything, std_obj included, bit for bit."""
    from helpers import bits_equal
    for name in VECS + (("r4v", "vals") if valued else ()):
        assert bits_equal(g.vec(name), t.vec(name)), f"{tag}: {name} (twin)"
    for name in TWIN_SCALARS + (() if valued else ("rho4Et",)):
        assert bits_equal([g.scalar(name)], [t.scalar(name)]), f"{tag}: {name} (twin)"


def want_r4v(vals, iter_end):
    """rho4_E_transpose, entry by entry: rho4_0 * val, scaled in place once per rho update that an iteration has consumed."""
    want = 25.0 * np.asarray(vals, np.float64)
    for _ in range((iter_end - 1) // 25):
        want = LEARNING_FACT * want
    return want
