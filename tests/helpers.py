"""Shared helpers for the test-suite (oracle = checker, lpbox_hip = product)."""
import os

import numpy as np

from oracle import oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def lp_instances(name):
    return O.load_lp_batch(os.path.join(GOLDEN, name))


def make_oracle(I, order=O.ORDER_EIGEN, T=512, positions=None, npos=0, row_split=None, col_split=None, x_update="pcg", direct_rows=None):
    s = O.LpOracle(0, order=order, T=T, positions=positions, npos=npos, row_split=row_split, col_split=col_split, x_update=x_update,
                   direct_rows=direct_rows)
    s.set_problem(I["n"], I["l"], I["colptr"], I["rowidx"], I["b"], I.get("f"))
    s.solve_init()
    return s


def scripted_fix_vec(xiters, lo=0.02, hi=0.98, last=20):
    """Deterministic stand-in for the trained policy (LP/trainer.py:101-135,216-252): fix a live variable to 1 (0) when
    its last `last` iterates are all > hi (< lo); everything else stays free (-1).  Returns (vec, num)."""
    tail = xiters[:, -last:]
    vec = -np.ones(xiters.shape[0])
    vec[np.all(tail > hi, axis=1)] = 1.0
    vec[np.all(tail < lo, axis=1)] = 0.0
    num = int(np.sum(vec != -1))
    return vec, num


def bits_equal(a, b):
    a = np.ascontiguousarray(a, np.float64)
    b = np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def bits_equal_nan(a, b):
    """bits_equal for data that may hold NaN: a NaN must meet a NaN in the same place, whatever the two NaNs' sign and payload bits (IEEE
    754 leaves both to the implementation, and a compiler may turn a - b into -(b - a), which flips a NaN's sign); every other value is compared by bit pattern, so -0.0 still differs from +0.0."""
    a = np.array(a, np.float64, ndmin=1)
    b = np.array(b, np.float64, ndmin=1)
    a[np.isnan(a)] = np.nan
    b[np.isnan(b)] = np.nan
    return bits_equal(a, b)


def scalar_bits_equal(a, b):
    """Two float64 scalars by the rule of bits_equal_nan: NaN equals NaN, -0.0 differs from +0.0."""
    return bits_equal_nan(np.array([a], np.float64), np.array([b], np.float64))


def oracle_like(g, I):
    """CPU oracle configured with the reduction tree of the HIP solver `g` (threads + storage positions)."""
    return oracle_for(g.batch if hasattr(g, "batch") else g, 0, I)


def oracle_for(batch, idx, I, x_update="pcg", direct_rows=None):
    cfg = batch.config()
    return make_oracle(I, O.ORDER_GPU, cfg["threads"], batch.layout(idx), cfg["threads"] * cfg["elems_per_thread"],
                       batch.row_split(idx), batch.col_split(idx), x_update=x_update, direct_rows=direct_rows)


def oracle_full_solve(args):
    """Worker (CPU): one instance solved to convergence by the oracle in the kernels' association."""
    I, T, npos, pos, rs, cs = args
    s = O.LpOracle(0, order=O.ORDER_GPU, T=T, positions=pos, npos=npos, row_split=rs, col_split=cs)
    s.set_problem(I["n"], I["l"], I["colptr"], I["rowidx"], I["b"])
    s.solve_init()
    ret = s.solve_iter(0, 20000)
    return ret, s.total_outer_iters, s.total_pcg_iters, s.cal_Obj(), s.vec("x"), s.get_x_sol().ravel()



# ------------------------------------------------------------------------------------------------
# The reference's own validation loops (LP/trainer.py:_valid_2, SEG/trainer.py:_my_valid) driven on the CPU oracle:
# adapters with the pyx surface that log every call, and a scripted stand-in for the trained network.
# Shared by tests/golden/make_trainer_fixtures.py (reference loop -> fixture) and tests/test_trainer_pins.py (our loop).
# ------------------------------------------------------------------------------------------------
class CallLog:
    """Per-solver call log, JSON-friendly: what the loop handed to the solver and what it read back."""

    def __init__(self):
        self.solvers = []

    def new_solver(self, tag):
        rec = dict(tag=tag, windows=[], final={})
        self.solvers.append(rec)
        return rec


def _vec_code(vec, n_live):
    return [int(v) for v in np.asarray(vec, np.float64).ravel()[:n_live]]


class LoggedLpSolver:
    """lpbox.PyLPboxADMMsolver (LP pyx:7-76) on oracle/lpbox_oracle.c; `instances` / `log` are set on the class by the caller."""
    instances = None
    log = None

    def __init__(self, print_info=0):
        self._o = O.LpOracle(int(print_info))
        self._rec = None

    def read_File(self, i, k, j):
        I = self.instances[int(i) - 1]                      # instance files are numbered from 1 (LP/trainer.py:502)
        self._o.set_problem(I["n"], I["l"], I["colptr"], I["rowidx"], I["b"])
        self._rec = self.log.new_solver("lp%d" % int(i))

    def solve_init(self):
        return self._o.solve_init()

    def solve_iter_l2f(self, i, j, vec, num):
        n_live = self._o.get_n()
        ret = self._o.solve_iter_l2f(i, j, np.ascontiguousarray(vec, np.float64), num)
        self._rec["windows"].append(dict(start=int(i), end=int(j), num=int(num), vec=_vec_code(vec, n_live) if num else [],
                                         ret=int(ret), n_live=int(self._o.get_n())))
        return ret

    def get_x_iters_2d(self, ws):
        X = self._o.get_x_iters_2d(ws)
        self._rec["windows"][-1]["xiters_shape"] = list(X.shape)
        self._rec["windows"][-1]["xiters_sum"] = float(X.sum())
        return X

    def check_infeasible_l2f(self):
        v = self._o.check_infeasible_l2f()
        self._rec["final"]["infeasible"] = int(v)
        return v

    def cal_Obj(self):
        v = self._o.cal_Obj()
        self._rec["final"]["cal_obj"] = float(v)
        return v

    def get_n(self):
        return self._o.get_n()


def synthetic_seg_problem(problem, rows=24, cols=20):
    """Small smooth-noise grayscale image -> (A, b, c) through the oracle's cost builder (SEGcpp:46-248)."""
    rs = np.random.RandomState(100 + int(problem))
    g = rs.rand(rows + 8, cols + 8)
    k = np.ones((5, 5)) / 25.0
    sm = np.zeros((rows, cols))
    for r in range(rows):
        for c in range(cols):
            sm[r, c] = (g[r:r + 5, c:c + 5] * k).sum()
    sm = (sm - sm.min()) / (sm.max() - sm.min())
    img = np.floor(255 * (0.25 * rs.rand(rows, cols) + 0.75 * sm)).astype(np.float64)
    return O.seg_build_costs(img)


class LoggedSegSolver:
    """lpbox.PyLPboxADMMsolver (SEG pyx:8-53) on oracle/seg_oracle.c; the image of `problem` is synthetic (the reference's
    numNodes = 1e4 is ignored: what is pinned is the loop, not the image pipeline)."""
    log = None

    def __init__(self, print_info, numNodes, problem):
        self._o = O.SegOracle(int(print_info), int(numNodes), int(problem))
        self._o.set_problem(synthetic_seg_problem(problem))
        self._rec = self.log.new_solver("seg%d" % int(problem))

    def solve_init(self):
        return self._o.solve_init()

    def solve_iter_l2f(self, i, j, vec, num):
        n_live = self._o.get_n()
        ret = self._o.solve_iter_l2f(i, j, np.ascontiguousarray(vec, np.float64), num)
        self._rec["windows"].append(dict(start=int(i), end=int(j), num=int(num), vec=_vec_code(vec, n_live) if num else [],
                                         ret=int(ret), n_live=int(self._o.get_n())))
        return ret

    def get_x_iters_2d(self, ws):
        X = self._o.get_x_iters_2d(ws)
        self._rec["windows"][-1]["xiters_shape"] = list(X.shape)
        self._rec["windows"][-1]["xiters_sum"] = float(X.sum())
        return X

    def get_obj(self):
        v = self._o.get_obj()
        self._rec["final"]["obj"] = float(v)
        return v

    def get_x_sol(self):
        x = self._o.get_x_sol()
        self._rec["final"]["x_sol_sum"] = float(x.sum())
        return x

    def get_n(self):
        return self._o.get_n()


def scripted_scores(x, hi=0.985, lo=0.015):
    """Deterministic stand-in for the trained network: x float32 (rows, tokens, width) -> sigmoid-like scores that sit far from
    the 0.9 / 0.1 thresholds: 0.95 where the mean of the LAST token's iterates exceeds `hi`, 0.05 below `lo`, else 0.5."""
    import torch
    x = torch.as_tensor(x, dtype=torch.float32)
    m = x[:, -1, :].mean(dim=1)
    return torch.where(m > hi, 0.95, torch.where(m < lo, 0.05, 0.5)).to(torch.float32)


def oracle_iters_fix(o, i, j, x_prev=None, consistency=5, fix_threshold=1e-3, min_fix=10):
    """ADMM_lp_iters_fix (LPcpp:1689-2286) restated in the reference's OWN order on the oracle's primitives: one iteration, the
    persistence counters (:1857-1871), the stop tests, then the fix AT THE END of the iteration (:1929-2043) -- applied here
    through a zero-length l2f call, i.e. the repaired fix block (see lpbox_hip.lp.PyLPboxADMMsolver.solve_iter_fix).
    Returns (ret, x_prev)."""
    n = o.get_n()
    prev = np.zeros(n) if x_prev is None or len(x_prev) != n else x_prev
    count, flag = np.zeros(n), np.zeros(n, bool)
    ret = 0
    for it in range(i, j):
        r = o.solve_iter_l2f(it, it + 1, np.zeros(n), 0)
        reason = o.last_stop_reason
        if reason in (3, 4) or (r and reason == 0):
            return 1, prev
        x = o.get_x_iters_2d(1)[:, 0]
        for k in range(n):                                   # the reference's loop, element by element
            if abs(x[k] - prev[k]) <= fix_threshold:
                count[k] += 1
                if count[k] >= consistency:
                    flag[k] = True
            else:
                count[k] = 0
        prev = x.copy()
        if reason == 1:
            break
        if reason == 2:
            ret = 1
            break
        fix_n = int(flag.sum())
        if fix_n <= min_fix:
            continue
        vec = np.where(flag, np.where(x >= 0.5, 1.0, 0.0), -1.0)
        r = o.solve_iter_l2f(it + 1, it + 1, vec, fix_n)     # the fix block alone
        keep = ~flag
        prev, count, flag = prev[keep], count[keep], flag[keep]
        n = int(keep.sum())
        if r:
            ret = 1
            break
    return ret, prev


# ------------------------------------------------------------------------------------------------
# Comparisons with the independent numpy restatement (oracle/bqp_numpy.py) and the problems they run on.
# ------------------------------------------------------------------------------------------------
BQP_VECS = ("x", "y1", "y2", "z1", "z2", "best_sol", "z3", "z4", "y3")
BQP_SCALARS = ("rho1", "rho3", "rho4", "gamma", "std_obj", "cvg1", "cvg2", "best_bin_obj", "obj_val", "cur_obj")


def spread_bound(e, g):
    """Tolerance B against the restatement: 10 x the oracle's own Eigen-order vs GPU-order spread, plus 1e-12 max(1, |v|)."""
    e, g = np.atleast_1d(np.asarray(e, float)), np.atleast_1d(np.asarray(g, float))
    return 10 * np.abs(e - g).max(initial=0.0) + 1e-12 * max(1.0, np.abs(e).max(initial=0.0))


# The factor c of the step-locked LP checks (tests/lp_steplock.py): B(v) = c * spread(v) + 1e-12 max(1, |v|), where the spread is that of
# an ensemble of 12 roundings of the restatement itself (no subject enters it).  The same 10 as in spread_bound above.  Calibration on the
# restatement alone (test_lp_steplock.py::test_calibration_of_c): the worst distance of a float64 permuted member from the natural member,
# divided by the spread of the other eleven, is at most 3.2 over all named cases (gen100_0) -- below c / 2, so c stays 10.
STEPLOCK_C = 10
# Instances with stored values are calibrated on their own (test_calibration_of_c_valued, the nine valued cases of test_lp_steplock.py):
# there the worst such ratio is 28.85 (uniform values on gen20_1) -- above 10 / 2, so by the same rule c is twice that value, rounded up.
STEPLOCK_C_VALUED = 60


def assert_within_bound(got, ref, e, g, tag):
    got, ref = np.atleast_1d(np.asarray(got, float)), np.atleast_1d(np.asarray(ref, float))
    assert got.shape == ref.shape, f"{tag}: shape {got.shape} vs {ref.shape}"
    d = np.abs(got - ref).max(initial=0.0)
    B = spread_bound(e, g)
    assert d <= B, f"{tag}: |got - restatement| = {d:.3e} > B = {B:.3e}"


def assert_within_bound_nan(got, ref, e, g, tag):
    """assert_within_bound where the data may hold NaN: an entry that is NaN in `got`, in the restatement AND in both oracle orders counts
    as agreement, a NaN on one side alone is a failure (the rule of tests/lp_steplock.py); the other entries are held to B of their own."""
    got, ref, e, g = (np.atleast_1d(np.asarray(v, float)) for v in (got, ref, e, g))
    assert got.shape == ref.shape == e.shape == g.shape, f"{tag}: shapes {got.shape}, {ref.shape}, {e.shape}, {g.shape}"
    nan = np.isnan(ref)
    for name, v in (("subject", got), ("eigen-order oracle", e), ("kernel-order oracle", g)):
        assert np.array_equal(np.isnan(v), nan), f"{tag}: NaN in other places in the {name} than in the restatement"
    assert_within_bound(got[~nan], ref[~nan], e[~nan], g[~nan], tag)


def common_prefix(*traces):
    k = min(len(t) for t in traces)
    for i in range(k):
        if len({int(t[i]) for t in traces}) != 1:
            return i
    return k


def bqp_params(ptype, K, rho_change_step=3):
    """The type's preset hyper-parameters (bqp_numpy.PRESETS) cut to K iterations, with a shorter rho schedule so that a short
    prefix holds rho / gamma updates."""
    from oracle.bqp_numpy import PRESETS
    p = list(PRESETS[ptype])
    p[4], p[5] = rho_change_step, K
    return p


def _csr_dense(M):
    rp, ci, va = [0], [], []
    for i in range(M.shape[0]):
        nz = np.nonzero(M[i])[0]
        ci += list(nz); va += list(M[i, nz])
        rp.append(len(ci))
    return np.array(rp, np.int32), np.array(ci, np.int32), np.array(va, np.float64)


def _constraint_rows(rows, n, rs, skip_col):
    """rows x n with row lengths 1, 2, 3, ... mod 4 (row 0 empty), non-unit values of both signs, column `skip_col` empty."""
    M = np.zeros((rows, n))
    cols = np.array([j for j in range(n) if j != skip_col]) if n > 1 else np.arange(n)
    for i in range(rows):
        if i == 0 and rows > 1:
            continue
        k = min(len(cols), 1 + (i % 7))
        pick = rs.choice(cols, k, replace=False)
        M[i, pick] = rs.uniform(0.3, 1.7, k) * np.where(rs.rand(k) < 0.25, -1.0, 1.0)
    return M


def bqp_problem(n, m=0, l=0, seed=0, offdiag=True, indefinite=False):
    """A generic constrained BQP for lpbox_hip.bqp / BqpOracle / NumpyBqp: A symmetric with every diagonal stored (off-diagonals of
    both signs, or none), C (m x n) and E (l x n) with an empty row and an empty column once they have more than one row, d = C xb
    and f = E xb + slack for a binary xb (feasible), x0 inside the box.  indefinite: A's diagonal made negative enough that
    2A + (rho1 + rho2) I is indefinite at the starting rho of the eq / both presets."""
    rs = np.random.RandomState(seed)
    A = np.zeros((n, n))
    if offdiag and n > 1:
        for _ in range(2 * n):
            i, j = rs.randint(n), rs.randint(n)
            if i != j:
                v = rs.uniform(-1, 1)
                A[i, j] += v; A[j, i] += v
    dg = np.abs(A).sum(axis=1) + rs.uniform(0.5, 2.0, n)
    if indefinite:
        dg = dg.copy()
        dg[: max(1, n // 8)] = -np.abs(A[: max(1, n // 8)]).sum(axis=1) - 40.0
    A[np.arange(n), np.arange(n)] = dg
    xb = (rs.rand(n) < 0.4).astype(float)
    P = dict(n=n, A=_csr_dense(A), b=rs.uniform(-2, 1, n), x0=rs.uniform(0.2, 0.8, n))
    skip = n - 1
    if m:
        Cm = _constraint_rows(m, n, rs, skip)
        P["C"], P["d"] = _csr_dense(Cm), Cm @ xb
    if l:
        Em = _constraint_rows(l, n, rs, skip)
        P["E"], P["f"] = _csr_dense(Em), Em @ xb + rs.uniform(0.0, 1.0, l)
    # a zero diagonal must still be stored (lpbox_bqp_set_problem): _csr_dense keeps only nonzeros, so put it back
    from lpbox_hip.bqp import with_diagonal
    P["A"] = with_diagonal(*P["A"], n)
    return P


def laplacian_seg_problem(n, width, seed=0):
    """A segmentation-flavour problem P (for PyLPboxADMMsolver.set_problem / SegOracle / NumpySeg) that is no image: A = D - W, a
    weighted graph Laplacian with non-integer weights (so 2A + rho I is positive definite), built on a chain (rows of 3 entries) plus
    hub rows whose extra neighbours are disjoint: the longest row holds exactly `width` entries (width >= 4), every other row at
    most 4.  b: non-integer costs of both signs."""
    rs = np.random.RandomState(seed)
    W = {}
    for i in range(n - 1):
        W[(i, i + 1)] = rs.uniform(0.2, 1.5)
    hubs = max(1, min(4, n // (2 * width)))
    pool = list(rs.permutation([i for i in range(n) if i % (n // hubs) != 0]))
    for h in range(hubs):
        hub = h * (n // hubs)
        have = {hub - 1, hub + 1} & set(range(n))
        extra = width - 1 - len(have)
        for j in [pool.pop() for _ in range(extra)]:
            W[(min(hub, j), max(hub, j))] = W.get((min(hub, j), max(hub, j)), 0.0) + rs.uniform(0.2, 1.5)
    rows = [dict() for _ in range(n)]
    for (i, j), w in W.items():
        rows[i][j] = rows[i].get(j, 0.0) - w
        rows[j][i] = rows[j].get(i, 0.0) - w
    rp, ci, va = [0], [], []
    for i in range(n):
        rows[i][i] = -sum(rows[i].values())
        for j in sorted(rows[i]):
            ci.append(j); va.append(rows[i][j])
        rp.append(len(ci))
    return dict(n=n, rowptr=np.array(rp, np.int32), colidx=np.array(ci, np.int32), vals=np.array(va), b=rs.uniform(-3, 3, n).round(3),
                c=0.0, rows=1, cols=n)


def banded_seg_problem(n, seed=0, fourth_offset=False):
    """Offsets +-1, +-2, +-3 with small integer weights (the shape lpbox_seg holds as diagonals, rows of at most 7 entries); with
    fourth_offset, one more symmetric pair (0, n-1): a fourth distinct offset on each side, so the matrix must stay in ELL."""
    rs = np.random.RandomState(seed)
    M = {}
    for i in range(n):
        for o in (1, 2, 3):
            if i + o < n:
                M[(i, i + o)] = float(rs.randint(0, 6))
    if fourth_offset:
        M[(0, n - 1)] = 2.0
    rows = [dict() for _ in range(n)]
    for (i, j), w in M.items():
        rows[i][j] = -w
        rows[j][i] = -w
    rp, ci, va = [0], [], []
    for i in range(n):
        rows[i][i] = -sum(rows[i].values())
        for j in sorted(rows[i]):
            ci.append(j); va.append(rows[i][j])
        rp.append(len(ci))
    return dict(n=n, rowptr=np.array(rp, np.int32), colidx=np.array(ci, np.int32), vals=np.array(va),
                b=rs.randint(-40, 40, n).astype(float), c=0.0, rows=1, cols=n)


def scaled_seg_problem(P, s):
    """P with every stored value of A multiplied by s (b, c and the shape as they are): 2A + (rho1 + rho2) I is the worse conditioned
    the larger s, so the PCG of an outer iteration runs the longer (tests/test_chain_resume_cases.py pins the counts)."""
    Q = dict(P)
    Q["vals"] = np.asarray(P["vals"], np.float64) * s
    return Q


def synthetic_gray(rows, cols, seed=0):
    """A blocky grayscale image with noise (uint8), fast at any size."""
    rs = np.random.RandomState(seed)
    coarse = rs.rand(rows // 24 + 2, cols // 24 + 2)
    img = np.kron(coarse, np.ones((24, 24)))[:rows, :cols] * 200 + 55 * rs.rand(rows, cols)
    return np.floor(img).astype(np.uint8)
