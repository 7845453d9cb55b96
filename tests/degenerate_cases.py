"""Degenerate scalar branches and out-of-range data for the segmentation (lpbox_seg_*) and generic BQP (lpbox_gen_*, lpbox_gen_ref_*,
lpbox_genb_*) kernels.  Shared by tests/test_degenerate_cases.py (CPU: the branch conditions asserted from the data, the outcomes pinned
on both oracle orders and the restatement) and tests/test_degenerate_gpu.py (the kernels, bit for bit against the oracle).  DESIGN.md
section 26 holds the branch table B1-B7 the docstrings refer to.  Pure numpy: every case is named and deterministic, no GPU, nothing read
from outside the repository."""
import functools

import numpy as np

from helpers import banded_seg_problem, bqp_params, bqp_problem

DBL_MIN = float(np.finfo(np.float64).tiny)
TINY_SCALES = {"1e-150": 1e-150, "1e-153": 1e-153, "1e-160": 1e-160, "1e-310": 1e-310, "0": 0.0}
ROWS = {0: (0, 0), 1: (25, 0), 2: (0, 25), 3: (15, 20)}          # (m, l) of the four problem types, as test_presets_... has them
SMALL = (2, 3, 257)                                               # below a wave, and one past a workgroup
K = 8                                                             # outer iterations of a BQP case unless it says otherwise


def _rows(ptype, n):
    m, l = ROWS[ptype]
    return (min(m, 1), min(l, 1)) if n < 10 else (m, l)


def _base(ptype, n, seed):
    m, l = _rows(ptype, n)
    return bqp_problem(n, m, l, seed=seed)


def _scale_A(P, s):
    Q = dict(P)
    Q["A"] = (P["A"][0], P["A"][1], np.asarray(P["A"][2], np.float64) * s)
    return Q


def empty_columns(P):
    """Columns that neither C nor E stores an entry in (their Csq / Esq is zero, so the preconditioner diagonal there is A's alone)."""
    used = np.zeros(P["n"], bool)
    for key in ("C", "E"):
        if P.get(key) is not None:
            used[np.asarray(P[key][1])] = True
    return np.nonzero(~used)[0]


def zero_precond_rows(P):
    """The rows zero_precond_diag works on: the first, the middle and the last column that C and E leave empty."""
    free = empty_columns(P)
    return np.unique(free[[0, len(free) // 2, -1]])


# ------------------------------------------------------------------------------------------------
# generic BQP
# ------------------------------------------------------------------------------------------------
def _bqp_zero_rhs(ptype, n):
    """B1 (rhsNorm2 == 0: no PCG iteration, x = 0) in both outer iterations, then B4 (norm(x) = 0 under the stop test's quotient).
    Unconstrained: x0 = 1 and b = 2 initial_rho, so y1 = y2 = 1 and rho1 y1 + rho2 y2 - b = 0.  Constrained: x0 = 0, b = 0, d = 0,
    f >= 0, so y1 = y2 = 0, y3 = f and every term of the right-hand side vanishes."""
    P = _base(ptype, n, 700 + 10 * ptype + n)
    prm = bqp_params(ptype, K)
    if ptype == 0:
        P["x0"] = np.ones(n)
        P["b"] = np.full(n, 2.0 * prm[6])
    else:
        P["x0"] = np.zeros(n)
        P["b"] = np.zeros(n)
        if "d" in P:
            P["d"] = np.zeros(len(P["d"]))
        if "f" in P:
            P["f"] = np.abs(np.asarray(P["f"], np.float64))
    return P, prm


def _bqp_tiny_b(n, scale):
    """x0 = 0 and b of order `scale`: rhs = -b.  1e-150: an ordinary PCG.  1e-153: tol^2 rhs^2 < DBL_MIN <= rhs^2, the clamp B3.
    1e-160: rhs^2 itself is subnormal or zero (B1 / B2 with the clamp).  1e-310 and 0: rhs^2 == 0 (B1).  Then B4: x = 0."""
    P = bqp_problem(300, seed=3) if n == 300 else bqp_problem(n, seed=3 + n)
    P["x0"] = np.zeros(n)
    P["b"] = np.asarray(P["b"], np.float64) * scale
    return P, bqp_params(0, K)


def _bqp_scaled(ptype, what, s):
    """b or A multiplied by s (A as a whole, so its diagonal stays dominant and the PCG short): the ordinary path on data that is not
    of order 1."""
    P = _base(ptype, 120, 720 + ptype)
    if what == "b":
        P["b"] = np.asarray(P["b"], np.float64) * s
    else:
        P = _scale_A(P, s)
    return P, bqp_params(ptype, K)


def _bqp_zero_precond_diag(ptype):
    """B5: a stored diagonal of -initial_rho on three rows whose columns in C and E are empty, so that 2 a_ii + rho1 + rho2 == 0 there
    at the first preconditioner build: dinv = 1 instead of 1 / 0."""
    P = _base(ptype, 120, 740 + ptype)
    prm = bqp_params(ptype, K)
    rp, ci, va = P["A"]
    va = np.array(va, np.float64)
    for i in zero_precond_rows(P):
        k = rp[i] + int(np.nonzero(ci[rp[i]:rp[i + 1]] == i)[0][0])
        va[k] = -float(prm[6])
    P["A"] = (rp, ci, va)
    return P, prm


def _bqp_centre_start(ptype):
    """B6: x0 = 0.5 everywhere, so the sphere projection divides by 2 sqrt(0): y2 is NaN, every PCG exit test is false and the PCG runs
    to pcg_maxiters.  ALWAYS with max_iters = 2 and pcg_maxiters = 30 (the presets would make it 10^7 PCG iterations)."""
    P = _base(ptype, 120, 760 + ptype)
    P["x0"] = np.full(120, 0.5)
    prm = bqp_params(ptype, 2)
    prm[10] = 30
    return P, prm


def _bqp_table():
    t = {}
    for ptype in range(4):
        for n in (120,) + SMALL:
            t[f"zero_rhs-t{ptype}-n{n}"] = functools.partial(_bqp_zero_rhs, ptype, n)
        for what, s in (("b", 1e-6), ("b", 1e6), ("A", 1e-6), ("A", 1e3)):
            t[f"scaled-{what}x{s:g}-t{ptype}"] = functools.partial(_bqp_scaled, ptype, what, s)
        t[f"zero_precond_diag-t{ptype}"] = functools.partial(_bqp_zero_precond_diag, ptype)
        t[f"centre_start-t{ptype}"] = functools.partial(_bqp_centre_start, ptype)
    for n in (300,) + SMALL:
        for tag, s in TINY_SCALES.items():
            t[f"tiny_b-x{tag}-n{n}"] = functools.partial(_bqp_tiny_b, n, s)
    return t


_BQP = _bqp_table()
BQP_NAMES = tuple(_BQP)


@functools.lru_cache(maxsize=None)
def bqp_case(name):
    """(P, params) of a named BQP case (shared: do not modify)."""
    P, prm = _BQP[name]()
    for key in ("b", "x0", "d", "f"):
        if key in P:
            P[key] = np.ascontiguousarray(P[key], np.float64)
            assert np.all(np.isfinite(P[key]))
    return P, list(prm)


def bqp_ptype(P):
    return (1 if P.get("C") is not None else 0) | (2 if P.get("E") is not None else 0)


# What the oracle does on each BQP case, the same in ORDER_EIGEN, in ORDER_GPU (T = 256, chunk = 512) and on the restatement:
# name -> (iterations returned, stop reason, PCG counts).  Stop reasons: 0 = the cap, 1 = residual, 2 = obj_std.  Every case is
# listed.
#   zero_rhs, unconstrained: x = 0 after iteration 0, y1 = y2 = 0 and rhs = 0 again in iteration 1, which stops on the residual test.
#   At n = 2 the sphere projection of x0 = 1 is one ulp off 1 (sqrt(2) is rounded): iteration 0 still takes B1, iteration 1 does not.
#   zero_rhs, constrained: x = y1 = y2 = 0 at once, the residual test stops iteration 0.
BQP_PINS = {f"zero_rhs-t0-n{n}": (1, 1, (0, 0)) for n in (120, 3, 257)}
BQP_PINS["zero_rhs-t0-n2"] = (6, 1, (0, 2, 2, 2, 2, 2, 0))
BQP_PINS.update({f"zero_rhs-t{t}-n{n}": (0, 1, (0,)) for t in (1, 2, 3) for n in (120,) + SMALL})
BQP_PINS.update({f"centre_start-t{t}": (2, 0, (30, 30)) for t in range(4)})
TINY_PCG = {(300, "1e-150"): 4, (300, "1e-153"): 3, (2, "1e-150"): 2, (2, "1e-153"): 1, (3, "1e-150"): 3, (3, "1e-153"): 2,
            (257, "1e-150"): 4, (257, "1e-153"): 3}
BQP_PINS.update({f"tiny_b-x{tag}-n{n}": (0, 1, (TINY_PCG.get((n, tag), 0),)) for n in (300,) + SMALL for tag in TINY_SCALES})
BQP_PINS.update({
    "zero_precond_diag-t0": (8, 0, (9, 10, 10, 12, 12, 12, 6, 6)), "zero_precond_diag-t1": (8, 0, (16, 16, 16, 20, 20, 20, 15, 15)),
    "zero_precond_diag-t2": (8, 0, (21, 23, 23, 14, 14, 14, 13, 13)), "zero_precond_diag-t3": (8, 0, (25, 27, 27, 15, 15, 15, 14, 14)),
    "scaled-bx1e-06-t0": (8, 0, (4, 3, 3, 3, 4, 4, 4, 4)), "scaled-bx1e+06-t0": (8, 0, (4,) * 8),
    "scaled-Ax1e-06-t0": (8, 0, (1,) * 8), "scaled-Ax1000-t0": (8, 0, (12,) + (7,) * 7),
    "scaled-bx1e-06-t1": (8, 0, (9, 8, 8, 7, 7, 7, 7, 6)), "scaled-bx1e+06-t1": (8, 0, (9, 9, 8, 8, 8, 8, 8, 8)),
    "scaled-Ax1e-06-t1": (8, 0, (12, 11, 11, 11, 10, 9, 9, 9)), "scaled-Ax1000-t1": (8, 0, (15,) + (9,) * 7),
    "scaled-bx1e-06-t2": (8, 0, (10,) * 5 + (9,) * 3), "scaled-bx1e+06-t2": (8, 0, (11, 12, 11, 12, 11, 11, 11, 11)),
    "scaled-Ax1e-06-t2": (8, 0, (10,) * 4 + (9,) * 4), "scaled-Ax1000-t2": (8, 0, (12,) + (9,) * 7),
    "scaled-bx1e-06-t3": (8, 0, (10,) * 8), "scaled-bx1e+06-t3": (8, 0, (12,) * 8),
    "scaled-Ax1e-06-t3": (8, 0, (11,) * 3 + (10,) * 5), "scaled-Ax1000-t3": (8, 0, (12, 9) + (8,) * 6),
})


# ------------------------------------------------------------------------------------------------
# segmentation
# ------------------------------------------------------------------------------------------------
def seg_from_pairs(n, M, b, diag=None):
    """P for set_problem from a dict (i, j) -> stored off-diagonal value of A (i < j, mirrored), the diagonal = minus the row sum of the
    off-diagonals unless `diag` (index -> value) overrides a row."""
    rows = [dict() for _ in range(n)]
    for (i, j), v in M.items():
        rows[i][j] = v
        rows[j][i] = v
    rp, ci, va = [0], [], []
    for i in range(n):
        rows[i][i] = -sum(rows[i].values()) + 0.0
        if diag and i in diag:
            rows[i][i] = diag[i]
        for j in sorted(rows[i]):
            ci.append(j); va.append(rows[i][j])
        rp.append(len(ci))
    return dict(n=n, rowptr=np.array(rp, np.int32), colidx=np.array(ci, np.int32), vals=np.array(va, np.float64),
                b=np.ascontiguousarray(b, np.float64), c=0.0, rows=1, cols=n)


SEG_B_SCALES = {"0": 0.0, "1e-310": 1e-310, "1e-160": 1e-160, "1e-155": 1e-155, "1e-153": 1e-153, "1e-150": 1e-150, "1e-6": 1e-6, "1e6": 1e6}
SEG_FULL_SOLVE = ("0", "1e-310", "1e-160", "1e-155", "1e-153", "1e-150")        # the b scalings whose legacy solve ends within a few iterations


def _seg_b_scaled(s):
    """banded_seg_problem(600, 5) with b x s (rhs = -b in iteration 0; sum(b^2) = 3.0e5 s^2).  0, 1e-310: rhs^2 == 0 (B1).  1e-160:
    rhs^2 is subnormal, the threshold is the clamp (B3) and the first residual lies below it (B2).  1e-155: tol^2 rhs^2 < DBL_MIN <= rhs^2,
    the clamp B3 with a PCG that runs.  1e-153, 1e-150: tiny, but the ordinary threshold.  Up to here norm(x) stays below the floor B4 and
    the solve stops in iteration 0.  1e-6, 1e6: the ordinary path; at 1e6 the energy does not fit an int."""
    P = banded_seg_problem(600, 5)
    return dict(P, b=np.asarray(P["b"], np.float64) * s)


def _seg_weights255(n, offsets, seed):
    """B7: weights drawn from 0..255 on symmetric bands, every band holding a 255, a 128 and a 0 (stored as -0.0): bytes above 5 in
    dpack and in ell_load's eval."""
    rs = np.random.RandomState(seed)
    M = {}
    for o in offsets:
        w = rs.randint(0, 256, max(n - o, 0)).astype(np.float64)
        if len(w) >= 3:
            at = rs.choice(len(w), 3, replace=False)
            w[at] = (255.0, 128.0, 0.0)
        else:
            w[:] = 255.0
        for i in range(n - o):
            M[(i, i + o)] = -w[i]
    return seg_from_pairs(n, M, rs.randint(-40, 40, n).astype(np.float64))


BOUNDARY_N = 40
BOUNDARY_AT = (11, 13)                     # the changed entry (and its mirror): offset 2 of banded_seg_problem


def _seg_boundary(value):
    """B7, the predicate of as_diagonals(): a copy of banded_seg_problem(40, 9) with the entry (11, 13) and its mirror set to `value`,
    the two diagonals recomputed as minus the row sums."""
    P = banded_seg_problem(BOUNDARY_N, 9)
    M = {}
    for i in range(P["n"]):
        for k in range(P["rowptr"][i], P["rowptr"][i + 1]):
            j = int(P["colidx"][k])
            if j > i:
                M[(i, j)] = float(P["vals"][k])
    assert BOUNDARY_AT in M
    M[BOUNDARY_AT] = value
    return seg_from_pairs(P["n"], M, P["b"])


def _seg_n1():
    """n = 1: one stored diagonal; ELL by the n >= 2 rule of the upload."""
    return dict(n=1, rowptr=np.array([0, 1], np.int32), colidx=np.array([0], np.int32), vals=np.array([1.0]), b=np.array([-7.0]), c=0.0,
                rows=1, cols=1)


ZERO_TD_ROWS = tuple(range(0, 600, 50))


def _seg_zero_td():
    """B5: the diagonal of A exactly -5 = -rho0 on every 50th row of banded_seg_problem(600, 5): td = 2 a_ii + rho1 + rho2 == 0 there at
    the first preconditioner build."""
    P = banded_seg_problem(600, 5)
    va = np.array(P["vals"], np.float64)
    for i in ZERO_TD_ROWS:
        k = P["rowptr"][i] + int(np.nonzero(P["colidx"][P["rowptr"][i]:P["rowptr"][i + 1]] == i)[0][0])
        va[k] = -5.0
    return dict(P, vals=va)


# name -> (builder, expected storage: True = diagonals, False = ELL)
_SEG = {f"b-x{tag}": (functools.partial(_seg_b_scaled, s), True) for tag, s in SEG_B_SCALES.items()}
_SEG.update({
    "weights255-o123": (functools.partial(_seg_weights255, 600, (1, 2, 3), 21), True),
    "weights255-o1": (functools.partial(_seg_weights255, 300, (1,), 22), True),
    "weights255-o1_37": (functools.partial(_seg_weights255, 300, (1, 37), 23), True),
    "weights255-n2": (functools.partial(_seg_weights255, 2, (1,), 24), True),
    "boundary-m255": (functools.partial(_seg_boundary, -255.0), True),
    "boundary-m256": (functools.partial(_seg_boundary, -256.0), False),
    "boundary-mhalf": (functools.partial(_seg_boundary, -0.5), False),
    "boundary-p1": (functools.partial(_seg_boundary, 1.0), False),
    "boundary-mzero": (functools.partial(_seg_boundary, -0.0), True),
    "boundary-pzero": (functools.partial(_seg_boundary, 0.0), True),
    "boundary-n1": (_seg_n1, False),
    "zero_td": (_seg_zero_td, True),
})
SEG_NAMES = tuple(_SEG)
SEG_FIX_CASES = ("weights255-o123", "zero_td")


@functools.lru_cache(maxsize=None)
def seg_case(name):
    """P of a named segmentation case (shared: do not modify)."""
    P = _SEG[name][0]()
    assert np.all(np.isfinite(P["vals"])) and np.all(np.isfinite(P["b"]))
    return P


def seg_as_diagonals(name):
    return _SEG[name][1]


def seg_fix_vec(x):
    """The scripted fix of the fix-step tests: every third live variable fixed to x >= 0.5.  Returns (vec, num)."""
    x = np.asarray(x, np.float64)
    vec = -np.ones(len(x))
    vec[::3] = (x[::3] >= 0.5).astype(np.float64)
    return vec, int(np.sum(vec != -1))


# What the oracle does in the first l2f window (0, 3) of each case, the same in both orders and on the restatement:
# name -> (ret, PCG counts of the window).
SEG_WINDOW_PINS = {
    "b-x0": (1, (0,)), "b-x1e-310": (1, (0,)), "b-x1e-160": (1, (0,)), "b-x1e-155": (1, (5,)), "b-x1e-153": (1, (9,)), "b-x1e-150": (1, (9,)),
    "b-x1e-6": (0, (9, 8, 8)), "b-x1e6": (0, (9, 8, 7)),
    "weights255-o123": (0, (55, 47, 45)), "weights255-o1": (0, (42, 36, 34)), "weights255-o1_37": (0, (35, 36, 33)),
    "weights255-n2": (0, (2, 1, 1)),
    "boundary-m255": (0, (12, 10, 10)), "boundary-m256": (0, (12, 10, 10)), "boundary-mhalf": (0, (8, 6, 6)), "boundary-p1": (0, (8, 6, 6)),
    "boundary-mzero": (0, (8, 6, 6)), "boundary-pzero": (0, (8, 6, 6)), "boundary-n1": (0, (1, 1, 1)),
    "zero_td": (0, (32, 33, 33)),
}
# The legacy solve of the SEG_FULL_SOLVE cases and of b x 1e6 (124 iterations): name -> (returned int, iterations + 1, stop reason,
# total PCG count).  (b x 1e-6 is no such case: its iteration count depends on the summation order, 715 / 725 / 697.)
SEG_LEGACY_PINS = {"b-x0": (0, 1, 1, 0), "b-x1e-310": (0, 1, 1, 0), "b-x1e-160": (0, 1, 1, 0), "b-x1e-155": (0, 1, 1, 5),
                   "b-x1e-153": (0, 1, 1, 9),
                   "b-x1e-150": (0, 1, 1, 9), "b-x1e6": (-2147483648, 124, 2, 718)}
# The fix step: a first window (0, 5) -- five iterations, so that the rho update of iteration 4 makes the preconditioner due for a rebuild
# at the fix, the only place the reference's own loop can take one (with a stale preconditioner its Eigen sizes disagree) -- then
# seg_fix_vec of the last iterate and the window (5, 8): name -> (variables fixed, ret, PCG counts of (5, 8)).
SEG_FIX_FIRST, SEG_FIX_SECOND = (0, 5), (5, 8)
SEG_FIX_PINS = {"weights255-o123": (200, 0, (7, 6, 5)), "zero_td": (200, 0, (24, 24, 24))}
SEG_1E6_OBJ =-5648997785.0              # get_obj() there: below INT_MIN
# b x 1e6: the energy is below INT_MIN, the returned int is the defined out-of-range value.
SEG_1E6_ENERGY_INT = -2147483648
