"""Shared by tests/test_oracle_lp_valued.py and tests/test_lp_valued_gpu.py: stored values for the committed 0/1 patterns, and the oracle
with values (helpers.make_oracle passes none)."""
import numpy as np

from oracle import oracle as O

FAMILIES = ("set", "uniform", "signed")


def draw_values(nnz, family, seed):
    """One value per stored entry: `set` = {0.5, 1, 1.25, 2, 3}, `uniform` = U[0.25, 4], `signed` = {-1, 0.5, 1, 2}."""
    rs = np.random.RandomState(1000 + seed)
    if family == "set":
        return rs.choice([0.5, 1.0, 1.25, 2.0, 3.0], size=nnz)
    if family == "uniform":
        return rs.uniform(0.25, 4.0, nnz)
    if family == "signed":
        return rs.choice([-1.0, 0.5, 1.0, 2.0], size=nnz)
    raise ValueError(family)


def valued(I, family, seed=0):
    return dict(I, vals=draw_values(len(I["rowidx"]), family, seed))


def valued_oracle(I, init=True):
    """The specification: the oracle in the reference's Eigen order, with the instance's values."""
    s = O.LpOracle(0, order=O.ORDER_EIGEN)
    s.set_problem(I["n"], I["l"], I["colptr"], I["rowidx"], I["b"], I.get("f"), I.get("vals"))
    if init:
        s.solve_init()
    return s


def edge_instance(n, seed):
    """A small valued instance with l != n that holds an empty row (l - 3), a one-entry row (l - 2), a long row (l - 1, every third
    column), an explicit zero, and 1e-3 next to 1e3 in one row."""
    rs = np.random.RandomState(seed)
    l = max(4, int(0.6 * n) + 2)
    if l == n:
        l += 1
    cols = []
    for j in range(n):
        k = 1 + int(rs.randint(0, min(3, l - 3)))
        c = sorted(set(rs.choice(l - 3, size=k, replace=False).tolist()))
        if j == 0:
            c.append(l - 2)
        if j % 3 == 0:
            c.append(l - 1)
        cols.append(c)
    colptr = np.zeros(n + 1, np.int32)
    colptr[1:] = np.cumsum([len(c) for c in cols])
    rowidx = np.array([r for c in cols for r in c], np.int32)
    vals = rs.uniform(0.25, 4.0, len(rowidx)) * np.where(rs.rand(len(rowidx)) < 0.2, -1.0, 1.0)
    pair = []
    for r in (l - 1, 0):                                       # 1e-3 and 1e3 in one row: the long row where it has two entries, else row 0
        at = np.where(rowidx == r)[0]
        if len(at) >= 2:
            pair = [int(at[0]), int(at[1])]
            vals[pair[0]], vals[pair[1]] = 1e-3, 1e3
            break
    zero = max(k for k in range(len(vals)) if k not in pair)   # an explicit zero: the last entry that is not one of that pair
    vals[zero] = 0.0
    return dict(n=n, l=l, colptr=colptr, rowidx=rowidx, b=-rs.uniform(1, 500, n), vals=vals)


def oracle_full_valued(I):
    """Worker (CPU): one valued instance solved to the stop or the 20 000 cap by the Eigen-order oracle."""
    s = valued_oracle(I)
    ret = s.solve_iter(0, 20000)
    return (ret, s.total_outer_iters, s.total_pcg_iters, s.last_stop_reason, s.vec("x"), s.get_x_sol().ravel(), s.cal_Obj(),
            s.check_infeasible_lpbox(), s.check_infeasible_l2f())
