"""Pins the yardstick of the valued LP kernels independently: the C oracle in Eigen order with stored values against the numpy
restatement (oracle/lpbox_numpy.py) given the same values (vals=) -- it computes Esq_diag and every product from the stored entries.  The restatement sums in numpy's own order, so agreement is to rounding: over the iterations before the first differing
PCG count, |dx| <= 1e-3 max(1, |x|inf), the PCG's own exit tolerance.  (Where the very first x-update already stops one PCG iteration
apart -- the two residuals straddle the exit test -- there is no such prefix and the draw pins nothing; each draw prints its prefix.)  CPU only; passes with or without the valued kernels."""
import numpy as np
import pytest

from helpers import common_prefix, lp_instances
from oracle.lpbox_numpy import NumpyLpBox
from valued_cases import FAMILIES, valued, valued_oracle

ITERS = 40


def restatement(I):
    s = NumpyLpBox(I["n"], I["l"], I["colptr"], I["rowidx"], I["b"], vals=I["vals"])
    s.solve_init()
    return s


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_valued_eigen_oracle_agrees_with_restatement(family, seed):
    I = valued(lp_instances("lp_100_500_seed0.npz")[0], family, seed)
    o, s = valued_oracle(I), restatement(I)
    ro = o.solve_iter_l2f(0, ITERS, np.zeros(I["n"]), 0)
    rs = s.solve_iter_l2f(0, ITERS, np.zeros(I["n"]), 0)
    xo, xs = o.get_x_iters_2d(ITERS), s.x_iters[:, :ITERS]
    k = common_prefix(o.pcg_trace(), s.pcg_trace)
    worst = max(np.abs(xo[:, c] - xs[:, c]).max() / max(1.0, np.abs(xs[:, c]).max()) for c in range(k)) if k else 0.0
    first = np.abs(xo[:, 0] - xs[:, 0]).max() / max(1.0, np.abs(xs[:, 0]).max())
    print(f"{family} seed {seed}: common PCG prefix {k} of {ITERS}, first iterate {first:.3e}, worst {worst:.3e}")
    for c in range(k):
        assert np.abs(xo[:, c] - xs[:, c]).max() <= 1e-3 * max(1.0, np.abs(xs[:, c]).max()), f"iteration {c}"
    if k == ITERS:
        assert ro == rs


@pytest.mark.parametrize("family", FAMILIES)
def test_preconditioner_diagonal_is_dI_plus_rho4_sum_of_squares(family):
    I = valued(lp_instances("lp_100_500_seed0.npz")[0], family, 0)
    o = valued_oracle(I)
    o.solve_iter_l2f(0, 1, np.zeros(I["n"]), 0)
    v = I["vals"]
    esq = np.zeros(I["n"])
    for j in range(I["n"]):                                    # down the column, one rounded square at a time (numpy's sum would pair them up)
        for q in range(I["colptr"][j], I["colptr"][j + 1]):
            esq[j] = esq[j] + v[q] * v[q]
    want = (25.0 + 25.0) + 25.0 * esq
    assert np.all(np.abs(o.vec("pd") - want) <= np.spacing(want))
