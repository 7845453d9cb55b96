"""GPU tests of the generic constrained BQP (lpbox_hip.bqp, the reference's ADMM_bqp) at the sizes and shapes where its kernels could
go wrong: n below a workgroup and around the multiples of 256 and 512, m = 1, l = 1, more rows than variables, empty rows and
columns in C and E, A diagonal-only or with off-diagonals of both signs, an indefinite operator, all four presets, and the
four-slot path above 2^21 variables.  Each case is bit-exact against oracle/bqp_oracle.c in the kernels' order and within B of the
numpy restatement oracle/bqp_numpy.py over the prefix where the PCG counts agree (tests/test_oracle_restatement.py states the rule)."""
import numpy as np
import pytest

from helpers import BQP_SCALARS, BQP_VECS, assert_within_bound, bits_equal, bqp_params, bqp_problem, common_prefix
from oracle import oracle as O
from oracle.bqp_numpy import NumpyBqp

pytestmark = pytest.mark.gpu


def hip(P, params):
    from lpbox_hip.bqp import BqpSolver
    g = BqpSolver(P["n"], P["A"], P["b"], P["x0"], P.get("C"), P.get("d"), P.get("E"), P.get("f"), params=params)
    return g, g.solve()


def oracle(P, params, g=None):
    if g is None:
        return O.BqpOracle(P, params=params)
    return O.BqpOracle(P, params=params, order=O.ORDER_GPU, T=int(g.scalar("threads")), chunk=int(g.scalar("chunk")))


def names(P):
    return [v for v in BQP_VECS if v not in ("z3",) or P.get("C") is not None
            if v not in ("z4", "y3") or P.get("E") is not None]


def bit_exact(g, it_g, o, it_o, P, tag):
    assert it_g == it_o and g.scalar("stop") == o.scalar("stop") and g.scalar("total_pcg") == o.scalar("total_pcg"), tag
    for name in names(P):
        assert bits_equal(g.vec(name), o.vec(name)), f"{tag} {name}: max diff {np.abs(g.vec(name) - o.vec(name)).max():.3e}"
    for name in BQP_SCALARS:
        assert g.scalar(name) == o.scalar(name), f"{tag} {name}"


def check_case(P, ptype, K, min_prefix):
    """K iterations bit-exact against the oracle; then the HIP state after the agreeing prefix within B of the restatement."""
    params = bqp_params(ptype, K)
    g, it_g = hip(P, params)
    o = oracle(P, params, g)
    bit_exact(g, it_g, o, o.solve(), P, f"n={P['n']} K={K}")
    r = NumpyBqp(P, params=params)
    r.solve(record=True)
    e = oracle(P, params)
    e.solve()
    k = common_prefix(o.pcg_trace(), e.pcg_trace(), r.pcg)
    assert k >= min_prefix, f"n={P['n']}: PCG counts agree over {k} iterations only: {list(o.pcg_trace())} vs {r.pcg}"
    prm = list(params)
    prm[5] = k
    g, it_g = hip(P, prm)
    o, e = oracle(P, prm, g), oracle(P, prm)
    it_o = o.solve()
    e.solve()
    bit_exact(g, it_g, o, it_o, P, f"n={P['n']} k={k}")
    snap = r.trace[k - 1]
    for name in names(P):
        assert_within_bound(g.vec(name), snap[name], e.vec(name), o.vec(name), f"n={P['n']} k={k} {name}")
    for name in BQP_SCALARS:
        assert_within_bound(g.scalar(name), snap[name], e.scalar(name), o.scalar(name), f"n={P['n']} k={k} {name}")
    return g, r, k


@pytest.mark.parametrize("n", [2, 3, 255, 256, 257, 511, 512, 513])
def test_sizes_around_a_workgroup(n):
    m, l = max(1, n // 12), max(1, n // 9)
    P = bqp_problem(n, m, l, seed=n)
    g, r, k = check_case(P, 3, 8, 4)
    assert (g.n, g.m, g.l) == (n, m, l)


@pytest.mark.parametrize("n,m,l", [(257, 1, 0), (257, 0, 1), (257, 1, 1), (256, 0, 300), (200, 20, 260)])
def test_single_rows_and_more_rows_than_variables(n, m, l):
    P = bqp_problem(n, m, l, seed=7 * n + m + l)
    ptype = (1 if m else 0) | (2 if l else 0)
    g, r, k = check_case(P, ptype, 8, 4)
    assert (g.m, g.l) == (m, l) and (l <= n or g.l > g.n)


def test_empty_rows_and_columns_and_unrolled_row_lengths():
    P = bqp_problem(300, 40, 50, seed=5)
    for key in ("C", "E"):
        rp, ci = P[key][0], P[key][1]
        lens = np.diff(rp)
        assert lens[0] == 0 and {1, 2, 3} <= set(lens % 4)                     # an empty row, lengths 1, 2, 3 mod 4
        assert 299 not in set(ci) and np.any(P[key][2] < 0) and np.any(np.abs(P[key][2]) != 1)
    check_case(P, 3, 8, 4)


@pytest.mark.parametrize("offdiag", [False, True])
@pytest.mark.parametrize("ptype", [0, 1, 2, 3])
def test_presets_with_diagonal_and_general_A(ptype, offdiag):
    """Each *_init preset's hyper-parameters (SEGcpp:587-672) on a problem of its type, A diagonal-only or with off-diagonals of both signs."""
    m, l = (0, 25, 0, 15)[ptype], (0, 0, 25, 20)[ptype]
    P = bqp_problem(400, m, l, seed=90 + ptype, offdiag=offdiag)
    off = P["A"][1] != np.repeat(np.arange(400), np.diff(P["A"][0]))
    assert off.any() == offdiag and (not offdiag or (np.any(P["A"][2][off] < 0) and np.any(P["A"][2][off] > 0)))
    check_case(P, ptype, 8, 4)


def test_indefinite_operator_first_iterations():
    """2A + (rho1 + rho2) I indefinite at the starting rho (checked on the restatement: p.Mp < 0 in the first outer iteration)."""
    P = bqp_problem(150, 15, 0, 60, indefinite=True)
    r0 = NumpyBqp(P, params=bqp_params(1, 3))
    r0.solve(record=True)
    assert r0.min_curvature[0] < 0
    g, r, k = check_case(P, 1, 3, 2)
    assert np.isfinite(g.vec("x")).all()


def test_above_2_pow_21_variables_takes_four_slots():
    """n just above 2,097,152: the gen kernels go to 4 slots per thread (chunk 1024); two iterations against the oracle only."""
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
    params = bqp_params(0, 2)
    g, it_g = hip(P, params)
    assert g.scalar("chunk") == 1024 and g.scalar("threads") == 256
    o = oracle(P, params, g)
    bit_exact(g, it_g, o, o.solve(), P, "n > 2^21")
    assert it_g == 2 and g.scalar("total_pcg") > 0
