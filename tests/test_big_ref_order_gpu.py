"""The large-instance LP path in the reference's summation order (lpbox_big_set_order), with and without stored
values of E: bit for bit against the oracle in ORDER_EIGEN -- iterates, duals, pd, the scalars and counters that
test_big_gpu_parity.py compares, return codes and x_iters.  The one tolerated deviation is the documented one of section 18: the std
stop test takes sqrt where the reference calls pow(v, 1/2) (std_obj within 2 ulp where the oracle's mismatch counter moved)."""
import os

import numpy as np
import pytest

from helpers import bits_equal, lp_instances, scripted_fix_vec
from oracle import oracle as O

pytestmark = pytest.mark.gpu

LEARNING_FACT = 1 + 1.0 / 100
FAMILY = np.array([0.25, 0.5, 1.0, 2.0, -1.0, 3.5])


def with_vals(P, family):
    """A copy of P with stored values: "set" draws from {0.25, 0.5, 1, 2, -1, 3.5}, "uniform" from [0.25, 4] (RandomState(7))."""
    if family is None:
        return P
    rs = np.random.RandomState(7)
    nnz = len(P["rowidx"])
    vals = FAMILY[rs.randint(0, len(FAMILY), nnz)] if family == "set" else rs.uniform(0.25, 4.0, nnz)
    return dict(P, vals=vals)


def eigen_oracle(P):
    o = O.LpOracle(0, order=O.ORDER_EIGEN)
    o.set_problem(P["n"], P["l"], P["colptr"], P["rowidx"], P["b"], P.get("f"), P.get("vals"))
    o.solve_init()
    return o


def ref_big(P):
    from lpbox_hip.big import BigLp
    g = BigLp(P, order="reference")
    g.solve_init()
    assert g.scalar("order") == 1.0 and int(g.scalar("row_slices")) == 1 and g.scalar("folded_reductions") == 0.0
    return g


def compare(g, o, tag, unit=True):
    left = o.vec("left_idx").astype(int)
    for name in ("x", "z1", "z2", "z4", "pd"):
        gv, ov = g.vec(name), o.vec(name)
        if name != "z4" and len(ov) == len(left):     # the device keeps the original order; the oracle compacts
            gv = gv[left]
        assert bits_equal(gv, ov), f"{tag}: {name} differs (max abs {np.abs(gv - ov).max():.3e})"
    assert (g.scalar("outer_total"), g.scalar("pcg_total")) == (o.total_outer_iters, o.total_pcg_iters), tag
    for name in ("rho1", "rho4", "gamma", "dI", "cur_obj", "cvg1", "cvg2", "obj_val", "sum_fix_obj", "best_bin_obj") + (("rho4Et",) if unit else ()):
        assert bits_equal([g.scalar(name)], [o.scalar(name)]), f"{tag}: scalar {name}"
    a, e = g.scalar("std_obj"), o.scalar("std_obj")
    if o.scalar("pow_sqrt_mismatch") > 0:
        assert abs(a - e) <= 2 * np.spacing(abs(e)), f"{tag}: std_obj {a!r} vs {e!r}"
    else:
        assert bits_equal([a], [e]), f"{tag}: std_obj"


def plain_windows(P, windows, tag):
    g, o = ref_big(P), eigen_oracle(P)
    for (a, b) in windows:
        rg, ro = g.solve_iter(a, b), o.solve_iter(a, b)
        assert rg == ro, f"{tag} [{a},{b})"
        compare(g, o, f"{tag} [{a},{b})", unit="vals" not in P)
        if "vals" in P and o.last_stop_reason == 0:
            # rho4_E_transpose, entry by entry: rho4_0 * val, scaled in place once per rho update that an iteration has consumed
            want = 25.0 * np.asarray(P["vals"], np.float64)
            for _ in range((b - 1) // 25):
                want = LEARNING_FACT * want
            assert bits_equal(g.vec("r4v"), want), f"{tag} [{a},{b}): rho4_E_transpose"
            assert bits_equal(g.vec("vals"), P["vals"])
    return g, o


def l2f_windows(P, ws, nwin, tag, lo=0.02, hi=0.98):
    """l2f windows with the scripted policy after each, against the oracle's real compaction.  Returns the live counts seen."""
    g, o = ref_big(P), eigen_oracle(P)
    vec, num, seen = np.zeros(P["n"]), 0, []
    for w in range(nwin):
        rg, ro = g.solve_iter_l2f(w * ws, (w + 1) * ws, vec, num), o.solve_iter_l2f(w * ws, (w + 1) * ws, vec, num)
        t = f"{tag} window {w}"
        assert rg == ro, t
        assert g.get_n() == o.get_n() and int(g.scalar("iter")) == o.get_iter(), t
        seen.append(g.get_n())
        assert g.cal_Obj() == o.cal_Obj(), t
        xg, xo = g.get_x_iters_2d(ws), o.get_x_iters_2d(ws)
        assert bits_equal(xg, xo), f"{t}: x_iters"
        assert g._L.lpbox_big_check_infeasible(g._h, 0) == o.check_infeasible_lpbox(), t
        assert g._L.lpbox_big_check_infeasible(g._h, 1) == o.check_infeasible_l2f(), t
        assert np.array_equal(g.local_x_sol(), o.get_x_sol().ravel()), t
        if o.get_n() == 0 or rg:
            break
        compare(g, o, t, unit="vals" not in P)
        assert bits_equal(g.vec("f"), o.vec("f")), t
        vec, num = scripted_fix_vec(xo, lo=lo, hi=hi)
    return seen


@pytest.fixture(scope="module")
def auction3000():
    from lpbox_hip.synth import make_auction_like
    return make_auction_like(3000, 1)


def test_unit_windows(auction3000):
    plain_windows(auction3000, ((0, 7), (7, 60), (60, 130)), "unit n=3000")


@pytest.mark.parametrize("family", ["set", "uniform"])
def test_valued_windows(auction3000, family):
    plain_windows(with_vals(auction3000, family), ((0, 7), (7, 60), (60, 130)), f"valued({family}) n=3000")


@pytest.mark.parametrize("family", [None, "set"])
def test_fixes_against_the_oracles_compaction(auction3000, family):
    seen = l2f_windows(with_vals(auction3000, family), 50, 3, f"fixes({family})")
    assert seen[-1] < seen[0], "the scripted policy never fixed anything: the re-ranking is not exercised"
    if family:
        assert seen[1] < seen[0] // 2, "the valued case is expected to fix more than half of the variables at the first fix"


def odd_instance(n, rs):
    """The generator of tests/test_lp_ref_order_gpu.py: empty rows in the middle, one-entry columns, l != n."""
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


@pytest.mark.parametrize("family", [None, "set"])
def test_every_redux_branch_and_the_chunk_edges(family):
    """Live counts 2..9 reached directly (every short branch of the redux, the left-over pair and the odd element); 511, 513 and 1025
    sit either side of the rank kernel's chunk and of the walker's tile of 1024."""
    rs = np.random.RandomState(11)
    insts = [with_vals(odd_instance(n, rs), family) for n in (2, 3, 4, 5, 6, 7, 9, 511, 513, 1025)]
    assert all(P["n"] != P["l"] and np.any(np.diff(P["colptr"]) == 1) for P in insts)            # one-entry columns everywhere
    assert all(len(set(P["rowidx"].tolist())) < P["l"] for P in insts if P["n"] > 9)             # empty rows in the larger ones
    seen = {P["n"]: l2f_windows(P, 50, 2, f"odd n={P['n']} ({family})") for P in insts}
    # what the scripted fix leaves (the oracle alone gives the same counts): the redux after a fix runs over 1, 2 and 3 live variables
    # too, and over counts that are 1, 2 and 3 modulo 4
    want = ({2: [2], 3: [3], 4: [4, 2], 5: [5, 2], 6: [6, 2], 7: [7, 3], 9: [9, 2], 511: [511, 199], 513: [513, 214], 1025: [1025, 430]}
            if family is None else
            {2: [2], 3: [3, 1], 4: [4, 1], 5: [5, 1], 6: [6, 2], 7: [7, 2], 9: [9, 3], 511: [511, 200], 513: [513, 205], 1025: [1025, 411]})
    assert seen == want


def test_nine_variables_fixed_down_to_three():
    from lpbox_hip.synth import make_auction_like
    seen = l2f_windows(with_vals(make_auction_like(9, 0), "set"), 50, 2, "n=9 valued")
    assert seen == [9, 3]


@pytest.mark.parametrize("family", [None, "set"])
def test_two_routes_one_answer(family):
    """A headline instance through the on-chip reference-order kernel and through the large-instance route: the same bits."""
    from lpbox_hip.lp import LpBatch
    I = with_vals(lp_instances("lp_100_500_seed0.npz")[4], family)
    B = LpBatch([I], order="reference")
    B.solve_init()
    g = ref_big(I)
    vec, num, fixed = np.zeros(I["n"]), 0, 0
    for w in range(3):
        rb = B.solve_iter_l2f(50 * w, 50 * (w + 1), vec[None, :], np.array([num], np.int32))
        rg = g.solve_iter_l2f(50 * w, 50 * (w + 1), vec, num)
        assert int(rb[0]) == rg
        xb, xg = B.get_x_iters_2d(50, 0), g.get_x_iters_2d(50)
        assert bits_equal(xb, xg), w
        live = g.vec("live") != 0
        for name in ("x", "z1", "z2", "pd"):
            assert bits_equal(B.debug_vec(name, 0)[: I["n"]][live], g.vec(name)[live]), (w, name)
        assert bits_equal(B.debug_vec("z4", 0)[: I["l"]], g.vec("z4")), w
        assert B.counters(0) == (int(g.scalar("outer_total")), int(g.scalar("pcg_total")))
        assert B.cal_obj(0) == g.cal_Obj() and B.get_n(0) == g.get_n()
        if rg:
            break
        vec, num = scripted_fix_vec(xg, lo=0.05, hi=0.95)
        fixed += num
        vec = np.concatenate([vec, -np.ones(I["n"] - len(vec))])
    assert fixed > 0


def _dropin_check(s, P):
    assert s.solve_init() == 1
    assert s.large
    o = eigen_oracle(P)
    rg, ro = s.solve_iter(0, 20000), o.solve_iter(0, 20000)
    assert rg == ro
    assert s.batch.stop(0) == (o.last_stop_reason, o.last_plain_iter_plus1)
    assert s.batch.counters(0) == (o.total_outer_iters, o.total_pcg_iters)
    assert s.cal_Obj() == o.cal_Obj()
    assert np.array_equal(s.get_x_sol().ravel(), o.get_x_sol().ravel())
    assert s.check_infeasible_l2f() == o.check_infeasible_l2f()


def test_dropin_unit_instance_beyond_the_on_chip_limit():
    from lpbox_hip.lp import PyLPboxADMMsolver
    P = odd_instance(2100, np.random.RandomState(3))
    s = PyLPboxADMMsolver(0)
    s.set_order("reference", large_ok=True)
    s.set_problem(P["n"], P["l"], P["colptr"], P["rowidx"], P["b"])
    _dropin_check(s, P)


def test_dropin_valued_instance_files(tmp_path):
    from lpbox_hip.lp import PyLPboxADMMsolver
    # the instance of the refusal test with ONE stored value of 2.0: the VALUED kernels run, and the solve reaches its stop after a few
    # hundred iterations (with every value drawn, the plain solve of this instance runs to the 20 000 cap: 11 s on the oracle alone)
    P = odd_instance(2100, np.random.RandomState(3))
    vals = np.ones(len(P["rowidx"]))
    vals[len(vals) // 2] = 2.0
    P = dict(P, vals=vals)
    d = tmp_path / "instance" / "1000_2100"
    os.makedirs(d)
    with open(d / "instance_1_C.txt", "w") as fh:               # the reference's row,col,val triplets, 1-based (LPcpp:2416-2444)
        for j in range(P["n"]):
            for k in range(P["colptr"][j], P["colptr"][j + 1]):
                fh.write("%d,%d,%r\n" % (P["rowidx"][k] + 1, j + 1, float(P["vals"][k])))
    with open(d / "instance_1_b.txt", "w") as fh:               # the reader negates b (LPcpp:2520)
        for v in P["b"]:
            fh.write("%r\n" % float(-v))
    s = PyLPboxADMMsolver(0)
    s.data_root = str(tmp_path)
    s.write_files = False
    s.set_order("reference", large_ok=True)
    s.read_File(1, 1000, 2100)
    _dropin_check(s, P)


def test_boundary_and_default_order_unchanged(auction3000):
    from lpbox_hip._lib import LpboxError
    from lpbox_hip.big import BigLp
    from lpbox_hip.lp import LpBatch
    P = auction3000
    # stored values on a default-order handle: refused, the message names the missing call
    with pytest.raises(LpboxError) as e:
        BigLp(with_vals(P, "set"))
    assert e.value.code == -7 and "lpbox_big_set_order" in str(e.value)
    # all-ones values are a unit instance, in either order
    BigLp(dict(P, vals=np.ones(len(P["rowidx"])))).close()
    # a non-finite value
    bad = with_vals(P, "set")
    bad["vals"] = bad["vals"].copy()
    bad["vals"][5] = np.inf
    with pytest.raises(LpboxError) as e:
        BigLp(bad, order="reference")
    assert e.value.code == -2
    # the comm-lean PCG (world != 1, the callback transport and both call orders: tests/test_big_ref_order_api.py, which needs no device;
    # a communicator created first: test_communicator_first below)
    with pytest.raises(LpboxError) as e:
        BigLp(P, order="reference", pcg_mode="lean")
    assert e.value.code == -7
    # too late: after the problem
    g = BigLp(P)
    with pytest.raises(LpboxError) as e:
        from lpbox_hip._lib import check
        check(g._L.lpbox_big_set_order(g._h, 1), "lpbox_big_set_order")
    assert e.value.code == -3
    # LpBatch keeps refusing an instance beyond the on-chip limit
    big = odd_instance(2100, np.random.RandomState(3))
    B = LpBatch([big], order="reference")
    with pytest.raises(LpboxError) as e:
        B.solve_init()
    assert e.value.code == -9
    # the default order in the same process still equals the oracle in the kernels' own order
    g.solve_init()
    assert g.scalar("order") == 0.0
    o = O.LpOracle(0, order=O.ORDER_GPU, T=int(g.scalar("threads")), chunk=int(g.scalar("chunk")))
    o.set_problem(P["n"], P["l"], P["colptr"], P["rowidx"], P["b"])
    o.solve_init()
    assert g.solve_iter(0, 40) == o.solve_iter(0, 40)
    for name in ("x", "z1", "z2", "z4"):
        assert bits_equal(g.vec(name), o.vec(name)), name
    assert (g.scalar("outer_total"), g.scalar("pcg_total")) == (o.total_outer_iters, o.total_pcg_iters)


def test_communicator_first():
    """lpbox_big_rccl_init (a one-rank communicator) and then lpbox_big_set_order: refused, the handle stays in the default order."""
    import ctypes as C
    from lpbox_hip import _lib
    L = _lib.load()
    h = C.c_void_p(L.lpbox_big_create(0, 1, 0))
    uid = (C.c_ubyte * 128)()
    assert L.lpbox_big_rccl_unique_id(uid) == 128
    assert L.lpbox_big_rccl_init(h, uid) == 0
    assert L.lpbox_big_set_order(h, 1) == -7 and b"transport" in L.lpbox_last_error()
    v = C.c_double(-1.0)
    assert L.lpbox_big_get_scalar(h, b"order", C.byref(v)) == 0 and v.value == 0.0
    L.lpbox_big_destroy(h)
