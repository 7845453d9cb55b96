"""CPU tests of the boundary for constraint matrices with stored values: the reference order accepts them, the
default order keeps refusing them, the handle gives them back bit for bit, and the file reader leaves what the oracle's reader leaves.
Host logic only: no call here needs a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from helpers import GOLDEN, bits_equal, lp_instances
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def some_values(I, seed=0):
    return np.random.RandomState(seed).choice([0.5, 1.0, 1.25, 2.0, 3.0, -1.0], size=len(I["rowidx"]))


def set_valued(b, I, vals, idx=0):
    b.set_problem(idx, I["n"], I["l"], I["colptr"], I["rowidx"], I["b"], vals=vals)


def test_default_order_still_refuses_and_says_which_call_is_missing():
    from lpbox_hip.lp import LpBatch, LpboxError
    I = lp_instances("lp_20_60_seed0.npz")[0]
    b = LpBatch(batch=1)
    with pytest.raises(LpboxError, match="!= 1") as e:
        set_valued(b, I, 2 * np.ones(len(I["rowidx"])))
    assert e.value.code == -7                                  # LPBOX_E_UNSUPPORTED
    assert "lpbox_set_order(LPBOX_ORDER_REFERENCE)" in str(e.value)


def test_reference_order_accepts_values_and_cannot_go_back():
    from lpbox_hip.lp import LpBatch, LpboxError
    I = lp_instances("lp_20_60_seed0.npz")[0]
    b = LpBatch(batch=2)
    b.set_order("reference")
    vals = some_values(I)
    vals[3], vals[5], vals[7] = 0.0, -2.5, 1e-300             # zeros, negative and tiny values are values like any other
    set_valued(b, I, vals)
    with pytest.raises(LpboxError) as e:
        b.set_order("default")
    assert e.value.code == -7
    # the constructor sets the order before the instances and passes vals through
    c = LpBatch([dict(I, vals=vals)], order="reference")
    assert c.order == "reference"
    assert bits_equal(c.get_problem(0)["vals"], vals)
    with pytest.raises(LpboxError, match="!= 1"):
        LpBatch([dict(I, vals=vals)])


def test_non_finite_value_is_a_bad_argument():
    from lpbox_hip.lp import LpBatch, LpboxError
    I = lp_instances("lp_20_60_seed0.npz")[0]
    for order in ("reference", "default"):
        for bad in (np.nan, np.inf, -np.inf):
            b = LpBatch(batch=1, order=order)
            vals = np.ones(len(I["rowidx"]))
            vals[-1] = bad
            with pytest.raises(LpboxError) as e:
                set_valued(b, I, vals)
            assert e.value.code == -2, (order, bad)            # LPBOX_E_BADARG


def test_non_finite_objective_entry_is_a_bad_argument(tmp_path):
    """b is checked on the host like vals: NaN and either infinity are refused with the index, before any device
    call, by lpbox_set_problem_lp and by both file readers; a subnormal, a zero and 1e300 are values like any other."""
    from lpbox_hip.lp import LpBatch, LpboxError
    I = lp_instances("lp_20_60_seed0.npz")[0]
    pc, pb, _, _, _ = oracle_read(3)
    price = np.loadtxt(pb)
    d = tmp_path / "instance" / "3_7"
    d.mkdir(parents=True)
    (d / "instance_1_C.txt").write_text(open(pc).read())
    for order in ("default", "reference"):
        for bad in (np.nan, np.inf, -np.inf):
            b = LpBatch(batch=1, order=order)
            v = I["b"].copy()
            v[17] = bad
            with pytest.raises(LpboxError, match=r"index 17\b") as e:
                b.set_problem(0, I["n"], I["l"], I["colptr"], I["rowidx"], v)
            assert e.value.code == -2, (order, bad)            # LPBOX_E_BADARG
            b.set_problem(0, I["n"], I["l"], I["colptr"], I["rowidx"], I["b"])         # the refused call left the handle usable
            p = price.copy()
            p[2] = bad
            (d / "instance_1_b.txt").write_text("".join("%r\n" % float(x) for x in p))
            b = LpBatch(batch=1, order="reference")            # the fixture stores values other than 1
            for call in (lambda: b.read_files(0, pc, str(d / "instance_1_b.txt"), 3), lambda: b.read_file(0, 1, 3, 7, str(tmp_path))):
                with pytest.raises(LpboxError, match=r"index 2\b") as e:
                    call()
                assert e.value.code == -2, (order, bad)
        b = LpBatch(batch=1, order=order)
        v = I["b"].copy()
        v[:6] = [5e-324, -1e-310, 0.0, -0.0, 1e300, -1e300]
        b.set_problem(0, I["n"], I["l"], I["colptr"], I["rowidx"], v)
        assert bits_equal(b.get_problem(0)["b"], v)
    p = price.copy()
    p[:4] = [1e-310, 0.0, 1e300, 5e-324]
    (d / "instance_1_b.txt").write_text("".join("%r\n" % float(x) for x in p))
    b = LpBatch(batch=1, order="reference")
    b.read_file(0, 1, 3, 7, str(tmp_path))
    assert bits_equal(b.get_problem(0)["b"], -p)


def test_all_ones_is_a_unit_instance():
    from lpbox_hip.lp import LpBatch
    I = lp_instances("lp_20_60_seed0.npz")[0]
    ones = np.ones(len(I["rowidx"]))
    b = LpBatch(batch=1, order="reference")
    set_valued(b, I, ones)
    assert "vals" not in b.get_problem(0)
    b.set_order("default")                                     # nothing valued in the handle: allowed
    d = LpBatch(batch=1)
    set_valued(d, I, ones)                                     # and the default order takes explicit ones, as before
    out = np.zeros(len(ones))
    assert d._L.lpbox_get_problem_lp_vals(d._h, 0, out.ctypes.data_as(ctypes.c_void_p)) == len(ones)
    assert bits_equal(out, ones)
    # a valued instance replaced by a unit one leaves a unit handle
    e = LpBatch(batch=1, order="reference")
    set_valued(e, I, some_values(I))
    set_valued(e, I, ones)
    e.set_order("default")


def test_values_round_trip_bitwise():
    from lpbox_hip.lp import LpBatch
    insts = lp_instances("lp_20_60_seed0.npz")[:3]
    b = LpBatch(batch=3, order="reference")
    want = []
    for i, I in enumerate(insts):
        v = np.random.RandomState(i).uniform(0.25, 4.0, len(I["rowidx"])) * np.where(np.arange(len(I["rowidx"])) % 5 == 0, -1.0, 1.0)
        v[0] = -0.0
        want.append(v)
        set_valued(b, I, v, i)
    for i, I in enumerate(insts):
        P = b.get_problem(i)
        assert np.array_equal(P["colptr"], I["colptr"]) and np.array_equal(P["rowidx"], I["rowidx"])
        assert bits_equal(P["vals"], want[i])
        assert b._L.lpbox_get_problem_lp_vals(b._h, i, None) == len(I["rowidx"])      # NULL only asks for the count
    assert b._L.lpbox_get_problem_lp_vals(b._h, 3, None) == -2
    assert b._L.lpbox_get_problem_lp_vals(None, 0, None) == -1


def oracle_read(k):
    """What the oracle's reader leaves (readSparseMat, LPcpp:2416-2444): the CSC arrays of E with its values."""
    d = os.path.join(GOLDEN, "instance", "%d_7" % k)
    pc, pb = os.path.join(d, "instance_1_C.txt"), os.path.join(d, "instance_1_b.txt")
    trips = [ln.strip().split(",") for ln in open(pc) if ln.strip()]
    r = np.array([int(t[0]) - 1 for t in trips]); c = np.array([int(t[1]) - 1 for t in trips])
    v = np.array([float(t[2]) for t in trips]) * (-1.0 if k == 2 else 1.0)
    return pc, pb, r, c, v


@pytest.mark.parametrize("k", [2, 3])
def test_read_file_leaves_what_the_oracle_reader_leaves(k):
    """Fixture tests/golden/instance/<k>_7 (make_valued_fixture.py): values other than 1, duplicate triplets, one cancelling pair.
    The handle must hold the arrays that setFromTriplets leaves (per column, rows ascending, duplicates added in file order), restated
    below.  The oracle has no getter for its matrix, so that the restatement IS what LpOracle.read_files leaves is shown through the
    oracle's arithmetic, bit for bit: fixing column j alone to 1 leaves f - E[:, j] (LPcpp:1276-1278), the first iteration leaves
    pd_j = (rho1 + rho2) + rho4 * sum of val^2 down column j (:2378-2391) and y3 = max(0, f - E x0)."""
    from lpbox_hip.lp import LpBatch, LpboxError, PyLPboxADMMsolver
    pc, pb, r, c, v = oracle_read(k)
    n, l = c.max() + 1, r.max() + 1
    assert n != l
    # setFromTriplets: per column, rows ascending, duplicates summed in file order
    colptr, rowidx, vals = [0], [], []
    for j in range(n):
        at = np.where(c == j)[0]
        at = at[np.argsort(r[at], kind="stable")]
        for q, t in enumerate(at):
            if q and r[t] == r[at[q - 1]]:
                vals[-1] = vals[-1] + v[t]
            else:
                rowidx.append(r[t]); vals.append(v[t])
        colptr.append(len(rowidx))
    vals = np.array(vals)
    assert np.any(vals == 0.0) and len(rowidx) < len(r) - 1, "the fixture must hold duplicates and a cancelling pair"
    assert np.any((vals != 1.0) & (vals != -1.0) & (vals != 0.0))
    # the oracle's reader agrees with this restatement
    def fresh():
        o = O.LpOracle(0, order=O.ORDER_EIGEN)
        o.read_files(pc, pb, k)
        o.solve_init()
        return o
    o = fresh()
    assert o.get_org_n() == n and o.L.lpo_get_l(o.h) == l
    o.solve_iter_l2f(0, 1, np.zeros(n), 0)                    # x0 = ones, z4 = 0, rho = 25
    ex, pd = np.zeros(l), np.zeros(n)
    for j in range(n):                                         # the order of Eigen's column-major product
        e = 0.0
        for q in range(colptr[j], colptr[j + 1]):
            ex[rowidx[q]] += vals[q] * 1.0
            e += vals[q] * vals[q]
        pd[j] = (0.0 + (25.0 + 25.0)) + 25.0 * e
    y3 = 1.0 - ex - 0.0 / 25.0
    assert bits_equal(o.vec("y3"), np.where(y3 < 0, 0.0, y3))
    assert bits_equal(o.vec("pd"), pd)
    for j in range(n):
        o = fresh()
        vec = -np.ones(n); vec[j] = 1.0
        o.solve_iter_l2f(0, 0, vec, 1)
        col = np.zeros(l)
        col[rowidx[colptr[j]:colptr[j + 1]]] = 0.0 + vals[colptr[j]:colptr[j + 1]] * 1.0
        assert bits_equal(o.vec("f"), 1.0 - col), f"column {j}"
    # the handle, through both file entry points
    for how in ("read_file", "read_files", "dropin"):
        if how == "dropin":
            s = PyLPboxADMMsolver(0)
            s.data_root = GOLDEN
            with pytest.raises(LpboxError, match="!= 1") as e:
                s.read_File(1, k, 7)
            assert "lpbox_set_order" in str(e.value)         # the error names the missing call
            s.set_order("reference")
            s.read_File(1, k, 7)
            P = s.batch.get_problem(0)
        else:
            b = LpBatch(batch=1, order="reference")
            if how == "read_file":
                b.read_file(0, 1, k, 7, GOLDEN)
            else:
                b.read_files(0, pc, pb, k)
            P = b.get_problem(0)
        assert (P["n"], P["l"]) == (n, l)
        assert np.array_equal(P["colptr"], colptr) and np.array_equal(P["rowidx"], rowidx)
        assert bits_equal(P["vals"], vals), how
        assert bits_equal(P["b"], -np.loadtxt(pb))


def test_header_declares_and_library_exports_the_getter():
    txt = open(os.path.join(ROOT, "include", "lpbox_hip.h")).read()
    assert re.search(r"^int\s+lpbox_get_problem_lp_vals\s*\(\s*lpbox_t\s*\*\s*h\s*,\s*int\s+idx\s*,\s*double\s*\*\s*vals\s*\)\s*;", txt, re.M)
    from lpbox_hip import _lib
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "lpbox_get_problem_lp_vals")
    assert "lpbox_get_problem_lp_vals" in _lib.SYMBOLS
