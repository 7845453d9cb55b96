"""CPU tests of the reference summation order of the segmentation flavour (lpbox_seg_set_order, PyLPboxADMMsolver.set_order): what
answers without a device -- the exported symbol, the call-order and bad-mode codes, the refusal of a mixed batch, the Python argument
checks -- and, from the oracle alone, the facts tests/test_seg_ref_order_gpu.py relies on (tests/seg_ref_cases.py)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import seg_ref_cases as S
from chain_cases import expected_resumes
from helpers import banded_seg_problem, bits_equal
from oracle import oracle as O

E_BADARG, E_STATE, E_UNSUPPORTED = -2, -3, -7
ORDER_DEFAULT, ORDER_REFERENCE = 0, 1


def handle(order=None, n=40, seed=0, problem=True):
    from lpbox_hip.seg import PyLPboxADMMsolver
    s = PyLPboxADMMsolver(0, n, seed)
    s.write_files = False
    if order:
        s.set_order(order)
    if problem:
        s.set_problem(banded_seg_problem(n, seed))
    return s


def test_library_exports_and_python_binds_the_symbol():
    from lpbox_hip import _lib, seg
    lib = C.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "lpbox_seg_set_order"), "liblpbox_hip.so does not export lpbox_seg_set_order"
    assert "lpbox_seg_set_order" in _lib.SYMBOLS
    assert hasattr(seg.PyLPboxADMMsolver, "set_order")
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lpbox_hip.h")) as f:
        assert "int lpbox_seg_set_order(lpbox_t *h, int mode);" in f.read()


def test_call_order_and_bad_mode_codes():
    from lpbox_hip import _lib
    L = _lib.load()
    s = handle(problem=False)
    assert s.debug_scalar("order") == ORDER_DEFAULT
    assert L.lpbox_seg_set_order(s._h, 2) == E_BADARG and b"summation order 2" in L.lpbox_last_error()
    assert L.lpbox_seg_set_order(s._h, -1) == E_BADARG
    assert s.debug_scalar("order") == ORDER_DEFAULT                          # a refused call changes nothing
    assert L.lpbox_seg_set_order(s._h, ORDER_REFERENCE) == 0 and s.debug_scalar("order") == ORDER_REFERENCE
    assert L.lpbox_seg_set_order(s._h, ORDER_DEFAULT) == 0 and s.debug_scalar("order") == ORDER_DEFAULT     # and back, while no problem is set
    assert L.lpbox_seg_set_order(s._h, ORDER_REFERENCE) == 0
    s.set_problem(banded_seg_problem(40, 0))
    for mode in (ORDER_DEFAULT, ORDER_REFERENCE):                            # after the problem: too late, whatever the mode
        assert L.lpbox_seg_set_order(s._h, mode) == E_STATE and b"before lpbox_seg_set_image" in L.lpbox_last_error()
    assert L.lpbox_seg_set_order(s._h, 7) == E_BADARG                        # arguments are checked first
    assert s.debug_scalar("order") == ORDER_REFERENCE
    # through set_image as well
    t = handle(problem=False)
    t.set_image(S.image_gray(), 600)
    assert L.lpbox_seg_set_order(t._h, ORDER_REFERENCE) == E_STATE
    # an LP-flavour handle; lpbox_set_order on a segmentation handle keeps its answer
    lp = L.lpbox_create(_lib.FLAVOUR_LP, 1, 0)
    assert lp
    assert L.lpbox_seg_set_order(C.c_void_p(lp), ORDER_REFERENCE) == E_STATE and b"segmentation flavour" in L.lpbox_last_error()
    L.lpbox_destroy(C.c_void_p(lp))
    u = handle(problem=False)
    assert L.lpbox_set_order(u._h, ORDER_REFERENCE) == E_STATE and b"LP flavour" in L.lpbox_last_error()
    assert u.debug_scalar("order") == ORDER_DEFAULT
    assert L.lpbox_seg_set_order(None, ORDER_REFERENCE) < 0


def test_python_argument_checks():
    s = handle(problem=False)
    for bad in ("eigen", "", None, 1, "Reference"):
        with pytest.raises(ValueError):
            s.set_order(bad)
    s.set_order("reference")
    assert s.order == "reference" and s.debug_scalar("order") == ORDER_REFERENCE
    s.set_order("default")
    assert s.order == "default" and s.debug_scalar("order") == ORDER_DEFAULT
    s.set_order("reference")
    s.set_problem(banded_seg_problem(40, 0))
    for late in ("default", "reference"):
        with pytest.raises(RuntimeError):
            s.set_order(late)
    assert s.order == "reference"
    t = handle(problem=False)
    t.set_image(S.image_gray(), 600)
    with pytest.raises(RuntimeError):
        t.set_order("reference")


def test_the_drop_in_module_re_exports_it():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "accelerated-lpbox-admm_amd", "Segmentation", "cython", "src", "lpbox.py")
    spec = importlib.util.spec_from_file_location("seg_drop_in_lpbox", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert hasattr(mod.PyLPboxADMMsolver, "set_order")


def test_a_mixed_batch_is_refused_by_index_without_a_device_call():
    from lpbox_hip import _lib
    from lpbox_hip.lp import LpboxError
    from lpbox_hip.seg import SegBatch, solve_batch
    L = _lib.load()
    d0, d1, r0, r1 = handle(None, 40, 0), handle(None, 48, 1), handle("reference", 40, 2), handle("reference", 48, 3)
    for members, idx, what in (([d0, d1, r0], 2, "reference summation order; the batch runs the default order"),
                               ([r0, d0, r1], 1, "default order; the batch runs the reference summation order")):
        with pytest.raises(LpboxError, match=f"problem {idx} of the batch runs in the {what}") as e:
            SegBatch(members)
        assert e.value.code == E_UNSUPPORTED
        with pytest.raises(LpboxError, match=f"problem {idx} of the batch runs in the {what}") as e:
            solve_batch(members)
        assert e.value.code == E_UNSUPPORTED
        with pytest.raises(LpboxError, match="solve_init has not been called"):      # nobody was flagged initialised by the refused call
            members[0].solve_iter_l2f(0, 10, np.zeros(members[0].get_org_n()), 0)
    SegBatch([r0, r1]).close()                                                # one order: accepted, no device call
    SegBatch([d0, d1]).close()
    assert L.lpbox_last_status() in (0, E_STATE, E_UNSUPPORTED)               # (the status of the last refused call stays readable)


# ---- the facts of the GPU file, from the oracle alone ----
@pytest.mark.parametrize("name", S.L2F_CASES)
def test_the_two_oracle_orders_differ_in_window_0_and_the_fixes_leave_the_listed_live_counts(name):
    e, g = S.l2f_reference(name), S.l2f_reference(name, O.ORDER_GPU)
    assert e[0]["x_iters"].shape == g[0]["x_iters"].shape and not bits_equal(e[0]["x_iters"], g[0]["x_iters"])
    assert S.live_counts(e) == S.LIVE[name]
    assert [r["num"] for r in e][0] == 0 and e[0]["n"] == S.problem(name)["n"]
    if name == "lap9":
        assert e[-1]["ret"] == S.LAP9_RET == 1 and e[-1]["n"] == 1 and len(e) == 3
    else:
        assert [r["ret"] for r in e] == [0] * S.WINDOWS


def test_storage_and_row_widths_of_the_cases():
    widths = {n: int(np.diff(S.problem(n)["rowptr"]).max()) for n in S.L2F_CASES}
    assert widths["lap600"] == 9 and widths["lap1029"] == 64 and widths["lap9"] == 4 and widths["syn0"] == 7 and widths["band1025"] == 7
    for n in ("lap600", "lap1029", "lap9"):                                   # non-integer weights and costs
        P = S.problem(n)
        assert np.any(P["vals"] != np.round(P["vals"])) and np.any(P["b"] != np.round(P["b"]))


def test_the_two_live_case():
    r = S.two_live_reference()
    assert [x["n"] for x in r] == [9, 2] and r[1]["num"] == 7 and r[1]["ret"] == 0 and len(r[1]["trace"]) == 10


def test_pow_and_sqrt_disagree_at_2921():
    if not S.pow_differs_from_sqrt():
        pytest.skip("this libm's pow(2921, 0.5) equals sqrt(2921): the c1 case cannot tell the two apart here")
    assert math.pow(2921.0, 0.5) != math.sqrt(2921.0)
    r = S.c1_reference()
    assert [x["n"] for x in r] == [S.C1_N, S.C1_LIVE] and r[1]["num"] == 79 and r[1]["ret"] == 0


def test_pcg_counts_of_the_resume_case():
    r = S.resume_reference()
    trace = r[0]["trace"] + r[1]["trace"]
    assert len(trace) == 20 and trace[:3] == S.RESUME_TRACE_HEAD and min(trace) > 4      # every iteration outruns kmax = 1 and 4
    assert (expected_resumes(trace, 1), expected_resumes(trace, 4)) == S.RESUME_COUNTS


def test_degenerate_cases_take_their_branches_in_the_eigen_order_too():
    import degenerate_cases as D
    for name in S.DEGENERATE:
        r = S.degenerate_reference(name)[0]
        assert (r["ret"], r["trace"]) == D.SEG_WINDOW_PINS[name], name
    z = S.problem("deg:zero_td")
    i = D.ZERO_TD_ROWS[1]
    k = z["rowptr"][i] + int(np.nonzero(z["colidx"][z["rowptr"][i]:z["rowptr"][i + 1]] == i)[0][0])
    assert z["vals"][k] == -5.0


def test_legacy_solves_end_quickly_and_differ_between_the_orders_somewhere():
    differ = 0
    for name in S.L2F_CASES:
        e, g = S.legacy_reference(name), S.legacy_reference(name, O.ORDER_GPU)
        assert e["stop"][0] in (1, 2) and e["counters"][0] < 1000
        differ += not bits_equal(e["vecs"]["x"], g["vecs"]["x"])
    assert differ > 0
    assert S.legacy_reference("lap600")["obj"] != round(S.legacy_reference("lap600")["obj"])        # get_obj sums non-integers there
