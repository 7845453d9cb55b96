"""GPU tests of segmentation-kernel branches the other suites never reach: 1, 4 and 8 slots per thread (forced and chosen by the
library for big images), ELL rows of 8, 9, 64 and 255 entries, the ELL fallback of a banded matrix with a fourth offset, the
255-entry limit, and a batched solve mixing diagonal and ELL storage.  Every case is bit-exact against oracle/seg_oracle.c in the
kernels' order and within B of the numpy restatement oracle/bqp_numpy.py (tests/test_oracle_restatement.py states the rule)."""
import os

import numpy as np
import pytest

from helpers import GOLDEN, assert_within_bound, banded_seg_problem, bits_equal, laplacian_seg_problem, synthetic_gray, synthetic_seg_problem
from seg_harness import SCALARS, solver, trio, windows

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("ept", [1, 4, 8])
def test_forced_elements_per_thread(monkeypatch, ept):
    from lpbox_hip.seg import load_gray
    monkeypatch.setenv("LPBOX_SEG_EPT", str(ept))
    g = solver(gray=load_gray(os.path.join(GOLDEN, "seg", "7.jpg")), nodes=10000)
    assert g.config()["elems_per_thread"] == ept and g.debug_scalar("matrix_as_diagonals") == 1.0
    o, e, r = trio(g)
    windows(g, o, e, r, 2, tag=f"EPT {ept}")


def test_image_above_262144_nodes_takes_four_slots_and_fixes():
    gray = synthetic_gray(520, 520, 1)
    g = solver(gray=gray, nodes=gray.size)
    assert g.get_org_n() == 270400 > 262144 and g.config()["elems_per_thread"] == 4
    o, e, r = trio(g)
    assert windows(g, o, e, r, 2, fix_after=0, tag="520x520") > 0


def test_image_above_524288_nodes_takes_eight_slots():
    gray = synthetic_gray(740, 720, 2)
    g = solver(gray=gray, nodes=gray.size)
    assert g.get_org_n() == 532800 > 524288 and g.config()["elems_per_thread"] == 8
    o, e, r = trio(g)
    windows(g, o, e, r, 1, tag="740x720")


@pytest.mark.parametrize("width,n", [(8, 3000), (9, 3000), (64, 4000), (255, 3000)])
def test_generic_laplacian_in_wide_ell(width, n):
    P = laplacian_seg_problem(n, width, seed=width)
    assert np.diff(P["rowptr"]).max() == width
    g = solver(P)
    assert g.debug_scalar("matrix_as_diagonals") == 0.0 and g.debug_scalar("ell_width") == width
    o, e, r = trio(g)
    fixed = windows(g, o, e, r, 3, fix_after=1 if width == 64 else None, tag=f"ELL width {width}")
    assert (fixed > 0) == (width == 64)


def test_banded_matrix_with_a_fourth_offset_stays_in_ell():
    a = solver(banded_seg_problem(3000, 5))
    assert a.debug_scalar("matrix_as_diagonals") == 1.0
    g = solver(banded_seg_problem(3000, 5, fourth_offset=True))
    assert g.debug_scalar("matrix_as_diagonals") == 0.0 and g.debug_scalar("ell_width") == 7
    o, e, r = trio(g)
    windows(g, o, e, r, 2, tag="fourth offset")


def test_row_of_256_entries_is_refused_before_any_launch():
    from lpbox_hip.lp import LpboxError
    from lpbox_hip.seg import PyLPboxADMMsolver
    P = laplacian_seg_problem(1200, 256, seed=3)
    assert np.diff(P["rowptr"]).max() == 256
    g = PyLPboxADMMsolver(0, P["n"], 0)
    g.write_files = False
    g.set_problem(P)
    with pytest.raises(LpboxError, match="at most 255") as ei:
        g.solve_init()
    assert ei.value.code == -7                                  # LPBOX_E_UNSUPPORTED


def test_batched_legacy_mixing_diagonal_and_ell_storage():
    """One lpbox_seg_legacy_batch over a diagonal-stored image, a narrow ELL problem and a wide ELL problem of different n: each equals
    its own single solve bit for bit, the oracle in the kernels' order, and -- the PCG counts agreeing to the end -- the restatement."""
    from lpbox_hip.seg import solve_batch
    probs = [synthetic_seg_problem(4), laplacian_seg_problem(700, 5, 1), laplacian_seg_problem(900, 40, 2)]
    single = [solver(P) for P in probs]
    assert [s.debug_scalar("matrix_as_diagonals") for s in single] == [1.0, 0.0, 0.0]
    assert [s.debug_scalar("ell_width") for s in single][1:] == [5.0, 40.0]
    ref = [(s.solve_iter(), s.get_obj(), s.counters(), s.stop(), s.get_x_sol().copy(), s.debug_vec("x")) for s in single]
    from lpbox_hip.seg import PyLPboxADMMsolver
    batch = []
    for P in probs:
        s = PyLPboxADMMsolver(0, P["n"], 0)
        s.write_files = False
        s.set_problem(P)
        batch.append(s)
    en = solve_batch(batch)
    for k, (s, P) in enumerate(zip(batch, probs)):
        assert en[k] == ref[k][0] and s.get_obj() == ref[k][1] and s.counters() == ref[k][2] and s.stop() == ref[k][3], k
        assert np.array_equal(s.get_x_sol(), ref[k][4]) and bits_equal(s.debug_vec("x"), ref[k][5]), k
        o, e, r = trio(single[k])
        eo, ee, er = o.solve_iter(), e.solve_iter(), r.solve_iter()
        assert en[k] == eo and s.counters() == (o.total_outer_iters, o.total_pcg_iters) and s.stop() == (o.last_stop, o.legacy_iter_plus1)
        assert np.array_equal(o.pcg_trace(), r.pcg) and np.array_equal(e.pcg_trace(), r.pcg), k
        assert eo == ee == er and np.array_equal(s.get_x_sol().ravel(), r.get_x_sol())
        assert_within_bound(s.debug_vec("x"), r.x, e.vec("x"), o.vec("x"), f"batch {k} x")
        for name in SCALARS:
            assert_within_bound(s.debug_scalar(name), getattr(r, "std" if name == "std_obj" else name), e.scalar(name), o.scalar(name),
                                f"batch {k} {name}")
