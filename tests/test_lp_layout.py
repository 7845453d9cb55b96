"""The host layout planner of the batched LP kernels (csrc/lpbox_lp_layout.cpp).

CPU: the layout of the tree's library equals, table for table, what the commit before the planner was split out of lpbox_capi.hip
produced (tests/golden/lp_layout_parent.npz, recorded from that commit, see tests/golden/make_lp_layout_fixture.py) -- where a row task
or a helper chunk sits changes no result, only the time, so no parity test would notice a slip there; the direct mode's row choice
equals the ascending greedy one; and the planner's invariants hold on generated instances under AddressSanitizer + UBSan
(tests/lp_layout_check.cpp, a stand-alone program).  GPU: what the getters report before solve_init is what the kernels then run with.
"""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from helpers import GOLDEN, bits_equal, lp_instances, oracle_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "accelerated-lpbox-admm_amd", "csrc")
sys.path.insert(0, GOLDEN)
import make_lp_layout_fixture as fixture  # noqa: E402


def test_layout_equals_the_recorded_one():
    want = fixture.load(fixture.OUT)
    got = fixture.record()
    assert sorted(got) == sorted(want)
    assert len(got) > 250 and any(k.endswith("/wave_classes") for k in got)
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


def test_direct_rows_are_the_ascending_greedy_ones():
    """lp_plan_direct_rows through lpbox_get_direct_rows, on a machine without a GPU: the split test_direct_x_update.greedy_split restates
    and objective_study_direct_100_500.npz was computed with (test_objective_gap.py)."""
    from lpbox_hip.lp import LpBatch
    from test_direct_x_update import greedy_split
    I, J = fixture._instances("lp_100_500_seed0.npz", 2)
    b = LpBatch([I])
    rows = b.direct_rows(0)
    assert np.array_equal(rows, greedy_split(I))
    b.set_problem(0, J["n"], J["l"], J["colptr"], J["rowidx"], J["b"])          # the answer follows the problem, it is not kept from the one before
    assert np.array_equal(b.direct_rows(0), greedy_split(J)) and not np.array_equal(greedy_split(J), rows)
    assert 0 < (rows >= 0).sum() < I["l"] and np.array_equal(np.sort(rows[rows >= 0]), np.arange((rows >= 0).sum()))


def test_planner_invariants_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "lp_layout_check")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = subprocess.run([gxx, *flags, "-x", "c++", "-", "-o", exe], input="int main() { return 0; }\n", text=True, capture_output=True)
    if probe.returncode != 0:
        pytest.skip("g++ cannot link the sanitizer runtimes")
    srcs = [os.path.join(ROOT, "tests", "lp_layout_check.cpp"), os.path.join(CSRC, "lpbox_lp_layout.cpp")]
    objs = [str(tmp_path / ("%d.o" % k)) for k in range(len(srcs))]
    jobs = [subprocess.Popen([gxx, *flags, "-I", CSRC, "-c", src, "-o", obj]) for src, obj in zip(srcs, objs)]      # side by side: the build is most of the time
    assert [j.wait() for j in jobs] == [0, 0]
    subprocess.run([gxx, *flags, *objs, "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "plans ok" in run.stdout


def _inspect(b):
    own, help4 = b.col_split(0)
    got = dict(layout=b.layout(0), row_split=b.row_split(0), col_split_own=own, col_split_help=help4, config=b.config())
    got.update((t, b.debug_table(t, 0)) for t in fixture.TABLES)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("case,x_update", [("lp_20_60", "pcg"), ("instance_3_7", "pcg"), ("lp_20_60", "direct")])
def test_what_the_getters_report_is_what_runs(case, x_update):
    """The inspection getters and debug_table answer before solve_init, answer the same afterwards, and 200 plain iterations are bit-equal
    to the oracle built from the arrays taken BEFORE solve_init (the direct mode: its row map comes from the planner's rid)."""
    from lpbox_hip.lp import LpBatch
    valued = case == "instance_3_7"        # a valued instance: reference order, identity layout, the oracle in the reference's Eigen order
    I = fixture._file_instance(3, 7) if valued else lp_instances("lp_20_60_seed0.npz")[0]
    b = LpBatch([I], order="reference" if valued else "default")
    before = _inspect(b)
    if valued:
        from valued_cases import valued_oracle
        assert np.array_equal(before["layout"], np.arange(I["n"])) and np.all(before["row_split"] == 1)
        o = valued_oracle(I)
    else:
        o = oracle_for(b, 0, I, x_update=x_update, direct_rows=b.direct_rows(0) if x_update == "direct" else None)
    if x_update == "direct":
        b.set_x_update("direct")
    b.solve_init()
    assert b.solve_iter(0, 200)[0] == o.solve_iter(0, 200)
    after = _inspect(b)
    for k in before:
        if k == "config":          # the geometry; which PCG loop runs follows the x-update mode (the direct mode has no PCG loop to specialise)
            assert {q: v for q, v in before[k].items() if q != "pcg_loop"} == {q: v for q, v in after[k].items() if q != "pcg_loop"}
            assert after[k]["pcg_loop"] == ("generic" if x_update == "direct" else before[k]["pcg_loop"])
        else:
            assert np.array_equal(before[k], after[k]), k
    left = o.vec("left_idx").astype(int)
    for name in ("x", "z1", "z2", "z4"):
        gv = b.debug_vec(name)
        assert bits_equal(gv[left] if name != "z4" else gv, o.vec(name)), name
    assert b.counters(0) == (o.total_outer_iters, o.total_pcg_iters)
    assert b.cal_obj(0) == o.cal_Obj()
