"""The HIP LP solvers, through their debug read-outs, against the independent numpy restatement, one outer iteration at a time
(tests/lp_steplock.py).  Until now the kernels were held to the C oracle bit for bit and only the oracle to the
restatement; here no oracle stands in between.

One test per kernel family, several instances per handle.  Every family runs iterations 0..74 as l2f windows of length 1 (rho updates at
25 and 50, the gamma decay, std_obj from iteration 10), then a scripted fix at 75, where a rho update is pending, and 30 more iterations.
After the fix the comparison goes through `live` (the kernels never compact) and the restatement's left_idx."""
import numpy as np
import pytest

import lp_steplock as S
from helpers import lp_instances
from lpbox_hip.big import BigLp
from lpbox_hip.lp import LpBatch
from lpbox_hip.synth import make_auction_like
from valued_cases import valued

pytestmark = pytest.mark.gpu

STEPS = S.l2f_steps(0, 75) + S.l2f_steps(75, 105, "scripted")


def gen(name, idx):
    return lp_instances(name)[idx]


def run_batch(insts, tags, order=None, x_update="pcg", slots=None, ceiling=None):
    b = LpBatch(insts, order=order)
    if x_update == "direct":
        b.set_x_update("direct")
    b.solve_init()
    if slots is not None:
        assert b.config()["elems_per_thread"] == slots, b.config()
    g = S.BatchGroup(b, insts)
    cases = [S.Case(I, v, t, x_update=x_update, calibrate=False) for I, v, t in zip(insts, g.views, tags)]
    S.run_cases(g, cases, STEPS)
    report(cases, ceiling)
    b.close()
    return cases


def run_big(P, tag, ceiling=None, **kw):
    g = BigLp(P, **kw)
    g.solve_init()
    grp = S.BigGroup(g)
    cases = [S.Case(P, grp.views[0], tag, calibrate=False)]
    S.run_cases(grp, cases, STEPS)
    report(cases, ceiling)
    g.close()


def report(cases, ceiling=None):
    for c in cases:
        print(f"{c.tag}: checked {c.checked}, weak before the fix {c.pre[1]} of {c.pre[0]}, after {c.post[1]} of {c.post[0]}, fixed {c.fixed}, "
              f"subject/spread {c.worst:.2f}, stop {c.stop_at}")
    S.assert_clean(cases, ceiling)           # ceiling: stored values, iterations 0..74 (see lp_steplock.assert_clean)
    for c in cases:
        assert c.fixed > 0 or c.done, f"{c.tag}: the scripted fix did not fire"


def test_onchip_default_order_one_slot():
    insts = [S.fuzz_instance("heavy_row_3"), S.fuzz_instance("empty_rows_65"), S.fuzz_instance("heavy_row_257"), gen("lp_100_500_seed0.npz", 0)]
    assert [I["n"] for I in insts] == [3, 65, 257, 500]
    run_batch(insts, ["n3", "n65", "n257", "n500"], slots=1)


def test_onchip_default_order_two_slots():
    """513 .. 1024 storage positions: two slots per thread."""
    insts = [S.fuzz_instance("one_entry_cols_513"), S.fuzz_instance("dup_cols_700")]
    run_batch(insts, ["n513", "n700"], slots=2)


def test_onchip_default_order_four_slots():
    """1025 .. 2048 storage positions: four slots per thread (n = 1200 is past the two-slot variant's 1024 positions)."""
    run_batch([S.fuzz_instance("dup_cols_1200"), S.fuzz_instance("heavy_row_2048")], ["n1200", "n2048"], slots=4)


def test_onchip_reference_order_unit():
    run_batch([gen("lp_100_500_seed0.npz", 2), S.fuzz_instance("empty_rows_65"), S.fuzz_instance("one_entry_cols_5")], ["gen100_2", "n65", "n5"],
              order="reference")


def test_onchip_reference_order_valued():
    insts = [valued(gen("lp_100_500_seed0.npz", 0), "uniform", 0), valued(gen("lp_20_60_seed0.npz", 1), "signed", 0),
             valued(S.fuzz_instance("empty_rows_65"), "set", 0)]
    run_batch(insts, ["uniform gen100_0", "signed gen20_1", "set n65"], order="reference",
              ceiling={"uniform gen100_0": 27, "set n65": 59})


def test_onchip_direct_x_update():
    insts = [gen("lp_100_500_seed0.npz", 0), gen("lp_20_60_seed0.npz", 1), S.fuzz_instance("empty_rows_65"), S.fuzz_instance("heavy_empty_65")]
    run_batch(insts, ["gen100_0", "gen20_1", "n65", "n65 heavy"], x_update="direct")


@pytest.mark.parametrize("pcg_mode", ["reference", "lean"])
def test_large_route_default_order(pcg_mode):
    run_big(make_auction_like(3000, seed=1), f"big {pcg_mode}", pcg_mode=pcg_mode)


@pytest.mark.parametrize("family", [None, "uniform"])
def test_large_route_reference_order(family):
    P = make_auction_like(3000, seed=1)
    run_big(P if family is None else valued(P, family, 0), f"big reference {family}", ceiling={"big reference uniform": 68}, order="reference")
