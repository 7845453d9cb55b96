"""The lockstep launch chains of a batch (ChainLockstep in csrc/lpbox_chain.h, chain_run_lockstep in csrc/lpbox_host.h, with the
launches of csrc/lpbox_seg_capi.hip and csrc/lpbox_big_capi.hip) reproduce, window for window, the bookkeeping recorded from the commit
before the two front ends shared one loop (tests/golden/chain_batch_parent.json, see tests/golden/make_chain_batch_fixture.py): resumes
per member, launches booked, kmax, walker launches, return values and iteration counters, with eager launches and with captured graphs.
The decisions themselves are held against a table on the CPU by tests/chain_check.cpp (tests/test_chain.py)."""
import functools
import json
import sys

import pytest

from helpers import GOLDEN

sys.path.insert(0, GOLDEN)
import make_chain_batch_fixture as fixture  # noqa: E402

FORCED = ("seg_kmax2", "big_kmax4_eager", "big_kmax4_graph", "big_l2f_kmax4_eager", "big_l2f_kmax4_graph")
PAIRS = [("big_eager", "big_graph"), ("big_kmax4_eager", "big_kmax4_graph"), ("big_l2f_eager", "big_l2f_graph"),
         ("big_l2f_kmax4_eager", "big_l2f_kmax4_graph"), ("big_ref_eager", "big_ref_graph")]


@functools.lru_cache(None)
def recorded():
    with open(fixture.OUT) as fh:
        return json.load(fh)


def test_the_record_holds_what_it_is_there_for():
    want = recorded()
    assert sorted(want) == sorted(fixture.CASES) and len(want) == 13
    for case in FORCED:                                                  # every member's PCG halted and was resumed
        assert all(r > 0 for r in want[case][-1]["pcg_resumes"]), case
    for case in ("big_eager", "big_graph", "big_l2f_eager", "big_l2f_graph", "big_ref_eager", "big_ref_graph"):
        assert want[case][-1]["kmax"] != fixture.BIG_KMAX_START, case      # the adaptive launch count moved
    for eager, graph in PAIRS:                                           # captured and eager count the same
        assert [r["graph"] for r in want[eager] + want[graph]] == [0] * len(want[eager]) + [1] * len(want[graph]), graph
        for key in ("launches", "walks", "pcg_resumes", "member_launches", "kmax"):
            assert [r.get(key) for r in want[eager]] == [r.get(key) for r in want[graph]], (graph, key)
    assert want["big_ref_graph"][-1]["walks"] > 0
    # the masked window books its launches on the first active member, and the member left out neither moves nor counts
    m = want["seg_masked"]
    assert m[1]["launches"][0] == m[0]["launches"][0] and m[1]["launches"][1] > m[0]["launches"][1] == 0
    assert m[1]["pcg_resumes"][0] == m[0]["pcg_resumes"][0] and m[2]["fixed"][0] > 0
    l = want["big_l2f_eager"]
    assert l[1]["member_outer_total"][1] == l[0]["member_outer_total"][1] and l[1]["fixed"][0] > 0 and l[1]["fix_launches"] == 8


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(fixture.CASES))
def test_bookkeeping_equals_the_recorded_one(case):
    got = fixture.record([case])[case]
    print(case, got)
    assert got == recorded()[case]
