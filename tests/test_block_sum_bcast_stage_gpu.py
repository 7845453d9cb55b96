"""block_sum with reduction steps on f64 arithmetic that takes a row-broadcast operand (RED_STAGE_PAIRS_BC): after the two quad steps
each row of 16 lanes is finished for its first lane only -- the one lane that is stored -- by three additions of a broadcast value
(lane 4, lane 12, then lane 8 of the row); and with the second stage in which a lane reads four wave partials and one cross-lane level
finishes, on that first stage (RED_STAGE_FOUR_BC, the stage of the 512 x 1 LP window kernel) and on the earlier one
(RED_STAGE_FOUR_LOW).  Every thread of every workgroup must still receive the
documented tree's bits, round after round on one scratch, for 1, 2, 3 and 6 values, with -0.0, NaN and infinity among the partials;
and partials that sit only in lanes 4, 8 and 12 of one row make a broadcast from any other lane change the total."""
import numpy as np
import pytest

from test_block_sum_stage_gpu import EXPECTED, INPUTS, ROUNDS, T, run_block_sum, tree_sum

NEW_STAGES = {"PAIRS_BC": 3, "FOUR_BC": 4, "FOUR_LOW": 5}
NVS = (1, 2, 3, 6)


def broadcast_lanes(nv):
    """Non-zero only in lanes 4, 8 and 12 of one row of one wave (another wave, row and magnitude set per round and value): the
    three lanes the row finish broadcasts from.  Magnitudes 2^0, 2^12 and 2^-12 with random mantissas: all three reach into the 53 bits
    of the total, so a total that misses one of them, or takes a neighbour's zero instead, has other bits."""
    rs = np.random.RandomState(77 + nv)
    a = np.zeros((ROUNDS, T, nv))
    for r in range(ROUNDS):
        for k in range(nv):
            wave, row = rs.randint(0, T // 64), rs.randint(0, 4)
            base = wave * 64 + row * 16
            for lane, e in zip((4, 8, 12), rs.permutation([0, 12, -12])):
                a[r, base + lane, k] = np.ldexp(rs.uniform(1.0, 2.0), int(e)) * (-1.0 if rs.rand() < 0.5 else 1.0)
    return a


CASES = {nv: dict(INPUTS[nv], **{"lanes 4, 8, 12 of one row": broadcast_lanes(nv)}) for nv in NVS}
WANT = {nv: dict(EXPECTED[nv], **{"lanes 4, 8, 12 of one row": np.stack([tree_sum(CASES[nv]["lanes 4, 8, 12 of one row"][r])
                                                                         for r in range(ROUNDS)])}) for nv in NVS}


def test_the_broadcast_case_tells_the_lanes_apart():
    """No GPU needed: dropping any one of the three lanes changes the expected total of every round and value."""
    for nv in NVS:
        a = CASES[nv]["lanes 4, 8, 12 of one row"]
        for lane in (4, 8, 12):
            b = a.copy()
            b[:, lane::16, :] = 0.0
            for r in range(ROUNDS):
                assert np.all(tree_sum(b[r]) != WANT[nv]["lanes 4, 8, 12 of one row"][r])


@pytest.mark.gpu
@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("nv", NVS)
@pytest.mark.parametrize("stage", sorted(NEW_STAGES.values()), ids=sorted(NEW_STAGES, key=NEW_STAGES.get))
def test_bcast_stage_matches_the_tree(stage, nv, groups):
    for name, a in CASES[nv].items():
        out = run_block_sum(nv, stage, groups, a)
        want = WANT[nv][name]                                        # (ROUNDS, nv)
        first = out[:, :, :1, :]
        assert np.array_equal(out.view(np.uint64), np.broadcast_to(first, out.shape).view(np.uint64)), f"{name}: threads disagree"
        got = out[:, :, 0, :]
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), np.broadcast_to(nan, got.shape)), f"{name}: NaN totals"
        assert np.array_equal(np.where(nan, 0.0, got).view(np.uint64), np.broadcast_to(np.where(nan, 0.0, want), got.shape).view(np.uint64)), \
            f"{name}: stage {stage}, {nv} values, {groups} workgroups: totals differ from the tree"
