"""block_sum with the first stage whose wide butterfly steps swap a value against an undefined register instead of a copy of itself
(RED_STAGE_PAIRS_LOW, the stage of the 512 x 1 LP window kernel): the lanes that are stored receive the same sums in the same
association, the others hold garbage that goes to slots nobody reads -- so every thread of every workgroup must still receive the
documented tree's bits, round after round on one scratch, for 1, 2, 3 and 6 values, with NaN and infinity among the partials."""
import numpy as np
import pytest

from test_block_sum_stage_gpu import EXPECTED, INPUTS, run_block_sum

pytestmark = pytest.mark.gpu

STAGE_PAIRS_LOW = 2


@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("nv", [1, 2, 3, 6])
def test_low_stage_matches_the_tree(nv, groups):
    for name, a in INPUTS[nv].items():
        out = run_block_sum(nv, STAGE_PAIRS_LOW, groups, a)
        want = EXPECTED[nv][name]                                    # (ROUNDS, nv)
        first = out[:, :, :1, :]
        assert np.array_equal(out.view(np.uint64), np.broadcast_to(first, out.shape).view(np.uint64)), f"{name}: threads disagree"
        got = out[:, :, 0, :]
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), np.broadcast_to(nan, got.shape)), f"{name}: NaN totals"
        assert np.array_equal(np.where(nan, 0.0, got).view(np.uint64), np.broadcast_to(np.where(nan, 0.0, want), got.shape).view(np.uint64)), \
            f"{name}: {nv} values, {groups} workgroups: totals differ from the tree"
