"""The workgroup reduction of the LP kernels (block_sum) with the second stage the 512-thread window kernel runs, next to the default
one: through lpbox_debug_block_sum bit for bit against a numpy restatement of the documented tree, and through the public API on
instances whose live lanes sit in one wave (n = 60), in two (n = 65) and in every lane (n = 512), against the oracle's mirror."""
import numpy as np
import pytest

from helpers import bits_equal, lp_instances, oracle_like, scripted_fix_vec
from test_lp_gpu_parity import compare_state, gpu_solver

pytestmark = pytest.mark.gpu

T, ROUNDS = 512, 3
STAGE_DEFAULT, STAGE_PAIRS = 0, 1


def tree_sum(a):
    """a: (T, NV) per-thread partials -> (NV,) totals in the kernels' association: inside a wavefront the partner lanes
    xor 32, 16, 1, 2, 4, 8, then the wave partials xor 1, 2, 4.  Addition is commutative, so every lane holds the same bits."""
    w = a.reshape(T // 64, 64, -1)
    lane = np.arange(64)
    for m in (32, 16, 1, 2, 4, 8):
        w = w + w[:, lane ^ m, :]
    p = w[:, 0, :]
    wave = np.arange(T // 64)
    for m in (1, 2, 4):
        p = p + p[wave ^ m]
    return p[0]


def spread(rs, shape):
    """Magnitudes from 2^-200 to 2^200 with both signs: a sum that pairs the wrong partners rounds differently."""
    return np.ldexp(rs.uniform(1.0, 2.0, shape), rs.randint(-200, 201, shape)) * np.where(rs.rand(*shape) < 0.5, -1.0, 1.0)


def inputs(nv):
    rs = np.random.RandomState(1000 + nv)
    cases = {"spread": spread(rs, (ROUNDS, T, nv))}
    cases["same magnitude"] = rs.uniform(-1.0, 1.0, (ROUNDS, T, nv))      # every addition of the tree rounds
    w0 = np.zeros((ROUNDS, T, nv))
    w0[:, :64, :] = spread(rs, (ROUNDS, 64, nv))
    cases["wave 0 only"] = w0
    cases["-0.0 everywhere"] = np.full((ROUNDS, T, nv), -0.0)
    ni = rs.uniform(-1.0, 1.0, (ROUNDS, T, nv))
    ni[1, 37, 0] = np.nan                      # value 0 of round 1 becomes NaN, the last value +inf (one sum holds both when nv = 1)
    ni[1, 300, nv - 1] = np.inf
    cases["one NaN, one +inf"] = ni
    return cases


INPUTS = {nv: inputs(nv) for nv in (1, 2, 3, 6)}
EXPECTED = {nv: {name: np.stack([tree_sum(a[r]) for r in range(ROUNDS)]) for name, a in cs.items()} for nv, cs in INPUTS.items()}


def run_block_sum(nv, stage, groups, a):
    from lpbox_hip import _lib
    out = np.empty((groups, ROUNDS, T, nv))
    _lib.check(_lib.load().lpbox_debug_block_sum(T, nv, stage, groups, ROUNDS, np.ascontiguousarray(a), out), "lpbox_debug_block_sum")
    return out


@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("nv", [1, 2, 3, 6])
@pytest.mark.parametrize("stage", [STAGE_DEFAULT, STAGE_PAIRS])
def test_block_sum_matches_the_tree(stage, nv, groups):
    for name, a in INPUTS[nv].items():
        out = run_block_sum(nv, stage, groups, a)
        want = EXPECTED[nv][name]                                    # (ROUNDS, nv)
        if name == "-0.0 everywhere":
            assert np.all(np.signbit(want)) and np.all(want == 0)
        if name == "one NaN, one +inf":
            assert np.isnan(want[1, 0]) and (nv == 1 or want[1, nv - 1] == np.inf) and np.all(np.isfinite(want[[0, 2]]))
        # every thread of every workgroup received the same bits ...
        first = out[:, :, :1, :]
        assert np.array_equal(out.view(np.uint64), np.broadcast_to(first, out.shape).view(np.uint64)), f"{name}: threads disagree"
        # ... and they are the tree's (a NaN total must be NaN on both sides; its payload is no property of the association)
        got = out[:, :, 0, :]
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), np.broadcast_to(nan, got.shape)), f"{name}: NaN totals"
        assert np.array_equal(np.where(nan, 0.0, got).view(np.uint64), np.broadcast_to(np.where(nan, 0.0, want), got.shape).view(np.uint64)), \
            f"{name}: stage {stage}, {nv} values, {groups} workgroups: totals differ from the tree"


def test_unbuilt_combination_is_rejected():
    from lpbox_hip import _lib
    a = np.zeros((ROUNDS, T, 4))
    with pytest.raises(_lib.LpboxError):
        run_block_sum(4, STAGE_PAIRS, 1, a)                          # four values: no LP kernel reduces four
    with pytest.raises(_lib.LpboxError):
        _lib.check(_lib.load().lpbox_debug_block_sum(256, 1, STAGE_PAIRS, 1, ROUNDS, np.zeros((ROUNDS, 256, 1)), np.zeros((1, ROUNDS, 256, 1))))


def generated(n, seed):
    from lpbox_hip.synth import make_auction_like
    return make_auction_like(n, seed=seed)


@pytest.mark.parametrize("make,n", [(lambda: lp_instances("lp_20_60_seed0.npz")[1], 60), (lambda: generated(512, 3), 512),
                                    (lambda: generated(65, 12), 65)], ids=["n60", "n512", "n65"])
def test_three_windows_with_a_fix_bit_exact(make, n):
    """Three launches of the 512 x 1 window kernel, an early-fix vector applied at the second: the masks and the launch boundaries meet
    the store and the read of the reduction.  Every iterate and, with compare_state's rule, every state vector and scalar."""
    I = make()
    assert I["n"] == n
    g = gpu_solver(I)
    cfg = g.batch.config()
    assert (cfg["threads"], cfg["elems_per_thread"]) == (512, 1)
    o = oracle_like(g, I)
    ws = 40
    vec, num = np.zeros(n), 0
    for w in range(3):
        rg, ro = g.solve_iter_l2f(w * ws, (w + 1) * ws, vec, num), o.solve_iter_l2f(w * ws, (w + 1) * ws, vec, num)
        assert rg == ro, f"window {w}"
        xg, xo = g.get_x_iters_2d(ws), o.get_x_iters_2d(ws)
        assert bits_equal(xg, xo), f"window {w}: iterates differ"
        compare_state(g, o, f"window {w}")
        assert g.batch.counters() == (o.total_outer_iters, o.total_pcg_iters)
        if w == 0:
            vec, num = scripted_fix_vec(xo, lo=0.02, hi=0.98, last=20)
            assert 0 < num < n, "the scripted vector must fix some variables and leave some"
        else:
            vec, num = np.zeros(g.get_n()), 0
        if rg:
            break
    assert w == 2, "the solve must run through all three windows"
    assert g.get_n() < n
