"""Objective vectors outside the auction range (b = -price, price in about [1, 5500]) for the LP tests, and the near-zero remainder after a
fix.  Shared by tests/test_lp_objective_cases.py (CPU: pins on the oracle, step-locked against the restatement) and
tests/test_lp_objective_gpu.py (the kernels, bit for bit against the oracle).  DESIGN.md section 24."""
import functools

import numpy as np

SCALES = {"scale1e-6": 1e-6, "scale1e6": 1e6, "scale1e-150": 1e-150, "scale1e-160": 1e-160, "subnormal": 1e-310}
VARIANTS = ("scale1e-6", "scale1e6", "scale1e-150", "scale1e-160", "subnormal", "positive", "mixed_sign", "some_zero", "all_zero", "all_equal",
            "wide")
# the variants of the multi-slot, reference-order, direct and large-route GPU tests
SHORT_LIST = ("subnormal", "scale1e-150", "positive", "mixed_sign", "all_zero", "wide")


def objective_variant(I, name):
    """A copy of instance I with b replaced.  The three draws are made in this order whatever the name, so every variant is independent of
    which others are asked for.  There is no variant whose squares overflow (scale1e150 makes the variance of the objective history
    infinite): out of scope."""
    n = int(I["n"])
    b = np.array(I["b"], np.float64)
    rs = np.random.RandomState(5)
    s = rs.rand(n) < 0.5
    z = rs.rand(n) < 0.3
    w = rs.uniform(-6, 6, n)
    if name == "base":
        nb = b
    elif name in SCALES:
        nb = b * SCALES[name]
    elif name == "positive":
        nb = -b
    elif name == "mixed_sign":
        nb = np.where(s, -b, b)
    elif name == "some_zero":
        nb = np.where(z, 0.0, b)
    elif name == "all_zero":
        nb = np.zeros(n)
    elif name == "all_equal":
        nb = np.full(n, -7.0)
    elif name == "wide":
        nb = -10.0 ** w
    else:
        raise ValueError(name)
    assert np.all(np.isfinite(nb))                       # no test hands a non-finite b to a solver
    return dict(I, b=np.ascontiguousarray(nb, np.float64))


# What a plain solve_iter(0, 20000) of the oracle does: (return, outer iterations, stop reason) in ORDER_EIGEN and in ORDER_GPU with T = 512.
# Stop reasons: 0 = the cap, 1 = residual (y1_y2), 2 = obj_std.
CAP = (0, 20000, 0)
FULL_SOLVE = {
    "gen20_1": {"base": ((0, 6754, 1), (0, 8410, 1)), "scale1e-6": ((0, 844, 1), (0, 846, 1)), "scale1e6": (CAP, CAP),
                "scale1e-150": ((0, 863, 1), (0, 863, 1)), "scale1e-160": ((1, 836, 2), (1, 835, 2)), "subnormal": ((1, 10, 2), (1, 10, 2)),
                "positive": (CAP, CAP), "mixed_sign": ((0, 15209, 1), (0, 10390, 1)), "some_zero": ((0, 8685, 1), (1, 8576, 2)),
                "all_zero": ((0, 863, 1), (0, 863, 1)), "all_equal": ((0, 154, 1), (0, 154, 1)), "wide": ((0, 18737, 1), (1, 17500, 2))},
    "heavy_row_3": {"base": ((1, 36, 2), (1, 36, 2)), "scale1e-6": ((1, 31, 2), (1, 31, 2)), "scale1e6": (CAP, CAP),
                    "scale1e-150": ((1, 31, 2), (1, 31, 2)), "scale1e-160": ((1, 31, 2), (1, 31, 2)), "subnormal": ((1, 10, 2), (1, 10, 2)),
                    "positive": ((1, 5015, 2), (1, 5015, 2)), "mixed_sign": ((0, 223, 1), (0, 223, 1)), "some_zero": ((1, 36, 2), (1, 36, 2)),
                    "all_zero": ((0, 67, 1), (0, 67, 1)), "all_equal": ((1, 22, 2), (1, 22, 2)), "wide": ((1, 147, 2), (1, 147, 2))},
    "empty_rows_65": {"base": ((0, 480, 1), (0, 480, 1)), "scale1e-6": (CAP, CAP), "scale1e6": (CAP, CAP),
                      "scale1e-150": ((1, 2396, 2), (1, 2396, 2)), "scale1e-160": ((1, 537, 2), (1, 537, 2)),
                      "subnormal": ((1, 10, 2), (1, 10, 2)), "positive": (CAP, CAP), "mixed_sign": ((0, 423, 1), (0, 423, 1)),
                      "some_zero": ((0, 553, 1), (0, 553, 1)), "all_zero": (CAP, CAP), "all_equal": ((1, 2565, 2), (0, 2659, 1)),
                      "wide": ((0, 12634, 1), (0, 12634, 1))},
}

# ------------------------------------------------------------------------------------------------
# The return after a fix that leaves a remainder of almost zero norm (`if (sqrt(px[0]) < 1e-3) ret = 1`, the reference's :1223)
# ------------------------------------------------------------------------------------------------
BELOW, ABOVE = 0.9e-3, 1.1e-3            # margins either side of the 1e-3 of that line: no summation order can move a kept norm across it
REMAINDER_AT = 75                        # l2f iterations of length 1 before the fix
REMAINDER_MORE = 5                       # iterations after it
# instance -> (largest k whose kept norm is below BELOW, smallest k whose kept norm is above ABOVE), on the oracle in the kernels' order
# (T = 512; auction3000: the large route's T = 256 in chunks of 512) and in Eigen order.  gen100_0: k = 8 keeps 6.5e-4, k = 10 8.9e-4.
REMAINDER_K = {"gen100_0": (10, 12), "gen100_2": (11, 14), "dup_cols_700": (4, 6), "dup_cols_1200": (8, 10), "heavy_row_2048": (2, 3),
               "auction3000": (20, 23)}
REMAINDER_K_EIGEN = dict(REMAINDER_K, auction3000=(20, 24))


@functools.lru_cache(maxsize=None)
def remainder_instance(name):
    """The instances of REMAINDER_K by name (shared: do not modify)."""
    from helpers import lp_instances
    from lp_steplock import FUZZ, fuzz_instance
    if name in FUZZ:
        return fuzz_instance(name)
    if name == "auction3000":
        from lpbox_hip.synth import make_auction_like
        return make_auction_like(3000, 1)
    fixture, idx = {"gen100_0": ("lp_100_500_seed0.npz", 0), "gen100_2": ("lp_100_500_seed0.npz", 2), "gen20_1": ("lp_20_60_seed0.npz", 1)}[name]
    return lp_instances(fixture)[idx]


def remainder_ks(x, below=BELOW, above=ABOVE):
    """x: the live iterate.  Keeping the k variables of smallest |x| free (1 <= k < n), the kept norm is the root of the sum of their squares.
    Returns (largest k whose kept norm is below `below`, smallest k whose kept norm is above `above`); None where there is no such k."""
    a = np.sort(np.abs(np.asarray(x, np.float64)))[:-1]
    norm = np.sqrt(np.cumsum(a * a))                     # norm[k - 1]: the k smallest
    lo, hi = np.nonzero(norm < below)[0], np.nonzero(norm > above)[0]
    return (int(lo[-1]) + 1 if len(lo) else None), (int(hi[0]) + 1 if len(hi) else None)


def keep_smallest_fix(x, k):
    """The fix vector (one entry per live variable) that leaves the k variables of smallest |x| free and fixes every other to x >= 0.5.
    Returns (vec, num)."""
    x = np.asarray(x, np.float64)
    vec = (x >= 0.5).astype(np.float64)
    vec[np.argsort(np.abs(x), kind="stable")[:k]] = -1.0
    return vec, len(x) - k
