"""The instances of the batched early-fixing tests on the large route (tests/test_big_l2f_batch_api.py on the CPU,
tests/test_big_l2f_batch_gpu.py on the GPU) and their oracle runs: LpOracle in the kernels' reduction order with the
geometry tests/big_batch_cases.py pins (T = 256, chunk = 512).  An oracle run is made once and its snapshots are shared and read-only.

The fix rule is scripted: helpers.scripted_fix_vec(x, lo=0.05, hi=0.95, last=5) on the window's iterates, with the trainer's guard
`num <= 10 -> nothing` (LP/trainer.py:533-535).  The same rule as a torch policy returns exactly 1.0, 0.0 or 0.5 per row, so the
float32 comparison in torch and the widened one on the device cannot differ."""
import functools

import numpy as np

import big_batch_cases as BC
from helpers import scripted_fix_vec

WS, NWIN, MIN_FIX, C_HI = 10, 8, 10, 0.9
RULE = dict(lo=0.05, hi=0.95, last=5)
MIXED = BC.MIXED
# (n, seed) -> variables fixed at the start of windows 1 ... 7 (window 0 fixes nothing), pinned by the CPU file.  In windows 6 and 7
# some members fix and others do not: `apply == 0` beside `apply == 1` in one prologue.
FIXES = {
    (300, 0): (141, 60, 21, 14, 13, 0, 12),
    (513, 2): (227, 84, 77, 20, 11, 0, 0),
    (1100, 4): (497, 232, 94, 36, 18, 0, 0),
    (2100, 6): (983, 432, 136, 85, 43, 33, 18),
    (2600, 7): (1182, 545, 233, 85, 41, 27, 47),
}
# largest PCG count of an outer iteration in window 0, and the range of the counts after it
PCG_W0_MAX = {(300, 0): 21, (513, 2): 21, (1100, 4): 21, (2100, 6): 22, (2600, 7): 22}
PCG_LATER = (4, 9)
SCALARS = ("rho1", "rho4", "gamma", "dI", "rho4Et", "std_obj", "cur_obj", "cvg1", "cvg2", "obj_val", "sum_fix_obj", "fix_obj")
LIVE_VECS = ("x", "z1", "z2", "b")
ROW_VECS = ("z4", "f")

# the shrinking live list: n = 2 * (the compaction's chunk) + 37, fixes that leave 4097, 4096, 4095, 1 and 0 live variables
COMPACT_CHUNK = 4096
SHRINK = (2 * COMPACT_CHUNK + 37, 9)
SHRINK_LEFT = (4097, 4096, 4095, 1, 0)
SHRINK_WS = 2
SHRINK_RETS = (0, 0, 0, 0, 1)


def guarded(x, min_fix=MIN_FIX):
    vec, num = scripted_fix_vec(x, **RULE)
    return (vec, num) if num > min_fix else (None, 0)


def frozen(v):
    v = np.array(v)
    v.setflags(write=False)
    return v


def snapshot(o, ret, ws, vec, num, new_trace):
    s = dict(ret=ret, vec=None if vec is None else frozen(vec), num=num, x_iters=frozen(o.get_x_iters_2d(ws)),
             left=frozen(o.vec("left_idx").astype(int)), n_live=o.get_n(), obj=o.cal_Obj(), outer_total=o.total_outer_iters,
             pcg_total=o.total_pcg_iters, trace=tuple(int(k) for k in new_trace), stop=o.last_stop_reason)
    for name in LIVE_VECS + ROW_VECS:
        s[name] = frozen(o.vec(name))
    for name in SCALARS:
        s[name] = o.scalar(name)
    return s


def _new_trace(o, outer_before):
    t = o.pcg_trace()
    return t[outer_before:] if len(t) == o.total_outer_iters else t      # (a trace kept over the calls, or one per call)


@functools.lru_cache(None)
def oracle_schedule(n, seed, schedule, min_fix=MIN_FIX):
    """Early-fixing windows (a, b, fix) on a fresh oracle: with `fix` the window applies the scripted rule to the iterates of the
    window before it, without it the window fixes nothing.  Returns (one snapshot per window, the binary solution at the end);
    snapshot["vec"] / ["num"]: the fix the window was called with."""
    o = BC.fresh_oracle(n, seed)
    out = []
    for (a, b, fix) in schedule:
        vec, num = guarded(out[-1]["x_iters"], min_fix) if fix and out else (None, 0)
        before = o.total_outer_iters
        ret = o.solve_iter_l2f(a, b, np.zeros(o.get_n()) if vec is None else vec, num)
        out.append(snapshot(o, ret, b - a, vec, num, _new_trace(o, before)))
        if ret:
            break
    return tuple(out), frozen(o.get_x_sol().ravel())


def oracle_l2f(n, seed, nwin=NWIN, ws=WS, min_fix=MIN_FIX):
    """`nwin` consecutive windows of `ws` iterations, every one after the first under the scripted rule."""
    return oracle_schedule(n, seed, tuple((ws * w, ws * (w + 1), w > 0) for w in range(nwin)), min_fix)


def shrink_vec(n_live, left_after, w):
    """A fix vector over `n_live` live variables that leaves `left_after`: the fixed ones are spread over the list (every chunk of the
    compaction keeps and drops entries), alternately to 1 and to 0."""
    vec = -np.ones(n_live)
    k = n_live - left_after
    idx = np.unique(np.linspace(0, n_live - 1, k).round().astype(int)) if k < n_live else np.arange(n_live)
    rest = np.setdiff1d(np.arange(n_live), idx)[:k - len(idx)]
    idx = np.sort(np.concatenate([idx, rest]))
    assert len(idx) == k
    vec[idx] = (np.arange(k) + w) % 2
    return vec, k


@functools.lru_cache(None)
def oracle_shrink():
    """The SHRINK instance through windows of SHRINK_WS: window 0 fixes nothing, window w + 1 leaves SHRINK_LEFT[w] live variables."""
    o = BC.fresh_oracle(*SHRINK)
    out, vec, num = [], None, 0
    for w in range(len(SHRINK_LEFT) + 1):
        before = o.total_outer_iters
        ret = o.solve_iter_l2f(SHRINK_WS * w, SHRINK_WS * (w + 1), np.zeros(o.get_n()) if vec is None else vec, num)
        out.append(snapshot(o, ret, SHRINK_WS, vec, num, _new_trace(o, before)))
        if w < len(SHRINK_LEFT):
            vec, num = shrink_vec(o.get_n(), SHRINK_LEFT[w], w)
    return tuple(out), frozen(o.get_x_sol().ravel())


def same_as_snapshot(g, s, tag, ws=WS, x_iters=None):
    """Handle `g` (a BigLp) against an oracle snapshot, bit for bit.  x_iters: the member's rows of the batch's pack, checked too."""
    from helpers import bits_equal
    xg = g.get_x_iters_2d(ws)
    assert bits_equal(xg, s["x_iters"]), f"{tag}: x_iters"
    if x_iters is not None:
        assert bits_equal(x_iters, s["x_iters"]), f"{tag}: packed x_iters"
    left = s["left"]
    assert g.get_n() == s["n_live"] == len(left) and g.scalar("n_live") == s["n_live"], f"{tag}: get_n"
    for name in LIVE_VECS:
        if s["n_live"] == 0:
            break                             # everything is fixed: the reference returns before it shrinks its vectors (LPcpp:1212-1217)
        assert bits_equal(g.vec(name)[left], s[name]), f"{tag}: {name}"
    for name in ROW_VECS:
        assert bits_equal(g.vec(name), s[name]), f"{tag}: {name}"
    for name in SCALARS:
        if name == "fix_obj" and np.isnan(s[name]):
            continue                          # uninitialised member in the reference until the first fix
        if name in ("dI", "rho4Et") and s["n_live"] == 0:
            continue                          # the oracle reads these two from the first entry of a matrix that has no entry left
        assert g.scalar(name) == s[name], f"{tag}: {name}"
    assert g.cal_Obj() == s["obj"], f"{tag}: cal_Obj"
    assert (g.scalar("outer_total"), g.scalar("pcg_total")) == (s["outer_total"], s["pcg_total"]), f"{tag}: counters"


TWIN_SCALARS = SCALARS + ("outer_total", "pcg_total", "iter", "stop", "ret", "last_pcg", "n_live", "c1", "best_bin_obj")


def same_as_twin(g, t, tag, ws=WS):
    """Handle `g` against a handle that ran the same windows alone, through solve_iter_l2f with the same vectors."""
    from helpers import bits_equal, scalar_bits_equal
    assert bits_equal(g.get_x_iters_2d(ws), t.get_x_iters_2d(ws)), f"{tag}: x_iters (twin)"
    for name in ("x", "z1", "z2", "b", "z4", "f", "pd", "live", "Ex"):
        assert bits_equal(g.vec(name), t.vec(name)), f"{tag}: {name} (twin)"
    for name in TWIN_SCALARS:
        assert scalar_bits_equal(g.scalar(name), t.scalar(name)), f"{tag}: {name} (twin)"
    assert g.get_n() == t.get_n() and g.cal_Obj() == t.cal_Obj(), f"{tag}: get_n / cal_Obj (twin)"


def state_of(g, ws=WS):
    """Everything a window can change in a handle, for `untouched` checks."""
    return dict(vecs={name: g.vec(name) for name in ("x", "z1", "z2", "z4", "f", "pd", "live", "Ex")},
                scalars={name: g.scalar(name) for name in TWIN_SCALARS + ("pcg_resumes",)}, n=g.get_n(), x_iters=g.get_x_iters_2d(ws))


def same_state(a, b):
    from helpers import bits_equal, scalar_bits_equal
    return (all(bits_equal(a["vecs"][k], b["vecs"][k]) for k in a["vecs"]) and a["n"] == b["n"] and bits_equal(a["x_iters"], b["x_iters"])
            and all(scalar_bits_equal(a["scalars"][k], b["scalars"][k]) for k in a["scalars"]))
