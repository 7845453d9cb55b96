"""Step-locked comparison of an LP solver (the C oracle in any configuration, or a HIP solver through its debug read-outs) with the
independent numpy restatement oracle/lpbox_numpy.py.  Shared by tests/test_lp_steplock.py (CPU) and tests/test_lp_steplock_gpu.py.

The iteration is chaotic only because rounding flips a PCG exit and the trajectories then separate.  Here every outer iteration is
compared on its own: before it the restatement's x, z1, z2, z4 are overwritten with the subject's, its PCG runs the subject's iteration
count, and everything else (rho, prev_rho, gamma, dI, pd, the rho4 E^T scale, rhoUpdated, f / b / left_idx / sum_fix_obj after fixes, the
objective history, std_obj, the stop decision) stays the restatement's own and is compared with the subject's as a result.

The tolerance comes from the restatement alone: each step is evaluated by an ensemble of 12 roundings of it (float64 in the natural
order, long double, 10 seeded permutations of variables and rows), and for a vector v
    B(v) = c * (largest element-wise max - min over the ensemble) + 1e-12 * max(1, |v|inf),
c = helpers.STEPLOCK_C for 0/1 matrices and STEPLOCK_C_VALUED for stored values, each calibrated on the restatement alone.
The subject must be within B(v) of the natural float64 member for x, z1, z2, z4 (and y3 where exposed), and its PCG count k must be
consistent with the restatement's recorded residualNorm2 / threshold: ratio[k-1] >= 1 - B and ratio[k] < 1 + B.  Quantities that do not
depend on the iterate (rho*, prev_rho*, gamma, dI, rho4Et, rhoUpdated, sum_fix_obj, pd, f, b) are held to 1e-12 max(1, |v|); the ones
computed from x (std_obj, cur_obj, best_bin_obj, obj_val, cvg1, cvg2) to B of their own ensemble spread; integers and index sets exactly.
A scalar that is NaN in the natural float64 member AND in the subject (std_obj = 0 / 0 when the objective vector is zero) counts as
agreement and is counted in Case.nan_agreed; a NaN on one side alone is a violation.  A call that returns 1 without a stop reason (the
fix left a remainder of norm < 1e-3, LPcpp:1223) does not end a case: its window and the following ones are compared like any other.
DESIGN.md sections 22 and 24."""
import copy
import os
import sys

import numpy as np

from helpers import STEPLOCK_C, STEPLOCK_C_VALUED, scripted_fix_vec
from oracle.lpbox_numpy import NumpyLpBox

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from fuzz_lp import random_instance  # noqa: E402

VECS = ("x", "z1", "z2", "z4")
N_PERM = 10
FLOOR = 1e-12
WEAK = 1e-4                                  # an iteration whose B(x) exceeds this pins little: at most a quarter of a case's may
STOP_CODE = {None: 0, "y1_y2": 1, "obj_std": 2, "pcg_alpha_negative": 3, "all_fixed": 4}
EXACT_SCALARS = ("rho1", "rho2", "rho4", "prev_rho1", "prev_rho4", "gamma", "dI", "rho4Et", "sum_fix_obj", "rhoUpdated")
ITERATE_SCALARS = ("std_obj", "cur_obj", "best_bin_obj", "obj_val", "cvg1", "cvg2")
_ATTR = {"gamma": "gamma_val", "rho4Et": "r4Et_scale"}


# name -> (seed, kind, n) of tools/fuzz_lp.random_instance: kind 0 empty rows, 1 one heavy row, 2 one-entry columns, 3 duplicate columns,
# 4 heavy row + empty rows + a few prices ten times larger, 5 any size
FUZZ = {"empty_rows_65": (15, 0, 65), "heavy_row_257": (76, 1, 257), "one_entry_cols_513": (6, 2, 513), "dup_cols_5": (81, 3, 5),
        "heavy_empty_65": (0, 4, 65), "heavy_row_3": (11, 1, 3), "one_entry_cols_5": (84, 2, 5), "any_257": (838, 5, 257),
        "dup_cols_700": (20, 3, 700), "dup_cols_1200": (12, 3, 1200), "heavy_row_2048": (35, 1, 2048)}      # the multi-slot kernels (GPU tests)


def fuzz_instance(name):
    seed, kind, n = FUZZ[name]
    I, k = random_instance(np.random.RandomState(seed))
    assert (k, I["n"]) == (kind, n), name
    return I


def ensemble(I, x_update="pcg", mutant=None, seed=0):
    """The 12 roundings of one instance: [natural float64, long double, 10 seeded permutations]."""
    rs = np.random.RandomState(1000 + seed)

    def mk(**kw):
        m = NumpyLpBox(I["n"], I["l"], I["colptr"], I["rowidx"], I["b"], I.get("f"), x_update=x_update, vals=I.get("vals"), mutant=mutant, **kw)
        m.solve_init()
        return m
    return [mk(), mk(dtype=np.longdouble)] + [mk(perm=(rs.permutation(I["n"]), rs.permutation(I["l"]))) for _ in range(N_PERM)]


def _spread(A):
    return float((A.max(axis=0) - A.min(axis=0)).max(initial=0.0))


def _floor(v):
    return FLOOR * max(1.0, float(np.abs(v).max(initial=0.0)))


# ------------------------------------------------------------------------------------------------
# subjects: one view per instance, one group per handle
# ------------------------------------------------------------------------------------------------
class OracleSubject:
    y3 = True

    def __init__(self, o):
        self.o = o

    def vec(self, name):
        return self.o.vec(name)

    def scalar(self, name):
        return self.o.scalar(name)

    def n(self):
        return self.o.get_n()

    def left_idx(self):
        return self.o.vec("left_idx").astype(int)

    def totals(self):
        return self.o.total_outer_iters, self.o.total_pcg_iters

    def last_pcg(self):
        return self.o.L.lpo_last_pcg_iters(self.o.h)

    def stop(self):
        return self.o.last_stop_reason


class OracleGroup:
    def __init__(self, oracles):
        self.views = [OracleSubject(o) for o in oracles]

    def run(self, a, e, fixes, active, plain):
        rets = []
        for v, (vec, num), on in zip(self.views, fixes, active):
            if not on:
                rets.append(0)
            elif plain:
                rets.append(v.o.solve_iter(a, e))
            else:
                rets.append(v.o.solve_iter_l2f(a, e, vec if num else np.zeros(max(v.n(), 1)), num))
        return rets


class BatchSubject:
    """One instance of an lpbox_hip.lp.LpBatch: the kernels never compact, fixed variables stay in place, masked by `live`."""
    y3 = False
    names = ("rho1", "rho2", "rho4", "prev_rho1", "prev_rho4", "gamma", "dI", "rho4Et", "std_obj", "cur_obj", "sum_fix_obj", "best_bin_obj",
             "cvg1", "cvg2", "obj_val", "rhoUpdated")

    def __init__(self, b, i, l):
        self.b, self.i, self.l = b, i, l

    def left_idx(self):
        return np.nonzero(self.b.debug_vec("live", self.i))[0]

    def vec(self, name):
        v = self.b.debug_vec(name, self.i)
        return v[: self.l] if name in ("z4", "f") else v[self.left_idx()]

    def scalar(self, name):
        return self.b.debug_scalar(name, self.i) if name in self.names else None

    def n(self):
        return self.b.get_n(self.i)

    def totals(self):
        return self.b.counters(self.i)

    def last_pcg(self):
        return int(self.b.debug_scalar("last_pcg", self.i))

    def stop(self):
        return self.b.stop(self.i)[0]


class BatchGroup:
    def __init__(self, batch, insts):
        self.b = batch
        self.views = [BatchSubject(batch, i, I["l"]) for i, I in enumerate(insts)]
        self.stride = max(I["n"] for I in insts)
        self.parked = False

    def run(self, a, e, fixes, active, plain):
        if self.parked or not all(active):
            self.b.set_active(np.array(active, np.int32))
            self.parked = True
        if plain:
            return list(self.b.solve_iter(a, e))
        V = -np.ones((len(fixes), self.stride))
        nums = np.zeros(len(fixes), np.int32)
        for i, (vec, num) in enumerate(fixes):
            if num and active[i]:
                V[i, : len(vec)] = vec
                nums[i] = num
        return list(self.b.solve_iter_l2f(a, e, V, nums))


class BigSubject:
    """lpbox_hip.big.BigLp on one rank (the large route)."""
    y3 = False
    names = ("rho1", "rho4", "gamma", "dI", "rho4Et", "std_obj", "cur_obj", "best_bin_obj", "cvg1", "cvg2", "obj_val", "sum_fix_obj")

    def __init__(self, g):
        self.g = g

    def left_idx(self):
        return np.nonzero(self.g.vec("live"))[0]

    def vec(self, name):
        v = self.g.vec(name)
        return v if name in ("z4", "f") else v[self.left_idx()]

    def scalar(self, name):
        return self.g.scalar(name) if name in self.names else None

    def n(self):
        return self.g.get_n()

    def totals(self):
        return int(self.g.scalar("outer_total")), int(self.g.scalar("pcg_total"))

    def last_pcg(self):
        return int(self.g.scalar("last_pcg"))

    def stop(self):
        return int(self.g.scalar("stop"))


class BigGroup:
    def __init__(self, g):
        self.views = [BigSubject(g)]

    def run(self, a, e, fixes, active, plain):
        g = self.views[0].g
        if plain:
            return [g.solve_iter(a, e)]
        vec, num = fixes[0]
        return [g.solve_iter_l2f(a, e, vec if num else None, num)]


# ------------------------------------------------------------------------------------------------
# the step-locked run of one instance
# ------------------------------------------------------------------------------------------------
def l2f_steps(a, e, fix=None):
    """Iterations a .. e-1 as l2f windows of length 1; `fix` ("scripted" / "all" / a (vec, num) pair) is applied by the first."""
    return [dict(a=it, e=it + 1, plain=False, fix=fix if it == a else None) for it in range(a, e)]


class Case:
    def __init__(self, I, view, tag="", x_update="pcg", mutant=None, c=None, check_from=0, calibrate=True):
        self.valued = I.get("vals") is not None                   # stored values: a c of their own, calibrated on valued cases
        self.I, self.view, self.tag, self.calibrate = I, view, tag, calibrate
        self.c = c if c is not None else (STEPLOCK_C_VALUED if self.valued else STEPLOCK_C)
        self.direct = x_update == "direct"
        self.members = ensemble(I, x_update, mutant)
        self.check_from = check_from           # steps before it drive the restatement but are compared by another test
        self.violations, self.done, self.first = [], False, True
        self.checked = self.weak = 0
        self.nan_agreed = 0                    # scalars that were NaN in the restatement's natural member and in the subject alike
        self.pre, self.post = [0, 0], [0, 0]   # [checked, weak] before the first fix of this case's steps / after it
        self.worst = self.loo = 0.0            # subject / spread and leave-one-out member / spread of the others, largest seen
        self.hist = []                         # the subject's x after every l2f step since the last fix
        self.fixed = 0
        self.stop_at = None                    # (iteration, reason) where subject and restatement stopped

    def fork(self, view, tag):
        """A second continuation from here: the restatement's state is copied, `view` is a subject brought to the same iteration."""
        assert np.array_equal(view.vec("x"), self.view.vec("x")) and view.totals() == self.view.totals(), "fork: the subjects differ"
        c = copy.copy(self)
        c.members, c.hist, c.view, c.tag = copy.deepcopy(self.members), list(self.hist), view, tag
        c.violations, c.checked, c.weak, c.worst, c.loo, c.pre, c.post, c.nan_agreed = [], 0, 0, 0.0, 0.0, [0, 0], [0, 0], 0
        return c

    def bad(self, it, msg):
        self.violations.append(f"{self.tag} it {it}: {msg}")

    def before(self, st):
        v = self.view
        self.state = None if self.first else {k: v.vec(k) for k in VECS}
        self.tot0 = v.totals()
        vec, num = np.zeros(0), 0
        if st["fix"] == "scripted":
            vec, num = scripted_fix_vec(np.stack(self.hist[-20:], axis=1), lo=0.05, hi=0.95, last=20)
        elif isinstance(st["fix"], tuple):                      # a fix vector made by the caller
            vec, num = st["fix"]
        elif st["fix"] == "all":
            vec = (v.vec("x") >= 0.5).astype(float)
            num = len(vec)
        self.fix = (vec, num)
        return self.fix

    def after(self, st, ret):
        v, a, e, nat = self.view, st["a"], st["e"], self.members[0]
        vec, num = self.fix
        outer, pcg = v.totals()
        ran, last = outer - self.tot0[0], v.last_pcg()
        counts = [last] if ran == 1 else ([pcg - self.tot0[1] - last, last] if ran == 2 else [])
        assert ran <= 2, "windows of at most two iterations"
        traced = len(nat.pcg_trace)
        for m in self.members:
            m.lock(self.state, counts)
            if st["plain"]:
                m.solve_iter(a, e)
            else:
                m.solve_iter_l2f(a, e, vec, num)
        self.first = False
        if num:
            self.hist, self.fixed = [], self.fixed + num
        # ---- integers and index sets: exactly ----
        ok = True
        for what, got, want in (("ret", int(ret), int(nat.ret)), ("stop reason", v.stop(), STOP_CODE[nat.stop]), ("live n", v.n(), nat.n),
                                ("iterations run", ran, len(nat.pcg_trace) - traced)):
            if got != want:
                self.bad(a, f"{what} {got}, restatement {want}")
                ok = False
        if ok and not np.array_equal(v.left_idx(), np.sort(nat.left_idx)):
            self.bad(a, "live index set differs")
            ok = False
        if nat.stop is not None:
            self.stop_at = (a + max(ran - 1, 0), nat.stop)
        # ret = 1 without a stop reason is the return after a fix that left a remainder of almost zero norm (LPcpp:1223): the window goes on
        if not ok or nat.n == 0 or ((ret or nat.ret) and nat.stop is not None):
            self.done = True
        if not ok or nat.n == 0 or ran == 0:
            return
        if a >= self.check_from:
            self.compare(a, counts, ran)
        if not st["plain"]:
            self.hist.append(v.vec("x"))

    def compare(self, it, counts, ran):
        v, ms, nat, c = self.view, self.members, self.members[0], self.c
        self.checked += 1
        part = self.post if self.fixed else self.pre
        part[0] += 1
        # ---- iterates: within B of the natural float64 member ----
        for name in VECS + (("y3",) if v.y3 else ()):
            A = np.array([m.natural(name) for m in ms])
            got = v.vec(name)
            spread, fl = _spread(A), _floor(A[0])
            B = c * spread + fl
            d = float(np.abs(got - A[0]).max(initial=0.0))
            self.worst = max(self.worst, d / (spread + fl))
            for i in range(2, len(ms) if self.calibrate else 0):    # calibration of c on the restatement alone: every float64 permuted member against the others
                self.loo = max(self.loo, float(np.abs(A[i] - A[0]).max(initial=0.0)) / (_spread(np.delete(A, i, axis=0)) + fl))
            if name == "x" and B > WEAK:
                self.weak += 1
                part[1] += 1
            if not d <= B:
                self.bad(it, f"{name}: |subject - restatement| = {d:.3e} > B = {B:.3e} (spread {spread:.3e})")
        # ---- what does not depend on the iterate: 1e-12 ----
        for name in ("pd", "f", "b"):
            got, want = v.vec(name), nat.natural(name)
            if got.shape != want.shape or not np.abs(got - want).max(initial=0.0) <= _floor(want):
                self.bad(it, f"{name} differs by {np.abs(got - want).max(initial=0.0):.3e}" if got.shape == want.shape else f"{name}: shape")
        for name in EXACT_SCALARS + ITERATE_SCALARS:
            got = v.scalar(name)
            if got is None:
                continue
            A = np.array([float(getattr(m, _ATTR.get(name, name))) for m in ms])
            B = _floor(A[:1]) + (c * (A.max() - A.min()) if name in ITERATE_SCALARS else 0.0)
            if np.isnan(A[0]) and np.isnan(got):   # 0/0 on both sides (std_obj with an objective of zero); a NaN on one side alone stays a violation
                self.nan_agreed += 1
                continue
            if not abs(got - A[0]) <= B:
                self.bad(it, f"{name}: subject {got!r}, restatement {A[0]!r}, B = {B:.3e}")
        # ---- the PCG exit: the subject's count against the restatement's residuals ----
        if self.direct:
            return
        for j, k in enumerate(counts):
            R = [m.pcg_ratios[len(m.pcg_ratios) - ran + j] for m in ms]
            if R[0] is None:                        # rhsNorm2 == 0: x = 0 and no iteration (LPcpp:262-266)
                if k != 0:
                    self.bad(it, f"PCG count {k} although the right-hand side is zero")
                continue
            for idx, low in ((k - 1, True), (k, False)):
                if idx < 0 or (not low and k >= nat.pcg_maxiters):
                    continue
                A = np.array([float(r[idx]) for r in R])
                B = c * (A.max() - A.min()) + _floor(A[:1])
                if low and not A[0] >= 1 - B:
                    self.bad(it, f"PCG ran {k} iterations but residual ratio after {idx} is {A[0]:.6g} < 1 - {B:.3e}")
                if not low and not A[0] < 1 + B:
                    self.bad(it, f"PCG stopped after {k} iterations but residual ratio is {A[0]:.6g} >= 1 + {B:.3e}")


def run_cases(group, cases, steps):
    """Drive every case of one handle through `steps` in lock-step; a case that stopped is parked."""
    for st in steps:
        active = [not c.done for c in cases]
        if not any(active):
            break
        fixes = [c.before(st) if on else (np.zeros(0), 0) for c, on in zip(cases, active)]
        rets = group.run(st["a"], st["e"], fixes, active, st["plain"])
        for c, r, on in zip(cases, rets, active):
            if on:
                c.after(st, r)
    return cases


def assert_clean(cases, ceiling=None):
    """No violation, and the weak-iteration cap: at most a quarter of a case's checked iterations may have B(x) > 1e-4.

    Instances with stored values: the cap is asserted on the iterations after the fix, and on the ones before it wherever it holds.
    Where it does not -- the PCG of a valued instance runs long enough before the first fix for the restatement's own roundings to
    part by more than 1e-4 -- `ceiling` {tag: count} records how many such iterations the case has, and no more are accepted, so the
    figure cannot drift (DESIGN.md section 22 lists them as a blind spot); every iteration is held to B either way."""
    bad = [m for c in cases for m in c.violations]
    assert not bad, "\n".join(bad[:20])
    for c in cases:
        assert c.checked > 0 or (c.stop_at or (0, None))[1] == "all_fixed", c.tag
        if not c.valued:
            assert 4 * c.weak <= c.checked, f"{c.tag}: {c.weak} of {c.checked} iterations have B(x) > {WEAK}"
            continue
        assert 4 * c.post[1] <= c.post[0], f"{c.tag}: after the fix {c.post[1]} of {c.post[0]} iterations have B(x) > {WEAK}"
        allowed = max(c.pre[0] // 4, (ceiling or {}).get(c.tag, 0))
        assert c.pre[1] <= allowed, f"{c.tag}: before the fix {c.pre[1]} of {c.pre[0]} iterations have B(x) > {WEAK}, recorded ceiling {allowed}"
