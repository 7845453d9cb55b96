"""The C oracle of the LP path, in every configuration the kernels are held to, against the independent numpy restatement, one outer
iteration at a time (tests/lp_steplock.py).  CPU only.

Windows, every iteration an l2f window of length 1 unless stated: iterations 0..74 without a fix (rho updates at 25 and 50, the gamma decay,
std_obj from iteration 10); then three continuations from the same state: a scripted fix at 75 where a rho update is pending (30
iterations), five more iterations and the same fix at 80 where none is pending (30 iterations), and the all-fixed call at 75.  The tiny
instances stop before 75 and are followed to their stop.  Plain solve_iter windows of length 1 and 2 (z4 restarted at it_start, no stop
test in a window's first iteration) have a test of their own, and so have the mutants of the restatement that the bound must catch."""
import functools

import numpy as np
import pytest

import lp_steplock as S
from helpers import STEPLOCK_C, STEPLOCK_C_VALUED, lp_instances
from oracle import oracle as O
from oracle.lpbox_numpy import MUTANTS
from valued_cases import FAMILIES, valued

FUZZ = S.FUZZ
GENERATOR = {"gen100_0": ("lp_100_500_seed0.npz", 0), "gen100_2": ("lp_100_500_seed0.npz", 2), "gen20_1": ("lp_20_60_seed0.npz", 1)}
CASES = tuple(GENERATOR) + tuple(k for k, v in FUZZ.items() if v[2] <= 513)
UNIT_CONFIGS = {"eigen": dict(order=O.ORDER_EIGEN), "gpu512": dict(order=O.ORDER_GPU, T=512),
                "gpu256c512": dict(order=O.ORDER_GPU, T=256, chunk=512),          # the large route's two-level tree
                "ranks2": dict(order=O.ORDER_GPU, T=256, chunk=512, ranks=2),
                "lean": dict(order=O.ORDER_GPU, T=256, chunk=512),                # + set_pcg_lean: the same algebra in another rounding
                "direct": dict(order=O.ORDER_EIGEN, x_update="direct")}


@functools.lru_cache(maxsize=None)
def instance(name):
    if name in GENERATOR:
        return lp_instances(GENERATOR[name][0])[GENERATOR[name][1]]
    return S.fuzz_instance(name)


def oracle(I, cfg):
    o = O.LpOracle(0, **UNIT_CONFIGS[cfg])
    if cfg == "lean":
        o.set_pcg_lean(True, 512)
    o.set_problem(I["n"], I["l"], I["colptr"], I["rowidx"], I["b"], I.get("f"), I.get("vals"))
    o.solve_init()
    return o


def run_all_windows(I, cfg, tag, mutant=None, forks=("fix75", "fix80", "all")):
    """The windows of the module docstring; returns the cases [main, fix at 75, fix at 80, all fixed] (main alone if it stopped early)."""
    xu = "direct" if cfg == "direct" else "pcg"

    def subject(upto):
        o = oracle(I, cfg)
        for it in range(upto):
            o.solve_iter_l2f(it, it + 1, np.zeros(I["n"]), 0)
        return o
    o = subject(0)
    main = S.Case(I, S.OracleSubject(o), tag, x_update=xu, mutant=mutant)
    S.run_cases(S.OracleGroup([o]), [main], S.l2f_steps(0, 75))
    out = [main]
    if main.done:
        return out
    for name, steps in (("fix75", S.l2f_steps(75, 105, "scripted")), ("fix80", S.l2f_steps(75, 80) + S.l2f_steps(80, 110, "scripted")),
                        ("all", S.l2f_steps(75, 76, "all"))):
        if name in forks:
            o2 = subject(75)
            c = main.fork(S.OracleSubject(o2), f"{tag} {name}")
            S.run_cases(S.OracleGroup([o2]), [c], steps)
            assert c.fixed > 0, f"{c.tag}: the scripted fix did not fire"
            out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def eigen_run(case):
    return run_all_windows(instance(case), "eigen", case)


def check(cases, ceiling=None):
    for c in cases:
        print(f"{c.tag}: checked {c.checked}, weak {c.weak} (before the fix {c.pre[1]} of {c.pre[0]}, after {c.post[1]} of {c.post[0]}), "
              f"subject/spread {c.worst:.2f}, leave-one-out {c.loo:.2f}, stop {c.stop_at}")
    S.assert_clean(cases, ceiling)
    allfixed = [c for c in cases if c.tag.endswith(" all")]
    assert all(c.stop_at[1] == "all_fixed" and c.view.n() == 0 for c in allfixed)


@pytest.mark.parametrize("case", CASES)
def test_eigen_order_oracle_every_window(case):
    check(eigen_run(case))


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("cfg", ["gpu512", "gpu256c512", "ranks2", "lean"])
def test_kernel_order_oracles_every_window(cfg, case):
    check(run_all_windows(instance(case), cfg, f"{cfg} {case}", forks=("fix75", "all")))


VALUED_CASES = ("gen100_0", "gen20_1", "empty_rows_65")
# iterations with B(x) > 1e-4 before the first fix, where they exceed a quarter (tag -> recorded count; see assert_clean)
VALUED_WEAK = {"set gen100_0": 43, "set gen100_0 fix80": 5, "set gen20_1": 20, "set empty_rows_65": 59,
               "uniform gen100_0": 27, "uniform gen20_1": 48, "uniform gen20_1 fix80": 5, "uniform empty_rows_65": 73,
               "uniform empty_rows_65 fix80": 5}


@functools.lru_cache(maxsize=None)
def valued_run(family, case):
    return run_all_windows(valued(instance(case), family, 0), "eigen", f"{family} {case}")


@pytest.mark.parametrize("case", VALUED_CASES)
@pytest.mark.parametrize("family", FAMILIES)
def test_stored_values_every_window(family, case):
    """Every iteration is held to B (with the valued c).  The weak-iteration cap is asserted after every fix, and before the first fix
    wherever it holds; where it does not (the PCG of a valued instance runs long before the first fix, and the restatement's own
    roundings part), the recorded count in VALUED_WEAK is a ceiling: the check has little power in those iterations, a blind spot that
    DESIGN.md section 22 lists, and it may not grow."""
    check(valued_run(family, case), VALUED_WEAK)


def test_calibration_of_c_valued():
    """The same calibration on the nine valued cases: single members stray much further from the others than on unit instances, so the
    valued checks carry a c of their own, twice the worst ratio (helpers.STEPLOCK_C_VALUED)."""
    worst = {(f, case): max(c.loo for c in valued_run(f, case)) for f in FAMILIES for case in VALUED_CASES}
    print({k: round(v, 2) for k, v in worst.items()})
    assert max(worst.values()) <= STEPLOCK_C_VALUED / 2


@pytest.mark.parametrize("case", ["gen20_1", "empty_rows_65", "heavy_empty_65", "heavy_row_3", "one_entry_cols_5", "dup_cols_5"])
def test_direct_x_update_every_window(case):
    """No PCG count to force: the restatement's x-update is its plain dense solve."""
    check(run_all_windows(instance(case), "direct", f"direct {case}"))


def test_direct_x_update_500_variables():
    check(run_all_windows(instance("gen100_0"), "direct", "direct gen100_0", forks=("fix75",)))


def test_tiny_instances_stop_where_the_restatement_stops():
    """n = 3 and n = 5 followed to their stop: iteration and reason are the restatement's own decision (compared exactly by the harness),
    and both stop rules are reached."""
    seen = {}
    for case in ("heavy_row_3", "one_entry_cols_5", "dup_cols_5"):
        for cfg in ("eigen", "gpu512"):
            (c,) = eigen_run(case) if cfg == "eigen" else run_all_windows(instance(case), cfg, f"{cfg} {case}")
            assert not c.violations and c.done and c.stop_at is not None, c.tag
            assert c.view.stop() == S.STOP_CODE[c.stop_at[1]] and c.view.totals()[0] == c.stop_at[0] + 1
            seen.setdefault(case, set()).add(c.stop_at)
    assert seen == {"heavy_row_3": {(35, "obj_std")}, "one_entry_cols_5": {(45, "y1_y2")}, "dup_cols_5": {(49, "y1_y2")}}


PLAIN = [("eigen", c) for c in ("gen100_0", "gen100_2", "gen20_1", "heavy_row_257", "heavy_empty_65", "one_entry_cols_5")] + \
        [("gpu512", "gen20_1"), ("gpu512", "heavy_empty_65")]


@pytest.mark.parametrize("cfg,case", PLAIN)
def test_plain_windows_of_length_one_and_two(cfg, case):
    """Among l2f steps over iterations 0..79, a solve_iter window of length 1 at iteration 25 and one of length 2 at 50 (a rho update is
    pending at both): such a window restarts z4 and skips the residual stop test in its first iteration; the window of two is replayed as
    two iterations of the restatement with the counts from the subject's PCG totals.  (Every restart of z4 brings back a few of the
    ill-conditioned iterations of the start, so the plain windows are few: the weak-iteration cap holds for these runs as well.)"""
    I = instance(case)
    o = oracle(I, cfg)
    plain = lambda a, ln: [dict(a=a, e=a + ln, plain=True, fix=None)]
    steps = S.l2f_steps(0, 25) + plain(25, 1) + S.l2f_steps(26, 50) + plain(50, 2) + S.l2f_steps(52, 80)
    c = S.Case(I, S.OracleSubject(o), f"plain {cfg} {case}")
    S.run_cases(S.OracleGroup([o]), [c], steps)
    check([c])
    assert c.done or (c.checked == len(steps) and o.total_outer_iters == 80)


@pytest.mark.parametrize("n,ranks", [(9000, 1), (17000, 2)])
def test_second_level_with_more_partials_than_threads(n, ranks):
    """The oracle's two-level order with MORE workgroup partials than threads (redux_sum_gpu_full(part, Gn, T) with Gn > T): T = 64 and
    chunks of 64 positions give a rank more than 128 partials, so every thread of the second level adds up to three of them (t, t + 64,
    t + 128) before the tree -- the multi-slot loop that the large route's kernels run above 256 workgroups.  Iterations 0..29 (the rho
    update at 25), the bound of the unit cases."""
    from lpbox_hip.synth import make_auction_like
    I = make_auction_like(n, 1)
    per_rank = -(-n // ranks)
    assert 128 < -(-per_rank // 64) <= 192                      # three slots per thread, the third partly filled
    o = O.LpOracle(0, order=O.ORDER_GPU, T=64, chunk=64, ranks=ranks)
    o.set_problem(I["n"], I["l"], I["colptr"], I["rowidx"], I["b"])
    o.solve_init()
    c = S.Case(I, S.OracleSubject(o), f"gpu64c64 ranks{ranks} auction{n}")
    assert c.c == STEPLOCK_C
    S.run_cases(S.OracleGroup([o]), [c], S.l2f_steps(0, 30))
    check([c])
    assert c.checked == 30 and not c.done and o.total_outer_iters == 30


def test_calibration_of_c():
    """c is calibrated on the restatement alone: the distance of every float64 permuted member from the natural member, over the spread of
    the other eleven; the worst over all named cases must stay below c / 2 (helpers.STEPLOCK_C)."""
    worst = {case: max(c.loo for c in eigen_run(case)) for case in CASES}
    print({k: round(v, 2) for k, v in worst.items()})
    assert max(worst.values()) <= STEPLOCK_C / 2


# mutant -> (case, values family or None): the input on which the bound must catch it
MUTANT_INPUT = {"pd_rho4": ("gen20_1", None), "drop_pending": ("gen20_1", None), "gamma_late": ("gen20_1", None),
                "z4_restart_l2f": ("gen20_1", None), "y3_noclamp": ("gen20_1", None), "sphere_org_n": ("gen20_1", None),
                "esq_count": ("gen20_1", "uniform")}


@pytest.mark.parametrize("mutant", MUTANTS)
def test_bound_catches_mutant_of_the_restatement(mutant):
    """Sensitivity: with the unchanged oracle as subject, a restatement with one misread expression must leave the bound on an ITERATE
    (x, z1, z2, z4) somewhere in the windows -- and the unmutated restatement must not, on the same input."""
    case, family = MUTANT_INPUT[mutant]
    I = instance(case) if family is None else valued(instance(case), family, 0)
    good = run_all_windows(I, "eigen", f"{case}")
    assert not [m for c in good for m in c.violations]
    bad = [m for c in run_all_windows(I, "eigen", f"{mutant} {case}", mutant=mutant) for m in c.violations]
    print("\n".join(bad[:3]))
    assert any(any(f" {v}: |subject" in m for v in S.VECS) for m in bad), f"{mutant} not caught"
