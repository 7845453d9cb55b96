"""GPU tests of the PCG halt-and-resume path of the segmentation and generic-BQP launch chains (chain_run in csrc/lpbox_host.h with the
operations of csrc/lpbox_seg_capi.hip and csrc/lpbox_gen_capi.hip, chain_run_lockstep with SegBatchOps for a batch): an outer iteration
enqueues kmax (matvec, update) pairs; a PCG that needs more halts the chain from `post`, every launch behind the halt falls through, and the host enqueues
resume + 16 pairs + post.  The problems (tests/chain_cases.py, pinned on the CPU by tests/test_chain_resume_cases.py) need up to 44 and
1000 PCG iterations, and LPBOX_SEG_KMAX / LPBOX_BQP_KMAX force the launch count down to 1.

Reference in every test: the C oracle in the kernels' order, bit for bit (iterates, x, z1, z2, b, scalars, counters, stop codes,
energies); where the PCG counts of the restatement agree, also the numpy restatement within B (helpers.spread_bound).  With a fixed
kmax = k the number of resumes is exact: sum of ceil((K_i - k) / 16) over the oracle's PCG counts K_i > k.

Run as a script (`python test_chain_resume_gpu.py OUT.npy`) the file runs S1 at kmax = 2 and the batched legacy solve and writes
every result to OUT: the statics test starts it in fresh child processes with LPBOX_SEG_NOGRAPH and LPBOX_SEG_KMARGIN set (they
used to be read once per process; now every handle and every batch reads them when it is created)."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    _ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_ROOT, os.path.join(_ROOT, "accelerated-lpbox-admm_amd")]

from chain_cases import (SEG_FIX_AFTER, SEG_FIXED, SEG_LEGACY, bqp_case, bqp_case_params, expected_resumes, oracle_windows, seg_case,
                         seg_oracle)
from helpers import BQP_SCALARS, assert_within_bound, bits_equal, scripted_fix_vec
from oracle import oracle as O
from oracle.bqp_numpy import NumpyBqp
from seg_harness import SCALARS, solver, trio, windows

pytestmark = pytest.mark.gpu

VECS = ("x", "z1", "z2", "b")
BATCH = ("S1", "S2", "S3", "S4")


def resumes(g):
    return int(g.debug_scalar("pcg_resumes"))


def plain(P):
    """A handle holding P, not initialised (the members of a batch)."""
    from lpbox_hip.seg import PyLPboxADMMsolver
    s = PyLPboxADMMsolver(0, P["n"], 0)
    s.write_files = False
    s.set_problem(P)
    return s


def oracle_of(g):
    cfg = g.config()
    assert (cfg["threads"], cfg["elems_per_thread"]) == (256, 2)              # the order the cached oracle results below are computed in
    return seg_oracle(g.get_problem())


@functools.lru_cache(None)
def trace30(name, fix_after):
    """The oracle's PCG counts over three windows of 10 (kernel order, T = 256, chunk = 512) with the case's scripted fix."""
    trace, fixed, _ = oracle_windows(seg_oracle(seg_case(name)), [10, 10, 10], fix_after)
    return tuple(int(k) for k in trace), fixed


@functools.lru_cache(None)
def oracle_legacy(name):
    o = seg_oracle(seg_case(name))
    energy = o.solve_iter()
    return dict(energy=energy, counters=(o.total_outer_iters, o.total_pcg_iters), stop=(o.last_stop, o.legacy_iter_plus1), obj=o.get_obj(),
                x_sol=o.get_x_sol(), x=o.vec("x"), scalars={s: o.scalar(s) for s in SCALARS}, trace=tuple(int(k) for k in o.pcg_trace()))


def same_as_oracle_state(g, o, tag):
    assert g.get_n() == o.get_n() and g.counters() == (o.total_outer_iters, o.total_pcg_iters), tag
    left = o.vec("left_idx").astype(int)
    for name in VECS:
        assert bits_equal(g.debug_vec(name)[left], o.vec(name)), f"{tag}: {name}"
    for name in SCALARS:
        assert g.debug_scalar(name) == o.scalar(name), f"{tag}: {name}"


def same_as_oracle_legacy(g, energy, name, tag):
    ref = oracle_legacy(name)
    assert (ref["energy"],) + ref["counters"] == SEG_LEGACY[name]
    assert energy == ref["energy"] and g.counters() == ref["counters"] and g.stop() == ref["stop"], tag
    if name in ("S1", "S2"):            # integer data: get_obj sums integers, in any order (the host getter sums S3's and S4's in its own)
        assert g.get_obj() == ref["obj"], tag
    assert np.array_equal(g.get_x_sol(), ref["x_sol"]) and bits_equal(g.debug_vec("x"), ref["x"]), tag
    for s in SCALARS:
        assert g.debug_scalar(s) == ref["scalars"][s], f"{tag}: {s}"


# ---- segmentation, one handle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kmax", [1, 2, 4])
def test_s1_three_windows_with_a_forced_launch_count(monkeypatch, kmax):
    """Every iteration of S1 (9 ... 5 PCG iterations) halts: once per iteration, with the fix after window 0 in between."""
    monkeypatch.setenv("LPBOX_SEG_KMAX", str(kmax))
    g = solver(seg_case("S1"))
    assert g.debug_scalar("matrix_as_diagonals") == 1.0 and g.debug_scalar("kmax") == kmax and resumes(g) == 0
    o, e, r = trio(g)
    assert windows(g, o, e, r, 3, fix_after=0, tag=f"S1 kmax {kmax}") == SEG_FIXED["S1"]
    trace, _ = trace30("S1", 0)
    assert resumes(g) == expected_resumes(trace, kmax) == 30 and g.debug_scalar("kmax") == kmax


@pytest.mark.parametrize("name", ["S2", "S3"])
def test_adaptive_chain_resumes_and_goes_on(name):
    """No knob: the chain starts at kmax = 10.  S2's iteration 0 needs 44 pairs (10 + 16 + 16 < 44: at least two resumes in a row) and
    drives kmax into its clamp of 24, which S2 goes on exceeding; S3's needs 18 (one resume)."""
    P = seg_case(name)
    g = solver(P)
    assert g.debug_scalar("matrix_as_diagonals") == (1.0 if name == "S2" else 0.0) and g.debug_scalar("kmax") == 10
    o = oracle_of(g)
    assert g.solve_iter_l2f(0, 1, np.zeros(P["n"]), 0) == o.solve_iter_l2f(0, 1, np.zeros(P["n"]), 0) == 0
    assert bits_equal(g.get_x_iters_2d(1), o.get_x_iters_2d(1))
    same_as_oracle_state(g, o, f"{name} iteration 0")
    print(f"{name} adaptive: pcg_resumes after iteration 0 = {resumes(g)}, kmax = {g.debug_scalar('kmax')}")
    if name == "S2":
        assert resumes(g) >= 2 and g.debug_scalar("kmax") == 24
    else:
        assert resumes(g) >= 1
    g = solver(P)
    o, e, r = trio(g)
    assert windows(g, o, e, r, 3, fix_after=1, tag=f"{name} adaptive") == SEG_FIXED[name]
    print(f"{name} adaptive: pcg_resumes after 30 iterations = {resumes(g)}, kmax = {g.debug_scalar('kmax')}")
    assert resumes(g) > 0
    if name == "S2":
        assert g.debug_scalar("kmax") == 24


@pytest.mark.parametrize("name", ["S2", "S3"])
def test_s2_s3_with_one_pair_per_iteration(monkeypatch, name):
    monkeypatch.setenv("LPBOX_SEG_KMAX", "1")
    P = seg_case(name)
    trace, _ = trace30(name, 1)
    g = solver(P)
    o = oracle_of(g)
    assert g.solve_iter_l2f(0, 1, np.zeros(P["n"]), 0) == o.solve_iter_l2f(0, 1, np.zeros(P["n"]), 0) == 0
    assert bits_equal(g.get_x_iters_2d(1), o.get_x_iters_2d(1))
    assert resumes(g) == expected_resumes(trace[:1], 1) == (3 if name == "S2" else 2)
    g = solver(P)
    o, e, r = trio(g)
    assert windows(g, o, e, r, 3, fix_after=1, tag=f"{name} kmax 1") == SEG_FIXED[name]
    assert resumes(g) == expected_resumes(trace, 1) and g.debug_scalar("kmax") == 1


def test_s5_every_iteration_ends_at_the_pcg_cap():
    """1000 PCG iterations three times.  From kmax = 10 the cap is met inside a resume's pairs (986 + 14); iterations 1 and 2 run at the
    clamp, 24 + 61 * 16 = 1000: there the `pcg_k >= SEG_PCG_MAXITERS` arm of the pending exit test in `post` ends the PCG."""
    P = seg_case("S5")
    g = solver(P)
    assert g.debug_scalar("matrix_as_diagonals") == 0.0 and g.debug_scalar("ell_width") == 9
    o = oracle_of(g)
    assert g.solve_iter_l2f(0, 3, np.zeros(P["n"]), 0) == o.solve_iter_l2f(0, 3, np.zeros(P["n"]), 0)
    assert list(o.pcg_trace()) == [1000, 1000, 1000]
    assert bits_equal(g.get_x_iters_2d(3), o.get_x_iters_2d(3))
    same_as_oracle_state(g, o, "S5")
    print(f"S5: counters {g.counters()}, pcg_resumes {resumes(g)}, kmax {g.debug_scalar('kmax')}")
    assert g.counters() == (3, 3000)
    assert resumes(g) > 0 and g.debug_scalar("kmax") == 24


def test_window_lengths_with_two_pairs_per_iteration(monkeypatch):
    """Consecutive windows of 1 and 3 (eager launches only), 4 (one graph), 7 (graph and eager tail), a fix, 10 and 5: a halt lands in
    every one of them, also in the last iteration of a window."""
    monkeypatch.setenv("LPBOX_SEG_KMAX", "2")
    P = seg_case("S1")
    g = solver(P)
    o = oracle_of(g)
    lengths, fix_after = [1, 3, 4, 7, 10, 5], 3
    vec, num, it, trace, before = np.zeros(P["n"]), 0, 0, [], 0
    for w, ws in enumerate(lengths):
        tag = f"window {w} of {ws}"
        assert g.solve_iter_l2f(it, it + ws, vec, num) == o.solve_iter_l2f(it, it + ws, vec, num) == 0, tag
        it += ws
        xg, xo = g.get_x_iters_2d(ws), o.get_x_iters_2d(ws)
        assert bits_equal(xg, xo), f"{tag}: max diff {np.abs(xg - xo).max():.3e}"
        same_as_oracle_state(g, o, tag)
        trace += [int(k) for k in o.pcg_trace()]
        print(f"{tag}: PCG counts {trace[-ws:]}, pcg_resumes {resumes(g)}")
        assert len(trace) == it and resumes(g) == expected_resumes(trace, 2) and resumes(g) > before, tag
        before = resumes(g)
        vec, num = scripted_fix_vec(xo, lo=0.05, hi=0.95, last=5) if w == fix_after else (np.zeros(g.get_n()), 0)
        assert (num > 0) == (w == fix_after)
    assert g.get_n() < P["n"]


def legacy(g, record=False):
    from lpbox_hip.seg import check
    check(g._L.lpbox_set_record(g._h, 1 if record else 0), "lpbox_set_record")
    e = ctypes.c_int()
    check(g._L.lpbox_seg_legacy(g._h, ctypes.byref(e)), "lpbox_seg_legacy")
    return e.value


@pytest.mark.parametrize("name,kmax", [("S1", 1), ("S2", 1), ("S2", None)])
def test_legacy_solve_to_convergence(monkeypatch, name, kmax):
    if kmax:
        monkeypatch.setenv("LPBOX_SEG_KMAX", str(kmax))
    g = solver(seg_case(name))
    same_as_oracle_legacy(g, g.solve_iter(), name, f"{name} kmax {kmax}")
    print(f"{name} kmax {kmax}: pcg_resumes = {resumes(g)}, kmax after = {g.debug_scalar('kmax')}")
    if kmax:
        assert resumes(g) == expected_resumes(oracle_legacy(name)["trace"], kmax)
    else:
        assert resumes(g) >= 2


def test_recorded_columns_around_the_resumes(monkeypatch):
    """S1's legacy solve with recording on: 548 recorded iterates, the same bits with one pair per iteration (a halt before every
    column is written) as on a handle without the knob; the first ten are the oracle's first window."""
    free = solver(seg_case("S1"))
    monkeypatch.setenv("LPBOX_SEG_KMAX", "1")
    forced = solver(seg_case("S1"))
    assert (free.debug_scalar("kmax"), forced.debug_scalar("kmax")) == (10, 1)
    ef, ek = legacy(free, record=True), legacy(forced, record=True)
    same_as_oracle_legacy(forced, ek, "S1", "recorded, kmax 1")
    same_as_oracle_legacy(free, ef, "S1", "recorded, no knob")
    hf, hk = free.x_history(), forced.x_history()
    assert hf.shape == hk.shape == (SEG_LEGACY["S1"][1], 480) and bits_equal(hk, hf)
    assert resumes(forced) == expected_resumes(oracle_legacy("S1")["trace"], 1) and resumes(free) == 0
    _, _, out = oracle_windows(seg_oracle(seg_case("S1")), [10])
    assert bits_equal(hk[:10].T, out[0][1])
    assert bits_equal(hk[-1], forced.debug_vec("x"))                            # the last column is the last iterate


# ---- segmentation, batches: one problem halts while the others run on ---------------------------------------------------------------
def batch_legacy(monkeypatch, kmax):
    """(members after solve_batch, their energies, unforced single handles after their own solve, their energies)"""
    from lpbox_hip.seg import solve_batch
    single = [solver(seg_case(n)) for n in BATCH]
    es = [s.solve_iter() for s in single]
    if kmax and monkeypatch is not None:
        monkeypatch.setenv("LPBOX_SEG_KMAX", str(kmax))
    batch = [plain(seg_case(n)) for n in BATCH]
    return batch, solve_batch(batch), single, es


@pytest.mark.parametrize("kmax", [None, 2])
def test_batched_legacy_with_one_member_far_behind(monkeypatch, kmax):
    """S4 never needs more than 4 pairs, S2 up to 44: S2 halts and is resumed while the launches of the others fall through."""
    batch, en, single, es = batch_legacy(monkeypatch, kmax)
    assert [s.debug_scalar("matrix_as_diagonals") for s in batch] == [1.0, 1.0, 0.0, 0.0]
    for k, name in enumerate(BATCH):
        s, t = batch[k], single[k]
        assert en[k] == es[k] and s.get_obj() == t.get_obj() and s.counters() == t.counters() and s.stop() == t.stop(), name
        assert np.array_equal(s.get_x_sol(), t.get_x_sol()) and bits_equal(s.debug_vec("x"), t.debug_vec("x")), name
        same_as_oracle_legacy(s, en[k], name, f"batch {name} kmax {kmax}")
        same_as_oracle_legacy(t, es[k], name, f"single {name}")
    got = [resumes(s) for s in batch]
    print(f"batch kmax {kmax}: pcg_resumes {got}")
    if kmax:
        assert got == [expected_resumes(oracle_legacy(n)["trace"], kmax) for n in BATCH]
    else:
        assert got[1] > 0 and got[3] == 0


@pytest.mark.parametrize("kmax", [None, 1])
def test_batched_windows_with_host_vectors(monkeypatch, kmax):
    """SegBatch over the four: three windows of 10, S1 fixes after window 0, S2 and S3 after window 1, S4 never.  Without the knob
    the launch count follows S2, the largest of the previous batch (never below 20), so S4 (at most 4) never halts -- also not at the
    start of a window whose predecessor ended on a resumed iteration of S2."""
    from lpbox_hip.seg import SegBatch
    if kmax:
        monkeypatch.setenv("LPBOX_SEG_KMAX", str(kmax))
    ss = [plain(seg_case(n)) for n in BATCH]
    B = SegBatch(ss)
    assert B.solve_init() == 1
    os_ = [oracle_of(s) for s in ss]
    nmax = max(s.get_org_n() for s in ss)
    vecs, nums, fixed = -np.ones((4, nmax)), np.zeros(4, np.int32), np.zeros(4, int)
    for w in range(3):
        rets = B.solve_iter_l2f(10 * w, 10 * w + 10, vecs, nums)
        for k, name in enumerate(BATCH):
            tag = f"window {w}, {name}"
            assert rets[k] == os_[k].solve_iter_l2f(10 * w, 10 * w + 10, vecs[k], int(nums[k])) == 0, tag
            fixed[k] += nums[k]
            xo = os_[k].get_x_iters_2d(10)
            assert bits_equal(ss[k].get_x_iters_2d(10), xo), tag
            same_as_oracle_state(ss[k], os_[k], tag)
            assert tuple(int(c) for c in os_[k].pcg_trace()) == trace30(name, SEG_FIX_AFTER[name])[0][10 * w:10 * w + 10], tag
            nums[k] = 0
            if SEG_FIX_AFTER[name] == w:
                v, n = scripted_fix_vec(xo, lo=0.05, hi=0.95, last=5)
                vecs[k, :len(v)], nums[k] = v, n
    assert list(fixed) == [SEG_FIXED["S1"], SEG_FIXED["S2"], SEG_FIXED["S3"], 0]
    got = [resumes(s) for s in ss]
    print(f"SegBatch kmax {kmax}: pcg_resumes {got}")
    if kmax:
        assert got == [expected_resumes(trace30(n, SEG_FIX_AFTER[n])[0], kmax) for n in BATCH]
    else:
        assert got[1] > 0 and got[3] == 0
    B.close()


# ---- statics, in fresh child processes -----------------------------------------------------------------------------------------------
def payload():
    """S1 at kmax = 2 through three windows with its fix, then the batched legacy solve under the environment as it stands.
    Returns (every result as one float64 array, pcg_resumes of S1 and of the four members)."""
    saved = os.environ.get("LPBOX_SEG_KMAX")
    os.environ["LPBOX_SEG_KMAX"] = "2"
    try:
        g = solver(seg_case("S1"))
    finally:
        if saved is None:
            del os.environ["LPBOX_SEG_KMAX"]
        else:
            os.environ["LPBOX_SEG_KMAX"] = saved
    parts = []
    vec, num = np.zeros(g.get_org_n()), 0
    for w in range(3):
        ret = g.solve_iter_l2f(10 * w, 10 * w + 10, vec, num)
        x = g.get_x_iters_2d(10)
        parts += [np.array([ret, g.get_n()], np.float64), x.ravel()] + [g.debug_vec(v) for v in VECS]
        parts.append(np.array([g.debug_scalar(s) for s in SCALARS] + list(g.counters()), np.float64))
        vec, num = scripted_fix_vec(x, lo=0.05, hi=0.95, last=5) if w == 0 else (np.zeros(g.get_n()), 0)
    res = [resumes(g)]
    from lpbox_hip.seg import solve_batch
    batch = [plain(seg_case(n)) for n in BATCH]
    en = solve_batch(batch)
    for s, e in zip(batch, en):
        parts += [np.array([e, s.get_obj()] + list(s.counters()) + list(s.stop()) + [s.debug_scalar(n) for n in SCALARS], np.float64),
                  s.get_x_sol().ravel(), s.debug_vec("x")]
        res.append(resumes(s))
    return np.concatenate(parts), np.array(res, np.float64)


@functools.lru_cache(None)
def payload_here(kmax):
    saved = os.environ.get("LPBOX_SEG_KMAX")
    if kmax:
        os.environ["LPBOX_SEG_KMAX"] = str(kmax)
    try:
        return payload()
    finally:
        if saved is None:
            os.environ.pop("LPBOX_SEG_KMAX", None)
        else:
            os.environ["LPBOX_SEG_KMAX"] = saved


def _child(out):
    data, res = payload()
    np.save(out, np.concatenate([data, res]))


@pytest.mark.parametrize("setting", ["nograph", "kmargin2", "nograph_kmargin2_kmax2"])
def test_results_do_not_depend_on_graphs_or_margin(tmp_path, setting):
    """The same runs in a fresh process with eager launches, with two spare pairs per iteration, and with both under a forced kmax = 2:
    the same bits; the same resumes wherever the launch count is the same."""
    assert not any(os.environ.get(k) for k in ("LPBOX_SEG_NOGRAPH", "LPBOX_SEG_KMARGIN", "LPBOX_SEG_KMAX"))
    env = dict(os.environ)
    if "nograph" in setting:
        env["LPBOX_SEG_NOGRAPH"] = "1"
    if "kmargin2" in setting:
        env["LPBOX_SEG_KMARGIN"] = "2"
    forced = 2 if "kmax2" in setting else None
    if forced:
        env["LPBOX_SEG_KMAX"] = "2"
    want, want_res = payload_here(forced)
    out = str(tmp_path / f"{setting}.npy")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.load(out)
    got, got_res = got[:-5], got[-5:]
    assert bits_equal(got, want)
    print(f"{setting}: pcg_resumes child {list(got_res)}, here {list(want_res)}")
    assert got_res[0] == want_res[0] == 30                                      # S1 at kmax = 2: forced in every process
    if setting == "kmargin2":
        assert got_res[2] > 0                                                   # S2 still resumes with two spare pairs
    else:
        assert np.array_equal(got_res, want_res)
    if forced:
        assert list(got_res[1:]) == [expected_resumes(oracle_legacy(n)["trace"], 2) for n in BATCH]


# ---- generic BQP ------------------------------------------------------------------------------------------------------------------------
def bqp_hip(P, params):
    from lpbox_hip.bqp import BqpSolver
    g = BqpSolver(P["n"], P["A"], P["b"], P["x0"], P.get("C"), P.get("d"), P.get("E"), P.get("f"), params=params)
    return g, g.solve()


def bqp_names(P):
    return ["x", "y1", "y2", "z1", "z2", "best_sol"] + (["z3"] if P.get("C") is not None else []) + (["z4", "y3"] if P.get("E") is not None else [])


def bqp_check(name, params, tag):
    """The case under `params` on the GPU: bit for bit the oracle in the kernels' order; the oracle's PCG trace and the solver."""
    P, _ = bqp_case(name)
    g, it_g = bqp_hip(P, params)
    assert (g.scalar("threads"), g.scalar("chunk")) == (256, 512)
    o = O.BqpOracle(P, params=params, order=O.ORDER_GPU, T=256, chunk=512)
    it_o = o.solve()
    assert it_g == it_o and g.scalar("stop") == o.scalar("stop") and g.scalar("total_pcg") == o.scalar("total_pcg"), tag
    for v in bqp_names(P):
        assert bits_equal(g.vec(v), o.vec(v)), f"{tag} {v}: max diff {np.abs(g.vec(v) - o.vec(v)).max():.3e}"
    for s in BQP_SCALARS:
        assert g.scalar(s) == o.scalar(s), f"{tag} {s}"
    return g, o


def bqp_within_restatement(name, params, g, o, tag):
    """The PCG counts of the restatement and of both oracle orders agree over all iterations: the final state within B."""
    P, _ = bqp_case(name)
    e = O.BqpOracle(P, params=params)
    e.solve()
    r = NumpyBqp(P, params=params)
    r.solve(record=True)
    assert list(o.pcg_trace()) == list(e.pcg_trace()) == [int(k) for k in r.pcg], tag
    snap = r.trace[len(r.pcg) - 1]
    for v in bqp_names(P):
        assert_within_bound(g.vec(v), snap[v], e.vec(v), o.vec(v), f"{tag} {v}")
    for s in BQP_SCALARS:
        assert_within_bound(g.scalar(s), snap[s], e.scalar(s), o.scalar(s), f"{tag} {s}")


@pytest.mark.parametrize("name,kmax", [("G0", 1), ("G1", 1), ("G1", 3), ("G2", 1), ("G2", 3), ("G3", 1), ("G3", 3)])
def test_bqp_with_a_forced_launch_count(monkeypatch, name, kmax):
    monkeypatch.setenv("LPBOX_BQP_KMAX", str(kmax))
    params = bqp_case_params(name)
    g, o = bqp_check(name, params, f"{name} kmax {kmax}")
    bqp_within_restatement(name, params, g, o, f"{name} kmax {kmax}")
    want = expected_resumes(o.pcg_trace(), kmax)
    assert g.scalar("pcg_resumes") == want and g.scalar("kmax") == kmax and g.scalar("iters") == 30
    assert want == 30                                                           # every iteration halts once


@pytest.mark.parametrize("name", ["G1", "G2", "G3"])
def test_bqp_pcg_capped_while_halted(monkeypatch, name):
    """pcg_maxiters = 5 with two launch groups per iteration: every PCG halts at k = 2 and meets its cap inside the resume."""
    monkeypatch.setenv("LPBOX_BQP_KMAX", "2")
    g, o = bqp_check(name, bqp_case_params(name, pcg_maxiters=5), f"{name} capped")
    assert list(o.pcg_trace()) == [5] * 30
    assert g.scalar("pcg_resumes") == 30 and g.scalar("total_pcg") == 150 and g.scalar("iters") == 30


def test_bqp_adaptive_chain_on_g4(monkeypatch):
    """No knob: the chain starts at kmax = 12 and G4's iteration 0 needs 31 launch groups (12 + 16 < 31: two resumes in a row); the
    counts then fall from 31 to 18, so the graph cache is asked for several kmax.  The same bits with eager launches."""
    g1, o1 = bqp_check("G4", bqp_case_params("G4", K=1), "G4 iteration 0")
    print(f"G4 adaptive: pcg_resumes after iteration 0 = {g1.scalar('pcg_resumes')}, kmax = {g1.scalar('kmax')}")
    assert list(o1.pcg_trace()) == [31] and g1.scalar("pcg_resumes") >= 2
    params = bqp_case_params("G4")
    g, o = bqp_check("G4", params, "G4 adaptive")
    bqp_within_restatement("G4", params, g, o, "G4 adaptive")
    print(f"G4 adaptive: pcg_resumes after 30 iterations = {g.scalar('pcg_resumes')}, kmax = {g.scalar('kmax')}")
    assert g.scalar("pcg_resumes") >= 2
    monkeypatch.setenv("LPBOX_BQP_NOGRAPH", "1")
    h, _ = bqp_check("G4", params, "G4 adaptive, eager")
    P, _ = bqp_case("G4")
    for v in bqp_names(P):
        assert bits_equal(h.vec(v), g.vec(v)), v
    for s in BQP_SCALARS + ("iters", "stop", "total_pcg", "last_pcg", "outer_total", "pcg_resumes", "kmax", "launches"):
        assert h.scalar(s) == g.scalar(s), s


if __name__ == "__main__":
    _child(sys.argv[1])
