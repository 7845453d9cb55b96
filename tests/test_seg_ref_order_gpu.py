"""GPU tests of the reference summation order of the segmentation flavour (lpbox_seg_set_order, csrc/lpbox_seg_ref_kernels.hip;
DESIGN.md section 33).  Reference in every test: the C oracle in its EIGEN order (oracle.SegOracle(order=ORDER_EIGEN): redux_sum_eigen
over the compacted live vector), bit for bit on the iterate windows, x, z1, z2, b, every scalar but std_obj (sqrt for the reference's
pow(v, 1/2): within 2 ulps), the (outer, PCG) counters, return codes, live counts, energies and objectives.  The cases and their oracle
runs are in tests/seg_ref_cases.py, pinned on the CPU by tests/test_seg_ref_order_api.py.

Run as a script (`python test_seg_ref_order_gpu.py OUT.npy`) the file runs the two windows of the resume case on a reference-order
handle and writes the iterates and the resume count to OUT: the resume test starts it in fresh child processes with LPBOX_SEG_KMAX set."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    _ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_ROOT, os.path.join(_ROOT, "accelerated-lpbox-admm_amd")]

import seg_ref_cases as S
from helpers import bits_equal, scripted_scores
from oracle import oracle as O
from seg_harness import SCALARS

pytestmark = pytest.mark.gpu

E_BADARG, E_STATE, E_UNSUPPORTED = -2, -3, -7


def handle(P=None, order="reference", gray=None, nodes=None, init=True):
    from lpbox_hip.seg import PyLPboxADMMsolver
    g = PyLPboxADMMsolver(0, nodes or P["n"], 0)
    g.write_files = False
    if order != "default":
        g.set_order(order)
    if gray is not None:
        g.set_image(gray, nodes)
    else:
        g.set_problem(P)
    if init:
        assert g.solve_init() == 1
    return g


def ulps(a, b):
    a, b = np.array([a], np.float64).view(np.int64)[0], np.array([b], np.float64).view(np.int64)[0]
    return abs(int(a) - int(b))


def same_scalars(g, ref, tag):
    for name in SCALARS:
        got, want = g.debug_scalar(name), ref[name]
        if name == "std_obj":
            assert ulps(got, want) <= 2, f"{tag}: std_obj {got!r} vs {want!r}"
        else:
            assert bits_equal(np.array([got]), np.array([want])), f"{tag}: {name} {got!r} vs {want!r}"


def same_state(g, r, tag):
    assert g.get_n() == r["n"] and g.counters() == r["counters"], f"{tag}: n {g.get_n()} vs {r['n']}, counters {g.counters()} vs {r['counters']}"
    for name in S.VECS:
        assert bits_equal(g.debug_vec(name)[r["left"]], r["vecs"][name]), f"{tag}: {name}"
    same_scalars(g, r["scalars"], tag)


def replay(g, rec, tag, ws=10):
    """The windows of an oracle run (seg_ref_cases.run_windows) on the handle g, everything compared after every window."""
    for w, r in enumerate(rec):
        ret = g.solve_iter_l2f(ws * w, ws * w + ws, r["vec"], r["num"])
        assert ret == r["ret"], f"{tag} window {w}: ret {ret} vs {r['ret']}"
        xg = g.get_x_iters_2d(ws)
        assert xg.shape == r["x_iters"].shape, f"{tag} window {w}: {xg.shape}"
        if not bits_equal(xg, r["x_iters"]):
            bad = np.where((xg != r["x_iters"]).any(axis=0))[0]
            raise AssertionError(f"{tag} window {w}: first differing iteration {bad[0]}, max diff {np.abs(xg - r['x_iters'])[:, bad[0]].max():.3e}")
        if r["n"]:
            same_state(g, r, f"{tag} window {w}")
        else:
            assert g.get_n() == 0


# ---- l2f windows -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.L2F_CASES)
def test_l2f_windows_with_scripted_fixes(name):
    g = handle(S.problem(name))
    assert g.debug_scalar("order") == 1.0
    assert g.debug_scalar("matrix_as_diagonals") == (0.0 if name.startswith("lap") else 1.0)
    rec = S.l2f_reference(name)
    replay(g, rec, name)
    assert S.live_counts(rec) == S.LIVE[name] and g.get_n() == S.LIVE[name][-1]
    assert np.array_equal(g.get_x_sol(), _x_sol_after(name)) if name != "lap9" else g.get_n() == 1


def _x_sol_after(name):
    o = S.oracle(S.problem(name))
    for w, r in enumerate(S.l2f_reference(name)):
        o.solve_iter_l2f(10 * w, 10 * w + 10, r["vec"], r["num"])
    return o.get_x_sol()


def test_fixed_down_to_two_live_variables():
    g = handle(S.problem("band9"))
    replay(g, S.two_live_reference(), "band9 -> 2")
    assert g.get_n() == 2


# ---- size edges ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", S.EDGE_N)
def test_sizes_around_the_short_branches_the_chunk_and_the_tile(n):
    P = S.problem(f"edge{n}")
    g = handle(P)
    assert g.config()["groups"] == (n + 511) // 512
    replay(g, S.run_windows(S.oracle(P), windows=1), f"n = {n}")


@pytest.mark.parametrize("ept", S.EPT_FORCED)
def test_forced_elements_per_thread(monkeypatch, ept):
    """The staged terms sit at the live rank whatever the chunking: the same bits at every EPT (G = 25, 7, 4 workgroups)."""
    monkeypatch.setenv("LPBOX_SEG_EPT", str(ept))
    P = S.problem(f"edge{S.EPT_N}")
    g = handle(P)
    cfg = g.config()
    assert cfg["elems_per_thread"] == ept and cfg["groups"] == -(-S.EPT_N // (256 * ept)) >= 3
    rec = S.run_windows(S.oracle(P), windows=3, fix_after=(0,))
    assert rec[1]["num"] > 0
    replay(g, rec, f"EPT {ept}")


# ---- c1 through libm's pow ---------------------------------------------------------------------------------------------------------
def test_c1_at_2921_live_variables():
    if not S.pow_differs_from_sqrt():
        pytest.skip("this libm's pow(2921, 0.5) equals sqrt(2921): the case cannot tell the two apart here")
    g = handle(S.problem("c1"))
    rec = S.c1_reference()
    replay(g, rec, "c1")
    assert g.get_n() == S.C1_LIVE


# ---- legacy solve ------------------------------------------------------------------------------------------------------------------
def same_legacy(g, energy, ref, tag):
    assert energy == ref["energy"], f"{tag}: energy {energy} vs {ref['energy']}"
    assert g.stop() == ref["stop"] and g.counters() == ref["counters"], f"{tag}: {g.stop()} {g.counters()} vs {ref['stop']} {ref['counters']}"
    assert np.array_equal(g.get_x_sol(), ref["x_sol"]), tag
    assert bits_equal(np.array([g.get_obj()]), np.array([ref["obj"]])), f"{tag}: get_obj {g.get_obj()!r} vs {ref['obj']!r}"
    for name in S.VECS:
        assert bits_equal(g.debug_vec(name)[ref["left"]], ref["vecs"][name]), f"{tag}: {name}"
    same_scalars(g, ref["scalars"], tag)


@pytest.mark.parametrize("name", S.L2F_CASES)
def test_legacy_solve_to_its_own_stop(name):
    g = handle(S.problem(name))
    same_legacy(g, g.solve_iter(), S.legacy_reference(name), name)


def test_legacy_solve_of_an_image_with_recording():
    """set_image -> the library's own cost builder; lpbox_set_record keeps every iterate (x_history) in this order too."""
    from lpbox_hip import _lib
    g = handle(gray=S.image_gray(), nodes=S.IMAGE_NODES)
    P = g.get_problem()
    assert P["n"] == S.IMAGE_NODES and g.debug_scalar("matrix_as_diagonals") == 1.0
    o = S.oracle(P)
    ref = S.legacy_snapshot(o, o.solve_iter())
    same_legacy(g, g.solve_iter(), ref, "image")
    # recorded: the same solve again, every iterate against the oracle's l2f columns of the first window
    g.solve_init()
    assert _lib.load().lpbox_set_record(g._h, 1) == 0
    e = ctypes.c_int()
    assert _lib.load().lpbox_seg_legacy(g._h, ctypes.byref(e)) == 0 and e.value == ref["energy"]
    H = g.x_history()
    assert H.shape == (ref["counters"][0], P["n"])
    o2 = S.oracle(P)
    o2.solve_iter_l2f(0, 10, np.zeros(P["n"]), 0)
    assert bits_equal(H[:10].T, o2.get_x_iters_2d(10))


# ---- PCG halt and resume -----------------------------------------------------------------------------------------------------------
def _resume_payload():
    g = handle(S.problem("resume"))
    xs = []
    for w in range(2):
        assert g.solve_iter_l2f(10 * w, 10 * w + 10, np.zeros(g.get_org_n()), 0) == 0
        xs.append(g.get_x_iters_2d(10).ravel())
    tail = np.array([g.debug_scalar("pcg_resumes"), g.debug_scalar("kmax"), g.counters()[1], g.debug_scalar("order")])
    return np.concatenate(xs + [g.debug_vec("x"), g.debug_vec("z2"), tail])


@pytest.mark.parametrize("kmax", [1, 4])
def test_halt_and_resume_with_a_forced_launch_count(tmp_path, kmax):
    """Every iteration of the case needs more (matvec, update) pairs than the chain enqueues: the chain halts from post, every launch
    and every walk behind the halt falls through, the resumed PCG finds its totals where the last walk left them."""
    rec = S.resume_reference()
    trace = rec[0]["trace"] + rec[1]["trace"]
    want_resumes = S.RESUME_COUNTS[0 if kmax == 1 else 1]
    env = dict(os.environ, LPBOX_SEG_KMAX=str(kmax))
    out = str(tmp_path / f"kmax{kmax}.npy")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.load(out)
    n = S.problem("resume")["n"]
    x0, x1, x, z2, tail = got[:10 * n], got[10 * n:20 * n], got[20 * n:21 * n], got[21 * n:22 * n], got[22 * n:]
    assert bits_equal(x0.reshape(n, 10), rec[0]["x_iters"]) and bits_equal(x1.reshape(n, 10), rec[1]["x_iters"])
    assert bits_equal(x, rec[1]["vecs"]["x"]) and bits_equal(z2, rec[1]["vecs"]["z2"])
    assert list(tail) == [want_resumes, kmax, sum(trace), 1.0], f"resumes, kmax, PCG total, order = {list(tail)}"


# ---- degenerate branches -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.DEGENERATE)
def test_degenerate_branches(name):
    g = handle(S.problem("deg:" + name))
    replay(g, S.degenerate_reference(name), name, ws=3)


# ---- both orders in one process ----------------------------------------------------------------------------------------------------
def test_both_orders_side_by_side_keep_their_own_graphs():
    P = S.problem("syn0")
    ref_e = S.run_windows(S.oracle(P), windows=2, fix_after=())
    ref_g = S.run_windows(S.oracle(P, O.ORDER_GPU), windows=2, fix_after=())
    d, r = handle(P, "default"), handle(P)
    assert (d.debug_scalar("order"), r.debug_scalar("order")) == (0.0, 1.0)
    replay(d, ref_g[:1], "default, before")
    replay(r, ref_e[:1], "reference, before")
    d.solve_iter_l2f(10, 20, ref_g[1]["vec"], 0)                 # each after the other has run, on graphs captured before it did
    r.solve_iter_l2f(10, 20, ref_e[1]["vec"], 0)
    assert bits_equal(d.get_x_iters_2d(10), ref_g[1]["x_iters"]) and bits_equal(r.get_x_iters_2d(10), ref_e[1]["x_iters"])
    same_state(r, ref_e[1], "reference, after")
    assert not bits_equal(d.get_x_iters_2d(10), r.get_x_iters_2d(10))
    for g, ref in ((d, S.legacy_reference("syn0", O.ORDER_GPU)), (r, S.legacy_reference("syn0"))):
        g.solve_init()
        assert g.solve_iter() == ref["energy"] and g.counters() == ref["counters"]
        assert bits_equal(g.debug_vec("x")[ref["left"]], ref["vecs"]["x"])


# ---- batches -----------------------------------------------------------------------------------------------------------------------
def test_solve_batch_of_six_members():
    from lpbox_hip.seg import solve_batch
    members = [handle(S.problem(n), init=False) for n in S.BATCH_LEGACY]
    assert len({m.get_org_n() for m in members}) == 6
    en = solve_batch(members)
    refs = [S.legacy_reference(n) for n in S.BATCH_LEGACY]
    assert len({r["counters"][0] for r in refs}) > 2                      # the members stop at different iterations
    assert {m.debug_scalar("matrix_as_diagonals") for m in members} == {0.0, 1.0}
    for k, (m, ref) in enumerate(zip(members, refs)):
        same_legacy(m, en[k], ref, f"member {k} ({S.BATCH_LEGACY[k]})")
    solo = handle(S.problem(S.BATCH_LEGACY[1]))                           # ... and its solo run
    assert solo.solve_iter() == en[1] and bits_equal(solo.debug_vec("x"), members[1].debug_vec("x")) and solo.counters() == members[1].counters()
    members[2].solve_init()                                               # a member goes on working on its own
    assert members[2].solve_iter() == en[2]


def _batch(names):
    from lpbox_hip.seg import SegBatch
    members = [handle(S.problem(n), init=False) for n in names]
    B = SegBatch(members)
    assert B.solve_init() == 1
    return B, members


def test_segbatch_windows_with_host_vectors():
    names = ("syn0", "lap600", "lap9", "band1025")
    B, members = _batch(names)
    recs = [S.l2f_reference(n) for n in names]
    stride = max(S.problem(n)["n"] for n in names)
    active = [True] * len(names)
    for w in range(S.WINDOWS):
        vecs, nums = -np.ones((len(names), stride)), np.zeros(len(names), np.int32)
        for k, rec in enumerate(recs):
            if w < len(rec):
                vecs[k, :len(rec[w]["vec"])] = rec[w]["vec"]
                nums[k] = rec[w]["num"]
            elif active[k]:
                active[k] = False                                         # lap9 has returned 1: out of the batch
                B.set_active(active)
        rets = B.solve_iter_l2f(10 * w, 10 * w + 10, vecs, nums)
        for k, rec in enumerate(recs):
            if w < len(rec):
                assert rets[k] == rec[w]["ret"], (w, k)
                assert bits_equal(members[k].get_x_iters_2d(10), rec[w]["x_iters"]), f"window {w}, member {k}"
                same_state(members[k], rec[w], f"window {w}, member {k}")
    assert not active[2] and members[2].get_n() == 1
    B.close()


def test_segbatch_windows_with_scripted_scores_and_a_member_that_becomes_all_fixed():
    """The l2f driver (lpbox_hip.l2f.run_l2f_seg_batch: x_iters_torch + solve_iter_l2f_scores) on a reference-order batch, against the
    same loop on the Eigen oracle; min_fix = 0 and the scripted scores fix band9 completely."""
    import torch
    names = ("syn0", "band9", "syn1-7x5")
    B, members = _batch(names)
    oracles = [S.oracle(S.problem(n)) for n in names]
    live = [True] * len(names)
    vecs = [(np.zeros(o.get_org_n()), 0) for o in oracles]
    scores = None
    all_fixed = False
    for w in range(4):
        rets, fixed = B.solve_iter_l2f_scores(10 * w, 10 * w + 10, scores, C=0.9, min_fix=0)
        for k, o in enumerate(oracles):
            if not live[k]:
                continue
            ro = o.solve_iter_l2f(10 * w, 10 * w + 10, *vecs[k])
            assert rets[k] == ro and fixed[k] == vecs[k][1] and members[k].get_n() == o.get_n(), (w, k)
            if o.get_n() == 0:
                all_fixed = True
            else:
                assert bits_equal(members[k].get_x_iters_2d(10), o.get_x_iters_2d(10)), f"window {w}, member {k}"
                same_state(members[k], S.snapshot(o, ro, 10), f"window {w}, member {k}")
            if ro:
                live[k] = False
        B.set_active(live)
        if not any(live):
            break
        X, off = B.x_iters_torch(10)
        s = scripted_scores(X.to(torch.float32).reshape(X.shape[0], 1, 10))
        if live[1] and w == 0:                                                # band9: every variable goes to its rounded value
            s[off[1]:off[1 + 1]] = torch.where(X[off[1]:off[2], -1] >= 0.5, 0.95, 0.05).to(torch.float32)
        scores = s
        sc = s.cpu().numpy().astype(np.float64)
        for k, o in enumerate(oracles):
            if live[k]:
                q = sc[off[k]:off[k + 1]]
                v = np.where(q > 0.9, 1.0, np.where(q < 0.1, 0.0, -1.0))
                num = int((v != -1).sum())
                vecs[k] = (v, num) if num > 0 else (np.zeros(len(q)), 0)
    assert all_fixed and members[1].get_n() == 0
    for k, o in enumerate(oracles):
        assert np.array_equal(members[k].get_x_sol(), o.get_x_sol()), k
    B.close()


def test_run_l2f_seg_batch_on_a_reference_order_batch():
    from lpbox_hip.l2f import run_l2f_seg_batch
    names = ("syn0", "syn1-7x5")
    members = [handle(S.problem(n), init=False) for n in names]
    solo = [handle(S.problem(n), init=False) for n in names]
    policy = lambda x: scripted_scores(x)                                       # noqa: E731
    out_b = run_l2f_seg_batch(members, policy)
    out_s = [run_l2f_seg_batch([s], policy) for s in solo]
    for k in range(len(names)):
        assert np.array_equal(members[k].get_x_sol(), solo[k].get_x_sol()) and members[k].counters() == solo[k].counters(), k
        assert members[k].debug_scalar("order") == 1.0
    assert out_b is not None and all(o is not None for o in out_s)


def test_a_batch_of_one_and_of_sixty_four():
    rec = S.l2f_reference("syn1-7x5")
    B, members = _batch(("syn1-7x5",))
    for w in range(3):
        vecs = rec[w]["vec"].reshape(1, -1)
        assert B.solve_iter_l2f(10 * w, 10 * w + 10, vecs, np.array([rec[w]["num"]], np.int32))[0] == rec[w]["ret"]
        same_state(members[0], rec[w], f"batch of one, window {w}")
    B.close()
    names = tuple(("syn1-7x5", "band9", "lap9", "edge5")[k % 4] for k in range(64))
    B, members = _batch(names)
    refs = {n: S.run_windows(S.oracle(S.problem(n)), windows=1) for n in set(names)}
    rets = B.solve_iter_l2f(0, 10, None, np.zeros(64, np.int32))
    for k, n in enumerate(names):
        assert rets[k] == refs[n][0]["ret"] and bits_equal(members[k].get_x_iters_2d(10), refs[n][0]["x_iters"]), (k, n)
        same_state(members[k], refs[n][0], f"member {k} ({n})")
    B.close()


def test_refusals_with_their_codes():
    from lpbox_hip import _lib
    from lpbox_hip.lp import LpboxError
    from lpbox_hip.seg import SegBatch, solve_batch
    L = _lib.load()
    P = S.problem("band9")
    d, r, r2 = handle(P, "default", init=False), handle(P, init=False), handle(P, init=False)
    for call in (SegBatch, solve_batch):
        with pytest.raises(LpboxError, match="problem 1 of the batch runs in the default order") as e:
            call([r, d])
        assert e.value.code == E_UNSUPPORTED
        with pytest.raises(LpboxError, match="problem 2 of the batch runs in the reference summation order") as e:
            call([d, handle(P, "default", init=False), r])
        assert e.value.code == E_UNSUPPORTED
    assert r.solve_init() == 1                                            # after the upload and after a solve: still too late
    assert L.lpbox_seg_set_order(r._h, 0) == E_STATE
    r.solve_iter()
    assert L.lpbox_seg_set_order(r._h, 1) == E_STATE and L.lpbox_seg_set_order(r._h, 3) == E_BADARG
    with pytest.raises(RuntimeError):
        r.set_order("default")
    assert r.debug_scalar("order") == 1.0
    assert solve_batch([r, r2]) == [S.legacy_reference("band9")["energy"]] * 2          # one order: accepted


def _child(out):
    np.save(out, _resume_payload())


if __name__ == "__main__":
    _child(sys.argv[1])
