"""The PCG halt-and-resume path of the large-instance LP route in every mode: BIG_HALT_PCG_MORE, big_launch_resume
and BigChainOps::resume_pcg under LPBOX_BIG_KMAX=4 and =1, where the PCG needs about 12 iterations, so every outer iteration halts in
`post`, the launches enqueued behind the halt fall through and the host resumes with 16 more launch groups.  With W > 1 ranks (and with
a one-rank RCCL communicator) the exchanges behind a halt still run, on buffers that already hold exchanged values.

The oracle knows nothing of launches: it is the uninterrupted arithmetic.  Every case asserts that the chain did resume and that the
result is the oracle's bit for bit."""
import os
import socket

import numpy as np
import pytest

from helpers import bits_equal, scripted_fix_vec
from oracle import oracle as O
from valued_cases import valued

pytestmark = pytest.mark.gpu

KMAX = [4, 1]


def auction(n, seed):
    from lpbox_hip.synth import make_auction_like
    return make_auction_like(n, seed)


def oracle_like(P, g=None, kind="reference", ranks=1, geo=None):
    """The oracle in the subject's own geometry (threads, chunk, row_chunk); kind "eigen": the reference's order, values included."""
    if kind == "eigen":
        o = O.LpOracle(0, order=O.ORDER_EIGEN)
    else:
        geo = geo or {k: int(g.scalar(k)) for k in ("threads", "chunk", "row_chunk")}
        o = O.LpOracle(0, order=O.ORDER_GPU, T=geo["threads"], chunk=geo["chunk"], ranks=ranks)
        if kind == "lean":
            o.set_pcg_lean(True, geo["row_chunk"])
    o.set_problem(P["n"], P["l"], P["colptr"], P["rowidx"], P["b"], P.get("f"), P.get("vals"))
    o.solve_init()
    return o


def same_state(g, o, tag):
    left = o.vec("left_idx").astype(int)
    for name in ("x", "z1", "z2"):
        assert bits_equal(g.vec(name)[left], o.vec(name)), f"{tag}: {name}"
    assert bits_equal(g.vec("z4"), o.vec("z4")), f"{tag}: z4"
    assert (g.scalar("outer_total"), g.scalar("pcg_total")) == (o.total_outer_iters, o.total_pcg_iters), tag
    assert g.scalar("cur_obj") == o.scalar("cur_obj"), tag


def plain_windows(g, o, windows, tag):
    for (a, b) in windows:
        assert g.solve_iter(a, b) == o.solve_iter(a, b), f"{tag} [{a},{b})"
        same_state(g, o, f"{tag} [{a},{b})")


def l2f_windows(g, o, windows, last, tag, vec=None, num=0):
    """l2f windows with the scripted fix after each; returns the number fixed."""
    fixed = 0
    for (a, b) in windows:
        live = o.get_n()
        rg, ro = g.solve_iter_l2f(a, b, vec, num), o.solve_iter_l2f(a, b, np.zeros(live) if vec is None else vec, num)
        assert rg == ro and g.get_n() == o.get_n(), f"{tag} [{a},{b})"
        fixed += num
        xg, xo = g.get_x_iters_2d(b - a), o.get_x_iters_2d(b - a)
        assert bits_equal(xg, xo), f"{tag} [{a},{b}): x_iters"
        same_state(g, o, f"{tag} [{a},{b})")
        assert bits_equal(g.vec("f"), o.vec("f")), f"{tag} [{a},{b}): f"
        if rg or o.get_n() == 0:
            break
        vec, num = scripted_fix_vec(xo, lo=0.05, hi=0.95, last=last)
    return fixed


def resumed(g, kmax):
    assert int(g.scalar("kmax")) == kmax                        # forced: the launch count never adapts
    print(f"kmax {kmax}: pcg_resumes {g.scalar('pcg_resumes'):.0f} over {g.scalar('outer_total'):.0f} outer iterations")
    return g.scalar("pcg_resumes")


@pytest.mark.parametrize("kmax", KMAX)
@pytest.mark.parametrize("family", [None, "set"])
def test_reference_order_resumed(family, kmax, monkeypatch):
    """The walker behind a halt and behind a finished PCG (bigref_k_walk, sidx): the resumed PCG must find in red[] the totals it halted
    on.  The walker skips there; nothing behind a halt writes the staged terms, so a walker that walked them again would leave the same
    bits -- what fails this test is a skip that loses red[].  Unit instance: plain windows; stored values: plain
    windows, then early-fixing windows with a fix."""
    from lpbox_hip.big import BigLp
    monkeypatch.setenv("LPBOX_BIG_KMAX", str(kmax))
    P = auction(3000, 1)
    if family:
        P = valued(P, family)
    g = BigLp(P, order="reference")
    g.solve_init()
    assert g.scalar("order") == 1.0
    o = oracle_like(P, kind="eigen")
    tag = f"reference order, values {family}, kmax {kmax}"
    plain_windows(g, o, ((0, 7), (7, 40)), tag)
    seen = resumed(g, kmax)
    assert seen > 0
    if family:
        assert l2f_windows(g, o, ((40, 60), (60, 80)), 20, tag) > 0
        assert resumed(g, kmax) > seen                          # the early-fixing windows halted and resumed as well
    g.close()


@pytest.mark.parametrize("kmax", KMAX)
@pytest.mark.parametrize("seed,slice_kb,windows", [(0, None, ((0, 7), (7, 40))), (2, 16, ((0, 9), (9, 40)))])
def test_comm_lean_resumed(seed, slice_kb, windows, kmax, monkeypatch):
    """The comm-lean chain: p.p / q.q partials in lsmall survive the launches that fall through behind the halt; with sliced rows the q.q
    partials come from the one-row-per-thread layout."""
    from lpbox_hip.big import BigLp
    monkeypatch.setenv("LPBOX_BIG_KMAX", str(kmax))
    if slice_kb:
        monkeypatch.setenv("LPBOX_BIG_SLICE_KB", str(slice_kb))
    P = auction(20000, seed)
    g = BigLp(P, pcg_mode="lean")
    g.solve_init()
    assert g.scalar("pcg_comm_lean") == 1.0 and int(g.scalar("row_slices")) == (20 if slice_kb else 1)
    o = oracle_like(P, g, "lean")
    plain_windows(g, o, windows, f"lean seed {seed} slice {slice_kb} kmax {kmax}")
    assert resumed(g, kmax) > 0
    g.close()


@pytest.mark.parametrize("kmax", KMAX)
def test_default_l2f_windows_resumed(kmax, monkeypatch):
    from lpbox_hip.big import BigLp
    monkeypatch.setenv("LPBOX_BIG_KMAX", str(kmax))
    P = auction(3000, 1)
    g = BigLp(P)
    g.solve_init()
    o = oracle_like(P, g)
    assert l2f_windows(g, o, ((0, 40), (40, 80), (80, 120)), 15, f"l2f kmax {kmax}") > 0
    assert resumed(g, kmax) > 0
    g.close()


@pytest.mark.parametrize("kmax", KMAX)
@pytest.mark.parametrize("mode", ["reference", "lean"])
def test_rccl_self_communicator_resumed(mode, kmax, monkeypatch):
    """A one-rank RCCL communicator: the grouped send/recv, the rank-ordered add and the all-gathers run behind every halt too."""
    from lpbox_hip.big import BigLp
    monkeypatch.setenv("LPBOX_BIG_KMAX", str(kmax))
    P = auction(20000, 0)
    g = BigLp(P, transport="rccl", pcg_mode=mode)
    g.solve_init()
    o = oracle_like(P, g, mode)
    plain_windows(g, o, ((0, 5), (5, 40)), f"rccl {mode} kmax {kmax}")
    assert resumed(g, kmax) > 0 and g.scalar("collectives") > 0
    g.close()


def test_adaptive_launch_count_without_margin(monkeypatch):
    """LPBOX_BIG_KMARGIN=0 and no forced count: kmax tracks the largest PCG count of the previous batch with no spare group, so a PCG that
    needs one iteration more than any of the batch before halts.  Only bit equality is asserted: whether a halt happens is the instance's
    business (DESIGN.md section 27 records what this one does)."""
    from lpbox_hip.big import BigLp
    monkeypatch.delenv("LPBOX_BIG_KMAX", raising=False)
    monkeypatch.setenv("LPBOX_BIG_KMARGIN", "0")
    P = auction(20000, 0)
    g = BigLp(P)
    g.solve_init()
    o = oracle_like(P, g)
    plain_windows(g, o, ((0, 7), (7, 60)), "kmargin 0")
    print(f"KMARGIN=0: pcg_resumes {g.scalar('pcg_resumes'):.0f}, kmax {g.scalar('kmax'):.0f}, pcg_total {g.scalar('pcg_total'):.0f}")
    g.close()


# ---- two ranks over the callback transport: every exchange behind a halt runs on buffers that were exchanged already ----
ITERS2 = 12


def _rank(rank, world, port, q, mode):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "accelerated-lpbox-admm_amd")]
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from lpbox_hip.big import BigLp
    from lpbox_hip.synth import make_auction_like
    P = make_auction_like(6000, 5)
    g = BigLp(P, rank, world, device=0, pcg_mode=mode)
    assert g.transport == "callback"
    g.solve_init()
    ret = g.solve_iter(0, ITERS2)
    q.put(dict(rank=rank, ret=ret, x=g.local_x(), z1=g.vec("z1"), z2=g.vec("z2"), z4=g.vec("z4"), cur_obj=g.scalar("cur_obj"),
               totals=(g.scalar("outer_total"), g.scalar("pcg_total")), resumes=g.scalar("pcg_resumes"), kmax=int(g.scalar("kmax")),
               geo={k: int(g.scalar(k)) for k in ("threads", "chunk", "row_chunk", "folded_reductions")}))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("mode,kmax,nofold", [("reference", 4, False), ("reference", 1, False), ("lean", 4, False), ("lean", 1, False),
                                              ("reference", 4, True)])
def test_two_ranks_resumed(mode, kmax, nofold, monkeypatch):
    """allreduce(q) on a q that already holds the reduced sum, gather_partials / exchange_q_lean on partials of an iteration long past
    (LPBOX_BIG_NOFOLD: the reduction launch and the all-reduce of red[] instead): everything they leave is rewritten before it is read
    again, so the resumed run is the oracle's rank model bit for bit."""
    import torch.multiprocessing as mp
    monkeypatch.setenv("LPBOX_BIG_KMAX", str(kmax))
    if nofold:
        monkeypatch.setenv("LPBOX_BIG_NOFOLD", "1")
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, q, mode)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = sorted([q.get(timeout=300) for _ in range(2)], key=lambda t: t["rank"])
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs)
    P = auction(6000, 5)
    assert res[0]["geo"] == res[1]["geo"] and res[0]["geo"]["folded_reductions"] == (0 if nofold else 1)
    o = oracle_like(P, kind=mode, ranks=2, geo=res[0]["geo"])
    ret = o.solve_iter(0, ITERS2)
    for name in ("x", "z1", "z2"):
        assert bits_equal(np.concatenate([r[name] for r in res]), o.vec(name)), name
    for r in res:
        assert r["kmax"] == kmax and r["resumes"] > 0
        assert r["ret"] == ret and bits_equal(r["z4"], o.vec("z4")) and r["cur_obj"] == o.scalar("cur_obj")
        assert r["totals"] == (o.total_outer_iters, o.total_pcg_iters)
