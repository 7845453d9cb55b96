"""The large-instance LP route at the workgroup counts and slot counts that lpbox_big_init picks above n = 131 072:
more than 256 workgroup partials per rank (slots 1..3 of get_red / fin_reduce, slots 1..7 of lean_total), the default row slicing
(row_slices > 1 without LPBOX_BIG_SLICE_KB), the step from two to four slots per thread at the fold cap, and LPBOX_BIG_EPT at a small
size.  Every case first asserts the geometry it is meant to reach, then runs a short early-fixing script and compares with the CPU
oracle, built from the subject's own threads / chunk / row_chunk, bit for bit.

The script: l2f window [0, 6), a scripted fix from the ORACLE's iterates (lo 0.05, hi 0.95, last 3: 27-28 % of the variables), l2f
window [6, 9).  One oracle run serves every route that must produce the same bits (folded and LPBOX_BIG_NOFOLD)."""
import functools
import os
import socket

import numpy as np
import pytest

from helpers import bits_equal, scripted_fix_vec
from oracle import oracle as O

pytestmark = pytest.mark.gpu

FIX = dict(lo=0.05, hi=0.95, last=3)
W0, W1 = (0, 6), (6, 9)


@functools.lru_cache(maxsize=2)
def instance(n, seed=0):
    from lpbox_hip.synth import make_auction_like
    return make_auction_like(n, seed)


def make_oracle(P, kind, T, chunk, row_chunk=0, ranks=1):
    """kind: "reference" (the kernels' order, the reference's PCG), "lean" (its comm-lean mirror) or "eigen" (the reference's order)."""
    if kind == "eigen":
        o = O.LpOracle(0, order=O.ORDER_EIGEN)
    else:
        o = O.LpOracle(0, order=O.ORDER_GPU, T=T, chunk=chunk, ranks=ranks)
        if kind == "lean":
            o.set_pcg_lean(True, row_chunk)
    o.set_problem(P["n"], P["l"], P["colptr"], P["rowidx"], P["b"])
    o.solve_init()
    return o


def snapshot(o):
    return dict(left=o.vec("left_idx").astype(int), x=o.vec("x"), z1=o.vec("z1"), z2=o.vec("z2"), z4=o.vec("z4"), f=o.vec("f"),
                totals=(o.total_outer_iters, o.total_pcg_iters), cur_obj=o.scalar("cur_obj"))


@functools.lru_cache(maxsize=2)
def oracle_script(n, kind, T, chunk, row_chunk, ranks=1):
    """The two windows on the oracle alone; the fix vector comes from its own iterates."""
    P = instance(n)
    o = make_oracle(P, kind, T, chunk, row_chunk, ranks)
    r0 = o.solve_iter_l2f(*W0, np.zeros(n), 0)
    x0 = o.get_x_iters_2d(W0[1] - W0[0])
    vec, num = scripted_fix_vec(x0, **FIX)
    r1 = o.solve_iter_l2f(*W1, vec, num)
    ref = dict(rets=(r0, r1), x0=x0, x1=o.get_x_iters_2d(W1[1] - W1[0]), vec=vec, num=num, **snapshot(o))
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def compare_state(g, ref, tag):
    left = ref["left"]
    for name in ("x", "z1", "z2"):
        assert bits_equal(g.vec(name)[left], ref[name]), f"{tag}: {name}"
    for name in ("z4", "f"):
        assert bits_equal(g.vec(name), ref[name]), f"{tag}: {name}"
    assert (g.scalar("outer_total"), g.scalar("pcg_total")) == ref["totals"], tag
    assert g.scalar("cur_obj") == ref["cur_obj"], tag


def run_script(g, ref, tag):
    n = len(ref["vec"])
    assert ref["num"] > 0, f"{tag}: the scripted fix did not fire on the oracle"
    r0 = g.solve_iter_l2f(*W0, None, 0)
    assert bits_equal(g.get_x_iters_2d(W0[1] - W0[0]), ref["x0"]), f"{tag}: x_iters of {W0}"
    r1 = g.solve_iter_l2f(*W1, ref["vec"], ref["num"])
    assert (r0, r1) == ref["rets"], tag
    assert g.get_n() == n - ref["num"] == len(ref["left"])
    assert bits_equal(g.get_x_iters_2d(W1[1] - W1[0]), ref["x1"]), f"{tag}: x_iters of {W1}"
    compare_state(g, ref, tag)


def geometry(g):
    return {k: int(g.scalar(k)) for k in ("threads", "chunk", "groups", "row_slices", "folded_reductions", "pcg_comm_lean", "row_chunk", "order")}


# n -> what lpbox_big_init must pick in the default environment (one rank)
SIZES = {131072: dict(chunk=512, groups=256, row_slices=1),       # the last size with slot 0 only
         131073: dict(chunk=512, groups=257, row_slices=2),       # one partial in slot 1; the default slicing starts
         393217: dict(chunk=512, groups=769, row_slices=4),       # one partial in slot 3
         524288: dict(chunk=512, groups=1024, row_slices=4),      # exactly the fold cap
         524289: dict(chunk=1024, groups=513, row_slices=5)}      # the first size with four slots per thread
CASES = [(131072, "reference"), (131073, "reference"), (131073, "nofold"), (393217, "reference"), (393217, "nofold"), (393217, "lean"),
         (524288, "reference"), (524289, "reference"), (524289, "lean")]


@pytest.mark.parametrize("n,mode", CASES)
def test_workgroup_count_edges_one_rank(n, mode, monkeypatch):
    from lpbox_hip.big import BigLp
    for knob in ("LPBOX_BIG_SLICE_KB", "LPBOX_BIG_EPT", "LPBOX_BIG_KMAX", "LPBOX_BIG_NOFOLD"):
        monkeypatch.delenv(knob, raising=False)
    if mode == "nofold":
        monkeypatch.setenv("LPBOX_BIG_NOFOLD", "1")
    P = instance(n)
    g = BigLp(P, pcg_mode="lean" if mode == "lean" else "reference")
    g.solve_init()
    geo = geometry(g)
    want = dict(SIZES[n], threads=256, folded_reductions=0 if mode == "nofold" else 1, pcg_comm_lean=1 if mode == "lean" else 0, order=0)
    if mode == "lean":
        want["row_chunk"] = 256                                    # sliced rows: one row per thread, q.q partials per 256 rows
        assert -(-P["l"] // 256) > 256                             # more q.q partials than threads, as well as p.p partials
    assert {k: geo[k] for k in want} == want, geo
    kind = "lean" if mode == "lean" else "reference"
    ref = oracle_script(n, kind, geo["threads"], geo["chunk"], geo["row_chunk"] if mode == "lean" else 0)
    run_script(g, ref, f"n={n} {mode}")
    g.close()


def test_reference_order_beyond_two_to_the_seventeen():
    """order="reference" at n = 131 073: one column slice whatever the default slicing would pick, the single-workgroup walker over more
    than 2^17 staged terms, the device prefix sum of the re-ranking over more than 512 chunks."""
    from lpbox_hip.big import BigLp
    n = 131073
    P = instance(n)
    g = BigLp(P, order="reference")
    g.solve_init()
    geo = geometry(g)
    assert (geo["order"], geo["row_slices"], geo["folded_reductions"]) == (1, 1, 0), geo
    ref = oracle_script(n, "eigen", 0, 0, 0)
    run_script(g, ref, f"n={n} reference order")
    g.close()


# ---- two ranks, 131 073 + 131 072 variables: Gr = {257, 256}, the gathered partials of both in slots 0 and 1 ----
N2 = 262145
PLAIN2 = 9


def _rank(rank, world, port, q, mode):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "accelerated-lpbox-admm_amd"), os.path.join(root, "tests")]
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from lpbox_hip.big import BigLp
    from lpbox_hip.synth import make_auction_like
    P = make_auction_like(N2, 0)

    def state(g):
        return dict(x=g.vec("x"), z1=g.vec("z1"), z4=g.vec("z4"), f=g.vec("f"), cur_obj=g.scalar("cur_obj"),
                    totals=(g.scalar("outer_total"), g.scalar("pcg_total")))
    g = BigLp(P, rank, world, device=0, pcg_mode=mode)
    g.solve_init()
    out = dict(rank=rank, geo={k: int(g.scalar(k)) for k in ("threads", "chunk", "groups", "row_chunk", "folded_reductions", "pcg_comm_lean")},
               n_loc=g.c1 - g.c0)
    out["plain_ret"] = g.solve_iter(0, PLAIN2)
    out["plain"] = state(g)
    g.close()
    g = BigLp(P, rank, world, device=0, pcg_mode=mode)         # the l2f script on a fresh handle; every rank scripts the fix of its own shard
    g.solve_init()
    r0 = g.solve_iter_l2f(*W0, None, 0)
    x0 = g.get_x_iters_2d(W0[1] - W0[0])
    vec, _ = scripted_fix_vec(x0, **FIX)
    r1 = g.solve_iter_l2f(*W1, vec, None)
    out.update(rets=(r0, r1), x0=x0, vec=vec, x1=g.get_x_iters_2d(W1[1] - W1[0]), l2f=state(g), n_live=g.get_n())
    q.put(out)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("mode", ["reference", "lean"])
def test_two_ranks_either_side_of_256_workgroups(mode, monkeypatch):
    """Callback transport, both ranks on one GPU.  Against the oracle's rank model: local x / z1 concatenated, the replicated z4 / f /
    cur_obj / counters on every rank.  The oracle runs in this process while the ranks run in theirs."""
    import torch.multiprocessing as mp
    for knob in ("LPBOX_BIG_SLICE_KB", "LPBOX_BIG_EPT", "LPBOX_BIG_KMAX", "LPBOX_BIG_NOFOLD"):
        monkeypatch.delenv(knob, raising=False)
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, q, mode)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        P = instance(N2)
        # threads / chunk / row_chunk are asserted below to be what the ranks report
        op = make_oracle(P, mode, 256, 512, 256, ranks=2)
        plain_ret = op.solve_iter(0, PLAIN2)
        plain = snapshot(op)
        ref = oracle_script(N2, mode, 256, 512, 256, 2)
        res = sorted([q.get(timeout=300) for _ in range(2)], key=lambda t: t["rank"])
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs)
    assert sorted(r["n_loc"] for r in res) == [131072, 131073]
    assert {r["geo"]["groups"] for r in res} == {256, 257}
    for r in res:
        assert (r["geo"]["threads"], r["geo"]["chunk"], r["geo"]["folded_reductions"]) == (256, 512, 1), r["geo"]
        assert r["geo"]["pcg_comm_lean"] == (1 if mode == "lean" else 0) and (mode != "lean" or r["geo"]["row_chunk"] == 256)
    cat = lambda part, name: np.concatenate([r[part][name] for r in res])
    # nine plain iterations
    assert all(r["plain_ret"] == plain_ret for r in res)
    assert bits_equal(cat("plain", "x"), plain["x"]) and bits_equal(cat("plain", "z1"), plain["z1"])
    for r in res:
        assert bits_equal(r["plain"]["z4"], plain["z4"]) and r["plain"]["cur_obj"] == plain["cur_obj"] and r["plain"]["totals"] == plain["totals"]
    # the early-fixing script
    assert ref["num"] > 0
    assert all(r["rets"] == ref["rets"] for r in res)
    assert bits_equal(np.concatenate([r["x0"] for r in res]), ref["x0"])
    assert np.array_equal(np.concatenate([r["vec"] for r in res]), ref["vec"])          # the same decisions on both sides
    assert sum(r["n_live"] for r in res) == N2 - ref["num"]
    assert bits_equal(np.concatenate([r["x1"] for r in res]), ref["x1"])
    left = ref["left"]
    assert bits_equal(cat("l2f", "x")[left], ref["x"]) and bits_equal(cat("l2f", "z1")[left], ref["z1"])
    for r in res:
        assert bits_equal(r["l2f"]["z4"], ref["z4"]) and bits_equal(r["l2f"]["f"], ref["f"])
        assert r["l2f"]["cur_obj"] == ref["cur_obj"] and r["l2f"]["totals"] == ref["totals"]


# ---- slots per thread at a small size: the loops `for q < d.EPT` with 4, 8 and 16 slots ----
@functools.lru_cache(maxsize=None)
def ept_oracle(chunk):
    """Plain windows (0, 7), (7, 40), l2f window (40, 60), a scripted fix from it, l2f window (60, 70) -- one oracle run per chunk."""
    P = instance(20000)
    o = make_oracle(P, "reference", 256, chunk)
    ref = dict(plain=[])
    for (a, b) in ((0, 7), (7, 40)):
        ret = o.solve_iter(a, b)
        ref["plain"].append(dict(ret=ret, **snapshot(o)))
    r0 = o.solve_iter_l2f(40, 60, np.zeros(P["n"]), 0)
    x0 = o.get_x_iters_2d(20)
    vec, num = scripted_fix_vec(x0, lo=0.05, hi=0.95, last=10)
    r1 = o.solve_iter_l2f(60, 70, vec, num)
    ref.update(rets=(r0, r1), x0=x0, x1=o.get_x_iters_2d(10), vec=vec, num=num, **snapshot(o))
    return ref


@pytest.mark.parametrize("ept,nofold", [(4, False), (8, False), (16, False), (16, True)])
def test_slots_per_thread(ept, nofold, monkeypatch):
    from lpbox_hip.big import BigLp
    monkeypatch.setenv("LPBOX_BIG_EPT", str(ept))
    if nofold:
        monkeypatch.setenv("LPBOX_BIG_NOFOLD", "1")
    P = instance(20000)
    g = BigLp(P)
    g.solve_init()
    geo = geometry(g)
    assert geo["chunk"] == 256 * ept and geo["groups"] == -(-20000 // (256 * ept)) and geo["folded_reductions"] == (0 if nofold else 1), geo
    ref = ept_oracle(geo["chunk"])
    tag = f"EPT {ept}{' nofold' if nofold else ''}"
    for (a, b), want in zip(((0, 7), (7, 40)), ref["plain"]):
        assert g.solve_iter(a, b) == want["ret"]
        compare_state(g, want, f"{tag} [{a},{b})")
    assert ref["num"] > 0
    r0 = g.solve_iter_l2f(40, 60, None, 0)
    assert bits_equal(g.get_x_iters_2d(20), ref["x0"]), tag
    r1 = g.solve_iter_l2f(60, 70, ref["vec"], ref["num"])
    assert (r0, r1) == ref["rets"]
    assert bits_equal(g.get_x_iters_2d(10), ref["x1"]), tag
    compare_state(g, ref, f"{tag} after the fix")
    g.close()
