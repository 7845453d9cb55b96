"""Speed of the segmentation flavour in the reference's summation order (PyLPboxADMMsolver.set_order("reference")).

One JSON line per workload:
  solo   one image at --nodes nodes (10000, and 0 = full resolution, 187 500): a warm-up window of 10 iterations (which also settles the
         number of enqueued PCG launches), then four l2f windows of 10 -- kernel microseconds per ADMM iteration in the reference order
         and in the default order in the same process, and the single-thread Eigen-order oracle's on this host over the same 40
         iterations after the same warm-up.
  batch  --batch images at 10000 nodes (crops of the two sample images): solve_batch to every member's own stop, and four l2f windows
         of a SegBatch after a warm-up window, in both orders; the oracle solves --cpu-sample of the members (legacy) one after the
         other on one thread, and its time is scaled to the whole batch by member-iterations.
Every record carries the PCG iterations per ADMM iteration of its stretch.  --modes picks among reference,default,oracle (a kernel-stats
run of one mode alone gives the walker's share of that chain).
usage: python tools/seg_ref_bench.py [--nodes 10000,0] [--batch 100] [--cpu-sample 5] [--modes reference,default,oracle]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "accelerated-lpbox-admm_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from lpbox_hip.seg import PyLPboxADMMsolver, SegBatch, load_gray, solve_batch  # noqa: E402
from oracle import oracle as O  # noqa: E402

ARGS = sys.argv[1:]


def _opt(name, default):
    return ARGS[ARGS.index(name) + 1] if name in ARGS else default


NODES = [int(s) for s in _opt("--nodes", "10000,0").split(",") if s != ""]
BATCH = int(_opt("--batch", 100))
CPU_SAMPLE = int(_opt("--cpu-sample", 5))
MODES = _opt("--modes", "reference,default,oracle").split(",")
SEG = os.path.join(ROOT, "tests", "golden", "seg")
WS, WINDOWS = 10, 4


def solver(gray, nodes, order):
    g = PyLPboxADMMsolver(0, nodes, 0)
    g.write_files = False
    if order == "reference":
        g.set_order("reference")
    g.set_image(gray, nodes)
    return g


def solo_gpu(gray, nodes, order):
    g = solver(gray, nodes, order)
    g.solve_init()
    z = np.zeros(g.get_org_n())
    g.solve_iter_l2f(0, WS, z, 0)
    g.kernel_time(reset=True)
    o0, p0 = g.counters()
    t0 = time.perf_counter()
    for w in range(1, 1 + WINDOWS):
        g.solve_iter_l2f(WS * w, WS * w + WS, z, 0)
    wall = time.perf_counter() - t0
    ms, launches = g.kernel_time()
    o1, p1 = g.counters()
    it = max(o1 - o0, 1)
    out = dict(us_per_iter=1e3 * ms / it, wall_us_per_iter=1e6 * wall / it, iters=int(o1 - o0), pcg_per_iter=(p1 - p0) / it,
               launches_per_iter=launches / it, kmax=g.debug_scalar("kmax"), pcg_resumes=g.debug_scalar("pcg_resumes"))
    g.close()
    return out


def solo_cpu(P):
    o = O.SegOracle(0, P["n"], 0)
    o.set_problem(P)
    o.solve_init()
    z = np.zeros(P["n"])
    o.solve_iter_l2f(0, WS, z, 0)
    o0, p0 = o.total_outer_iters, o.total_pcg_iters
    t0 = time.perf_counter()
    for w in range(1, 1 + WINDOWS):
        o.solve_iter_l2f(WS * w, WS * w + WS, z, 0)
    dt = time.perf_counter() - t0
    it = max(o.total_outer_iters - o0, 1)
    return dict(us_per_iter=1e6 * dt / it, iters=int(it), pcg_per_iter=(o.total_pcg_iters - p0) / it)


def batch_images(count):
    a, b = load_gray(os.path.join(SEG, "0.jpg")), load_gray(os.path.join(SEG, "7.jpg"))
    out = []
    for k in range(count):
        src = a if k % 2 == 0 else b
        r0, c0 = (7 * k) % 60, (11 * k) % 90
        out.append(np.ascontiguousarray(src[r0:r0 + 300, c0:c0 + 400]))
    return out


def batch_gpu(images, order):
    members = [solver(g, 10000, order) for g in images]
    solve_batch(members)                                              # uploads, warms up
    for m in members:
        m.kernel_time(reset=True)
    t0 = time.perf_counter()
    solve_batch(members)
    wall = time.perf_counter() - t0
    ms = members[0].kernel_time()[0]
    outer = np.array([m.counters()[0] for m in members])
    pcg = np.array([m.counters()[1] for m in members])
    legacy = dict(kernel_ms=ms, wall_ms=1e3 * wall, lockstep_iters=int(outer.max()), member_iters=int(outer.sum()),
                  us_per_lockstep_iter=1e3 * ms / outer.max(), us_per_member_iter=1e3 * ms / outer.sum(), pcg_per_iter=pcg.sum() / outer.sum())
    B = SegBatch(members)
    B.solve_init()
    nums = np.zeros(len(members), np.int32)
    B.solve_iter_l2f(0, WS, None, nums)
    for m in members:
        m.kernel_time(reset=True)
    o0 = sum(m.counters()[0] for m in members)
    p0 = sum(m.counters()[1] for m in members)
    t0 = time.perf_counter()
    for w in range(1, 1 + WINDOWS):
        B.solve_iter_l2f(WS * w, WS * w + WS, None, nums)
    wall = time.perf_counter() - t0
    ms = members[0].kernel_time()[0]
    it = sum(m.counters()[0] for m in members) - o0
    pc = sum(m.counters()[1] for m in members) - p0
    l2f = dict(kernel_ms=ms, wall_ms=1e3 * wall, lockstep_iters=WS * WINDOWS, member_iters=int(it), us_per_lockstep_iter=1e3 * ms / (WS * WINDOWS),
               us_per_member_iter=1e3 * ms / max(it, 1), pcg_per_iter=pc / max(it, 1))
    B.close()
    for m in members:
        m.close()
    return dict(solve_batch=legacy, segbatch_windows=l2f)


def batch_cpu(images, sample):
    iters, pcg, secs = 0, 0, 0.0
    for g in images[:sample]:
        s = solver(g, 10000, "default")
        P = s.get_problem()
        s.close()
        o = O.SegOracle(0, P["n"], 0)
        o.set_problem(P)
        o.solve_init()
        t0 = time.perf_counter()
        o.solve_iter()
        secs += time.perf_counter() - t0
        iters += o.total_outer_iters
        pcg += o.total_pcg_iters
    return dict(sample=sample, member_iters=int(iters), us_per_member_iter=1e6 * secs / max(iters, 1), pcg_per_iter=pcg / max(iters, 1))


for nodes in NODES:
    gray = load_gray(os.path.join(SEG, "0.jpg"))
    n_nodes = nodes or gray.size
    rec = dict(workload="solo", nodes=n_nodes)
    for mode in ("reference", "default"):
        if mode in MODES:
            rec[mode] = solo_gpu(gray, n_nodes, mode)
    if "oracle" in MODES:
        s = solver(gray, n_nodes, "default")
        P = s.get_problem()
        s.close()
        rec["n"] = int(P["n"])
        rec["oracle"] = solo_cpu(P)
    print(json.dumps(rec), flush=True)

if BATCH > 0:
    images = batch_images(BATCH)
    rec = dict(workload="batch", members=BATCH, nodes=10000)
    for mode in ("reference", "default"):
        if mode in MODES:
            rec[mode] = batch_gpu(images, mode)
    if "oracle" in MODES and CPU_SAMPLE > 0:
        rec["oracle"] = batch_cpu(images, min(CPU_SAMPLE, BATCH))
    print(json.dumps(rec), flush=True)
