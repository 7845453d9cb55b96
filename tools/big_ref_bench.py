"""Speed of the large-instance route in the reference's summation order (BigLp(order="reference")).

Per size n (make_auction_like(n, 0)) one JSON line: microseconds per ADMM iteration of a 200-iteration plain window (after a
25-iteration warm-up window, which also settles the number of enqueued PCG launches) in reference order without and with stored
values, the default order in the same process, and the single-thread Eigen-order oracle's milliseconds per iteration on the same
instance on this host, timed over the first --cpu-iters iterations of the SAME window after the same warm-up (0 skips the oracle).
Every record carries the PCG iterations per ADMM iteration of its stretch.
--modes picks among unit,valued,default (a kernel-stats run of one mode alone gives the walker's share of that chain).
usage: python tools/big_ref_bench.py [--sizes 2500,20000,100000] [--cpu-iters 40] [--window 200] [--modes unit,valued,default]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "accelerated-lpbox-admm_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from lpbox_hip.big import BigLp  # noqa: E402
from lpbox_hip.synth import make_auction_like  # noqa: E402
from oracle import oracle as O  # noqa: E402

ARGS = sys.argv[1:]


def _opt(name, default):
    return ARGS[ARGS.index(name) + 1] if name in ARGS else default


SIZES = [int(s) for s in _opt("--sizes", "2500,20000,100000").split(",")]
CPU_ITERS = int(_opt("--cpu-iters", 40))
WINDOW = int(_opt("--window", 200))
MODES = _opt("--modes", "unit,valued,default").split(",")
WARM = 25
FAMILY = np.array([0.25, 0.5, 1.0, 2.0, -1.0, 3.5])


def gpu_window(P, order):
    g = BigLp(P, order=order)
    g.solve_init()
    g.solve_iter(0, WARM)
    k0, p0, o0 = g.scalar("kernel_ms"), g.scalar("pcg_total"), g.scalar("outer_total")
    t0 = time.perf_counter()
    g.solve_iter(WARM, WARM + WINDOW)
    wall = time.perf_counter() - t0
    iters = g.scalar("outer_total") - o0
    out = dict(us_per_iter=1e3 * (g.scalar("kernel_ms") - k0) / max(iters, 1), wall_us_per_iter=1e6 * wall / max(iters, 1),
               iters=int(iters), pcg_per_iter=(g.scalar("pcg_total") - p0) / max(iters, 1), stop=int(g.scalar("stop")))
    g.close()
    return out


def cpu_window(P):
    o = O.LpOracle(0, order=O.ORDER_EIGEN)
    o.set_problem(P["n"], P["l"], P["colptr"], P["rowidx"], P["b"], P.get("f"), P.get("vals"))
    o.solve_init()
    o.solve_iter(0, WARM)
    p0 = o.total_pcg_iters
    t0 = time.perf_counter()
    o.solve_iter(WARM, WARM + CPU_ITERS)
    return dict(ms_per_iter=1e3 * (time.perf_counter() - t0) / CPU_ITERS, iters=CPU_ITERS, pcg_per_iter=(o.total_pcg_iters - p0) / CPU_ITERS)


for n in SIZES:
    P = make_auction_like(n, 0)
    V = dict(P, vals=FAMILY[np.random.RandomState(7).randint(0, len(FAMILY), len(P["rowidx"]))])
    rec = dict(n=n, l=int(P["l"]), nnz=int(len(P["rowidx"])), window=WINDOW)
    if "unit" in MODES:
        rec["reference_unit"] = gpu_window(P, "reference")
    if "valued" in MODES:
        rec["reference_valued"] = gpu_window(V, "reference")
    if "default" in MODES:
        rec["default"] = gpu_window(P, "default")
    if CPU_ITERS > 0:
        rec["oracle_unit"] = cpu_window(P)
        rec["oracle_valued"] = cpu_window(V)
    print(json.dumps(rec), flush=True)
