"""Speed of the opt-in reference summation order (LpBatch.set_order("reference")).

For the 256-instance headline batch (config 2: 100 items / 500 bids) and the config-4 batch (500 items / 2000 bids) it prints
  * the solve to convergence (solve_init + solve_iter(0, 20000), as bench.py runs the default): ms per batch and instance-iterations/s;
  * the fixed 2000-iteration window of tools/window.py (no instance has stopped yet): us per ADMM iteration;
and the same two numbers for the default order, measured in the same process.  One JSON line per configuration.
usage: python tools/ref_order_bench.py [repeats=2]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "accelerated-lpbox-admm_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from lpbox_hip.lp import LpBatch  # noqa: E402
from oracle import oracle as O  # noqa: E402

R = int(sys.argv[1]) if len(sys.argv) > 1 else 2
WINDOW = 2000


def batch(insts, order):
    b = LpBatch(insts)
    b.set_order(order)
    return b


def solve(b):
    """best of R solves to convergence: (ms per batch, outer iterations summed over the batch)"""
    best = None
    for _ in range(R):
        b.solve_init()
        t0 = time.perf_counter()
        b.solve_iter(0, 20000)
        ms = 1e3 * (time.perf_counter() - t0)
        best = ms if best is None else min(best, ms)
    return best, sum(b.counters(i)[0] for i in range(b.B))


def window(b):
    """best of R timed windows of the first WINDOW iterations (kernel time): us per ADMM iteration, mean PCG iterations per iteration"""
    best = None
    for _ in range(R):
        b.solve_init()
        b.kernel_time(reset=True)
        b.solve_iter(0, WINDOW)
        ms, _ = b.kernel_time()
        best = ms if best is None else min(best, ms)
    pcg = sum(b.counters(i)[1] for i in range(b.B))
    outer = sum(b.counters(i)[0] for i in range(b.B))
    return 1e3 * best / WINDOW, pcg / outer


def main():
    for cfg, fx in ((2, "lp_100_500_seed0.npz"), (4, "lp_500_2000_seed0.npz")):
        insts = O.load_lp_batch(os.path.join(ROOT, "tests", "golden", fx))[:256]
        row = dict(config=cfg, instances=len(insts))
        for order in ("reference", "default"):
            b = batch(insts, order)
            ms, outer = solve(b)
            us, k = window(b)
            c = b.config()
            row[order] = dict(ms_per_batch=round(ms, 2), outer_iterations=int(outer),
                              instance_iterations_per_s=round(outer / (ms / 1e3), 1), window_us_per_iteration=round(us, 2),
                              window_pcg_per_iteration=round(k, 3), geometry=f"{c['threads']}x{c['elems_per_thread']}", lds_bytes=c["lds_bytes"])
            b.close()
        row["window_ratio_reference_to_default"] = round(row["reference"]["window_us_per_iteration"] / row["default"]["window_us_per_iteration"], 3)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
