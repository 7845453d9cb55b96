"""Speed of the opt-in reference summation order (LpBatch.set_order("reference")).

For the 256-instance headline batch (config 2: 100 items / 500 bids) and the config-4 batch (500 items / 2000 bids) it prints
  * the solve to convergence (solve_init + solve_iter(0, 20000), as bench.py runs the default): ms per batch and instance-iterations/s;
  * the fixed 2000-iteration window of tools/window.py (no instance has stopped yet): us per ADMM iteration;
and the same two numbers for the default order, measured in the same process.  One JSON line per configuration.

With --vals FAMILY (set = {0.5, 1, 1.25, 2, 3}, uniform = U[0.25, 4], signed = {-1, 0.5, 1, 2}) the patterns get stored values
 and each line holds instead: the valued batch in reference order (values in LDS for config 2, in global memory
for config 4), the unit batch in reference order on the same patterns, the ratio of their window figures, and -- config 2 only, with
--cpu N -- the Eigen-order CPU oracle on the same valued instances, N of them over 16 single-thread processes.
usage: python tools/ref_order_bench.py [repeats=2] [--vals FAMILY] [--cpu N] [--configs 2,4]"""
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

ARGS = sys.argv[1:]


def _opt(name, default=None):
    if name in ARGS:
        k = ARGS.index(name)
        v = ARGS[k + 1]
        del ARGS[k:k + 2]
        return v
    return default


VALS = _opt("--vals")
CPU_N = int(_opt("--cpu", 0))
CONFIGS = [int(c) for c in _opt("--configs", "2,4").split(",")]
R = int(ARGS[0]) if ARGS else 2
WINDOW = 2000
CPU_PROCS = 16


def with_values(insts, family):
    out = []
    for k, I in enumerate(insts):
        rs = np.random.RandomState(1000 + k)
        nnz = len(I["rowidx"])
        v = {"set": lambda: rs.choice([0.5, 1.0, 1.25, 2.0, 3.0], size=nnz), "uniform": lambda: rs.uniform(0.25, 4.0, nnz),
             "signed": lambda: rs.choice([-1.0, 0.5, 1.0, 2.0], size=nnz)}[family]()
        out.append(dict(I, vals=v))
    return out


def _cpu_solve(I):
    s = O.LpOracle(0, order=O.ORDER_EIGEN)
    s.set_problem(I["n"], I["l"], I["colptr"], I["rowidx"], I["b"], I.get("f"), I.get("vals"))
    s.solve_init()
    s.solve_iter(0, 20000)
    return s.total_outer_iters


def cpu_oracle(insts):
    """the Eigen-order CPU oracle over CPU_PROCS single-thread processes: instance-iterations/s to convergence (or the cap)"""
    from multiprocessing import get_context
    O.build()
    with get_context("spawn").Pool(CPU_PROCS) as p:
        p.map(_cpu_solve, insts[:CPU_PROCS])          # warm-up: library load
        t0 = time.perf_counter()
        its = p.map(_cpu_solve, insts, chunksize=1)
        dt = time.perf_counter() - t0
    return dict(processes=CPU_PROCS, instances=len(insts), outer_iterations=int(sum(its)), seconds=round(dt, 2),
                instance_iterations_per_s=round(sum(its) / dt, 1))


def batch(insts, order):
    return LpBatch(insts, order=order)


def measure(b):
    ms, outer = solve(b)
    us, k = window(b)
    c = b.config()
    return dict(ms_per_batch=round(ms, 2), outer_iterations=int(outer),
                instance_iterations_per_s=round(outer / (ms / 1e3), 1), window_us_per_iteration=round(us, 2),
                window_pcg_per_iteration=round(k, 3), geometry=f"{c['threads']}x{c['elems_per_thread']}", lds_bytes=c["lds_bytes"])


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
        if cfg not in CONFIGS:
            continue
        insts = O.load_lp_batch(os.path.join(ROOT, "tests", "golden", fx))[:256]
        row = dict(config=cfg, instances=len(insts))
        if VALS:
            vinsts = with_values(insts, VALS)
            row["vals"] = VALS
            for key, ii in (("valued_reference", vinsts), ("unit_reference", insts)):
                b = batch(ii, "reference")
                row[key] = measure(b)
                b.close()
            row["window_ratio_valued_to_unit"] = round(row["valued_reference"]["window_us_per_iteration"] / row["unit_reference"]["window_us_per_iteration"], 3)
            if cfg == 2 and CPU_N:
                row["cpu_oracle_valued"] = cpu_oracle(vinsts[:CPU_N])
                row["gpu_over_cpu"] = round(row["valued_reference"]["instance_iterations_per_s"] / row["cpu_oracle_valued"]["instance_iterations_per_s"], 2)
            print(json.dumps(row), flush=True)
            continue
        for order in ("reference", "default"):
            b = batch(insts, order)
            row[order] = measure(b)
            b.close()
        row["window_ratio_reference_to_default"] = round(row["reference"]["window_us_per_iteration"] / row["default"]["window_us_per_iteration"], 3)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
