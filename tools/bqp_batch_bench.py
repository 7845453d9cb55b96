"""Speed of the batch of small generic BQPs (lpbox_hip.bqp.BqpBatch) against the loop over BqpSolver.

Two workloads, each run to every problem's own stop under its type preset:
  constrained    COUNT problems bqp_problem(400, 25, 20, seed=s), preset 3 (equality + inequality);
  unconstrained  COUNT problems bqp_problem(2000, seed=s), preset 0.
It times BqpBatch.solve() (wall and the `kernel_ms` the batch reports) and, in the same process on the same problems, the loop
`for P in problems: BqpSolver(P).solve()` (the handles are built before the clock starts, as the batch is).  The two alternate
REPEATS times and the medians are reported.  A full-length loop over the constrained workload runs for minutes (10^4 iterations of a
launch-bound chain per problem), so --loop-count N runs the loop over the first N problems only; the line then holds the measured
time of those N and the time scaled to COUNT, and says so.  One JSON line per workload, appended to profiles/bqp_batch_bench.jsonl.

usage: python tools/bqp_batch_bench.py [--count 256] [--repeats 3] [--loop-count N] [--workloads constrained,unconstrained]
                                       [--cache FILE.npz] [--out FILE.jsonl]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "accelerated-lpbox-admm_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

ARGS = sys.argv[1:]


def _opt(name, default=None):
    if name in ARGS:
        k = ARGS.index(name)
        v = ARGS[k + 1]
        del ARGS[k:k + 2]
        return v
    return default


COUNT = int(_opt("--count", 256))
REPEATS = int(_opt("--repeats", 3))
LOOP_COUNT = int(_opt("--loop-count", 0)) or COUNT
WORKLOADS = _opt("--workloads", "constrained,unconstrained").split(",")
CACHE = _opt("--cache")
OUT = _opt("--out", os.path.join(ROOT, "profiles", "bqp_batch_bench.jsonl"))
SHAPES = {"constrained": (400, 25, 20), "unconstrained": (2000, 0, 0)}
KEYS = ("A", "C", "E")


def problems_of(workload):
    """COUNT problems of the workload; with --cache they are generated once and kept in FILE.npz (generation is CPU work)."""
    from helpers import bqp_problem
    n, m, l = SHAPES[workload]
    store = {}
    if CACHE and os.path.exists(CACHE):
        store = dict(np.load(CACHE))
    out = []
    for s in range(COUNT):
        tag = "%s_%d_" % (workload, s)
        if tag + "b" in store:
            P = dict(n=n, b=store[tag + "b"], x0=store[tag + "x0"])
            for k in KEYS:
                if tag + k + "0" in store:
                    P[k] = tuple(store[tag + k + str(q)] for q in range(3))
            for k in ("d", "f"):
                if tag + k in store:
                    P[k] = store[tag + k]
        else:
            P = bqp_problem(n, m, l, seed=s)
            store[tag + "b"], store[tag + "x0"] = P["b"], P["x0"]
            for k in KEYS:
                if k in P:
                    for q in range(3):
                        store[tag + k + str(q)] = P[k][q]
            for k in ("d", "f"):
                if k in P:
                    store[tag + k] = P[k]
        out.append(P)
    if CACHE:
        np.savez(CACHE, **store)
    return out


def run_batch(problems):
    from lpbox_hip.bqp import BqpBatch
    B = BqpBatch(problems)
    t0 = time.perf_counter()
    its = B.solve()
    wall = time.perf_counter() - t0
    r = dict(wall_s=wall, kernel_ms=B.scalar(0, "kernel_ms"), iters=its.copy(), launches=B.scalar(0, "launches"),
             slots=B.scalar(0, "slots"), window=B.scalar(0, "window"), x=[B.vec(i, "x") for i in range(min(LOOP_COUNT, len(problems)))],
             pcg=sum(B.scalar(i, "total_pcg") for i in range(B.count)))
    B.close()
    return r


def run_loop(problems):
    from lpbox_hip.bqp import BqpSolver
    solvers = [BqpSolver(P["n"], P["A"], P["b"], P["x0"], P.get("C"), P.get("d"), P.get("E"), P.get("f")) for P in problems]
    t0 = time.perf_counter()
    its = [s.solve() for s in solvers]
    wall = time.perf_counter() - t0
    r = dict(wall_s=wall, kernel_ms=sum(s.scalar("kernel_ms") for s in solvers), iters=np.array(its), x=[s.vec("x") for s in solvers])
    for s in solvers:
        s.close()
    return r


def main():
    for w in WORKLOADS:
        problems = problems_of(w)
        sub = problems[:LOOP_COUNT]
        run_batch(problems[:2])                                   # warm-up: library load, first launch
        run_loop(problems[:1])
        bs, ls = [], []
        for _ in range(REPEATS):
            bs.append(run_batch(problems))
            ls.append(run_loop(sub))
        same = all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(bs[-1]["x"], ls[-1]["x"])) and \
            np.array_equal(bs[-1]["iters"][:len(sub)], ls[-1]["iters"])
        med = statistics.median
        b_wall, b_ker, l_wall = med(r["wall_s"] for r in bs), med(r["kernel_ms"] for r in bs), med(r["wall_s"] for r in ls)
        its = bs[-1]["iters"]
        scaled = l_wall * len(problems) / len(sub)
        row = dict(workload=w, shape=SHAPES[w], problems=len(problems), repeats=REPEATS, slots=int(bs[-1]["slots"]), window=int(bs[-1]["window"]),
                   launches=int(bs[-1]["launches"]), iters_min=int(its.min()), iters_max=int(its.max()), iters_sum=int(its.sum()),
                   pcg_per_iteration=round(bs[-1]["pcg"] / max(int(its.sum()), 1), 3),
                   batch_wall_s=round(b_wall, 4), batch_kernel_ms=round(b_ker, 2), batch_wall_s_all=[round(r["wall_s"], 4) for r in bs],
                   us_per_iteration_slowest_problem=round(1e3 * b_ker / max(int(its.max()), 1), 2),
                   problems_per_s=round(len(problems) / b_wall, 1), problem_iterations_per_s=round(int(its.sum()) / b_wall, 1),
                   loop_problems=len(sub), loop_wall_s=round(l_wall, 4), loop_wall_s_all=[round(r["wall_s"], 4) for r in ls],
                   loop_us_per_iteration=round(1e6 * l_wall / max(int(ls[-1]["iters"].sum()), 1), 2),
                   loop_wall_s_scaled_to_all=round(scaled, 4), loop_scaled=len(sub) != len(problems),
                   ratio_loop_to_batch=round(scaled / b_wall, 2), same_bits_as_loop=bool(same))
        print(json.dumps(row), flush=True)
        with open(OUT, "a") as f:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
