"""Speed of the batch of small generic BQPs (lpbox_hip.bqp.BqpBatch) against the loop over BqpSolver.

Two workloads, each run to every problem's own stop under its type preset:
  constrained    COUNT problems bqp_problem(400, 25, 20, seed=s), preset 3 (equality + inequality);
  unconstrained  COUNT problems bqp_problem(2000, seed=s), preset 0.
It times BqpBatch.solve() (wall and the `kernel_ms` the batch reports) and, in the same process on the same problems, the loop
`for P in problems: BqpSolver(P).solve()` (the handles are built before the clock starts, as the batch is).  The two alternate
REPEATS times and the medians are reported.  A full-length loop over the constrained workload runs for minutes (10^4 iterations of a
launch-bound chain per problem), so --loop-count N runs the loop over the first N problems only; the line then holds the measured
time of those N and the time scaled to COUNT, and says so.  One JSON line per workload, appended to profiles/bqp_batch_bench.jsonl.

--order reference measures what the reference's summation order costs (BqpBatch(order="reference")) instead:
the batch in reference order and the batch in the default order alternate REPEATS times in one process, and the single-thread CPU
oracle in its Eigen order (oracle/bqp_oracle.c, what the mode reproduces) solves the first --oracle-count N problems on the same host
(default: all; the line holds the measured time of those N, the time scaled to COUNT, and whether the mode's x has the oracle's bits
on them).  Lines go to profiles/bqp_batch_ref_bench.jsonl.

usage: python tools/bqp_batch_bench.py [--count 256] [--repeats 3] [--loop-count N] [--workloads constrained,unconstrained]
                                       [--order {default,reference}] [--oracle-count N] [--cache FILE.npz] [--out FILE.jsonl]"""
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
ORDER = _opt("--order", "default")
if ORDER not in ("default", "reference"):
    sys.exit("--order: default or reference")
ORACLE_COUNT = int(_opt("--oracle-count", 0)) or COUNT
OUT = _opt("--out", os.path.join(ROOT, "profiles", "bqp_batch_ref_bench.jsonl" if ORDER == "reference" else "bqp_batch_bench.jsonl"))
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


def run_batch(problems, order="default", keep=None):
    from lpbox_hip.bqp import BqpBatch
    B = BqpBatch(problems, order=order) if order != "default" else BqpBatch(problems)
    t0 = time.perf_counter()
    its = B.solve()
    wall = time.perf_counter() - t0
    keep = LOOP_COUNT if keep is None else keep
    pcgs = np.array([B.scalar(i, "total_pcg") for i in range(B.count)])
    r = dict(wall_s=wall, kernel_ms=B.scalar(0, "kernel_ms"), iters=its.copy(), launches=B.scalar(0, "launches"),
             slots=B.scalar(0, "slots"), window=B.scalar(0, "window"), x=[B.vec(i, "x") for i in range(min(keep, len(problems)))],
             pcg=pcgs.sum(), pcg_max=pcgs.max())
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


def run_oracle(problems):
    """The single-thread CPU oracle in the reference's (Eigen) order; the handles are built before the clock starts."""
    from oracle import oracle as O
    os_ = [O.BqpOracle(P) for P in problems]
    t0 = time.perf_counter()
    its = [o.solve() for o in os_]
    wall = time.perf_counter() - t0
    return dict(wall_s=wall, iters=np.array(its), x=[o.vec("x") for o in os_], pcg=sum(o.scalar("total_pcg") for o in os_))


def main_reference():
    med = statistics.median
    for w in WORKLOADS:
        problems = problems_of(w)
        sub = problems[:ORACLE_COUNT]
        run_batch(problems[:2], "reference")                      # warm-up: library load, first launch of either order
        run_batch(problems[:2])
        rs, ds = [], []
        for _ in range(REPEATS):
            rs.append(run_batch(problems, "reference", keep=len(sub)))
            ds.append(run_batch(problems, keep=0))
        o = run_oracle(sub)
        same = all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(rs[-1]["x"], o["x"])) and \
            np.array_equal(rs[-1]["iters"][:len(sub)], o["iters"])
        r_wall, r_ker = med(r["wall_s"] for r in rs), med(r["kernel_ms"] for r in rs)
        d_wall, d_ker = med(r["wall_s"] for r in ds), med(r["kernel_ms"] for r in ds)
        ri, di = rs[-1]["iters"], ds[-1]["iters"]
        scaled = o["wall_s"] * len(problems) / len(sub)
        row = dict(workload=w, order="reference", shape=SHAPES[w], problems=len(problems), repeats=REPEATS, slots=int(rs[-1]["slots"]),
                   window=int(rs[-1]["window"]), launches=int(rs[-1]["launches"]),
                   iters_min=int(ri.min()), iters_max=int(ri.max()), iters_sum=int(ri.sum()), pcg_sum=int(rs[-1]["pcg"]), pcg_max=int(rs[-1]["pcg_max"]),
                   batch_wall_s=round(r_wall, 4), batch_kernel_ms=round(r_ker, 2), batch_wall_s_all=[round(r["wall_s"], 4) for r in rs],
                   us_per_iteration_slowest_problem=round(1e3 * r_ker / max(int(ri.max()), 1), 2),
                   us_per_pcg_step_longest_problem=round(1e3 * r_ker / max(int(rs[-1]["pcg_max"]), 1), 2),
                   default_iters_max=int(di.max()), default_iters_sum=int(di.sum()), default_pcg_sum=int(ds[-1]["pcg"]), default_pcg_max=int(ds[-1]["pcg_max"]),
                   default_wall_s=round(d_wall, 4), default_kernel_ms=round(d_ker, 2), default_wall_s_all=[round(r["wall_s"], 4) for r in ds],
                   default_us_per_iteration_slowest_problem=round(1e3 * d_ker / max(int(di.max()), 1), 2),
                   default_us_per_pcg_step_longest_problem=round(1e3 * d_ker / max(int(ds[-1]["pcg_max"]), 1), 2),
                   ratio_reference_to_default_kernel=round(r_ker / d_ker, 3), ratio_reference_to_default_wall=round(r_wall / d_wall, 3),
                   oracle_problems=len(sub), oracle_wall_s=round(o["wall_s"], 4), oracle_iters_sum=int(o["iters"].sum()),
                   oracle_us_per_iteration=round(1e6 * o["wall_s"] / max(int(o["iters"].sum()), 1), 2),
                   oracle_wall_s_scaled_to_all=round(scaled, 4), oracle_scaled=len(sub) != len(problems),
                   ratio_oracle_to_batch=round(scaled / r_wall, 2), same_bits_as_oracle=bool(same))
        print(json.dumps(row), flush=True)
        with open(OUT, "a") as f:
            f.write(json.dumps(row) + "\n")


def main():
    if ORDER == "reference":
        return main_reference()
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
