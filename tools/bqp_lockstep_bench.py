"""A batch of generic BQPs just above the on-chip limit (max(n, m, l) > 2048): one problem after the other (a loop over BqpSolver
handles, the only route without the batch) against all problems in one lockstep launch chain (BqpLockstep), in one process.

Workloads: bqp_problem(2500, 64, 64) and bqp_problem(4000, 64, 64) under the eq-and-ineq preset (rho_change_step 5, the problem behind
README's per-iteration figure for n = 2500), a distinct seed per member, a fixed number of iterations with thresholds that never trigger;
and, per size, 16 members each to its own stop (std_threshold raised to 1e-4 and max_iters cut to 1500: the members of n = 2500 then end
anywhere between 75 iterations and the cap; with the preset as it is every one of them runs its 10 000 iterations).  A repetition of
either side includes every member's init launches; the uploads are outside every timed window.  The loop is timed over the first --loop-members members and scaled to the member
count (stated in the record); the remaining members are solved solo once, untimed, so that EVERY member of every batch is checked against
its solo bits.  The batch runs with eager launches (the default) and with captured iterations (LPBOX_BQP_LOCKSTEP_GRAPH=1).  One JSON line
per (n, count, workload) goes to profiles/bqp_lockstep_bench.jsonl; the run fails if a member differs from its solo bits.
usage: bqp_lockstep_bench.py [--sizes 2500,4000] [--counts 16,64,256] [--iters 100] [--reps 3] [--loop-members 16] [--oracle 2]"""
import argparse
import json
import multiprocessing
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "accelerated-lpbox-admm_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="2500,4000")
ap.add_argument("--counts", default="16,64,256")
ap.add_argument("--iters", type=int, default=100)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--loop-members", type=int, default=16)
ap.add_argument("--oracle", type=int, default=2, help="members timed on the single-thread CPU oracle (0: none)")
ap.add_argument("--workers", type=int, default=8, help="processes that build the problems (before the GPU is opened)")
args = ap.parse_args()
REPS = args.reps
BQP_VECS = ("x", "y1", "y2", "z1", "z2", "best_sol", "z3", "z4", "y3")


def make(job):
    from helpers import bqp_problem
    n, seed = job
    return bqp_problem(n, 64, 64, seed=seed)


def params(iters=None):
    from helpers import bqp_params
    p = bqp_params(3, iters if iters is not None else 1500, rho_change_step=5)
    if iters is not None:
        p[0] = p[1] = -1.0                                   # cvg <= -1 and std_obj <= -1 never hold: exactly `iters` iterations
    else:
        p[1] = 1e-4                                          # own stops
    return p


def median(ts):
    return sorted(ts)[len(ts) // 2]


def timed(fn):
    """REPS repetitions after one warm-up; every call ends synchronised (a solve reads the control state back)."""
    fn()
    times = []
    for _ in range(REPS):
        t = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t) * 1e3)
    return times


def state(g):
    return tuple(g.vec(v).tobytes() for v in BQP_VECS) + (g.scalar("iters"), g.scalar("stop"), g.scalar("total_pcg"), g.scalar("best_bin_obj"))


def main():
    sizes = [int(v) for v in args.sizes.split(",")]
    counts = [int(v) for v in args.counts.split(",")]
    with multiprocessing.Pool(args.workers) as pool:         # forked before this process touches the GPU
        problems = {n: pool.map(make, [(n, seed) for seed in range(max(counts + [16]))]) for n in sizes}
    from lpbox_hip import _lib
    from lpbox_hip.bqp import BqpLockstep, BqpSolver
    if _lib.load().lpbox_device_count() < 1:
        sys.exit("bqp_lockstep_bench: no HIP device")

    def solver(P, p):
        return BqpSolver(P["n"], P["A"], P["b"], P["x0"], P.get("C"), P.get("d"), P.get("E"), P.get("f"), params=p)

    def oracle_rate(Ps, p):
        from oracle import oracle as O
        t = time.perf_counter()
        its = 0
        for P in Ps:
            o = O.BqpOracle(P, params=p, order=O.ORDER_GPU, T=256, chunk=512)
            its += o.solve()
        return its / (time.perf_counter() - t)

    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    failed = False
    with open(os.path.join(ROOT, "profiles", "bqp_lockstep_bench.jsonl"), "a") as out:
        for n in sizes:
            for workload, count, p in [("fixed", c, params(args.iters)) for c in counts] + [("own_stop", 16, params())]:
                Ps = problems[n][:count]
                gs = [solver(P, p) for P in Ps]
                L = min(args.loop_members, count)
                for g in gs:
                    g.solve()                                # the uploads, outside every timed window; and every member's solo bits
                want = [state(g) for g in gs]
                iters = sum(g.scalar("iters") for g in gs)
                loop_iters = sum(g.scalar("iters") for g in gs[:L])
                tl = timed(lambda: [g.solve() for g in gs[:L]])
                loop_kernel_ms = sum(g.scalar("kernel_ms") for g in gs[:L])
                os.environ.pop("LPBOX_BQP_LOCKSTEP_GRAPH", None)
                Be = BqpLockstep(gs)
                os.environ["LPBOX_BQP_LOCKSTEP_GRAPH"] = "1"
                Bg = BqpLockstep(gs)
                os.environ.pop("LPBOX_BQP_LOCKSTEP_GRAPH")
                assert (Be.scalar("graph"), Bg.scalar("graph")) == (0.0, 1.0)
                te = timed(Be.solve)
                same = [state(g) for g in gs] == want
                tg = timed(Bg.solve)
                same = same and [state(g) for g in gs] == want
                scale = iters / loop_iters                   # the loop over all members, from the members it was timed on
                loop_ms = median(tl) * scale
                rec = dict(tool="bqp_lockstep_bench", n=n, m=64, l=64, count=count, workload=workload,
                           iterations=args.iters if workload == "fixed" else None, instance_iterations=int(iters), reps=REPS,
                           every_member_equals_its_solo_bits=bool(same),
                           loop_members_timed=L, loop_scaled_by=round(scale, 3), loop_timed_ms=[round(t, 1) for t in tl],
                           loop_ms_scaled_median=round(loop_ms, 1), loop_spread_ms_scaled=round((max(tl) - min(tl)) * scale, 1),
                           loop_kernel_us_per_iteration=round(loop_kernel_ms * 1e3 / loop_iters, 1),
                           batch_eager_ms=[round(t, 1) for t in te], batch_eager_ms_median=round(median(te), 1),
                           batch_graph_ms=[round(t, 1) for t in tg], batch_graph_ms_median=round(median(tg), 1),
                           batch_eager_kernel_ms=round(Be.scalar("kernel_ms"), 1), batch_eager_launches=int(Be.scalar("launches")),
                           batch_graph_kernel_ms=round(Bg.scalar("kernel_ms"), 1), batch_kmax=int(Be.scalar("kmax")),
                           batch_resumes=int(sum(Be.scalar("pcg_resumes_%d" % i) for i in range(count))),
                           speedup_eager=round(loop_ms / median(te), 2), speedup_graph=round(loop_ms / median(tg), 2),
                           loop_instance_iters_per_s=round(iters / loop_ms * 1e3), batch_eager_instance_iters_per_s=round(iters / median(te) * 1e3),
                           batch_graph_instance_iters_per_s=round(iters / median(tg) * 1e3),
                           faster_than_loop_by_more_than_its_spread=bool(loop_ms - median(te) > (max(tl) - min(tl)) * scale))
                if args.oracle:
                    po = list(p)
                    po[5] = min(int(p[5]), 100)
                    rec["oracle_single_thread_instance_iters_per_s"] = round(oracle_rate(Ps[:args.oracle], po))
                line = json.dumps(rec)
                print(line, flush=True)
                out.write(line + "\n")
                out.flush()
                failed |= not rec["every_member_equals_its_solo_bits"]
                Be.close(); Bg.close()
                for g in gs:
                    g.close()
    if failed:
        sys.exit("bqp_lockstep_bench: FAILED -- a member of a batch differs from its solo bits")


if __name__ == "__main__":
    main()
