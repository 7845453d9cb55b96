"""A batch of LP instances just above the on-chip limit (max(n, l) > 2048) on the large route: one instance after the other
(a loop over BigLp handles, the only route without the batch) against all instances in one lockstep launch chain (BigLpBatch), in one
process on the same handles.

Workloads: a fixed window of iterations and, with --solve, every instance to its own stop.  A repetition of either side includes
every instance's solve_init.  The batch runs with eager launches (the default) and with captured iterations (LPBOX_BIG_BATCH_GRAPH=1).  The run
fails unless every batch gives the loop's bits and the default's median beats the loop's median by more than the loop's own spread (max - min).  One
JSON line per (n, count, workload) goes to profiles/big_batch_bench.jsonl.
usage: big_batch_bench.py [--sizes 2500,4000] [--counts 64,256] [--window 200] [--solve] [--reps 5] [--oracle 2]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "accelerated-lpbox-admm_amd"))
sys.path.insert(0, ROOT)
from lpbox_hip import _lib
from lpbox_hip.big import BigLp, BigLpBatch
from lpbox_hip.synth import make_auction_like

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="2500,4000")
ap.add_argument("--counts", default="64,256")
ap.add_argument("--window", type=int, default=200)
ap.add_argument("--solve", action="store_true", help="also solve every instance to its own stop")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--oracle", type=int, default=2, help="instances timed on the single-thread CPU oracle (0: none)")
args = ap.parse_args()
if _lib.load().lpbox_device_count() < 1:
    sys.exit("big_batch_bench: no HIP device")
REPS = args.reps


def median(ts):
    return sorted(ts)[len(ts) // 2]


def timed(fn):
    """REPS repetitions after one warm-up; every call ends synchronised (the windows read the control state back)."""
    fn()
    times = []
    for _ in range(REPS):
        t = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t) * 1e3)
    return times


def loop(gs, end):
    for g in gs:
        g.solve_init()
        g.solve_iter(0, end)


def batch_run(B, end):
    B.solve_init()
    B.solve_iter(0, end)


def state(gs):
    return [(g.vec("x").tobytes(), g.vec("z4").tobytes(), g.scalar("outer_total"), g.scalar("pcg_total"), g.scalar("stop")) for g in gs]


def counters(objs):
    return sum(o.scalar("kernel_ms") for o in objs), sum(o.scalar("launches") for o in objs)


def oracle_rate(Ps, iters):
    from oracle import oracle as O
    t = time.perf_counter()
    for P in Ps:
        o = O.LpOracle(0, order=O.ORDER_GPU, T=256, chunk=512)
        o.set_problem(P["n"], P["l"], P["colptr"], P["rowidx"], P["b"])
        o.solve_init()
        o.solve_iter(0, iters)
    return len(Ps) * iters / (time.perf_counter() - t)


os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
failed = False
with open(os.path.join(ROOT, "profiles", "big_batch_bench.jsonl"), "a") as out:
    for n in [int(float(v)) for v in args.sizes.split(",")]:
        for count in [int(v) for v in args.counts.split(",")]:
            Ps = [make_auction_like(n, seed) for seed in range(count)]
            gs = [BigLp(P) for P in Ps]
            for g in gs:
                g.solve_init()                       # the uploads, outside every timed window
            os.environ.pop("LPBOX_BIG_BATCH_GRAPH", None)
            Be = BigLpBatch(gs)
            os.environ["LPBOX_BIG_BATCH_GRAPH"] = "1"
            Bg = BigLpBatch(gs)
            os.environ.pop("LPBOX_BIG_BATCH_GRAPH")
            assert (Be.scalar("graph"), Bg.scalar("graph")) == (0.0, 1.0)
            for workload, end in (("window", args.window),) + ((("solve", 20000),) if args.solve else ()):
                c0 = counters(gs)
                tl = timed(lambda: loop(gs, end))
                c1 = counters(gs)
                want = state(gs)
                iters = sum(g.scalar("outer_total") for g in gs)
                b0 = counters([Be])
                te = timed(lambda: batch_run(Be, end))
                same = state(gs) == want
                c2 = tuple(a - b for a, b in zip(counters([Be]), b0))
                b0 = counters([Bg])
                tg = timed(lambda: batch_run(Bg, end))
                same = same and state(gs) == want
                c3 = tuple(a - b for a, b in zip(counters([Bg]), b0))
                runs = REPS + 1
                rec = dict(tool="big_batch_bench", n=n, l=Ps[0]["l"], count=count, workload=workload, iterations=end if workload == "window" else None,
                           instance_iterations=int(iters), reps=REPS, same_results=bool(same),
                           loop_ms=[round(t, 1) for t in tl], loop_ms_median=round(median(tl), 1), loop_spread_ms=round(max(tl) - min(tl), 1),
                           batch_eager_ms=[round(t, 1) for t in te], batch_eager_ms_median=round(median(te), 1),
                           batch_graph_ms=[round(t, 1) for t in tg], batch_graph_ms_median=round(median(tg), 1),
                           speedup_eager=round(median(tl) / median(te), 2), speedup_graph=round(median(tl) / median(tg), 2),
                           loop_kernel_ms_per_rep=round((c1[0] - c0[0]) / runs, 1), loop_launches_per_rep=int((c1[1] - c0[1]) / runs),
                           batch_eager_kernel_ms_per_rep=round(c2[0] / runs, 1), batch_eager_launches_per_rep=int(c2[1] / runs),
                           batch_graph_kernel_ms_per_rep=round(c3[0] / runs, 1), batch_graph_launches_per_rep=int(c3[1] / runs),
                           loop_instance_iters_per_s=round(iters / median(tl) * 1e3), batch_eager_instance_iters_per_s=round(iters / median(te) * 1e3),
                           batch_graph_instance_iters_per_s=round(iters / median(tg) * 1e3),
                           beats_loop_by_more_than_its_spread=bool(median(tl) - median(te) > max(tl) - min(tl)))
                if args.oracle:
                    rec["oracle_single_thread_instance_iters_per_s"] = round(oracle_rate(Ps[:args.oracle], min(end, 100)))
                line = json.dumps(rec)
                print(line, flush=True)
                out.write(line + "\n")
                out.flush()
                failed |= not (rec["same_results"] and rec["beats_loop_by_more_than_its_spread"])
            Be.close(); Bg.close()
            for g in gs:
                g.close()
if failed:
    sys.exit("big_batch_bench: FAILED -- a batch differs from the loop, or does not beat it by more than the loop's own spread")
