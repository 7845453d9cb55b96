"""A batch of LP instances just above the on-chip limit on the large route in the REFERENCE summation order: a
loop over solo BigLp(order="reference") handles, the only route without the batch, against all instances in one lockstep launch chain
(BigLpBatch of the same handles), in one process.  Unit instances and the same instances with stored values ("set": drawn from
{0.25, 0.5, 1, 2, -1, 3.5}, RandomState(7), as in the tests).

Method of tools/big_batch_bench.py and tools/big_l2f_batch_bench.py: distinct make_auction_like(n, seed) instances, one warm-up and
--reps repetitions a side, every repetition includes every instance's solve_init.  The loop runs the first --loop-cap members only
(recorded as loop_members); its median and spread are scaled by count / loop_members for the comparison (the members are independent
and run one after the other), the raw numbers are recorded too.  The remaining members run alone once, untimed, so that EVERY member
of every batch is checked against the bits it gets alone.  The batch runs with eager launches (the default) and with captured iterations
(LPBOX_BIG_BATCH_GRAPH=1).  Beside it, with no threshold: the default-order batch on the same (unit) instances -- what the order costs.
The run fails unless every batch gives the loop's bits and the eager batch's median beats the loop's scaled median by more than the
loop's scaled spread (max - min).  One JSON line per (n, count, kind) goes to profiles/big_ref_batch_bench.jsonl.
--batch-only: the eager batch alone, unchecked and unrecorded -- for a kernel trace of its own (the walker's share of kernel time).
usage: big_ref_batch_bench.py [--sizes 2500,4000] [--counts 64,256] [--kinds unit,valued] [--window 200] [--reps 5] [--loop-cap 16] [--batch-only]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "accelerated-lpbox-admm_amd"))
sys.path.insert(0, ROOT)
from lpbox_hip import _lib
from lpbox_hip.big import BigLp, BigLpBatch
from lpbox_hip.synth import make_auction_like

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="2500,4000")
ap.add_argument("--counts", default="64,256")
ap.add_argument("--kinds", default="unit,valued")
ap.add_argument("--window", type=int, default=200)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--loop-cap", type=int, default=16, help="members the one-at-a-time loop runs timed (0: all)")
ap.add_argument("--batch-only", action="store_true")
args = ap.parse_args()
if _lib.load().lpbox_device_count() < 1:
    sys.exit("big_ref_batch_bench: no HIP device")
REPS = args.reps
FAMILY = np.array([0.25, 0.5, 1.0, 2.0, -1.0, 3.5])


def with_vals(P):
    rs = np.random.RandomState(7)
    return dict(P, vals=FAMILY[rs.randint(0, len(FAMILY), len(P["rowidx"]))])


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


def make_batch(gs, graph):
    if graph:
        os.environ["LPBOX_BIG_BATCH_GRAPH"] = "1"
    else:
        os.environ.pop("LPBOX_BIG_BATCH_GRAPH", None)
    B = BigLpBatch(gs)
    os.environ.pop("LPBOX_BIG_BATCH_GRAPH", None)
    assert B.scalar("graph") == (1.0 if graph else 0.0)
    return B


os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
failed = False
end = args.window
with open(os.path.join(ROOT, "profiles", "big_ref_batch_bench.jsonl"), "a") as out:
    for n in [int(float(v)) for v in args.sizes.split(",")]:
        for count in [int(v) for v in args.counts.split(",")]:
            units = [make_auction_like(n, seed) for seed in range(count)]
            for kind in args.kinds.split(","):
                Ps = units if kind == "unit" else [with_vals(P) for P in units]
                gs = [BigLp(P, order="reference") for P in Ps]
                for g in gs:
                    g.solve_init()                   # the uploads, outside every timed window
                Be = make_batch(gs, False)
                assert Be.scalar("order") == 1.0 and Be.scalar("valued_members") == (count if kind == "valued" else 0)
                if args.batch_only:
                    tb = timed(lambda: batch_run(Be, end))
                    print(json.dumps(dict(n=n, count=count, kind=kind, batch_only_ms=[round(t, 1) for t in tb], walks=Be.scalar("walks"), launches=Be.scalar("launches"))), flush=True)
                    Be.close()
                    for g in gs:
                        g.close()
                    continue
                L = count if args.loop_cap <= 0 else min(count, args.loop_cap)
                c0 = counters(gs[:L])
                tl = timed(lambda: loop(gs[:L], end))
                c1 = counters(gs[:L])
                loop(gs[L:], end)                    # untimed: what every other member gets alone
                want = state(gs)
                iters = sum(g.scalar("outer_total") for g in gs)
                b0 = counters([Be])
                w0 = Be.scalar("walks")
                te = timed(lambda: batch_run(Be, end))
                same = state(gs) == want
                c2 = tuple(a - b for a, b in zip(counters([Be]), b0))
                walks = (Be.scalar("walks") - w0) / (REPS + 1)
                Bg = make_batch(gs, True)
                tg = timed(lambda: batch_run(Bg, end))
                same_graph = state(gs) == want
                graph_kept = Bg.scalar("graph") == 1.0
                # the default-order batch on the same instances without their values: what the order costs
                gd = [BigLp(P) for P in units]
                for g in gd:
                    g.solve_init()
                Bd = BigLpBatch(gd)
                d0 = counters([Bd])
                td = timed(lambda: batch_run(Bd, end))
                c3 = tuple(a - b for a, b in zip(counters([Bd]), d0))
                runs = REPS + 1
                scale = count / L
                spread = max(tl) - min(tl)
                rec = dict(tool="big_ref_batch_bench", n=n, l=Ps[0]["l"], count=count, kind=kind, iterations=end, instance_iterations=int(iters), reps=REPS,
                           loop_members=L, checked_members=count, same_results=bool(same), same_results_graph=bool(same_graph), graph_kept=bool(graph_kept),
                           loop_ms=[round(t, 1) for t in tl], loop_ms_median=round(median(tl), 1), loop_spread_ms=round(spread, 1),
                           loop_scale=round(scale, 2), loop_ms_median_scaled=round(median(tl) * scale, 1), loop_spread_ms_scaled=round(spread * scale, 1),
                           batch_eager_ms=[round(t, 1) for t in te], batch_eager_ms_median=round(median(te), 1),
                           batch_graph_ms=[round(t, 1) for t in tg], batch_graph_ms_median=round(median(tg), 1),
                           default_order_batch_ms=[round(t, 1) for t in td], default_order_batch_ms_median=round(median(td), 1),
                           speedup_eager=round(median(tl) * scale / median(te), 2), order_cost=round(median(te) / median(td), 2),
                           loop_us_per_instance_iteration=round(median(tl) * 1e3 / (L * end), 1), batch_us_per_iteration=round(median(te) * 1e3 / end, 1),
                           loop_kernel_ms_per_rep=round((c1[0] - c0[0]) / runs, 1), loop_launches_per_rep=int((c1[1] - c0[1]) / runs),
                           batch_eager_kernel_ms_per_rep=round(c2[0] / runs, 1), batch_eager_launches_per_rep=int(c2[1] / runs), batch_walks_per_rep=int(walks),
                           default_order_batch_kernel_ms_per_rep=round(c3[0] / runs, 1), default_order_batch_launches_per_rep=int(c3[1] / runs),
                           beats_loop_by_more_than_its_spread=bool(median(tl) * scale - median(te) > spread * scale))
                line = json.dumps(rec)
                print(line, flush=True)
                out.write(line + "\n")
                out.flush()
                failed |= not (rec["same_results"] and rec["same_results_graph"] and rec["beats_loop_by_more_than_its_spread"])
                Be.close(); Bg.close(); Bd.close()
                for g in gs + gd:
                    g.close()
if failed:
    sys.exit("big_ref_batch_bench: FAILED -- a batch differs from the loop, or does not beat it by more than the loop's own spread")
