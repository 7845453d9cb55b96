"""The early-fixing loop (a window of iterations, a policy forward over the window's iterates, a fix, the next window) for a batch of LP
instances just above the on-chip limit on the large route: the loop over l2f.run_l2f_big on solo BigLp handles (the only route without
the batch) against l2f.run_l2f_big_batch (one lockstep launch chain, one pack and one policy call per window, the fix decided on the
device), in one process on the same handles.

Policies: `scripted`, an on-device rule that fixes (last 20 iterates all > 0.95 / < 0.05), and `fused`, the fused MHA policy with
reference-style random weights (last layer scaled so that its scores spread beyond the thresholds).  A repetition of either side
includes every instance's solve_init.  Where the loop over all members would take minutes it runs over the first --loop-cap members
only (recorded as loop_members) and its times are scaled by count / loop_members for the comparison (the members are independent and run
one after the other: the loop's cost is linear in them); the raw times are recorded too.  The batch always runs all members.
The run fails unless the batch returns the loop's per-member results for the members the loop ran, and the batch's median beats the
loop's (scaled) median by more than the loop's own (scaled) spread (max - min).  One JSON line per (n, count, policy) goes to
profiles/big_l2f_batch_bench.jsonl.
usage: big_l2f_batch_bench.py [--sizes 2500,4000] [--counts 64,256] [--ws 100] [--tokens 20] [--windows 4] [--reps 5] [--loop-cap 16]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "accelerated-lpbox-admm_amd"))
sys.path.insert(0, ROOT)
from lpbox_hip import _lib, l2f
from lpbox_hip.big import BigLp, BigLpBatch
from lpbox_hip.synth import make_auction_like

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="2500,4000")
ap.add_argument("--counts", default="64,256")
ap.add_argument("--ws", type=int, default=100)
ap.add_argument("--tokens", type=int, default=20)
ap.add_argument("--windows", type=int, default=4)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--loop-cap", type=int, default=16, help="members the one-at-a-time loop runs (0: all)")
ap.add_argument("--policies", default="scripted,fused")
args = ap.parse_args()
if _lib.load().lpbox_device_count() < 1:
    sys.exit("big_l2f_batch_bench: no HIP device")
import torch
from lpbox_hip.policy import FusedEarlyFixPolicy, random_state

REPS, WS, TOKENS = args.reps, args.ws, args.tokens
MAX_ITER = WS * args.windows


def scripted(x):                              # float32 (rows, tokens, ws / tokens)
    tail = x.reshape(x.shape[0], -1)[:, -20:]
    return torch.where((tail > 0.95).all(dim=1), 1.0, torch.where((tail < 0.05).all(dim=1), 0.0, 0.5))


def fused():
    sd = random_state(TOKENS, 0)
    sd["classify.fc4.weight"] = sd["classify.fc4.weight"] * 400.0
    return FusedEarlyFixPolicy(sd, tokens=TOKENS)


def median(ts):
    return sorted(ts)[len(ts) // 2]


def timed(fn):
    """REPS repetitions after one warm-up; every call ends synchronised (the windows read the control state back)."""
    res = fn()
    times = []
    for _ in range(REPS):
        t = time.perf_counter()
        res = fn()
        times.append((time.perf_counter() - t) * 1e3)
    return times, res


def loop(gs, policy):
    out = []
    for g in gs:
        g.solve_init()
        out.append(l2f.run_l2f_big(g, policy, ws=WS, max_iter=MAX_ITER, tokens=TOKENS))
    return out


def batch_run(B, policy):
    for g in B.solvers:                       # (the batch's own solve_init refuses members that still have fixed variables)
        g.solve_init()
    return l2f.run_l2f_big_batch(B, policy, ws=WS, max_iter=MAX_ITER, tokens=TOKENS)


def counters(objs):
    return sum(o.scalar("kernel_ms") for o in objs), sum(o.scalar("launches") for o in objs)


os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
failed = False
with open(os.path.join(ROOT, "profiles", "big_l2f_batch_bench.jsonl"), "a") as out:
    for n in [int(float(v)) for v in args.sizes.split(",")]:
        for count in [int(v) for v in args.counts.split(",")]:
            Ps = [make_auction_like(n, seed) for seed in range(count)]
            gs = [BigLp(P) for P in Ps]
            for g in gs:
                g.solve_init()                       # the uploads, outside every timed window
            B = BigLpBatch(gs)
            B.solve_init()
            loop_members = count if args.loop_cap <= 0 else min(count, args.loop_cap)
            for name in args.policies.split(","):
                policy = scripted if name == "scripted" else fused()
                c0 = counters(gs)
                tl, want = timed(lambda: loop(gs[:loop_members], policy))
                c1 = counters(gs)
                b0 = counters([B])
                tb, got = timed(lambda: batch_run(B, policy))
                c2 = tuple(a - b for a, b in zip(counters([B]), b0))
                same = got[:loop_members] == want
                runs = REPS + 1
                scale = count / loop_members
                rec = dict(tool="big_l2f_batch_bench", n=n, l=Ps[0]["l"], count=count, policy=name, ws=WS, tokens=TOKENS, windows=args.windows,
                           reps=REPS, loop_members=loop_members, same_results=bool(same),
                           fixed_per_member=round(sum(r["fixed"] for r in got) / count, 1), windows_run=max(r["windows"] for r in got),
                           loop_ms=[round(t, 1) for t in tl], loop_ms_median=round(median(tl), 1), loop_spread_ms=round(max(tl) - min(tl), 1),
                           batch_ms=[round(t, 1) for t in tb], batch_ms_median=round(median(tb), 1), batch_spread_ms=round(max(tb) - min(tb), 1),
                           loop_ms_per_member=round(median(tl) / loop_members, 2), batch_ms_per_member=round(median(tb) / count, 2),
                           speedup_per_member=round((median(tl) / loop_members) / (median(tb) / count), 2),
                           loop_kernel_ms_per_rep=round((c1[0] - c0[0]) / runs, 1), loop_launches_per_rep=int((c1[1] - c0[1]) / runs),
                           batch_kernel_ms_per_rep=round(c2[0] / runs, 1), batch_launches_per_rep=int(c2[1] / runs),
                           loop_scale=round(scale, 2), loop_ms_median_scaled=round(median(tl) * scale, 1), loop_spread_ms_scaled=round((max(tl) - min(tl)) * scale, 1),
                           beats_loop_by_more_than_its_spread=bool(median(tl) * scale - median(tb) > (max(tl) - min(tl)) * scale))
                line = json.dumps(rec)
                print(line, flush=True)
                out.write(line + "\n")
                out.flush()
                failed |= not (rec["same_results"] and rec["beats_loop_by_more_than_its_spread"])
            B.close()
            for g in gs:
                g.close()
if failed:
    sys.exit("big_l2f_batch_bench: FAILED -- the batch differs from the loop, or does not beat it by more than the loop's own spread")
