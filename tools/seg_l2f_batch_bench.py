"""The learned early-fixing loop of the segmentation trainer (SEG/trainer.py:699-745: windows of 10 iterations, a policy forward, a
fix) on 100 distinct 1e4-node problems cut from the two committed sample images (random windows, as tools/seg_batch_bench.py cuts
them): one image at a time (lpbox_hip.l2f.run_l2f_seg_device, the yardstick) against all images at once
(lpbox_hip.l2f.run_l2f_seg_batch), in one process.

Shapes: the reference's validation shape (3 windows of 10) and 40 windows; policies: the fused encoder on random weights and a
scripted on-device policy that does fix variables.  Five repetitions each.  A batch repetition includes creating the batch object
(its stream, the pinned staging bytes, the packing buffer); a repetition of either side includes every image's solve_init.  The run
fails unless every batch gives the loop's results and its median beats the loop's median by more than the loop's own spread.  One
JSON line per (shape, policy) goes to profiles/seg_l2f_batch_bench.jsonl.  usage: seg_l2f_batch_bench.py [images] [nodes]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "accelerated-lpbox-admm_amd"))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from lpbox_hip.l2f import run_l2f_seg_batch, run_l2f_seg_device
from lpbox_hip.policy import FusedEarlyFixPolicy
from lpbox_hip.seg import PyLPboxADMMsolver, load_gray

B = int(sys.argv[1]) if len(sys.argv) > 1 else 100
nodes = int(float(sys.argv[2])) if len(sys.argv) > 2 else 10000
REPS = int(os.environ.get("SEG_BATCH_REPS", "5"))
WS = 10
src = [load_gray(os.path.join(ROOT, "tests", "golden", "seg", f)) for f in ("0.jpg", "7.jpg")]
rs = np.random.RandomState(0)


def make(k):
    g = src[k % 2]
    h, w = g.shape
    hh, ww = rs.randint(h // 2, h + 1), rs.randint(w // 2, w + 1)
    y, x = rs.randint(0, h - hh + 1), rs.randint(0, w - ww + 1)
    s = PyLPboxADMMsolver(0, nodes, k)
    s.write_files = False
    s.set_image(np.ascontiguousarray(g[y:y + hh, x:x + ww]))
    return s


class ScriptedPolicy:
    """Stands in for a trained network, on the device: the sigmoid of a steep affine function of the mean of iterates 4..8 of the
    window, in float32 -- settled variables score beyond 0.9 / 0.1 and get fixed."""

    def scores_from_xiters(self, flat, row_off, tok_stride=1):
        idx = row_off[:, None] + torch.arange(4, 9, device=flat.device)
        t = flat[idx].to(torch.float32)
        m = ((((t[:, 0] + t[:, 1]) + t[:, 2]) + t[:, 3]) + t[:, 4]) * 0.2
        return torch.sigmoid((m - 0.5) * 5.0)


def counters(ss):
    ms = n = 0
    for s in ss:
        a, b = s.kernel_time(reset=True)
        ms, n = ms + a, n + b
    return ms, n


def loop(ss, policy, max_iter):
    out = []
    for s in ss:
        s.solve_init()
        out.append(run_l2f_seg_device(s, policy, ws=WS, max_iter=max_iter))
    return out


def timed(fn):
    times, res = [], None
    for _ in range(REPS):
        torch.cuda.synchronize()
        t = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) * 1e3)
    return times, res


ss = [make(k) for k in range(B)]
policies = (("fused, random weights", FusedEarlyFixPolicy.random(tokens=5)), ("scripted on-device", ScriptedPolicy()))
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
failed = False
with open(os.path.join(ROOT, "profiles", "seg_l2f_batch_bench.jsonl"), "a") as out:
    for windows in (3, 40):
        for pname, policy in policies:
            loop(ss[:2], policy, WS * windows)                                   # warm up both paths
            run_l2f_seg_batch(ss[:2], policy, ws=WS, max_iter=WS * windows)
            counters(ss)
            tl, rl = timed(lambda: loop(ss, policy, WS * windows))
            kl = counters(ss)
            tb, rb = timed(lambda: run_l2f_seg_batch(ss, policy, ws=WS, max_iter=WS * windows))
            kb = counters(ss)
            rec = dict(tool="seg_l2f_batch_bench", device=torch.cuda.get_device_name(0), images=B, nodes=nodes, windows=windows, ws=WS,
                       policy=pname, reps=REPS, same_results=rl == rb, fixed_total=int(sum(r["fixed"] for r in rb)),
                       windows_run=int(sum(r["windows"] for r in rb)),
                       loop_ms=[round(t, 2) for t in tl], loop_ms_min=round(min(tl), 2), loop_ms_median=round(sorted(tl)[REPS // 2], 2),
                       batch_ms=[round(t, 2) for t in tb], batch_ms_min=round(min(tb), 2), batch_ms_median=round(sorted(tb)[REPS // 2], 2),
                       loop_kernel_ms_per_rep=round(kl[0] / REPS, 2), loop_launches_per_rep=kl[1] // REPS,
                       batch_kernel_ms_per_rep=round(kb[0] / REPS, 2), batch_launches_per_rep=kb[1] // REPS,
                       speedup_min=round(min(tl) / min(tb), 2), speedup_median=round(sorted(tl)[REPS // 2] / sorted(tb)[REPS // 2], 2),
                       loop_spread_ms=round(max(tl) - min(tl), 2),
                       beats_loop_by_more_than_its_spread=bool(sorted(tl)[REPS // 2] - sorted(tb)[REPS // 2] > max(tl) - min(tl)))
            line = json.dumps(rec)
            print(line, flush=True)
            out.write(line + "\n")
            failed |= not (rec["same_results"] and rec["beats_loop_by_more_than_its_spread"])
if failed:
    sys.exit("seg_l2f_batch_bench: FAILED -- a batch differs from the loop, or does not beat it by more than the loop's own spread")
