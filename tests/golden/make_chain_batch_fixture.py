"""Records chain_batch_parent.json: the bookkeeping of the LOCKSTEP launch chains of a batch (per member pcg_resumes, the launches
booked, kmax, walker launches, return values, iteration counters) after every window of the cases below.

    LPBOX_LIB_VARIANT=parent python tests/golden/make_chain_batch_fixture.py [OUT.json]

The committed file was recorded on a GPU from the commit BEFORE the two lockstep loops (batch_run_chain of lpbox_seg_capi.hip,
bigb_run_chain of lpbox_big_capi.hip) moved into ChainLockstep (csrc/lpbox_chain.h) and chain_run_lockstep (csrc/lpbox_host.h), its
library built as a variant (make -C csrc variant NAME=parent).  It is never recorded again from a later tree: tests/test_chain_batch.py
calls record() on the library of the tree and compares every number, and a number that differs is a bug of the tree (DESIGN.md
section 32).

The cases use shapes the suite already has: SegBatch over S1..S4 of tests/chain_cases.py through the three windows and scripted fixes of
test_batched_windows_with_host_vectors (adaptive, LPBOX_SEG_KMAX=2, and with member 0 masked out of the second window, its fix waiting
for the third); BigLpBatch over three instances of tests/big_batch_cases.py through plain windows and through two early-fixing
windows of tests/big_l2f_batch_cases.py (member 1 masked out of the second), adaptive and with LPBOX_BIG_KMAX=4, with eager launches and
with LPBOX_BIG_BATCH_GRAPH=1; BigLpBatch(order="reference") over a unit and a valued member of tests/big_ref_batch_cases.py, eager
and captured.
"""
import contextlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "accelerated-lpbox-admm_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

OUT = os.path.join(HERE, "chain_batch_parent.json")
KNOBS = ("LPBOX_SEG_KMAX", "LPBOX_SEG_KMARGIN", "LPBOX_SEG_NOGRAPH", "LPBOX_BIG_KMAX", "LPBOX_BIG_KMARGIN", "LPBOX_BIG_NOGRAPH", "LPBOX_BIG_BATCH_GRAPH")
SEG_BATCH = ("S1", "S2", "S3", "S4")
BIG_BATCH = ((300, 0), (1100, 4), (2600, 7))
BIG_WINDOWS = ((0, 7), (7, 40))
BIG_KMAX_START = 28
REF_BATCH = (((300, 0), None), ((1100, 4), "set"))


@contextlib.contextmanager
def environment(**knobs):
    """The chain knobs as given and nothing else; handles and batches read them when they are created."""
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    try:
        os.environ.update(knobs)
        yield
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in saved.items() if v is not None})


def seg_batch(masked=False, **knobs):
    from chain_cases import SEG_FIX_AFTER, seg_case
    from helpers import scripted_fix_vec
    from lpbox_hip.seg import PyLPboxADMMsolver, SegBatch
    with environment(**knobs):
        ss = []
        for name in SEG_BATCH:
            s = PyLPboxADMMsolver(0, seg_case(name)["n"], 0)
            s.write_files = False
            s.set_problem(seg_case(name))
            ss.append(s)
        B = SegBatch(ss)
        assert B.solve_init() == 1
        nmax = max(s.get_org_n() for s in ss)
        vecs, nums, rows = -np.ones((4, nmax)), np.zeros(4, np.int32), []
        for w in range(3):
            act = [not (masked and w == 1 and k == 0) for k in range(4)]
            B.set_active(act)
            rets = B.solve_iter_l2f(10 * w, 10 * w + 10, vecs, nums)
            rows.append(dict(pcg_resumes=[int(s.debug_scalar("pcg_resumes")) for s in ss], launches=[int(s.kernel_time()[1]) for s in ss],
                             rets=[int(r) for r in rets], fixed=[int(n) if a else 0 for n, a in zip(nums, act)]))
            for k, name in enumerate(SEG_BATCH):
                if not act[k]:
                    continue                                  # its fix waits for the window it is next part of
                vecs[k], nums[k] = -1.0, 0
                if SEG_FIX_AFTER[name] == w:
                    v, n = scripted_fix_vec(ss[k].get_x_iters_2d(10), lo=0.05, hi=0.95, last=5)
                    vecs[k, :len(v)], nums[k] = v, n
        B.close()
    return rows


def big_row(B, extra=()):
    row = {s: int(B.scalar(s)) for s in ("launches", "kmax", "parity_copies", "graph") + tuple(extra)}
    row["pcg_resumes"] = [int(B.scalar("pcg_resumes_%d" % k)) for k in range(len(B))]
    for s in ("outer_total", "pcg_total", "launches"):
        row["member_" + s] = [int(g.scalar(s)) for g in B.solvers]
    return row


def big_batch(**knobs):
    import big_batch_cases as BC
    from lpbox_hip.big import BigLpBatch
    with environment(**knobs):
        B = BigLpBatch([BC.problem(n, s) for (n, s) in BIG_BATCH])
        assert B.solve_init() == 1
        rows = []
        for a, b in BIG_WINDOWS:
            rets = B.solve_iter(a, b)
            rows.append(dict(big_row(B), rets=[int(r) for r in rets]))
        B.close()
    return rows


def big_l2f_batch(**knobs):
    import big_batch_cases as BC
    import big_l2f_batch_cases as LC
    from lpbox_hip.big import BigLpBatch
    with environment(**knobs):
        B = BigLpBatch([BC.problem(n, s) for (n, s) in BIG_BATCH])
        assert B.solve_init() == 1
        rows = []
        rets = B.solve_iter_l2f(0, LC.WS, None, [0, 0, 0])
        rows.append(dict(big_row(B, ("fix_launches",)), rets=[int(r) for r in rets], fixed=[0, 0, 0]))
        vecs, nums = map(list, zip(*(LC.guarded(B[k].get_x_iters_2d(LC.WS)) for k in range(3))))
        B.set_active([True, False, True])
        rets = B.solve_iter_l2f(LC.WS, 2 * LC.WS, vecs, nums)
        rows.append(dict(big_row(B, ("fix_launches",)), rets=[int(r) for r in rets], fixed=[int(nums[0]), 0, int(nums[2])]))
        B.close()
    return rows


def big_ref_batch(**knobs):
    import big_ref_batch_cases as RC
    from lpbox_hip.big import BigLpBatch
    with environment(**knobs):
        B = BigLpBatch([RC.problem(key, fam) for (key, fam) in REF_BATCH], order="reference")
        assert B.solve_init() == 1
        rows = []
        for a, b in BIG_WINDOWS:
            rets = B.solve_iter(a, b)
            rows.append(dict(big_row(B, ("walks",)), rets=[int(r) for r in rets]))
        B.close()
    return rows


def _modes(fn, forced=True):
    """case suffix -> a run of fn: adaptive and (forced) LPBOX_BIG_KMAX=4, each with eager launches and with captured graphs"""
    out = {}
    for kname, kmax in (("", None),) + ((("_kmax4", "4"),) if forced else ()):
        for mode, graph in (("eager", "0"), ("graph", "1")):
            knobs = dict(LPBOX_BIG_BATCH_GRAPH=graph, **({"LPBOX_BIG_KMAX": kmax} if kmax else {}))
            out["%s_%s" % (kname, mode)] = (lambda fn=fn, knobs=knobs: fn(**knobs))
    return out


CASES = {"seg": seg_batch, "seg_kmax2": lambda: seg_batch(LPBOX_SEG_KMAX="2"), "seg_masked": lambda: seg_batch(masked=True)}
CASES.update({"big" + k: f for k, f in _modes(big_batch).items()})
CASES.update({"big_l2f" + k: f for k, f in _modes(big_l2f_batch).items()})
CASES.update({"big_ref" + k: f for k, f in _modes(big_ref_batch, forced=False).items()})


def record(names=None):
    """case -> one row of numbers per window, from the library lpbox_hip loads"""
    return {name: CASES[name]() for name in (names or sorted(CASES))}


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    got = record()
    with open(out, "w") as fh:
        json.dump(got, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("%s (library variant %r): %d cases" % (out, os.environ.get("LPBOX_LIB_VARIANT", ""), len(got)))
