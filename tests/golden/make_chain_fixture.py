"""Records chain_parent.json: the bookkeeping of the adaptive launch chains (pcg_resumes, kmax, launches; large LP: collectives and
the iteration counters) after every window of the cases below.

    LPBOX_LIB_VARIANT=parent python tests/golden/make_chain_fixture.py eager [OUT.json]

The committed file was recorded on a GPU from the commit BEFORE the host loops moved into csrc/lpbox_chain.h and csrc/lpbox_host.h
(its library built as a variant: make -C csrc variant NAME=parent), under EAGER launches (LPBOX_SEG_NOGRAPH, LPBOX_BQP_NOGRAPH,
LPBOX_BIG_NOGRAPH), where that commit's counters are right: on a hit of its graph cache after kmax had moved away and come back it
added the launch count of the graph captured last, not of the graph it replayed.  One mode (`eager` or `graph`) per process,
because that commit read the segmentation knobs once per process, at its first window.  tests/test_chain.py calls record() on the
library of the tree, with eager launches and with graphs, and compares every number.

Run with `graph`, the script records the same cases with graphs on; against the parent variant the difference to the committed file is
the drift (DESIGN.md section 25 has the figures).

What the cases must do is checked where the library allows it, on the tree's library by tests/test_chain.py: an adaptive BQP case and
the adaptive large-LP case must come back to a cached graph of another kmax than the one captured last (graph_revisits > 0: otherwise
the drift is not exercised), and no BQP / large-LP case may start a batch with pcg_max == 0 after iterations have run (kmax_kept == 0:
there the tree keeps kmax and the parent fell to its floor).  G4's kmax only falls (31 ... 18 over 30 iterations) and
make_auction_like(2000, 3) does not come back to a kmax within 40 iterations (nor does any seed 0..7), so the BQP case G3 over 120
iterations (kmax 12 ... 9 ... 10: two revisits) and a third large-LP window (40, 100) (one revisit) are recorded as well.  The launches of an iteration follow kmax (8 + 3 kmax per iteration of
the large LP), so a case that did the latter would not reproduce the recorded launches either.
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

OUT = os.path.join(HERE, "chain_parent.json")
NOGRAPH = ("LPBOX_SEG_NOGRAPH", "LPBOX_BQP_NOGRAPH", "LPBOX_BIG_NOGRAPH")
KNOBS = NOGRAPH + ("LPBOX_SEG_KMAX", "LPBOX_SEG_KMARGIN", "LPBOX_BQP_KMAX", "LPBOX_BIG_KMAX", "LPBOX_BIG_KMARGIN")
BATCH = ("S1", "S2", "S3", "S4")
BIG_WINDOWS = ((0, 7), (7, 40), (40, 100))
EXTRAS = ("graph_revisits", "kmax_kept")      # scalars the parent does not have; the large LP's pcg_resumes is one more


@contextlib.contextmanager
def environment(eager, **knobs):
    """The chain knobs as given and nothing else; handles read them when they are created."""
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    try:
        os.environ.update(knobs)
        if eager:
            os.environ.update({k: "1" for k in NOGRAPH})
        yield
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in saved.items() if v is not None})


def seg_windows(name, eager, **knobs):
    from chain_cases import SEG_FIX_AFTER, seg_case
    from helpers import scripted_fix_vec
    from seg_harness import solver
    with environment(eager, **knobs):
        g = solver(seg_case(name))
        rows, vec, num = [], np.zeros(g.get_org_n()), 0
        for w in range(3):
            g.solve_iter_l2f(10 * w, 10 * w + 10, vec, num)
            rows.append(dict(pcg_resumes=int(g.debug_scalar("pcg_resumes")), kmax=int(g.debug_scalar("kmax")), launches=int(g.kernel_time()[1])))
            vec, num = scripted_fix_vec(g.get_x_iters_2d(10), lo=0.05, hi=0.95, last=5) if SEG_FIX_AFTER[name] == w else (np.zeros(g.get_n()), 0)
    return rows


def seg_batch_legacy(eager):
    from chain_cases import seg_case
    from lpbox_hip.seg import PyLPboxADMMsolver, solve_batch
    with environment(eager):
        batch = []
        for name in BATCH:
            s = PyLPboxADMMsolver(0, seg_case(name)["n"], 0)
            s.write_files = False
            s.set_problem(seg_case(name))
            batch.append(s)
        energies = solve_batch(batch)
        return [dict(pcg_resumes=[int(s.debug_scalar("pcg_resumes")) for s in batch], kmax=int(batch[0].debug_scalar("kmax")),
                     launches=int(batch[0].kernel_time()[1]), energies=[int(e) for e in energies])]


def bqp_solve(name, eager, extras, K=30, **knobs):
    from chain_cases import bqp_case, bqp_case_params
    from lpbox_hip.bqp import BqpSolver
    P, _ = bqp_case(name)
    with environment(eager, **knobs):
        g = BqpSolver(P["n"], P["A"], P["b"], P["x0"], P.get("C"), P.get("d"), P.get("E"), P.get("f"), params=bqp_case_params(name, K=K))
        g.solve()
        return [{s: int(g.scalar(s)) for s in ("pcg_resumes", "kmax", "launches") + (EXTRAS if extras else ())}]


def big_windows(eager, extras, **knobs):
    from lpbox_hip.big import BigLp
    from lpbox_hip.synth import make_auction_like
    with environment(eager, **knobs):
        g = BigLp(make_auction_like(2000, 3))
        g.solve_init()
        rows = []
        for a, b in BIG_WINDOWS:
            g.solve_iter(a, b)
            rows.append({s: int(g.scalar(s)) for s in ("kmax", "launches", "collectives", "outer_total", "pcg_total") + (EXTRAS + ("pcg_resumes",) if extras else ())})
        g.close()
    return rows


def record(eager, extras=False):
    """case -> one row of numbers per window, from the library lpbox_hip loads.  extras: also the scalars only the tree has."""
    return {
        "S2": seg_windows("S2", eager), "S3": seg_windows("S3", eager), "S1_kmax2": seg_windows("S1", eager, LPBOX_SEG_KMAX="2"),
        "batch_legacy": seg_batch_legacy(eager),
        "G4": bqp_solve("G4", eager, extras), "G3_120": bqp_solve("G3", eager, extras, K=120), "G1_kmax3": bqp_solve("G1", eager, extras, LPBOX_BQP_KMAX="3"),
        "big": big_windows(eager, extras), "big_kmax4": big_windows(eager, extras, LPBOX_BIG_KMAX="4"),
    }


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "eager"
    assert mode in ("eager", "graph")
    out = sys.argv[2] if len(sys.argv) > 2 else OUT
    got = record(mode == "eager")
    with open(out, "w") as fh:
        json.dump(got, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("%s (%s, library variant %r): %d cases" % (out, mode, os.environ.get("LPBOX_LIB_VARIANT", ""), len(got)))
