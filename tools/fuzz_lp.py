"""Differential fuzz of the LP window kernel against the oracle in the kernel's order: random instances with structures the auction
generator rarely makes -- empty rows, one-entry columns, one row shared by most columns, duplicate columns, sizes that are not multiples
of anything -- plain and early-fixing windows, every iterate bit for bit.  usage: python tools/fuzz_lp.py [count=120] [seed=0] [direct]
With `direct` the cases have n <= 512 and run the opt-in direct x-update (set_x_update("direct")) against the
oracle's mirror of it; a batch the mode refuses (more than 128 rows of E sharing columns, or more LDS than a CU has) is reported as such."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'accelerated-lpbox-admm_amd'), os.path.join(ROOT, 'tests')]
import numpy as np


SIZES = [3, 5, 17, 31, 64, 65, 100, 257, 511, 513, 700, 1200, 2048]
DIRECT_NMAX = 512                                       # the direct x-update is built for the one-slot geometry


def random_instance(rs, nmax=None):
    """nmax: draw n from the sizes <= nmax only (the direct x-update's cases); None: the stream of draws every earlier seed produced."""
    kind = rs.randint(0, 6)
    sizes = SIZES if nmax is None else [s for s in SIZES if s <= nmax]
    n = int(rs.choice(sizes)) if kind != 5 else int(rs.randint(3, 400))
    l = max(2, int(n * rs.uniform(0.1, 0.9)))
    cols = []
    heavy = rs.randint(0, l) if kind in (1, 4) else -1
    for j in range(n):
        k = 1 if kind == 2 else int(rs.randint(1, min(l, 7) + 1))
        rows = set(rs.choice(l, size=k, replace=False).tolist())
        if heavy >= 0 and rs.rand() < 0.8:
            rows.add(int(heavy))
        if kind == 3 and j > 0 and rs.rand() < 0.3:
            rows = set(cols[j - 1])                     # duplicate column
        cols.append(sorted(rows))
    if kind in (0, 4):                                  # a few empty rows in the middle (items nobody bids on); keep the last row used
        dead = set(rs.choice(l, size=max(1, l // 5), replace=False).tolist()) - {l - 1}
        cols = [[r for r in c if r not in dead] or [l - 1] for c in cols]
    used_max = max(max(c) for c in cols)
    l = used_max + 1                                    # readSparseMat: l = largest row index present (LPcpp:2426-2441)
    colptr = np.zeros(n + 1, np.int32); colptr[1:] = np.cumsum([len(c) for c in cols])
    rowidx = np.array([r for c in cols for r in c], np.int32)
    price = rs.uniform(1, 500, n) * (1 + (kind == 4) * rs.randint(0, 2, n) * 10)
    return dict(n=n, l=l, colptr=colptr, rowidx=rowidx, b=-price), kind


def main():
    from helpers import bits_equal, oracle_for, oracle_like, scripted_fix_vec
    from lpbox_hip.lp import LpboxError, PyLPboxADMMsolver
    count = int(sys.argv[1]) if len(sys.argv) > 1 else 120
    rs = np.random.RandomState(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
    direct = len(sys.argv) > 3 and sys.argv[3] == "direct"
    bad = refused = 0
    for t in range(count):
        I, kind = random_instance(rs, DIRECT_NMAX if direct else None)
        g = PyLPboxADMMsolver(0); g.set_problem(I["n"], I["l"], I["colptr"], I["rowidx"], I["b"])
        if direct:
            try:
                g.batch.set_x_update("direct")
            except LpboxError as err:
                print("case %3d kind %d n %4d l %4d nnz %5d: refused (%s)" % (t, kind, I["n"], I["l"], len(I["rowidx"]), err), flush=True)
                refused += 1
                continue
        g.solve_init()
        if getattr(g, "large", False):                  # handed to the large-instance path (index sets beyond a CU's LDS): another oracle order,
            print("case %3d kind %d n %4d l %4d nnz %5d: large-instance route, skipped here" % (t, kind, I["n"], I["l"], len(I["rowidx"])), flush=True)
            continue                                    # covered by tests/test_dropin_large_gpu.py
        o = oracle_for(g.batch, 0, I, x_update="direct", direct_rows=g.batch.direct_rows(0)) if direct else oracle_like(g, I)
        ok = True
        vec, num = np.zeros(I["n"]), 0
        for w in range(2):
            rg, ro = g.solve_iter_l2f(w * 60, (w + 1) * 60, vec, num), o.solve_iter_l2f(w * 60, (w + 1) * 60, vec, num)
            xg, xo = g.get_x_iters_2d(60), o.get_x_iters_2d(60)
            ok = ok and rg == ro and xg.shape == xo.shape and bits_equal(xg, xo)
            if not ok or rg:
                break
            vec, num = scripted_fix_vec(xg, lo=0.05, hi=0.95, last=20)
        if ok and not rg:
            ok = g.solve_iter(120, 400) == o.solve_iter(120, 400) and bits_equal(g.batch.debug_vec("z4"), o.vec("z4"))
        print("case %3d kind %d n %4d l %4d nnz %5d: %s" % (t, kind, I["n"], I["l"], len(I["rowidx"]), "ok" if ok else "MISMATCH"), flush=True)
        bad += not ok
    print("fuzz: %d of %d cases differ%s" % (bad, count, ", %d refused by the direct mode" % refused if direct else ""))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
