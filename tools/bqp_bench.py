"""The generic constrained-BQP path on larger problems: (a) the full-resolution segmentation problem as `unconstrained` beside the
specialised segmentation path; (b) an auction LP with 1e5 variables as `linear_ineq`; (c) a clustering-style problem with one-of-k
equality constraints.  `--order reference` runs the three in the reference's summation order.

`--compare OUT.jsonl` instead measures the two orders side by side on three workloads -- a constrained bqp_problem at n = 2500, (b) and
(c) -- one handle per order, a warm-up solve each, then the orders alternating `--reps` times in this process; and the single-thread
oracle in Eigen order over the first `--oracle-iters` iterations of the same problem.  One JSON row per workload is appended to OUT."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'accelerated-lpbox-admm_amd')); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--order", choices=("default", "reference"), default="default", help="summation order of the three workloads")
ap.add_argument("--compare", metavar="OUT.jsonl", help="measure both orders and the Eigen-order oracle; append the rows to OUT.jsonl")
ap.add_argument("--reps", type=int, default=3, help="--compare: timed solves per order (alternating)")
ap.add_argument("--oracle-iters", type=int, default=32, help="--compare: outer iterations the oracle is timed over")
ap.add_argument("--only", choices=("n2500", "auction", "assignment"), action="append", help="--compare: only these workloads")
args = ap.parse_args()
ORDER = {} if args.order == "default" else {"order": args.order}       # (the default order is the call it has always been)

from lpbox_hip.bqp import BqpSolver
from lpbox_hip.seg import PyLPboxADMMsolver, load_gray
from lpbox_hip.synth import make_auction_like

def report(tag, g, t):
    it = g.scalar("iters"); print("%s: %d iterations (stop %d) in %.1f ms wall, %.1f ms stream, %.1f us/iteration, %.0f launches/iteration, PCG/iter %.2f" % (
        tag, it, g.scalar("stop"), t * 1e3, g.scalar("kernel_ms"), g.scalar("kernel_ms") * 1e3 / max(it, 1), g.scalar("launches") / max(g.scalar("outer_total"), 1), g.scalar("total_pcg") / max(g.scalar("outer_total"), 1)))

def auction_problem():
    P = make_auction_like(100000, 0)
    n, l = P["n"], P["l"]
    cols = np.repeat(np.arange(n), np.diff(P["colptr"])); order = np.lexsort((cols, P["rowidx"]))
    Er = np.concatenate([[0], np.cumsum(np.bincount(P["rowidx"], minlength=l))]).astype(np.int32)
    A = (np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.zeros(n))
    return dict(n=n, A=A, b=P["b"], x0=np.ones(n), E=(Er, cols[order].astype(np.int32), np.ones(len(order))), f=np.ones(l)), \
        [1e-4, 1e-6, 1.6, 0.95, 5, 300, 25, 3, 1.01, 1e-4, 1000]

def assignment_problem(pts=20000, k=8):
    """assign 20000 points to 8 clusters: x[p*k + c], one cluster per point, quadratic within-cluster cost"""
    rs = np.random.RandomState(0)
    n = pts * k
    feat = rs.randn(pts, 2) + rs.randint(0, k, pts)[:, None] * 3.0
    nbr = [rs.choice(pts, 6, replace=False) for _ in range(pts)]
    rows, colsA, vals = [], [], []
    for p in range(pts):
        for q in nbr[p]:
            if q == p: continue
            w = float(np.sum((feat[p] - feat[q]) ** 2)) * 0.05
            for c in range(k):
                rows += [p * k + c, q * k + c]; colsA += [q * k + c, p * k + c]; vals += [w, w]
    import scipy.sparse as sp
    Am = sp.coo_matrix((vals, (rows, colsA)), shape=(n, n)).tocsr()
    Am = Am + sp.diags(np.asarray(np.abs(Am).sum(axis=1)).ravel() + 0.1)
    Cp = np.arange(0, n + 1, k, dtype=np.int32)
    return dict(n=n, A=Am, b=rs.uniform(-0.1, 0.1, n), x0=np.full(n, 1.0 / k), C=(Cp, np.arange(n, dtype=np.int32), np.ones(n)), d=np.ones(pts)), \
        [1e-4, 1e-6, 1.6, 0.95, 5, 1000, 1, 3, 1.05, 1e-4, 1000]

def solver(P, params, **kw):
    return BqpSolver(P["n"], P["A"], P["b"], P["x0"], C_=P.get("C"), d=P.get("d"), E=P.get("E"), f=P.get("f"), params=params, **kw)

def compare(name, P, params):
    """One row: kernel time per outer iteration in both orders (medians of alternating solves after a warm-up), the oracle's."""
    from oracle import oracle as O
    hs = {o: solver(P, params, order=o) for o in ("default", "reference")}
    for g in hs.values():
        g.solve()
    ms = {o: [] for o in hs}
    for rep in range(args.reps):
        for o, g in hs.items():
            g.solve()
            ms[o].append(g.scalar("kernel_ms"))
    row = dict(workload=name, n=int(P["n"]), m=len(P["d"]) if P.get("C") is not None else 0, l=len(P["f"]) if P.get("E") is not None else 0, reps=args.reps)
    for o, g in hs.items():
        it = max(g.scalar("iters"), 1)
        row[o] = dict(iters=int(g.scalar("iters")), stop=int(g.scalar("stop")), total_pcg=int(g.scalar("total_pcg")), kernel_ms=ms[o],
                      us_per_iter=float(np.median(ms[o])) * 1e3 / it, launches=int(g.scalar("launches")), kmax=int(g.scalar("kmax")),
                      pcg_resumes=int(g.scalar("pcg_resumes")), best_bin_obj=g.scalar("best_bin_obj"))
    A = P["A"]
    if hasattr(A, "tocsr"):
        A = A.tocsr().sorted_indices(); A = (A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64))
    Po = dict(P, A=A)
    prm = list(params); prm[5] = min(args.oracle_iters, int(params[5]))
    o = O.BqpOracle(Po, preset=(1 if row["m"] else 0) | (2 if row["l"] else 0), params=prm, order=O.ORDER_EIGEN)
    t = time.perf_counter(); it_o = o.solve(); to = time.perf_counter() - t
    g = solver(P, prm, order="reference"); it_g = g.solve()
    row["oracle"] = dict(iters=int(it_o), seconds=to, us_per_iter=to * 1e6 / max(it_o, 1), total_pcg=int(o.scalar("total_pcg")),
                         same_x_bits=bool(it_g == it_o and np.array_equal(g.vec("x").view(np.uint64), o.vec("x").view(np.uint64))),
                         gpu_us_per_iter_same_window=g.scalar("kernel_ms") * 1e3 / max(it_g, 1))
    print(json.dumps(row), flush=True)
    with open(args.compare, "a") as f:
        f.write(json.dumps(row) + "\n")

if args.compare:
    from helpers import bqp_params, bqp_problem
    todo = args.only or ["n2500", "auction", "assignment"]
    if "n2500" in todo:
        compare("bqp_problem(2500, 64, 64, seed=1), preset 3, 2000 iterations", bqp_problem(2500, 64, 64, seed=1), bqp_params(3, 2000, rho_change_step=5))
    if "auction" in todo:
        compare("auction LP as linear_ineq BQP, 300 iterations", *auction_problem())
    if "assignment" in todo:
        compare("one-of-8 assignment as linear_eq BQP", *assignment_problem())
    sys.exit(0)

gray = load_gray(os.path.join(ROOT, 'tests', 'golden', 'seg', '0.jpg'))
s = PyLPboxADMMsolver(0, gray.size, 0); s.set_image(gray); S = s.get_problem(); s.solve_init()
t = time.perf_counter(); s.solve_iter(); ts = time.perf_counter() - t
g = BqpSolver(S["n"], (S["rowptr"], S["colidx"], S["vals"]), S["b"], np.zeros(S["n"]), **ORDER)
for rep in range(2):
    t = time.perf_counter(); g.solve(); tg = time.perf_counter() - t
report("(a) segmentation n=%d as unconstrained BQP" % S["n"], g, tg)
print("    specialised segmentation path: %.1f ms; same binary solution: %s" % (ts * 1e3, np.array_equal((g.vec("x") >= 0.5).astype(float), np.asarray(s.get_x_sol()).ravel())))

P, prm = auction_problem()
g = solver(P, prm, **ORDER)
t = time.perf_counter(); g.solve(); tg = time.perf_counter() - t
report("(b) auction LP n=%d l=%d as linear_ineq BQP, 300 iterations" % (P["n"], len(P["f"])), g, tg)

P, prm = assignment_problem()
pts, k = len(P["d"]), 8
g = solver(P, prm, **ORDER)
t = time.perf_counter(); g.solve(); tg = time.perf_counter() - t
xb = (g.vec("x") >= 0.5).reshape(pts, k)
report("(c) one-of-%d assignment, n=%d m=%d as linear_eq BQP" % (k, P["n"], pts), g, tg)
print("    points with exactly one cluster: %.3f" % np.mean(xb.sum(axis=1) == 1))
