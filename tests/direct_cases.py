"""The instances of the direct x-update's edge tests (tests/test_direct_edges.py on the CPU, tests/test_lp_direct_edges_gpu.py on the GPU;
DESIGN.md section 17): plain numpy, no GPU, no oracle.  Every constructor is deterministic and returns the usual instance dict
(n, l, colptr, rowidx, b); the cases are named (FITTING, REFUSED), so a failure names its case.  G = the rows of E that go through the dense inverse, D = the
closed-form rows; greedy_split restates the host's rule for the split and the functions at the end restate the limits of the mode."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from fuzz_lp import DIRECT_NMAX, random_instance  # noqa: E402

MAX_G = 128                 # the dense inverse holds at most 128 x 132 doubles
LDS_LIMIT = 160 * 1024      # bytes of LDS per CU
RANDOM_SEED, RANDOM_COUNT = 16, 24


def greedy_split(I, ascending=True):
    """The host rule restated (lp_plan_direct_rows): rows by ascending length, ties by ascending row index; a row is D (-1) if none of
    its columns is used yet, else G; the G rows get dense indices 0, 1, ... in row order.  ascending=False: by descending length, another
    admissible split (the D rows are still pairwise column-disjoint) for the CPU tests of the mirror's math."""
    n, l, cp, ri = I["n"], I["l"], I["colptr"], I["rowidx"]
    rows = [[] for _ in range(l)]
    for j in range(n):
        for e in range(cp[j], cp[j + 1]):
            rows[ri[e]].append(j)
    order = sorted(range(l), key=lambda r: len(rows[r]) if ascending else -len(rows[r]))
    used, is_d = np.zeros(n, bool), np.zeros(l, bool)
    for r in order:
        if not used[rows[r]].any():
            is_d[r] = True
            used[rows[r]] = True
    g = -np.ones(l, np.int32)
    g[~is_d] = np.arange((~is_d).sum())
    return g


def rows_of(I):
    rows = [[] for _ in range(I["l"])]
    for j in range(I["n"]):
        for e in range(I["colptr"][j], I["colptr"][j + 1]):
            rows[I["rowidx"][e]].append(j)
    return rows


def from_rows(n, rows, seed, **extra):
    """rows[r] = the columns of row r (an empty list = an empty row; the last row is used, readSparseMat takes l from the largest row
    index present); every column has an entry.  Prices as tools/fuzz_lp.py draws them."""
    assert rows[-1], "the last row must be used"
    cols = [[] for _ in range(n)]
    for r, cs in enumerate(rows):
        assert len(set(cs)) == len(cs)
        for j in cs:
            cols[j].append(r)
    assert all(cols), "a column without an entry"
    colptr = np.zeros(n + 1, np.int32)
    colptr[1:] = np.cumsum([len(c) for c in cols])
    rowidx = np.array([r for c in cols for r in sorted(c)], np.int32)
    price = np.random.RandomState(seed).uniform(1, 500, n)
    return dict(n=n, l=len(rows), colptr=colptr, rowidx=rowidx, b=-price, **extra)


def from_cols(n, l, cols, seed):
    return from_rows(n, [[j for j in range(n) if r in cols[j]] for r in range(l)], seed)


def all_disjoint(n):
    """Every column has one entry: rows of 1, 2, 3, 5, 1, ... consecutive columns, all of them D, |G| = 0."""
    rows, j, t = [], 0, 0
    while j < n:
        k = min((1, 2, 3, 5)[t % 4], n - j)
        rows.append(list(range(j, j + k)))
        j += k; t += 1
    return from_rows(n, rows, 100 + n)


def g_small(k):
    """Exactly k G rows, n = 2 (k + 5) + 1 <= 40.  D rows: the pairs {0,1}, {2,3}, ... and the one-entry row of the last column.  G rows:
    {1,2}, as long as the pairs but with the highest row index (the tie goes to the lower index), and k - 1 rows of three columns with the
    LOWEST row indices (they are longer, so the sort moves them behind the pairs).  kill: fixing the columns 0, 1, 2 leaves the D row
    {0,1} and the G row {1,2} without a live variable."""
    d = k + 5 if k > 1 else 6
    n = 2 * d + 1
    rows = [[2 * i, 2 * i + 3, 2 * i + 6] for i in range(1, k)]
    rows += [[2 * t, 2 * t + 1] for t in range(d)] + [[n - 1], [1, 2]]
    return from_rows(n, rows, 200 + k, kill=[0, 1, 2])


def overlap(n, k, seed, dcols=None):
    """k G rows (distinct sets) over short D rows; the row order is shuffled, so dense index, row index and storage index of a G row all
    differ.  dcols None: the D rows partition the columns into triples, the G rows hold 4 to 6 random columns.  dcols = d: the D rows are
    the pairs of the columns 0 .. d-1 only, every G row holds two of those columns and every other column sits in two random G rows --
    fewer rows and fewer entries, which is what lets 128 G rows with n = 512 pass the LDS limit."""
    rs = np.random.RandomState(seed)
    if dcols is None:
        rows = [list(range(j, min(j + 3, n))) for j in range(0, n, 3)]
        seen = set()
        while len(seen) < k:
            seen.add(tuple(sorted(rs.choice(n, size=int(rs.randint(4, 7)), replace=False).tolist())))
        rows += [list(s) for s in sorted(seen)]
    else:
        rows = [[j, j + 1] for j in range(0, dcols, 2)]
        grows = [set(rs.choice(dcols, size=2, replace=False).tolist()) for _ in range(k)]
        for j in range(dcols, n):
            for g in rs.choice(k, size=2, replace=False):
                grows[g].add(j)
        assert len({tuple(sorted(s)) for s in grows}) == k and min(len(s) for s in grows) > 2
        rows += [sorted(s) for s in grows]
    rows = [rows[i] for i in rs.permutation(len(rows))]
    return from_rows(n, rows, seed)


def heavy_row():
    """n = 300, one row holds 80 % of the columns (8 lanes share its sum in the kernel), the rest is sparse and random."""
    rs = np.random.RandomState(31)
    n, l, heavy = 300, 60, 7
    cols = [set(rs.choice(l, size=int(rs.randint(1, 4)), replace=False).tolist()) - {heavy} for _ in range(n)]
    for j in range(n):
        if j % 5 != 0:
            cols[j].add(heavy)
        elif not cols[j]:
            cols[j].add(l - 1)
    cols[n - 1].add(l - 1)
    return from_cols(n, l, cols, 31)


def dup_cols():
    """A third of the columns are copies of their left neighbour."""
    rs = np.random.RandomState(32)
    n, l = 90, 40
    cols = []
    for j in range(n):
        c = set(rs.choice(l, size=int(rs.randint(1, 5)), replace=False).tolist())
        cols.append(set(cols[j - 1]) if j % 3 == 1 else c)
    cols[n - 1].add(l - 1)
    return from_cols(n, l, cols, 32)


def empty_rows():
    """A fifth of the rows have no entry; the last row is used (tools/fuzz_lp.py does the same)."""
    rs = np.random.RandomState(33)
    n, l = 120, 50
    dead = set(rs.choice(l - 1, size=l // 5, replace=False).tolist())
    cols = []
    for j in range(n):
        c = set(rs.choice(l, size=int(rs.randint(1, 4)), replace=False).tolist()) - dead
        cols.append(c or {l - 1})
    return from_cols(n, l, cols, 33)


def n_512_full():
    """n = 512: every lane of the 512 x 1 kernel holds a variable.  128 D rows of four columns, 90 G rows of 5 to 7 random columns
    (l = 218 and fewer than 1 136 stored entries, so that the mixed batch below, whose HL is 128, stays inside the LDS limit)."""
    rs = np.random.RandomState(34)
    n = 512
    rows = [list(range(j, j + 4)) for j in range(0, n, 4)]
    seen = set()
    while len(seen) < 90:
        seen.add(tuple(sorted(rs.choice(n, size=int(rs.randint(5, 8)), replace=False).tolist())))
    rows += [list(s) for s in sorted(seen)]
    return from_rows(n, rows, 34)


def n_513():
    """One variable more than the one-slot geometry holds: the batch takes the two-slot kernels, which have no direct variant."""
    I = all_disjoint(513)
    return from_rows(513, rows_of(I) + [[0, 5, 9, 512]], 35)


def fix_with_kill(I, x):
    """The fix of the edge tests at iteration 50 -> (vec, num): min(n // 3, 40) variables, first the case's `kill` columns to 0 (one G row
    and one D row lose all their live columns), then the most decided ones to their rounding.  x: the iterate, no variable fixed so far."""
    n = I["n"]
    k = min(n // 3, 40)
    vec = -np.ones(n)
    vec[list(I.get("kill", []))[:k]] = 0.0
    for j in np.argsort(np.minimum(x, 1.0 - x), kind="stable"):
        if (vec != -1).sum() >= k:
            break
        if vec[j] == -1:
            vec[j] = 1.0 if x[j] >= 0.5 else 0.0
    return vec, int((vec != -1).sum())


def lds_family(extra):
    """n = 512, l = 160, |G| = 128, 1 120 + extra stored entries, extra = 0 ... 960.  32 one-entry D rows on the columns 0 .. 31; the
    G row g holds column g % 32 (used by a D row, so the row is G) and its share of the columns 32 .. 511: each of those sits in two G
    rows, the first `extra` of them (taken in two rounds) in one or two more.  The LDS need of the direct mode moves with the two index
    pools, 4 bytes per stored entry in steps of eight entries, so the family crosses the limit one step at a time."""
    n, G = 512, MAX_G
    rows = [[j] for j in range(32)] + [[g % 32] for g in range(G)]
    for j in range(32, n):
        cnt = 2 + (j - 32 < extra) + (j - 32 + 480 < extra)
        for t in range(cnt):
            rows[32 + (j * 7 + t * 43) % G].append(j)
    return from_rows(n, rows, 36)


def lds_pair(base_of):
    """(lds_fit, lds_over): the members of lds_family with the largest direct-mode LDS need <= LDS_LIMIT and the smallest one above it,
    found by bisection (the need grows with the stored entries).  base_of(I) = the LDS bytes of the default kernel for a batch of I alone
    (lpbox_get_config), which the caller supplies: this module stays free of the library."""
    lo, hi = 0, 960
    assert direct_need(base_of(lds_family(lo)), MAX_G) <= LDS_LIMIT < direct_need(base_of(lds_family(hi)), MAX_G), "the family does not straddle the limit"
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if direct_need(base_of(lds_family(mid)), MAX_G) <= LDS_LIMIT:
            lo = mid
        else:
            hi = mid
    return lds_family(lo), lds_family(hi)


def direct_need(base, ng_max):
    """LDS bytes of the direct kernel, restated from LdsLayout's carve-up (every block rounded up to 16 bytes): the default kernel's
    bytes, the inverse (HL rows of pitch HLD doubles), the pivot column and row of its build and the map from dense to storage index."""
    def a16(v):
        return (v + 15) & ~15
    HL = max(int(ng_max), 1)
    HLD = ((HL + 27) // 32) * 32 + 4
    return base + a16(8 * HL * HLD) + 2 * a16(8 * (HL + 1)) + a16(4 * (HL + 1))


def refusal(insts, base):
    """None if the restated rule accepts the batch, else the text its refusal must carry.  base: lpbox_get_config's lds_bytes."""
    if max(max(I["n"], I["l"]) for I in insts) > DIRECT_NMAX:
        return "n <= 512"
    gmax = max(int((greedy_split(I) >= 0).sum()) for I in insts)
    if gmax > MAX_G:
        return "%d rows of E share columns" % gmax
    need = direct_need(base, gmax)
    return "%d B of LDS" % need if need > LDS_LIMIT else None


def random_direct(rs):
    """tools/fuzz_lp.py's random_instance restricted to n <= 512 -> (instance, kind)."""
    return random_instance(rs, nmax=DIRECT_NMAX)


def random_cases():
    rs = np.random.RandomState(RANDOM_SEED)
    return [random_direct(rs) for _ in range(RANDOM_COUNT)]


# name -> (constructor, |G|); the refused ones and the LDS pair are listed apart
FITTING = {
    "all_disjoint_5": (lambda: all_disjoint(5), 0),
    "all_disjoint_100": (lambda: all_disjoint(100), 0),
    "all_disjoint_511": (lambda: all_disjoint(511), 0),
    "g_1": (lambda: g_small(1), 1),
    "g_2": (lambda: g_small(2), 2),
    "g_3": (lambda: g_small(3), 3),
    "g_5": (lambda: g_small(5), 5),
    "g_128_n257": (lambda: overlap(257, 128, 41), 128),
    "g_128_n512": (lambda: overlap(512, 128, 42, dcols=120), 128),
    "heavy_row": (heavy_row, None),
    "dup_cols": (dup_cols, None),
    "empty_rows": (empty_rows, None),
    "n_512_full": (n_512_full, 90),
}
REFUSED = {
    "g_129": (lambda: overlap(131, 129, 43), 129),       # the overlap family at the smallest n whose triples leave room for 129 distinct rows
    "n_513": (n_513, 1),
}
# one batch whose members differ in |G| (0, 3, 128, 47, 90) and in n (100, 17, 257, 300, 512)
MIXED = ("all_disjoint_100", "g_3", "g_128_n257", "heavy_row", "n_512_full")
_cache = {}


def case(name):
    if name not in _cache:
        _cache[name] = (FITTING.get(name) or REFUSED[name])[0]()
    return _cache[name]
