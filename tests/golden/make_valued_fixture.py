"""Writes the valued LP instance files of tests/test_lp_valued_api.py and tests/test_lp_valued_gpu.py:

    tests/golden/instance/2_7/instance_1_{C,b}.txt      k == 2: readSparseMat negates every value (LPcpp:2436-2439)
    tests/golden/instance/3_7/instance_1_{C,b}.txt      the same files under a k != 2

One small auction-like pattern from lpbox_hip.synth.make_auction_like (n = 40 bids) whose stored values are NOT all 1, in the
reference's on-disk format `<row>,<col>,<value>` (1-based).  Besides plain entries the C file holds
  * duplicate triplets: an entry written as two lines, far apart in the file, whose values the reader must add in file order;
  * one pair of duplicates that cancels to 0: an entry outside the pattern written as +1.5 and -1.5 -- a stored explicit zero.
Under k == 2 the negated values are mostly negative (constraints -E x <= 1 that bind nothing); the directory exists for the reader's
negation path and for the kernels' arithmetic with negative entries, not as a meaningful auction.

usage: python tests/golden/make_valued_fixture.py        (deterministic; rewrites the four files)"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "accelerated-lpbox-admm_amd"))

from lpbox_hip.synth import make_auction_like  # noqa: E402

N = 40
SEED = 5


def triplets():
    I = make_auction_like(N, seed=SEED)
    n, l = I["n"], I["l"]
    assert n != l
    rs = np.random.RandomState(SEED)
    cols = np.repeat(np.arange(n), np.diff(I["colptr"]))
    rows = I["rowidx"]
    vals = rs.choice([0.5, 1.0, 1.25, 2.0, 3.0], size=len(rows))
    vals[rs.rand(len(rows)) < 0.1] = 0.3                     # not a dyadic number: the duplicate sums below round
    order = np.lexsort((cols, rows))                         # the generator's file order: by row, then by column
    t = [(int(rows[k]), int(cols[k]), float(vals[k])) for k in order]
    # duplicates: five entries split into two lines; the second half goes to the end of the file
    tail = []
    for k in rs.choice(len(t), size=5, replace=False):
        r, c, v = t[k]
        a = float(np.round(v * rs.uniform(0.2, 0.8), 3))
        t[k] = (r, c, a)
        tail.append((r, c, v - a))
    # a cancelling pair outside the pattern: row 0 of the last column that does not already hold row 0
    have = {(r, c) for r, c, _ in t}
    c0 = max(c for c in range(n) if (0, c) not in have)
    t.insert(len(t) // 2, (0, c0, 1.5))
    tail.append((0, c0, -1.5))
    return I, t + tail


def main():
    I, t = triplets()
    for k in (2, 3):
        d = os.path.join(HERE, "instance", "%d_7" % k)
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "instance_1_C.txt"), "w") as f:
            for r, c, v in t:
                f.write("%d,%d,%r\n" % (r + 1, c + 1, v))
        with open(os.path.join(d, "instance_1_b.txt"), "w") as f:
            for v in np.asarray(I["b"], np.float64):
                f.write("%r\n" % float(-v))
    print("n=%d l=%d triplets=%d" % (I["n"], I["l"], len(t)))


if __name__ == "__main__":
    main()
