"""The PCG loop of the 512 x 1 LP window kernel in its two forms: per wavefront a copy compiled for the lengths of the wave's three
gather lists ("specialised", the default), or the one loop that dispatches on the lengths in every iteration ("generic",
LPBOX_LP_PCGLOOP=generic).  Both run the same expressions on the same operands, so both must equal the oracle -- and each other -- bit
for bit.  The instances are chosen by what their wavefronts look like (LpBatch.wave_classes): empty waves, a wave with one lane, every
lane in use, and a workgroup in which one wave has a list tail (it must take the generic loop) next to waves that have none."""
import numpy as np
import pytest

from helpers import bits_equal, lp_instances, oracle_full_solve, oracle_like, scripted_fix_vec
from test_lp_gpu_parity import compare_state, gpu_solver

pytestmark = pytest.mark.gpu

MODES = ("specialised", "generic")
WS = 40


def generated(n, seed):
    from lpbox_hip.synth import make_auction_like
    return make_auction_like(n, seed=seed)


def dense_row_long_column(n=300, l=150, row_len=130, col_len=45, seed=5):
    """Row 0 meets `row_len` variables (more than 8 lanes x 12 register entries: its lanes keep a tail), column 0 sits in `col_len` rows
    (more than 12 + 3 x 8: its own lane keeps a tail); every other column has 1 to 4 entries."""
    rs = np.random.RandomState(seed)
    cols = []
    for j in range(n):
        rows = set(rs.choice(np.arange(1, l), rs.randint(1, 4), replace=False).tolist())
        rows.add(1 + j % (l - 1))                             # every row is used
        if j == 0:
            rows |= set(rs.choice(np.arange(1, l), col_len, replace=False).tolist())
        if j < row_len:
            rows.add(0)
        cols.append(sorted(rows))
    colptr = np.cumsum([0] + [len(c) for c in cols]).astype(np.int64)
    rowidx = np.concatenate(cols).astype(np.int64)
    assert len(np.unique(rowidx)) == l, "every row is used"
    return dict(n=n, l=l, colptr=colptr, rowidx=rowidx, b=-(1.0 + 99.0 * rs.rand(n)))


SHAPES = {
    "n60": lambda: lp_instances("lp_20_60_seed0.npz")[1],
    "n65": lambda: generated(65, 12),
    "n512": lambda: generated(512, 3),
    "mixed": dense_row_long_column,
    # make_auction_like(60, seed=0) under the CPU oracle, no fix applied: the solve stops after 75 iterations, the PCG of iteration 57
    # runs ONE iteration and that of iteration 63 NONE (the start vector already meets the tolerance) -- the two ways of leaving the loop
    # at once.  Found by a search over seeds 0..199 at n = 60, 96, 128: 198 of them hold a 0-iteration PCG, 158 a 1-iteration one; this
    # is the shortest solve among them.
    "pcg01": lambda: generated(60, 0),
}


class Snapshot:
    """What compare_state reads of an oracle, frozen after a window."""

    VECS = ("x", "z1", "z2", "z4", "f", "left_idx")
    SCALARS = ("rho1", "rho4", "gamma", "dI", "rho4Et", "std_obj", "cur_obj", "sum_fix_obj", "best_bin_obj", "cvg1", "cvg2", "obj_val")

    def __init__(self, o):
        self._v = {k: o.vec(k).copy() for k in self.VECS}
        self._s = {k: o.scalar(k) for k in self.SCALARS}

    def vec(self, name):
        return self._v[name]

    def scalar(self, name):
        return self._s[name]


def solver_in_mode(monkeypatch, I, mode):
    if mode == "generic":
        monkeypatch.setenv("LPBOX_LP_PCGLOOP", "generic")
    else:
        monkeypatch.delenv("LPBOX_LP_PCGLOOP", raising=False)
    g = gpu_solver(I)
    cfg = g.batch.config()                      # (uploads the problem: the switch is read here)
    monkeypatch.delenv("LPBOX_LP_PCGLOOP", raising=False)
    assert (cfg["threads"], cfg["elems_per_thread"]) == (512, 1)
    assert cfg["pcg_loop"] == mode
    return g


_ORACLE = {}


def oracle_windows(name, g, I):
    """Three windows of WS iterations with a scripted fix at the second, once per shape on the CPU oracle in the kernel's summation
    order (the layout does not depend on the loop mode): per window the return code, the iterates, the state and the counters."""
    if name not in _ORACLE:
        o = oracle_like(g, I)
        vec, num, out = np.zeros(I["n"]), 0, []
        for w in range(3):
            ret = o.solve_iter_l2f(w * WS, (w + 1) * WS, vec, num)
            x = o.get_x_iters_2d(WS)
            out.append(dict(vec=vec, num=num, ret=ret, x=x, state=Snapshot(o), counters=(o.total_outer_iters, o.total_pcg_iters), n=o.get_n(),
                            trace=o.pcg_trace()))
            if w == 0 and name != "pcg01":
                vec, num = scripted_fix_vec(x, lo=0.02, hi=0.98, last=20)
                assert 0 < num < I["n"], "the scripted vector must fix some variables and leave some"
            else:
                vec, num = np.zeros(o.get_n()), 0
            if ret:
                break
        _ORACLE[name] = out
    return _ORACLE[name]


def triples(cls):
    return {tuple(int(v) for v in c[:3]) for c in cls}


def check_classes(name, cls):
    assert cls.shape == (8, 4)
    no_tail_busy = [c for c in cls if c[3] == 0 and c[:3].sum() > 0]
    if name == "mixed":
        assert any(c[3] == 1 for c in cls) and no_tail_busy, f"one wave with a tail next to a busy one without: {cls.tolist()}"
    else:
        assert not cls[:, 3].any(), f"no list of these instances is longer than its registers: {cls.tolist()}"
    assert len(triples(cls)) >= 3, f"at least three wave classes in one workgroup: {cls.tolist()}"
    if name in ("n60", "n65", "pcg01"):
        assert (0, 0, 0) in triples(cls), "some wavefront holds neither a row task nor a column"
    if name == "n512":
        assert all(c[1] > 0 for c in cls), "every wavefront holds columns"


@pytest.mark.parametrize("name", list(SHAPES))
def test_three_windows_with_a_fix_bit_exact_in_both_modes(monkeypatch, name):
    I = SHAPES[name]()
    runs = {}
    for mode in MODES:
        g = solver_in_mode(monkeypatch, I, mode)
        check_classes(name, g.batch.wave_classes())
        want = oracle_windows(name, g, I)
        got = []
        for w, ow in enumerate(want):
            rg = g.solve_iter_l2f(w * WS, (w + 1) * WS, ow["vec"], ow["num"])
            assert rg == ow["ret"], f"{mode}, window {w}"
            xg = g.get_x_iters_2d(WS)
            assert bits_equal(xg, ow["x"]), f"{mode}, window {w}: iterates differ"
            compare_state(g, ow["state"], f"{mode}, window {w}")
            assert g.batch.counters() == ow["counters"], f"{mode}, window {w}"
            assert g.get_n() == ow["n"]
            got.append((rg, xg, {k: g.batch.debug_vec(k) for k in ("x", "z1", "z2", "z4", "f")}, g.batch.counters()))
        runs[mode] = got
    if name == "pcg01":
        trace = want[-1]["trace"]                # (of the window the solve stops in)
        assert 0 in trace and 1 in trace, f"the instance was picked for a PCG of 0 and one of 1 iteration: {sorted(set(trace.tolist()))}"
        assert want[-1]["ret"] == 1 and len(want) == 2, "it stops in the second window"
    else:
        assert len(want) == 3 and want[2]["n"] < I["n"], "the solve runs through all three windows, with fewer variables after the fix"
    for (ra, xa, va, ca), (rb, xb, vb, cb) in zip(runs["specialised"], runs["generic"]):
        assert ra == rb and ca == cb and bits_equal(xa, xb)
        for k in va:
            assert bits_equal(va[k], vb[k]), k


def test_four_instances_to_convergence_in_both_modes(monkeypatch):
    """Whole solves of four j = 20 / k = 60 instances as one batch: return code, iteration counts, final iterate, objective and binary
    solution against the oracle in the kernels' order, in both modes."""
    from lpbox_hip.lp import LpBatch
    insts = lp_instances("lp_20_60_seed0.npz")[:4]
    want = None
    for mode in MODES:
        if mode == "generic":
            monkeypatch.setenv("LPBOX_LP_PCGLOOP", "generic")
        B = LpBatch(insts)
        cfg = B.config()
        monkeypatch.delenv("LPBOX_LP_PCGLOOP", raising=False)
        assert cfg["pcg_loop"] == mode and (cfg["threads"], cfg["elems_per_thread"]) == (512, 1)
        B.solve_init()
        rets = B.solve_iter(0, 20000)
        if want is None:
            want = [oracle_full_solve((I, 512, 512, B.layout(i), B.row_split(i), B.col_split(i))) for i, I in enumerate(insts)]
        for i, (ret, outer, pcg, obj, x, xs) in enumerate(want):
            assert int(rets[i]) == ret and B.counters(i) == (outer, pcg), (mode, i)
            assert bits_equal(B.debug_vec("x", i), x) and B.cal_obj(i) == obj, (mode, i)
            assert np.array_equal(B.get_x_sol(i).ravel(), xs), (mode, i)


def test_other_geometries_report_the_generic_loop(monkeypatch):
    """Only the 512 x 1 kernel has specialised loops; the accessor of the wave classes is defined for it alone."""
    from lpbox_hip import _lib
    I = lp_instances("lp_100_500_seed0.npz")[0]
    monkeypatch.setenv("LPBOX_LP_THREADS", "256")
    g = gpu_solver(I)
    cfg = g.batch.config()
    monkeypatch.delenv("LPBOX_LP_THREADS")
    assert (cfg["threads"], cfg["elems_per_thread"]) == (256, 2) and cfg["pcg_loop"] == "generic"
    with pytest.raises(_lib.LpboxError):
        g.batch.wave_classes()
