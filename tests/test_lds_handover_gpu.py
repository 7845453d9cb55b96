"""The assumption behind lds_handover() (csrc/lpbox_dev_common.h), stressed on its own: a workgroup barrier WITHOUT a drain of the LDS
counter in front of it still hands a value written to LDS over to the other wavefronts -- a ds_read issued behind the barrier sees every
ds_write issued in front of it, and a ds_write behind it does not overtake a ds_read in front of it.

lpbox_debug_handover runs 20 000 rounds on ONE 512-vector in LDS, 256 workgroups at once (every CU busy, two wavefronts per SIMD as in the
solver).  A round: thread t writes v to element t; barrier; it adds L gathered elements in order (positions from a seeded permutation,
held in registers); barrier; block_sum of the sums with the window kernel's second stage; the next v is formed from the thread's sum and
the block total.  The same buffer is written in every round, so both directions are exercised, and one stale read changes every value
after it.  Every thread's last value and the block totals of every round are compared bit for bit with a numpy restatement.

Cases: L = 1, 2, 12 in every wavefront; L = 12 in wavefronts 0-3 and 1 in 4-7 and the reverse (a fast wavefront's read directly behind a
slow one's write, and its next write directly behind the slow one's read); one case with block_sum<2>.  Each also runs with
__syncthreads() in place of the bare barrier, which shows that the restatement is right."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T, GROUPS, ROUNDS, LMAX = 512, 256, 20000, 12
FORM_SYNC, FORM_HANDOVER = 0, 1
CASES = {                      # name -> (nv, L of wavefronts 0-3, L of wavefronts 4-7)
    "L1": (1, 1, 1),
    "L2": (1, 2, 2),
    "L12": (1, 12, 12),
    "L12_then_L1": (1, 12, 1),
    "L1_then_L12": (1, 1, 12),
    "L12_two_values": (2, 12, 12),
}


def setup_vectors():
    rs = np.random.RandomState(20240)
    pos = np.stack([rs.permutation(T) for _ in range(LMAX)]).astype(np.int32)       # pos[q, t]: the q-th element thread t reads
    v0 = rs.uniform(0.0, 1.0, T)
    return pos, v0


POS, V0 = setup_vectors()


def tree_sum(a):
    """a: (T,) per-thread partials -> the total in the kernels' association: inside a wavefront the partner lanes xor 32, 16, 1, 2, 4, 8,
    then the wave partials xor 1, 2, 4.  Addition is commutative, so folding each step onto the lower partner gives lane 0's bits."""
    w = a.reshape(T // 64, 2, 32)
    w = w[:, 0] + w[:, 1]                      # xor 32
    w = w.reshape(-1, 2, 16)
    w = w[:, 0] + w[:, 1]                      # xor 16 -> (8, 16)
    for _ in range(4):                         # xor 1, 2, 4, 8
        w = w.reshape(w.shape[0], -1, 2)
        w = w[:, :, 0] + w[:, :, 1]
    p = w.reshape(-1)
    for _ in range(3):                         # waves xor 1, 2, 4
        p = p.reshape(-1, 2)
        p = p[:, 0] + p[:, 1]
    return p[0]


def restate(nv, l_lo, l_hi):
    """The rounds in numpy float64: the same expressions in the same order, no fused multiply-add."""
    L = np.where(np.arange(T) < T // 2, l_lo, l_hi)
    ct = np.arange(T, dtype=np.float64) * (1.0 / 1024.0)
    masks = [L > q for q in range(LMAX)]
    lmax = max(l_lo, l_hi)
    v = V0.copy()
    totals = np.empty((ROUNDS, nv))
    for r in range(ROUNDS):
        g = v[POS[:lmax]]                      # (lmax, T)
        s = g[0].copy()
        for q in range(1, lmax):
            s = np.where(masks[q], s + g[q], s) if l_lo != l_hi else s + g[q]
        tot = tree_sum(s)
        totals[r, 0] = tot
        u = s * 1.37 + tot * 0.113
        if nv == 2:
            tot1 = tree_sum(v)
            totals[r, 1] = tot1
            u = u + tot1 * 0.0271
        u = u + ct
        v = u - np.floor(u)
    return v, totals


_EXPECTED = {}


def expected(name):
    if name not in _EXPECTED:
        _EXPECTED[name] = restate(*CASES[name])
    return _EXPECTED[name]


def run(form, name):
    from lpbox_hip import _lib
    nv, l_lo, l_hi = CASES[name]
    last, totals = np.empty((GROUPS, T)), np.empty((GROUPS, ROUNDS, nv))
    _lib.check(_lib.load().lpbox_debug_handover(form, nv, l_lo, l_hi, GROUPS, ROUNDS, POS, V0, last, totals), "lpbox_debug_handover")
    return last, totals


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("form", [FORM_SYNC, FORM_HANDOVER], ids=["syncthreads", "handover"])
def test_handover_rounds_match_the_restatement(form, name):
    last, totals = run(form, name)
    want_last, want_totals = expected(name)
    assert np.all((want_last >= 0) & (want_last < 1)) and len(np.unique(want_last)) > T // 2, "the restatement keeps the values apart"
    tu, wu = totals.view(np.uint64), want_totals.view(np.uint64)
    bad = np.argwhere((tu != wu[None]).any(axis=2))
    assert bad.size == 0, f"{name}: block totals differ first in workgroup {bad[0][0]}, round {bad[:, 1].min()} ({len(set(bad[:, 0]))} workgroups)"
    assert np.array_equal(last.view(np.uint64), np.broadcast_to(want_last, last.shape).view(np.uint64)), f"{name}: final values differ"


def test_unbuilt_combination_is_rejected():
    from lpbox_hip import _lib
    last, totals = np.empty((1, T)), np.empty((1, 4, 1))
    with pytest.raises(_lib.LpboxError):
        _lib.check(_lib.load().lpbox_debug_handover(FORM_HANDOVER, 1, 3, 3, 1, 4, POS, V0, last, totals))
    with pytest.raises(_lib.LpboxError):
        _lib.check(_lib.load().lpbox_debug_handover(2, 1, 1, 1, 1, 4, POS, V0, last, totals))
