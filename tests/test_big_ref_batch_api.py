"""CPU tests of the batched large route in the reference summation order (lpbox_big_batch_* with every member in that order,
BigLpBatch(order="reference")): what is accepted and refused without a device, the argument errors that come
before the library is touched, and the pins on the oracle in ORDER_EIGEN that tests/test_big_ref_batch_gpu.py rests on."""
import numpy as np
import pytest

import big_ref_batch_cases as RC
from helpers import bits_equal

E_UNSUPPORTED = -7


def test_a_batch_in_the_reference_order_is_created():
    from lpbox_hip.big import BigLp, BigLpBatch
    P, Q = RC.problem((300, 0)), RC.problem((300, 1))
    a, b = BigLp(P, order="reference"), BigLp(Q, order="reference")
    B = BigLpBatch([a, b])                                   # borrowed handles keep their own order: the batch takes member 0's
    assert B.scalar("order") == 1.0 and B.scalar("count") == 2.0 and B.scalar("valued_members") == 0.0 and B.scalar("walks") == 0.0
    B.close()
    assert a.scalar("order") == 1.0                          # borrowed, not closed with the batch
    B = BigLpBatch([P, Q], order="reference")                # problem dicts become BigLp(m, order="reference")
    assert B.scalar("order") == 1.0 and all(s.order == "reference" and s.scalar("order") == 1.0 for s in B.solvers)
    B.close()
    B = BigLpBatch([P, Q])                                   # the default stays the default order
    assert B.scalar("order") == 0.0 and B.scalar("valued_members") == 0.0
    B.close()


def test_valued_members_are_accepted_and_counted():
    from lpbox_hip.big import BigLpBatch
    P = RC.problem((300, 0))
    ones = dict(P, vals=np.ones(len(P["rowidx"])))          # all ones: a unit instance
    B = BigLpBatch([RC.problem((300, 0), "set"), RC.problem((300, 1)), RC.problem((513, 2), "uniform"), ones], order="reference")
    assert B.scalar("order") == 1.0 and B.scalar("valued_members") == 2.0
    assert [s.scalar("valued") for s in B.solvers] == [1.0, 0.0, 1.0, 0.0]
    B.close()


def test_mixed_orders_are_refused_naming_the_member():
    from lpbox_hip._lib import LpboxError
    from lpbox_hip.big import BigLp, BigLpBatch
    r, d = BigLp(RC.problem((300, 0)), order="reference"), BigLp(RC.problem((300, 1)))
    with pytest.raises(LpboxError) as e:
        BigLpBatch([r, d])
    assert e.value.code == E_UNSUPPORTED and "problem 1" in str(e.value) and "reference summation order" in str(e.value)
    assert "default order" in str(e.value)
    with pytest.raises(LpboxError) as e:
        BigLpBatch([d, r])
    assert e.value.code == E_UNSUPPORTED and "problem 1" in str(e.value) and "reference summation order" in str(e.value)
    with pytest.raises(LpboxError) as e:                     # a borrowed handle keeps its order whatever the batch is asked for
        BigLpBatch([d, RC.problem((300, 0))], order="reference")
    assert e.value.code == E_UNSUPPORTED and "problem 1" in str(e.value)
    BigLpBatch([r]).close()                                  # both handles are usable afterwards
    BigLpBatch([d]).close()


def test_stored_values_in_the_default_order_leave_no_handle_open(monkeypatch):
    from lpbox_hip import _lib
    from lpbox_hip._lib import LpboxError
    from lpbox_hip.big import BigLpBatch
    L = _lib.load()
    opened, closed = [], []
    create, destroy = L.lpbox_big_create, L.lpbox_big_destroy

    class Spy:                                               # the loaded library with create / destroy counted
        def __getattr__(self, name):
            return getattr(L, name)

        def lpbox_big_create(self, *a):
            h = create(*a)
            opened.append(h)
            return h

        def lpbox_big_destroy(self, h):
            closed.append(h.value if hasattr(h, "value") else h)
            return destroy(h)

    monkeypatch.setattr(_lib, "load", lambda: Spy())
    with pytest.raises(LpboxError) as e:
        BigLpBatch([RC.problem((300, 0)), RC.problem((300, 1), "set")])          # order="default": BigLp's own refusal
    assert e.value.code == E_UNSUPPORTED and "lpbox_big_set_order" in str(e.value)
    import gc
    gc.collect()
    assert len(opened) == 2 and sorted(opened) == sorted(closed)


def test_order_is_checked_before_the_library_is_loaded(monkeypatch):
    from lpbox_hip import _lib
    from lpbox_hip.big import BigLpBatch, solve_many

    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_load)
    with pytest.raises(ValueError, match="order"):
        BigLpBatch([RC.problem((300, 0))], order="eigen")
    with pytest.raises(ValueError, match="order"):
        solve_many([RC.problem((300, 0))], order="eigen")


def test_early_fixing_calls_are_refused_without_a_device():
    """The order is looked at before anything else, the device included."""
    import ctypes as C
    from lpbox_hip import _lib
    from lpbox_hip._lib import LpboxError
    from lpbox_hip.big import BigLpBatch
    L = _lib.load()
    B = BigLpBatch([RC.problem((300, 0)), RC.problem((300, 1))], order="reference")
    with pytest.raises(LpboxError) as e:
        B.solve_iter_l2f(0, 5, None, np.zeros(2, np.int64))
    assert e.value.code == E_UNSUPPORTED and "reference summation order" in str(e.value) and "default order" in str(e.value)
    rets, fixed = np.zeros(2, np.int32), np.zeros(2, np.int32)
    assert L.lpbox_big_batch_iterate_l2f_scores(B._h, 0, 5, None, 0.9, 0.1, 10, rets.ctypes.data_as(C.c_void_p), fixed.ctypes.data_as(C.c_void_p)) == E_UNSUPPORTED
    ptr, off = C.c_void_p(), np.zeros(3, np.int64)
    assert L.lpbox_big_batch_get_x_iters_device(B._h, 5, C.byref(ptr), off.ctypes.data_as(C.c_void_p)) == E_UNSUPPORTED
    assert not ptr.value and B.scalar("launches") == 0.0 and B.scalar("fix_launches") == 0.0 and B.scalar("packs") == 0.0
    B.close()


# ---- the pins the GPU file rests on, on the oracle in ORDER_EIGEN ----
def test_pin_the_orders_differ():
    """x differs between the two orders after every window on every mixed-size instance: a batch that silently ran the default order
    cannot pass the GPU file."""
    for key in RC.MIXED:
        for w, (s, x) in enumerate(zip(RC.oracle_windows(key), RC.default_order_x(key))):
            assert not bits_equal(s["x"], x), (key, w)


def test_pin_pcg_counts_make_kmax_4_halt_every_iteration():
    """Over the 130 iterations the PCG needs 9 ... 22 iterations per outer iteration (unit), 18 ... 43 ("set") and 19 ... 50
    ("uniform"), so LPBOX_BIG_KMAX=4 halts every iteration.  (Re-derived; the issue's figures were 10 ... 21 and up to 35.)"""
    from chain_cases import expected_resumes
    span = {}
    for fam in (None, "set", "uniform"):
        lo, hi = [], []
        for key in RC.MIXED:
            trace = np.concatenate([w["trace"] for w in RC.oracle_windows(key, fam)])
            assert len(trace) == 130 and trace.min() > 4
            lo.append(trace.min())
            hi.append(trace.max())
        span[fam] = (min(lo), max(hi))
    assert span == {None: (9, 22), "set": (18, 43), "uniform": (19, 50)}
    members = [((300, 0), None), ((513, 2), None), ((1100, 4), None), ((300, 0), "set")]
    want = [expected_resumes(RC.oracle_windows(key, fam, ((0, 40),))[0]["trace"], 4) for (key, fam) in members]
    assert want == [41, 41, 41, 75]
    assert {(-(-n // RC.CHUNK), -(-RC.problem((n, s))["l"] // RC.CHUNK)) for (n, s) in RC.MIXED} == {(1, 1), (2, 1), (3, 1), (5, 2), (6, 3)}


@pytest.mark.parametrize("key", sorted(RC.OWN_STOPS))
def test_pin_own_stops(key):
    s = RC.oracle_solve(key)
    assert (s["stop"], s["plain_iter_p1"], s["ret"]) == RC.OWN_STOPS[key]
    assert s["outer_total"] == s["plain_iter_p1"]


def test_pin_own_stops_cover_both_rules():
    stops = RC.OWN_STOPS.values()
    assert {s[0] for s in stops} == {1, 2} and len({s[1] for s in stops}) == 3
    assert {-(-n // RC.CHUNK) for (n, _) in RC.OWN_STOPS} == {1, 2}


@pytest.mark.parametrize("family", [None, "set"])
def test_pin_odd_sizes(family):
    """Which odd members stop inside the second window, and where; nobody produces a NaN or moves pow_sqrt_mismatch."""
    stops = {}
    for n in RC.ODD_NS:
        P = RC.problem(("odd", n), family)
        assert P["n"] == n != P["l"] and np.any(np.diff(P["colptr"]) == 1)
        snaps = RC.oracle_windows(("odd", n), family, RC.ODD_WINDOWS)
        assert snaps[0]["stop"] == 0 and snaps[0]["outer_total"] == 7
        s = snaps[1]
        assert s["pow_sqrt_mismatch"] == 0 and not any(np.isnan(s[v]).any() for v in RC.VECS)
        if s["stop"]:
            assert s["stop"] == 1
            stops[n] = (s["outer_total"], s["pcg_total"])
        else:
            assert s["outer_total"] == 60
    assert stops == RC.ODD_STOPS[family]
