"""CPU tests of the batched large-route boundary (lpbox_big_batch_*, lpbox_hip.big.BigLpBatch): the declarations, the argument errors
that come before the library is touched, what _create refuses without a device, and the oracle pins tests/test_big_batch_gpu.py
rests on."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import big_batch_cases as BC

E_BADARG, E_STATE, E_NODEVICE, E_UNSUPPORTED = -2, -3, -6, -7
NAMES = ["lpbox_big_batch_create", "lpbox_big_batch_destroy", "lpbox_big_batch_init", "lpbox_big_batch_iterate", "lpbox_big_batch_get_scalar"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_library_exports_python_binds():
    from lpbox_hip import _lib, big
    header = open(os.path.join(ROOT, "include", "lpbox_hip.h")).read()
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), f"include/lpbox_hip.h does not declare {name}"
        assert hasattr(lib, name), f"liblpbox_hip.so does not export {name}"
        assert name in _lib.SYMBOLS
    assert "typedef struct lpbox_big_batch lpbox_big_batch_t;" in header
    assert hasattr(big, "BigLpBatch") and hasattr(big, "solve_many")


def test_argument_errors_come_before_the_library(monkeypatch):
    from lpbox_hip import _lib
    from lpbox_hip.big import BigLpBatch, solve_many

    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_load)
    with pytest.raises(ValueError):
        BigLpBatch([])
    with pytest.raises(ValueError):
        BigLpBatch(None)
    with pytest.raises(ValueError, match="member 1"):
        BigLpBatch([BC.problem(300, 0), "not a problem"])
    with pytest.raises(ValueError, match="member 0"):
        BigLpBatch([dict(n=3, l=2)])                         # a dict, but not a problem
    with pytest.raises(ValueError):
        solve_many([])


def test_create_refuses_without_a_device_call():
    from lpbox_hip import _lib
    from lpbox_hip._lib import LpboxError
    from lpbox_hip.big import BigLp, BigLpBatch
    L = _lib.load()
    assert not L.lpbox_big_batch_create(None, 0)
    assert L.lpbox_last_status() == E_BADARG and b"empty" in L.lpbox_last_error()
    a, b = BigLp(BC.problem(300, 0)), BigLp(BC.problem(300, 1))
    assert not L.lpbox_big_batch_create((C.c_void_p * 1)(a._h), 0)
    assert L.lpbox_last_status() == E_BADARG

    def refused(members):
        with pytest.raises(LpboxError) as e:
            BigLpBatch(members)
        return e.value

    e = refused([a, b, a])
    assert e.code == E_BADARG and "problem 0 and problem 2" in str(e) and "same handle" in str(e)
    e = refused([a, BigLp(BC.problem(300, 1), device=1)])
    assert e.code == E_BADARG and "problem 1" in str(e) and "another device" in str(e)
    raw = C.c_void_p(L.lpbox_big_create(0, 1, 0))            # a handle without a problem
    assert not L.lpbox_big_batch_create((C.c_void_p * 2)(a._h, raw), 2)
    assert L.lpbox_last_status() == E_STATE and b"problem 1" in L.lpbox_last_error()
    L.lpbox_big_destroy(raw)
    e = refused([a, BigLp(BC.problem(300, 1), order="reference")])
    assert e.code == E_UNSUPPORTED and "problem 1" in str(e) and "reference summation order" in str(e)
    e = refused([BigLp(BC.problem(300, 1), pcg_mode="lean"), a])
    assert e.code == E_UNSUPPORTED and "problem 0" in str(e) and "comm-lean" in str(e)
    assert L.lpbox_big_set_record(b._h, 1) == 0
    e = refused([a, b])
    assert e.code == E_UNSUPPORTED and "problem 1" in str(e) and "recording" in str(e)
    assert L.lpbox_big_set_record(b._h, 0) == 0

    B = BigLpBatch([a, b])                                   # and now it is accepted -- without a device call
    assert len(B) == 2 and B[1] is b and B.scalar("count") == 2.0 and B.scalar("pcg_resumes_1") == 0.0
    with pytest.raises(LpboxError) as e:
        B.solve_iter(0, 5)                                   # before solve_init
    assert e.value.code == E_STATE and "lpbox_big_batch_init has not been called" in str(e.value)
    with pytest.raises(LpboxError) as e:
        B.scalar("pcg_resumes_2")
    assert e.value.code == E_BADARG
    if L.lpbox_device_count() < 1:                           # no CPU fallback
        with pytest.raises(LpboxError, match="no HIP device") as e:
            B.solve_init()
        assert e.value.code == E_NODEVICE
    B.close()
    assert a.scalar("order") == 0.0                          # the members are still there: borrowed, not closed with the batch
    assert L.lpbox_big_batch_init(None) < 0 and L.lpbox_big_batch_iterate(None, 0, 5, None) < 0


@pytest.mark.parametrize("n,seed", sorted(BC.OWN_STOPS))
def test_own_stop_pins(n, seed):
    """Where each instance of the own-stops test stops on the oracle: both stop rules, four different iterations."""
    s = BC.oracle_solve(n, seed)
    assert (s["stop"], s["plain_iter_p1"], s["ret"]) == BC.OWN_STOPS[(n, seed)]
    assert s["outer_total"] == s["plain_iter_p1"]


def test_own_stops_cover_both_rules_and_both_group_counts():
    stops = BC.OWN_STOPS.values()
    assert {s[0] for s in stops} == {1, 2} and len({s[1] for s in stops}) == 4
    assert {-(-n // BC.CHUNK) for (n, _) in BC.OWN_STOPS} == {1, 2}


def test_pcg_counts_make_kmax_4_halt_every_iteration():
    """The PCG needs 9 ... 22 iterations in the first 130 outer iterations of every mixed-size instance: a chain with LPBOX_BIG_KMAX=4
    halts in every iteration, once (K <= 20) or twice."""
    from chain_cases import expected_resumes
    for (n, seed) in BC.MIXED:
        trace = np.concatenate([w["trace"] for w in BC.oracle_windows(n, seed)])
        assert len(trace) == 130 and trace.min() > 4 and 20 <= trace.max() <= 22, (n, seed, trace.min(), trace.max())
        assert 130 <= expected_resumes(trace, 4) <= 260
    assert {(-(-n // BC.CHUNK), -(-BC.problem(n, s)["l"] // BC.CHUNK)) for (n, s) in BC.MIXED} == {(1, 1), (2, 1), (3, 1), (5, 2), (6, 3)}
