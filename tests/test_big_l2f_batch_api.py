"""CPU tests of the batched early-fixing boundary on the large route (lpbox_big_batch_iterate_l2f*, BigLpBatch.solve_iter_l2f*,
l2f.run_l2f_big_batch): the declarations, the refusals that need no device, the argument errors that come before
the library is touched, and the oracle pins tests/test_big_l2f_batch_gpu.py rests on."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import big_batch_cases as BC
import big_l2f_batch_cases as LC

E_BADARG, E_BADHANDLE = -2, -1
NAMES = ["lpbox_big_batch_set_active", "lpbox_big_batch_iterate_l2f", "lpbox_big_batch_get_x_iters_device", "lpbox_big_batch_iterate_l2f_scores"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_library_exports_python_binds():
    from lpbox_hip import _lib, big, l2f
    header = open(os.path.join(ROOT, "include", "lpbox_hip.h")).read()
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), f"include/lpbox_hip.h does not declare {name}"
        assert hasattr(lib, name), f"liblpbox_hip.so does not export {name}"
        assert name in _lib.SYMBOLS
    for meth in ("set_active", "solve_iter_l2f", "x_iters_torch", "solve_iter_l2f_scores"):
        assert hasattr(big.BigLpBatch, meth), meth
    assert hasattr(l2f, "run_l2f_big_batch")
    for word in ("active", "fix_launches", "packs", "compact_chunk"):
        assert '"%s"' % word in header, f"the header does not name the scalar {word}"


def test_null_handle_refusals():
    from lpbox_hip import _lib
    L = _lib.load()
    status = L.lpbox_last_status
    rets, fixed, off, ptr = (C.c_int * 1)(), (C.c_int * 1)(), (C.c_long * 2)(), C.c_void_p()
    assert L.lpbox_big_batch_set_active(None, None) < 0 and status() < 0
    assert L.lpbox_big_batch_iterate_l2f(None, 0, 10, None, 0, None, C.cast(rets, C.c_void_p)) < 0 and b"handle" in L.lpbox_last_error()
    assert L.lpbox_big_batch_get_x_iters_device(None, 10, C.byref(ptr), C.cast(off, C.c_void_p)) < 0 and b"handle" in L.lpbox_last_error()
    assert L.lpbox_big_batch_iterate_l2f_scores(None, 0, 10, None, 0.9, 0.1, 10, C.cast(rets, C.c_void_p), C.cast(fixed, C.c_void_p)) < 0
    assert b"handle" in L.lpbox_last_error() and ptr.value is None
    v = C.c_double()
    assert L.lpbox_big_batch_get_scalar(None, b"packs", C.byref(v)) == E_BADARG


def test_counters_and_argument_refusals_need_no_device():
    """A batch that was created but not initialised answers the new counters; argument errors come first, then the call order."""
    from lpbox_hip._lib import LpboxError
    from lpbox_hip.big import BigLp, BigLpBatch
    a, b = BigLp(BC.problem(300, 0)), BigLp(BC.problem(300, 1))
    B = BigLpBatch([a, b])
    assert (B.scalar("active"), B.scalar("fix_launches"), B.scalar("packs")) == (2.0, 0.0, 0.0)
    assert int(B.scalar("compact_chunk")) == LC.COMPACT_CHUNK and LC.SHRINK[0] == 2 * LC.COMPACT_CHUNK + 37
    B.set_active([True, False])
    assert B.scalar("active") == 1.0
    B.set_active(None)
    assert B.scalar("active") == 2.0
    for call, code, text in (
            (lambda: B.solve_iter_l2f(0, 501, None, [0, 0]), E_BADARG, "501"),
            (lambda: B.solve_iter_l2f(0, 10, None, [0, 301]), E_BADARG, "problem 1"),
            (lambda: B.solve_iter_l2f(0, 10, None, [0, -1]), E_BADARG, "problem 1"),
            (lambda: B.solve_iter_l2f(0, 10, None, [0, 5]), E_BADARG, "fix vector missing"),
            (lambda: B.solve_iter_l2f(0, 10, [None, np.r_[1.0, 0.0, -np.ones(298)]], [0, 3]), E_BADARG, "problem 1 of the batch: vec fixes 2"),
            (lambda: B.solve_iter_l2f(0, 10, None, [0, 0]), -3, "lpbox_big_batch_init"),
            (lambda: B.solve_iter_l2f_scores(0, 501, None), E_BADARG, "501"),
            (lambda: B.solve_iter_l2f_scores(0, 10, None), -3, "lpbox_big_batch_init")):
        with pytest.raises(LpboxError) as e:
            call()
        assert e.value.code == code and text in str(e.value), str(e.value)
    B.close()
    a.close()
    b.close()


def test_argument_errors_come_before_the_library(monkeypatch):
    from lpbox_hip import _lib, l2f
    from lpbox_hip.big import BigLpBatch

    class NoLib:
        def __getattr__(self, name):
            raise AssertionError(f"the library was called ({name})")

    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_load)
    B = BigLpBatch.__new__(BigLpBatch)
    B.solvers, B._own, B._L, B._h = [object(), object(), object()], [False] * 3, NoLib(), None
    with pytest.raises(ValueError, match="one entry per member"):
        B.set_active([True, False])
    with pytest.raises(ValueError, match="nums"):
        B.solve_iter_l2f(0, 10, None, [0, 0])
    with pytest.raises(ValueError, match="vecs"):
        B.solve_iter_l2f(0, 10, [None, None], [0, 0, 0])
    with pytest.raises(ValueError):
        l2f.run_l2f_big_batch([], lambda x: x)
    with pytest.raises(ValueError, match="member 0"):
        l2f.run_l2f_big_batch(["not a problem"], lambda x: x)


@pytest.mark.parametrize("n,seed", LC.MIXED)
def test_fix_pins(n, seed):
    """The scripted rule on the oracle: the fixes per window, every return 0 through window 7, the PCG counts (window 0 needs up to 21 /
    22 launch groups, the windows after it 4 to 9: LPBOX_BIG_KMAX=4 halts almost every iteration)."""
    snaps, x_sol = LC.oracle_l2f(n, seed)
    assert len(snaps) == LC.NWIN and all(s["ret"] == 0 for s in snaps)
    assert snaps[0]["num"] == 0 and tuple(s["num"] for s in snaps[1:]) == LC.FIXES[(n, seed)]
    assert all(len(s["trace"]) == LC.WS for s in snaps)
    assert max(snaps[0]["trace"]) == LC.PCG_W0_MAX[(n, seed)]
    later = [k for s in snaps[1:] for k in s["trace"]]
    assert LC.PCG_LATER[0] <= min(later) and max(later) <= LC.PCG_LATER[1]
    live = n
    for s in snaps:
        live -= s["num"]
        assert s["n_live"] == live and np.all(np.diff(s["left"]) > 0)
        assert s["num"] == 0 or s["num"] > LC.MIN_FIX
    assert set(np.unique(x_sol)) <= {0.0, 1.0}


def test_some_members_fix_while_others_do_not():
    """Windows 6 and 7: `apply == 0` beside `apply == 1` in one prologue; every earlier fixing window has all members fixing."""
    per_window = list(zip(*(LC.FIXES[c] for c in LC.MIXED)))
    assert all(all(k > 0 for k in w) for w in per_window[:5])
    for w in per_window[5:]:
        assert any(k == 0 for k in w) and any(k > 0 for k in w)
    assert {(min(LC.oracle_l2f(*c)[0][w]["trace"]) >= 4) for c in LC.MIXED for w in range(1, LC.NWIN)} == {True}


def test_shrinking_live_list_pins():
    """n = 2 * chunk + 37 under fixes that leave 4097, 4096, 4095, 1 and 0 live variables: the list lengths around the compaction's
    chunk boundary, and the all-fixed stop at the end."""
    snaps, x_sol = LC.oracle_shrink()
    assert LC.SHRINK[0] == 8229
    assert tuple(s["ret"] for s in snaps[1:]) == LC.SHRINK_RETS and snaps[0]["ret"] == 0
    assert tuple(s["n_live"] for s in snaps) == (8229,) + LC.SHRINK_LEFT
    assert snaps[-1]["stop"] == 4 and all(s["stop"] != 4 for s in snaps[:-1])            # LP_STOP_ALLFIXED
    for s in snaps[1:]:
        fixed = np.flatnonzero(s["vec"] != -1)
        assert len(fixed) == s["num"] and ((s["vec"] == 1).any() and (s["vec"] == 0).any() or s["num"] == 1)
    first = np.flatnonzero(snaps[1]["vec"] != -1)                                        # the first fix drops entries of all three chunks
    assert (first < 4096).any() and ((first >= 4096) & (first < 8192)).any() and (first >= 8192).any()
    assert set(np.unique(x_sol)) <= {0.0, 1.0}
