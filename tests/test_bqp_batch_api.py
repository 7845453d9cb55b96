"""CPU tests of the batched small-BQP boundary (lpbox_bqp_batch_*, lpbox_hip.bqp.BqpBatch): the header declares the nine functions
and the library exports them, the Python-side refusals raise before the library is touched, and without a device the batch refuses
to exist (no CPU fallback)."""
import ctypes
import os
import re

import numpy as np
import pytest

from helpers import bqp_params, bqp_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["lpbox_bqp_batch_create", "lpbox_bqp_batch_destroy", "lpbox_bqp_batch_preset", "lpbox_bqp_batch_set_params",
         "lpbox_bqp_batch_set_problem", "lpbox_bqp_batch_solve", "lpbox_bqp_batch_get_vec", "lpbox_bqp_batch_get_scalar"]


def test_header_declares_and_library_exports_the_batch_functions():
    from lpbox_hip import _lib
    txt = open(os.path.join(ROOT, "include", "lpbox_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"typedef\s+struct\s+lpbox_bqp_batch\s+lpbox_bqp_batch_t\s*;", txt)      # the ninth declaration: the handle type
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, txt), f"{name} is not declared"
        assert hasattr(lib, name), f"liblpbox_hip.so does not export {name}"
        assert name in _lib.SYMBOLS
    assert re.search(r"lpbox_bqp_batch_set_problem\s*\(\s*lpbox_bqp_batch_t\s*\*h,\s*int idx,\s*int n,", txt)


def test_python_side_refusals_need_no_device(monkeypatch):
    from lpbox_hip import _lib, bqp
    assert hasattr(bqp, "BqpBatch") and hasattr(bqp, "solve_many")

    def touched(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", touched)
    P = bqp_problem(6, 1, 1, seed=1)
    with pytest.raises(ValueError):
        bqp.BqpBatch([])
    with pytest.raises(ValueError):
        bqp.BqpBatch([P, P], presets=[3])
    with pytest.raises(ValueError):
        bqp.BqpBatch([P, P], params=[bqp_params(3, 4)] * 3)
    with pytest.raises(ValueError):
        bqp.BqpBatch([P], params=[1.0, 2.0])
    with pytest.raises(TypeError):
        bqp.BqpBatch([P], params=dict(max_iters=4))
    with pytest.raises(TypeError):
        bqp.BqpBatch([P, P], params=[bqp_params(3, 4), dict(max_iters=4)])
    with pytest.raises(TypeError):
        bqp.BqpBatch([dict(n=3)])


def test_no_device_no_batch():
    from lpbox_hip import _lib
    from lpbox_hip.bqp import BqpBatch
    from lpbox_hip.lp import LpboxError
    L = _lib.load()
    P = bqp_problem(6, 1, 1, seed=1)
    if L.lpbox_device_count() == 0:
        with pytest.raises(LpboxError, match="no HIP device") as e:
            BqpBatch([P])
        assert e.value.code == _lib.E_NODEVICE
        assert not L.lpbox_bqp_batch_create(1, 0)
    # host-side argument checks of the C boundary that need no handle
    assert not L.lpbox_bqp_batch_create(0, 0)
    assert L.lpbox_bqp_batch_solve(None, None) < 0
    out = np.zeros(4)
    assert L.lpbox_bqp_batch_get_vec(None, 0, b"x", out, 4) < 0
