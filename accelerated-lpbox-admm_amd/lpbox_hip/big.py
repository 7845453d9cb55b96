"""One large LP, variable-sharded over the ranks of a process group (BASELINE config 5).

Every rank holds a contiguous block of columns of E and runs the large-instance kernels of liblpbox_hip.so on its GPU.  Where the
algorithm sums over all variables (E*v: an l-vector per PCG iteration; a handful of scalars per reduction) the ranks exchange their
contributions and every rank adds them in rank order (reproducible; exact CPU model in the oracle).  Transport:

* `transport="rccl"` (default when torch.distributed runs on "nccl"): the LIBRARY drives RCCL itself on its stream -- grouped
  send/recv of row blocks + one all-gather per E*v, one all-gather per scalar group; Python only hands the 128-byte communicator id
  from rank 0 to the others once (control plane).
* `transport="callback"` (default on "gloo", used by the tests on the one-GPU box): the library calls back into `_allgather`, a
  `torch.distributed.all_gather` through host staging.

With world == 1 no collective is issued and torch is not needed (transport="rccl" with world == 1 builds a one-rank communicator
and runs the whole exchange path against itself: a test of that path on a single GPU).
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check
from .dist import shard_range


def _dev_tensor(ptr, count):
    """Zero-copy torch view of `count` doubles of device memory owned by the library."""
    import torch

    class _Dev:
        __cuda_array_interface__ = {"shape": (int(count),), "typestr": "<f8", "data": (int(ptr), False), "version": 2}
    return torch.as_tensor(_Dev(), device="cuda")


class BigLp:
    def __init__(self, problem, rank=0, world=1, device=0, use_torch_stream=None, transport=None, pcg_mode="reference", order="default"):
        """problem: dict(n, l, colptr, rowidx, b[, f][, vals]) of the WHOLE instance (CSC, b already negated).

        order="reference": the reference's summation order (lpbox_big_set_order; one rank, no transport, the reference's PCG), bit-exact
        against the oracle in ORDER_EIGEN; only then may problem["vals"] (the stored values of E in the order of rowidx) differ from 1."""
        if order not in ("default", "reference"):
            raise ValueError("order must be 'default' or 'reference'")
        self.order = order
        self._L = _lib.load()
        self.rank, self.world = int(rank), int(world)
        n, l = int(problem["n"]), int(problem["l"])
        self.n, self.l = n, l
        self.c0, self.c1 = shard_range(n, world, rank)
        cp = np.asarray(problem["colptr"], np.int64)
        lo, hi = cp[self.c0], cp[self.c1]
        colptr = np.ascontiguousarray(cp[self.c0:self.c1 + 1] - lo, np.int32)
        rowidx = np.ascontiguousarray(np.asarray(problem["rowidx"])[lo:hi], np.int32)
        b = np.ascontiguousarray(np.asarray(problem["b"], np.float64)[self.c0:self.c1])
        f = problem.get("f")
        h = self._L.lpbox_big_create(self.rank, self.world, int(device))
        if not h:
            check(-2, "lpbox_big_create")
        self._h = C.c_void_p(h)
        if transport is None and world > 1:
            import torch.distributed as dist
            transport = "rccl" if dist.get_backend() == "nccl" else "callback"
        self.transport = transport
        self._stream = None
        if world > 1 or use_torch_stream or transport:
            import torch
            torch.cuda.set_device(device)
            self._stream = torch.cuda.current_stream()
            check(self._L.lpbox_big_set_stream(self._h, C.c_void_p(self._stream.cuda_stream)), "lpbox_big_set_stream")
        if transport == "rccl":
            uid = (C.c_ubyte * 128)()
            if self.rank == 0:
                check(self._L.lpbox_big_rccl_unique_id(uid), "lpbox_big_rccl_unique_id")
            if world > 1:                                    # control plane: the id travels once, through whatever group exists
                import torch
                import torch.distributed as dist
                t = torch.tensor(list(bytes(uid)), dtype=torch.uint8, device="cuda" if dist.get_backend() == "nccl" else "cpu")
                dist.broadcast(t, 0)
                uid = (C.c_ubyte * 128)(*t.cpu().tolist())
            check(self._L.lpbox_big_rccl_init(self._h, uid), "lpbox_big_rccl_init")
        elif transport == "callback":
            self._cb = _lib.ALLGATHER_FN(self._allgather)
            check(self._L.lpbox_big_set_allgather(self._h, C.cast(self._cb, C.c_void_p), None), "lpbox_big_set_allgather")
        elif world > 1:
            raise ValueError(f"unknown transport {transport!r}")
        fp = None
        if f is not None:
            f = np.ascontiguousarray(f, np.float64)
            fp = f.ctypes.data_as(C.c_void_p)
        if order == "reference":                             # after the transport: the library refuses the combination, either call order
            check(self._L.lpbox_big_set_order(self._h, 1), "lpbox_big_set_order")
        vals = problem.get("vals")
        if vals is None:
            check(self._L.lpbox_big_set_problem(self._h, n, self.c0, self.c1 - self.c0, l, colptr, rowidx, b, fp), "lpbox_big_set_problem")
        else:
            vals = np.ascontiguousarray(np.asarray(vals, np.float64)[lo:hi])
            check(self._L.lpbox_big_set_problem_vals(self._h, n, self.c0, self.c1 - self.c0, l, colptr, rowidx, b, fp,
                                                     vals.ctypes.data_as(C.c_void_p)), "lpbox_big_set_problem_vals")
        self._nnz = int(colptr[-1])
        if pcg_mode not in ("reference", "lean"):
            raise ValueError("pcg_mode must be 'reference' or 'lean'")
        if pcg_mode == "lean":       # opt-in comm-lean PCG: not the reference's arithmetic (lpbox_big_set_pcg_mode in include/lpbox_hip.h)
            check(self._L.lpbox_big_set_pcg_mode(self._h, 1), "lpbox_big_set_pcg_mode")

    def _allgather(self, send_ptr, count, recv_ptr, user):
        """recv[r*count:(r+1)*count] := rank r's send[0:count], ordered on the library's stream."""
        try:
            import torch
            import torch.distributed as dist
            with torch.cuda.stream(self._stream):
                send = _dev_tensor(send_ptr, count)
                recv = _dev_tensor(recv_ptr, count * self.world)
                if self.world == 1:
                    recv.copy_(send)
                elif dist.get_backend() == "nccl":
                    dist.all_gather_into_tensor(recv, send)
                else:                       # gloo (tests): stage through the host
                    c = send.cpu()
                    parts = [torch.empty_like(c) for _ in range(self.world)]
                    dist.all_gather(parts, c)
                    recv.copy_(torch.cat(parts))
            return 0
        except Exception as e:          # never let an exception cross the C boundary
            print("lpbox big all-gather failed:", e)
            return 1

    def close(self):
        if getattr(self, "_h", None):
            self._L.lpbox_big_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def solve_init(self):
        return check(self._L.lpbox_big_init(self._h), "lpbox_big_init")

    def solve_iter(self, i, j):
        ret = C.c_int()
        check(self._L.lpbox_big_iterate(self._h, int(i), int(j), C.byref(ret)), "lpbox_big_iterate")
        return ret.value

    def local_x(self):
        out = np.zeros(self.c1 - self.c0)
        check(self._L.lpbox_big_get_x(self._h, out), "lpbox_big_get_x")
        return out

    def vec(self, name):
        out = np.zeros(max(self.c1 - self.c0, self.l, self._nnz if name in ("r4v", "vals") else 1))
        k = check(self._L.lpbox_big_get_vec(self._h, name.encode(), out, len(out)), "lpbox_big_get_vec")
        return out[:k].copy()

    def scalar(self, name):
        v = C.c_double()
        check(self._L.lpbox_big_get_scalar(self._h, name.encode(), C.byref(v)), "lpbox_big_get_scalar")
        return v.value

    def cal_Obj(self):
        v = C.c_double()                       # LPcpp:1630-1642
        check(self._L.lpbox_big_cal_obj(self._h, C.byref(v)), "lpbox_big_cal_obj")
        return v.value

    # ---- early fixing on the sharded instance (ADMM_lp_iters_l2f, LPcpp:1098-1574) ----
    def get_n(self):
        """Live variables of THIS rank."""
        return check(self._L.lpbox_big_get_n(self._h), "lpbox_big_get_n")

    def solve_iter_l2f(self, i, j, vec_local=None, num_global=0):
        """vec_local: fix vector over this rank's live variables (1 / 0 fix, -1 leave); num_global: fixes over all ranks
        (None: count the local ones and sum them over the process group)."""
        vp = None
        if vec_local is not None:
            vec_local = np.ascontiguousarray(vec_local, np.float64).ravel()
            if vec_local.shape[0] < self.get_n():
                raise ValueError("fix vector shorter than this rank's live variables")
            vp = vec_local.ctypes.data_as(C.c_void_p)
        if num_global is None:
            k = 0 if vec_local is None else int(np.count_nonzero((vec_local[:self.get_n()] == 1) | (vec_local[:self.get_n()] == 0)))
            num_global = self.sum_over_ranks(k)
        ret = C.c_int()
        check(self._L.lpbox_big_iterate_l2f(self._h, int(i), int(j), vp, int(num_global), C.byref(ret)), "lpbox_big_iterate_l2f")
        return ret.value

    def sum_over_ranks(self, k):
        if self.world == 1:
            return int(k)
        import torch
        import torch.distributed as dist
        t = torch.tensor([int(k)], dtype=torch.int64, device="cuda" if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(t)
        return int(t.item())

    def get_x_iters_2d(self, ws):
        rows = check(self._L.lpbox_big_get_x_iters(self._h, int(ws), None), "lpbox_big_get_x_iters")
        out = np.zeros((rows, int(ws)))
        if rows:
            check(self._L.lpbox_big_get_x_iters(self._h, int(ws), out.ctypes.data_as(C.c_void_p)), "lpbox_big_get_x_iters")
        return out

    def x_iters_torch(self, ws):
        """This rank's (rows x ws) iterate windows as a zero-copy torch CUDA tensor."""
        import torch
        ptr, rows = C.c_void_p(), C.c_int()
        check(self._L.lpbox_big_get_x_iters_device(self._h, int(ws), C.byref(ptr), C.byref(rows)), "lpbox_big_get_x_iters_device")
        if rows.value == 0:
            return torch.zeros((0, int(ws)), dtype=torch.float64, device="cuda")

        class _Dev:
            __cuda_array_interface__ = {"shape": (rows.value * int(ws),), "typestr": "<f8", "data": (ptr.value, False), "version": 2}
        return torch.as_tensor(_Dev(), device="cuda").view(rows.value, int(ws))

    def local_x_sol(self):
        out = np.zeros(self.c1 - self.c0)
        check(self._L.lpbox_big_get_x_sol(self._h, out), "lpbox_big_get_x_sol")
        return out


def _is_problem(p):
    return isinstance(p, dict) and all(k in p for k in ("n", "l", "colptr", "rowidx", "b"))


class BigLpBatch:
    """A batch of large-route instances through ONE launch chain in lockstep (lpbox_big_batch_* in include/lpbox_hip.h): plain windows
    of all members at once, each member on its own control state, bit for bit what `BigLp.solve_iter` gives it alone.

    members: problem dicts (a `BigLp(m, device=device, order=order)` is built for each and closed with the batch) and / or `BigLp`
    objects (borrowed: one rank, no transport, reference PCG; they keep their own order).  All members run in one summation order, member
    0's: the library refuses a mismatch.  order="reference": per member the bits of `BigLp(order="reference")`, i.e. the oracle's in
    ORDER_EIGEN; only then may a problem carry `vals`, and the early-fixing calls are refused.  `batch[k]` is member k's `BigLp`: its
    getters, and a `solve_iter` of its own, work between the batch's windows."""

    def __init__(self, members, device=0, order="default"):
        if order not in ("default", "reference"):
            raise ValueError("order must be 'default' or 'reference'")
        self.order = order
        members = list(members) if members is not None else []
        if not members:
            raise ValueError("BigLpBatch needs at least one problem")
        for k, m in enumerate(members):
            if not isinstance(m, BigLp) and not _is_problem(m):
                raise ValueError(f"member {k} is neither a BigLp nor a problem dict (n, l, colptr, rowidx, b)")
        self._L = _lib.load()
        self._own = [not isinstance(m, BigLp) for m in members]
        self.solvers = []
        try:
            for m in members:
                if isinstance(m, BigLp):
                    self.solvers.append(m)
                    continue
                s = BigLp.__new__(BigLp)
                try:
                    s.__init__(m, device=device, order=order)
                except Exception:                            # BigLp's own error (e.g. stored values in the default order) ...
                    s.close()                                # ... and its handle does not wait for the garbage collector
                    raise
                self.solvers.append(s)
        except Exception:                                    # no handle of ours stays open
            for s, own in zip(self.solvers, self._own):
                if own:
                    s.close()
            raise
        arr = (C.c_void_p * len(self.solvers))(*[s._h for s in self.solvers])
        h = self._L.lpbox_big_batch_create(arr, len(self.solvers))
        if not h:
            rc = self._L.lpbox_last_status()
            for s, own in zip(self.solvers, self._own):
                if own:
                    s.close()
            check(rc if rc < 0 else -2, "lpbox_big_batch_create")
        self._h = C.c_void_p(h)

    def __len__(self):
        return len(self.solvers)

    def __getitem__(self, k):
        return self.solvers[k]

    def close(self):
        if getattr(self, "_h", None):
            self._L.lpbox_big_batch_destroy(self._h)
            self._h = None
            for s, own in zip(self.solvers, self._own):
                if own:
                    s.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def solve_init(self):
        return check(self._L.lpbox_big_batch_init(self._h), "lpbox_big_batch_init")

    def solve_iter(self, i, j):
        """Iterations [i, j) of every member (ADMM_lp_iters); the members' return values as an int32 array."""
        rets = np.zeros(len(self.solvers), np.int32)
        check(self._L.lpbox_big_batch_iterate(self._h, int(i), int(j), rets.ctypes.data_as(C.c_void_p)), "lpbox_big_batch_iterate")
        return rets

    def scalar(self, name):
        v = C.c_double()
        check(self._L.lpbox_big_batch_get_scalar(self._h, name.encode(), C.byref(v)), "lpbox_big_batch_get_scalar")
        return v.value

    # ---- early-fixing windows of all active members in one lockstep chain (lpbox_big_batch_iterate_l2f* in include/lpbox_hip.h) ----
    def set_active(self, mask):
        """mask: one truth value per member, or None for all.  It governs solve_iter_l2f, x_iters_torch and solve_iter_l2f_scores;
        solve_iter keeps running every member."""
        if mask is None:
            return check(self._L.lpbox_big_batch_set_active(self._h, None), "lpbox_big_batch_set_active")
        m = np.ascontiguousarray(np.asarray(mask).astype(bool).astype(np.uint8))
        if m.shape != (len(self.solvers),):
            raise ValueError("mask must have one entry per member")
        return check(self._L.lpbox_big_batch_set_active(self._h, m.ctypes.data_as(C.c_void_p)), "lpbox_big_batch_set_active")

    def solve_iter_l2f(self, i, j, vecs, nums):
        """vecs: one fix vector per member over its live variables (1 / 0 fix, anything else leave) or None, or None for all; nums: the
        members' fix counts.  Returns the int32 array of return values (entries of inactive members stay 0)."""
        B = len(self.solvers)
        nums = np.ascontiguousarray(nums, np.int64).ravel()
        if nums.shape[0] != B:
            raise ValueError("nums must have one entry per member")
        ptr, stride = None, 0
        if vecs is not None:
            vecs = list(vecs)
            if len(vecs) != B:
                raise ValueError("vecs must have one entry (an array or None) per member")
            vecs = [None if v is None else np.asarray(v, np.float64).ravel() for v in vecs]
            stride = max([v.shape[0] for v in vecs if v is not None], default=0)
            if stride:
                flat = np.full((B, stride), -1.0)
                for k, v in enumerate(vecs):
                    if v is not None:
                        flat[k, :v.shape[0]] = v
                ptr = flat.ctypes.data_as(C.c_void_p)
        rets = np.zeros(B, np.int32)
        check(self._L.lpbox_big_batch_iterate_l2f(self._h, int(i), int(j), ptr, stride, nums.ctypes.data_as(C.c_void_p),
                                                  rets.ctypes.data_as(C.c_void_p)), "lpbox_big_batch_iterate_l2f")
        return rets

    def x_iters_torch(self, ws):
        """(tensor (rows, ws) float64, zero-copy on the device; row_off int64 (members + 1)): rows row_off[k] .. row_off[k+1] are member
        k's live variables when its window started, in ascending original index (none for an inactive member).  Valid until the next call
        on the batch."""
        import torch
        ws = int(ws)
        ptr = C.c_void_p()
        off = np.zeros(len(self.solvers) + 1, np.int64)
        check(self._L.lpbox_big_batch_get_x_iters_device(self._h, ws, C.byref(ptr), off.ctypes.data_as(C.c_void_p)),
              "lpbox_big_batch_get_x_iters_device")
        rows = int(off[-1])
        self._packed_rows = rows
        if rows == 0:
            return torch.zeros((0, ws), dtype=torch.float64, device="cuda"), off
        return _dev_tensor(ptr.value, rows * ws).view(rows, ws), off

    def solve_iter_l2f_scores(self, i, j, scores, C=0.9, min_fix=10):
        """The window with deter_fix_2 (threshold C: hi = C, lo = 1 - C) and the `<= min_fix -> none` guard applied on the device:
        scores = float32 CUDA tensor, one score per row of the last x_iters_torch(), or None (fix nothing).  Returns (rets, fixed),
        int32 arrays."""
        import ctypes
        ptr = None
        if scores is not None:
            import torch
            if not (scores.is_cuda and scores.dtype == torch.float32):
                raise TypeError("scores must be a float32 CUDA tensor")
            scores = scores.contiguous().reshape(-1)
            if scores.numel() != getattr(self, "_packed_rows", -1):
                raise ValueError("scores must hold one entry per row of the last x_iters_torch()")
            torch.cuda.current_stream(scores.device).synchronize()      # the batch runs on a stream of its own
            ptr = ctypes.c_void_p(scores.data_ptr())
        B = len(self.solvers)
        rets, fixed = np.zeros(B, np.int32), np.zeros(B, np.int32)
        check(self._L.lpbox_big_batch_iterate_l2f_scores(self._h, int(i), int(j), ptr, float(C), 1 - float(C), int(min_fix),
                                                         rets.ctypes.data_as(ctypes.c_void_p), fixed.ctypes.data_as(ctypes.c_void_p)),
              "lpbox_big_batch_iterate_l2f_scores")
        return rets, fixed


def solve_many(problems, max_iters=20000, device=0, order="default"):
    """Solve every problem to its own stop in one lockstep chain: (rets, binary solutions, objectives cal_Obj()).  order: as BigLpBatch."""
    batch = BigLpBatch(problems, device=device, order=order)
    try:
        batch.solve_init()
        rets = batch.solve_iter(0, int(max_iters))
        return rets, [s.local_x_sol() for s in batch.solvers], np.array([s.cal_Obj() for s in batch.solvers])
    finally:
        batch.close()
