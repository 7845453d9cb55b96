"""Generic constrained binary QP on the GPU:  min x'Ax + b'x  s.t.  Cx = d,  Ex <= f,  x in {0,1}^n.

The reference's `ADMM_bqp` (Segmentation/.../LPboxADMMsolver.cpp:1384-1832) with its four entry points `ADMM_bqp_unconstrained`,
`_linear_eq`, `_linear_ineq`, `_linear_eq_and_uneq` (:1834-2109) -- C++ only in the reference (nothing in its pyx reaches them);
here through the C-ABI `lpbox_bqp_*`.  Matrices: (rowptr, colidx, vals) CSR with ascending columns, or scipy.sparse matrices.
A must store every diagonal entry (explicit zeros where needed): the reference adds rho to `A.diagonal()` in place (:1483).
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import LpboxError, check

PRESET_UNCONSTRAINED, PRESET_EQ, PRESET_INEQ, PRESET_EQ_INEQ = 0, 1, 2, 3
PARAM_NAMES = ("stop_threshold", "std_threshold", "gamma_val", "gamma_factor", "rho_change_step", "max_iters", "initial_rho",
               "history_size", "learning_fact", "pcg_tol", "pcg_maxiters")


def _csr(M, rows):
    if M is None:
        return None
    if hasattr(M, "tocsr"):                 # scipy.sparse
        M = M.tocsr().sorted_indices()
        M = (M.indptr, M.indices, M.data)
    p, i, v = (np.ascontiguousarray(M[0], np.int32), np.ascontiguousarray(M[1], np.int32), np.ascontiguousarray(M[2], np.float64))
    if p.shape[0] != rows + 1:
        raise ValueError("row pointer has %d entries, expected %d" % (p.shape[0], rows + 1))
    return p, i, v


def with_diagonal(rowptr, colidx, vals, n):
    """CSR -> CSR with an explicit (possibly zero) diagonal entry in every row, columns ascending."""
    rp, ci, va = [0], [], []
    for i in range(n):
        cols = list(colidx[rowptr[i]:rowptr[i + 1]])
        vs = list(vals[rowptr[i]:rowptr[i + 1]])
        if i not in cols:
            cols.append(i); vs.append(0.0)
        order = np.argsort(cols, kind="stable")
        ci += [cols[k] for k in order]; va += [vs[k] for k in order]
        rp.append(len(ci))
    return np.array(rp, np.int32), np.array(ci, np.int32), np.array(va, np.float64)


class BqpSolver:
    """One problem per handle, any size.  order: "default", or "reference" (see `set_order`)."""

    def __init__(self, n, A, b, x0, C_=None, d=None, E=None, f=None, preset=None, params=None, device=0, order="default"):
        mode = _order_mode(order)
        self._L = _lib.load()
        self.n = int(n)
        self.m = 0 if C_ is None else len(d)
        self.l = 0 if E is None else len(f)
        h = self._L.lpbox_bqp_create(int(device))
        if not h:
            check(-2, "lpbox_bqp_create")
        self._h = C.c_void_p(h)
        keep = []

        def ptrs(M):
            if M is None:
                return [None, None, None]
            keep.extend(M)
            return [a.ctypes.data_as(C.c_void_p) for a in M]

        def vec(v):
            if v is None:
                return None
            a = np.ascontiguousarray(v, np.float64)
            keep.append(a)
            return a.ctypes.data_as(C.c_void_p)
        A_ = _csr(A, self.n)
        if any(i not in A_[1][A_[0][i]:A_[0][i + 1]] for i in range(self.n)):
            A_ = with_diagonal(A_[0], A_[1], A_[2], self.n)
        args = [self._h, self.n] + ptrs(A_) + [vec(b), vec(x0), self.m] + ptrs(_csr(C_, self.m)) + [vec(d), self.l] + \
            ptrs(_csr(E, self.l)) + [vec(f)]
        check(self._L.lpbox_bqp_set_problem(*args), "lpbox_bqp_set_problem")
        ptype = (1 if self.m else 0) | (2 if self.l else 0)
        check(self._L.lpbox_bqp_preset(self._h, ptype if preset is None else int(preset)), "lpbox_bqp_preset")
        if params is not None:
            if isinstance(params, dict):
                raise TypeError("params: the 11 values in the order of bqp.PARAM_NAMES")
            check(self._L.lpbox_bqp_set_params(self._h, np.ascontiguousarray(params, np.float64)), "lpbox_bqp_set_params")
        self.order = "default"
        if mode:
            self.set_order(order)

    def set_order(self, name="default"):
        """Summation order of the kernel chain, chosen at any time, also between two solves.  "default": the kernels' own reduction
        tree.  "reference": an opt-in that associates every sum over the n elements as the reference's Eigen path does (DESIGN.md
        section 14.3) -- the reference's iterates, iteration counts and binary answers, except that the std stop test takes sqrt where
        the reference calls pow(v, 1/2); each reduction becomes a sequential walk by one workgroup, so an iteration costs more.  A
        call that changes the order discards the results of the previous solve."""
        mode = _order_mode(name)
        check(self._L.lpbox_bqp_set_order(self._h, mode), "lpbox_bqp_set_order")
        self.order = name

    def close(self):
        if getattr(self, "_h", None):
            self._L.lpbox_bqp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def solve(self):
        it = C.c_int()
        check(self._L.lpbox_bqp_solve(self._h, C.byref(it)), "lpbox_bqp_solve")
        return it.value

    def vec(self, name):
        out = np.zeros(max(self.n, self.m, self.l, 1))
        k = check(self._L.lpbox_bqp_get_vec(self._h, name.encode(), out, len(out)), "lpbox_bqp_get_vec")
        return out[:k].copy()

    def scalar(self, name):
        v = C.c_double()
        check(self._L.lpbox_bqp_get_scalar(self._h, name.encode(), C.byref(v)), "lpbox_bqp_get_scalar")
        return v.value

    def solution(self):
        """The reference's Solution struct (LPh): x_sol, y1, y2, best_sol; the binary answer is x_sol >= 0.5."""
        return dict(x_sol=self.vec("x"), y1=self.vec("y1"), y2=self.vec("y2"), best_sol=self.vec("best_sol"))


# ---- the reference's four entry points by name (SEGcpp:1834-2109); each returns the Solution dict -------------------------------
def _run(n, A, b, x0, C_=None, d=None, E=None, f=None, preset=0, params=None, device=0, order="default"):
    s = BqpSolver(n, A, b, x0, C_, d, E, f, preset=preset, params=params, device=device, order=order)
    it = s.solve()
    sol = s.solution()
    sol.update(iterations=it, stop=int(s.scalar("stop")), best_bin_obj=s.scalar("best_bin_obj"), time_elapsed_ms=s.scalar("kernel_ms"))
    s.close()
    return sol


def ADMM_bqp_unconstrained(n, A, b, x0, **kw):
    return _run(n, A, b, x0, preset=PRESET_UNCONSTRAINED, **kw)


def ADMM_bqp_linear_eq(n, A, b, x0, m, C_, d, **kw):
    return _run(n, A, b, x0, C_=C_, d=np.asarray(d)[:m], preset=PRESET_EQ, **kw)


def ADMM_bqp_linear_ineq(n, A, b, x0, l, E, f, **kw):
    return _run(n, A, b, x0, E=E, f=np.asarray(f)[:l], preset=PRESET_INEQ, **kw)


def ADMM_bqp_linear_eq_and_uneq(n, A, b, x0, m, C_, d, l, E, f, **kw):
    return _run(n, A, b, x0, C_=C_, d=np.asarray(d)[:m], E=E, f=np.asarray(f)[:l], preset=PRESET_EQ_INEQ, **kw)


# ---- many small problems at once (max(n, m, l) <= 2048 each): one persistent workgroup per problem ---------------------------------
BATCH_MAX_DIM = 2048
ORDERS = {"default": 0, "reference": 1}            # LPBOX_ORDER_DEFAULT, LPBOX_ORDER_REFERENCE


def _order_mode(name):
    if name not in ORDERS:
        raise ValueError("summation order must be 'default' or 'reference'")
    return ORDERS[name]


def _per_problem(value, count, what):
    """None, one value for every problem, or a sequence with one entry per problem."""
    if value is None:
        return [None] * count
    if isinstance(value, dict):
        raise TypeError("%s: a single value or one per problem, not a dict" % what)
    if what == "presets" and np.isscalar(value):
        return [int(value)] * count
    value = list(value)
    if any(isinstance(v, dict) for v in value):
        raise TypeError("%s: the 11 values in the order of bqp.PARAM_NAMES, not a dict" % what)
    if what == "params" and value and all(np.isscalar(v) for v in value):       # one parameter vector for every problem
        if len(value) != len(PARAM_NAMES):
            raise ValueError("params: the %d values in the order of bqp.PARAM_NAMES" % len(PARAM_NAMES))
        return [value] * count
    if len(value) != count:
        raise ValueError("%s: %d entries for %d problems" % (what, len(value), count))
    if what == "params" and any(v is not None and len(v) != len(PARAM_NAMES) for v in value):
        raise ValueError("params: the %d values in the order of bqp.PARAM_NAMES" % len(PARAM_NAMES))
    return value


class BqpBatch:
    """A batch of independent small BQPs solved together; every problem gives the bits `BqpSolver` gives for it alone.

    problems: a sequence of dicts with the keys n, A, b, x0 and optionally C, d, E, f (CSR triples or scipy.sparse matrices).
    presets / params: None, a single value, or one per problem; the default preset follows the constraints present.
    order: "default", or "reference" (see `set_order`)."""

    def __init__(self, problems, presets=None, params=None, device=0, order="default"):
        mode = _order_mode(order)
        problems = list(problems)
        if not problems:
            raise ValueError("BqpBatch: no problems")
        count = len(problems)
        presets = _per_problem(presets, count, "presets")
        params = _per_problem(params, count, "params")
        for P in problems:
            if not isinstance(P, dict) or any(k not in P for k in ("n", "A", "b", "x0")):
                raise TypeError("BqpBatch: every problem is a dict with the keys n, A, b, x0 (and C, d, E, f)")
        self._L = _lib.load()
        self.count = count
        self.dims = []
        self._h = None
        h = self._L.lpbox_bqp_batch_create(count, int(device))
        if not h:
            msg = self._L.lpbox_last_error()
            err = LpboxError("lpbox_bqp_batch_create failed: %s" % (msg.decode() if msg else ""))
            err.code = _lib.E_NODEVICE if msg and b"no HIP device" in msg else -2
            raise err
        self._h = C.c_void_p(h)
        try:
            for i, P in enumerate(problems):
                self._set(i, P, presets[i], params[i])
            self.order = "default"
            if mode:
                self.set_order(order)
        except Exception:
            self.close()
            raise

    def _set(self, i, P, preset, params):
        n = int(P["n"])
        m = 0 if P.get("C") is None else len(P["d"])
        l = 0 if P.get("E") is None else len(P["f"])
        keep = []

        def ptrs(M):
            if M is None:
                return [None, None, None]
            keep.extend(M)
            return [a.ctypes.data_as(C.c_void_p) for a in M]

        def vec(v):
            if v is None:
                return None
            a = np.ascontiguousarray(v, np.float64)
            keep.append(a)
            return a.ctypes.data_as(C.c_void_p)
        A_ = _csr(P["A"], n)
        if any(j not in A_[1][A_[0][j]:A_[0][j + 1]] for j in range(n)):
            A_ = with_diagonal(A_[0], A_[1], A_[2], n)
        args = [self._h, i, n] + ptrs(A_) + [vec(P["b"]), vec(P["x0"]), m] + ptrs(_csr(P.get("C"), m)) + [vec(P.get("d") if m else None), l] + \
            ptrs(_csr(P.get("E"), l)) + [vec(P.get("f") if l else None)]
        check(self._L.lpbox_bqp_batch_set_problem(*args), "lpbox_bqp_batch_set_problem")
        ptype = (1 if m else 0) | (2 if l else 0)
        check(self._L.lpbox_bqp_batch_preset(self._h, i, ptype if preset is None else int(preset)), "lpbox_bqp_batch_preset")
        if params is not None:
            check(self._L.lpbox_bqp_batch_set_params(self._h, i, np.ascontiguousarray(params, np.float64)), "lpbox_bqp_batch_set_params")
        self.dims.append((n, m, l))

    def set_order(self, name="default"):
        """Summation order of the batch kernels, chosen at any time before a solve.  "default": the kernels' own reduction tree, the
        bits of `BqpSolver`.  "reference": an opt-in that associates every sum over a problem's n elements as the reference's Eigen path
        does -- the reference's iterates, iteration counts and binary answers, except that the std stop test
        takes sqrt where the reference calls pow(v, 1/2); each reduction becomes a sequential walk, so a PCG step costs more."""
        mode = _order_mode(name)
        check(self._L.lpbox_bqp_batch_set_order(self._h, mode), "lpbox_bqp_batch_set_order")
        self.order = name

    def close(self):
        if getattr(self, "_h", None):
            self._L.lpbox_bqp_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def solve(self):
        it = np.zeros(self.count, np.int32)
        check(self._L.lpbox_bqp_batch_solve(self._h, it.ctypes.data_as(C.c_void_p)), "lpbox_bqp_batch_solve")
        return it

    def vec(self, i, name):
        out = np.zeros(BATCH_MAX_DIM)
        k = check(self._L.lpbox_bqp_batch_get_vec(self._h, int(i), name.encode(), out, len(out)), "lpbox_bqp_batch_get_vec")
        return out[:k].copy()

    def scalar(self, i, name):
        v = C.c_double()
        check(self._L.lpbox_bqp_batch_get_scalar(self._h, int(i), name.encode(), C.byref(v)), "lpbox_bqp_batch_get_scalar")
        return v.value

    def solution(self, i):
        """The same dict as `BqpSolver.solution`, for problem i."""
        return dict(x_sol=self.vec(i, "x"), y1=self.vec(i, "y1"), y2=self.vec(i, "y2"), best_sol=self.vec(i, "best_sol"))


def solve_many(problems, **kw):
    """Solve a sequence of small problems in one batch; a list of the dicts the ADMM_bqp_* entry points return.
    Keywords are those of `BqpBatch` (presets, params, device, order)."""
    s = BqpBatch(problems, **kw)
    its = s.solve()
    out = []
    for i in range(s.count):
        sol = s.solution(i)
        sol.update(iterations=int(its[i]), stop=int(s.scalar(i, "stop")), best_bin_obj=s.scalar(i, "best_bin_obj"),
                   time_elapsed_ms=s.scalar(0, "kernel_ms"))
        out.append(sol)
    s.close()
    return out


# ---- many problems of any size at once: one launch chain in lockstep ---------------------------------------
def _is_problem(P):
    return isinstance(P, dict) and all(k in P for k in ("n", "A", "b", "x0"))


def _as_problem(P):
    """A problem dict, or the positional tuple (n, A, b, x0[, C, d[, E, f]]) of `BqpSolver`."""
    if isinstance(P, (tuple, list)) and len(P) in (4, 6, 8):
        return dict(zip(("n", "A", "b", "x0", "C", "d", "E", "f"), P))
    return P


def _dims(P):
    return (int(P["n"]), 0 if P.get("C") is None else len(P["d"]), 0 if P.get("E") is None else len(P["f"]))


class BqpLockstep:
    """A batch of BQPs of any size through ONE launch chain in lockstep (lpbox_bqp_lockstep_* in include/lpbox_hip.h): every launch of
    `BqpSolver`'s chain runs once for all members over a (workgroups, members) grid, each member on its own control state, to its own
    stop.  Meant for many problems with a dimension above `BATCH_MAX_DIM`, where `BqpBatch` does not reach and a loop over `BqpSolver`
    handles is bound by its launches; every member gets the bits `BqpSolver` gives it alone.

    members: problem dicts as for `BqpBatch` (or the tuples (n, A, b, x0[, C, d[, E, f]])) -- a `BqpSolver` is built for each and closed
    with the batch -- and / or `BqpSolver` objects (borrowed; default summation order only).  presets / params: None, a single value, or one
    per member; they apply to the members built here (a borrowed solver keeps its own).  `batch[i]` is member i's
    `BqpSolver`: its getters, and a `solve` of its own, work after the batch's solve."""

    def __init__(self, members, presets=None, params=None, device=0):
        members = [_as_problem(m) for m in members] if members is not None else []
        if not members:
            raise ValueError("BqpLockstep: no problems")
        count = len(members)
        presets = _per_problem(presets, count, "presets")
        params = _per_problem(params, count, "params")
        for k, m in enumerate(members):
            if not isinstance(m, BqpSolver) and not _is_problem(m):
                raise TypeError("member %d is neither a BqpSolver nor a problem with n, A, b, x0 (and C, d, E, f)" % k)
        self._L = _lib.load()
        self._h = None
        self._own = [not isinstance(m, BqpSolver) for m in members]
        self.solvers = []
        try:
            for k, m in enumerate(members):
                if isinstance(m, BqpSolver):
                    self.solvers.append(m)
                    continue
                s = BqpSolver.__new__(BqpSolver)
                self.solvers.append(s)                       # before __init__: a handle it made is closed below when it raises
                s.__init__(m["n"], m["A"], m["b"], m["x0"], m.get("C"), m.get("d"), m.get("E"), m.get("f"), preset=presets[k], params=params[k],
                           device=device)
            arr = (C.c_void_p * count)(*[s._h for s in self.solvers])
            h = self._L.lpbox_bqp_lockstep_create(arr, count)
            if not h:
                rc = self._L.lpbox_last_status()
                check(rc if rc < 0 else -2, "lpbox_bqp_lockstep_create")
        except Exception:                                    # no handle of ours stays open
            self._close_own()
            raise
        self._h = C.c_void_p(h)
        self.count = count

    def _close_own(self):
        for s, own in zip(self.solvers, self._own):
            if own:
                s.close()

    def __len__(self):
        return len(self.solvers)

    def __getitem__(self, i):
        return self.solvers[i]

    def close(self):
        if getattr(self, "_h", None):
            self._L.lpbox_bqp_lockstep_destroy(self._h)
            self._h = None
            self._close_own()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def solve(self):
        """ADMM_bqp of every member, each to its own stop; the iteration counts as an int32 array."""
        it = np.zeros(len(self.solvers), np.int32)
        check(self._L.lpbox_bqp_lockstep_solve(self._h, it.ctypes.data_as(C.c_void_p)), "lpbox_bqp_lockstep_solve")
        return it

    def scalar(self, name):
        v = C.c_double()
        check(self._L.lpbox_bqp_lockstep_get_scalar(self._h, name.encode(), C.byref(v)), "lpbox_bqp_lockstep_get_scalar")
        return v.value


def _solution_of(s, iterations, kernel_ms):
    sol = s.solution()
    sol.update(iterations=int(iterations), stop=int(s.scalar("stop")), best_bin_obj=s.scalar("best_bin_obj"), time_elapsed_ms=kernel_ms)
    return sol


def solve_large_many(problems, **kw):
    """Solve a sequence of problems of any size in one lockstep batch; a list of the dicts the ADMM_bqp_* entry points return
    (`time_elapsed_ms` is the batch's).  Keywords are those of `BqpLockstep` (presets, params, device)."""
    s = BqpLockstep(problems, **kw)
    try:
        its = s.solve()
        ms = s.scalar("kernel_ms")
        return [_solution_of(s[i], its[i], ms) for i in range(len(s))]
    finally:
        s.close()


def split_by_size(problems):
    """(indices for `BqpBatch`, indices for `BqpLockstep`): a problem with max(n, m, l) <= BATCH_MAX_DIM goes to the first."""
    small, large = [], []
    for i, P in enumerate(problems):
        (small if max(_dims(P)) <= BATCH_MAX_DIM else large).append(i)
    return small, large


def solve_any(problems, presets=None, params=None, device=0):
    """Solve a sequence of problems of any sizes: those with max(n, m, l) <= BATCH_MAX_DIM in one `BqpBatch` (`solve_many`), the rest in
    one `BqpLockstep` (`solve_large_many`); the Solution dicts in the order of `problems`.  presets / params as for `BqpBatch`."""
    problems = [_as_problem(P) for P in problems]
    if not problems:
        raise ValueError("solve_any: no problems")
    for k, P in enumerate(problems):
        if not _is_problem(P):
            raise TypeError("problem %d is not a problem with n, A, b, x0 (and C, d, E, f)" % k)
    count = len(problems)
    presets = _per_problem(presets, count, "presets")
    params = _per_problem(params, count, "params")
    out = [None] * count
    for idx, solver in zip(split_by_size(problems), (solve_many, solve_large_many)):
        if not idx:
            continue
        res = solver([problems[i] for i in idx], presets=[presets[i] for i in idx], params=[params[i] for i in idx], device=device)
        for i, sol in zip(idx, res):
            out[i] = sol
    return out
