"""Second, independent CPU restatement of the reference's generic BQP and segmentation loops in numpy/scipy.  TEST INFRASTRUCTURE ONLY.

Written from the reference source, not from oracle/bqp_oracle.c or oracle/seg_oracle.c, so that the two can pin each other:
  SEGcpp = Segmentation/Segmentation/cython/src/LPboxADMMsolver.cpp
  NumpyBqp -- ADMM_bqp (SEGcpp:1384-1832) for the four problem types of its entry points (:1834-2109)
  NumpySeg -- ADMM_bqp_unconstrained_init's solver state (:658-810), the l2f window loop with its fix step (:917-1195) and the
              legacy loop (:1200-1380)

High precision: every dot product, squared norm and norm is math.fsum over the element-wise products (correctly rounded sum), and
sparse products are scipy's float64.  The restatement therefore differs from exact arithmetic only by element-wise rounding, in an
association that is neither Eigen's nor the GPU tree's; agreement with the C oracles is to rounding, not bitwise.  Above FSUM_MAX
elements a reduction is np.dot / np.sum instead (the full-size segmentation images of the GPU tests), to keep their CPU time small.
"""
import math

import numpy as np
import scipy.sparse as sp

FSUM_MAX = 100000

# the 11 hyper-parameters in the order of lpbox_bqp_set_params: stop_threshold, std_threshold, gamma_val, gamma_factor,
# rho_change_step, max_iters, initial_rho, history_size, learning_fact, pcg_tol, pcg_maxiters
PRESETS = {
    0: [1e-3, 1e-6, 1.0, 0.99, 5, 1e4, 5, 5, 1 + 3.0 / 100, 1e-3, 1e3],      # ADMM_bqp_unconstrained_init SEGcpp:658-672
    1: [1e-4, 1e-6, 1.6, 0.95, 5, 5e3, 1, 3, 1 + 5.0 / 100, 1e-4, 1e3],      # ADMM_bqp_linear_eq_init :587-601
    2: [1e-4, 1e-6, 1.6, 0.95, 5, 1e4, 25, 3, 1 + 1.0 / 100, 1e-4, 1e3],     # ADMM_bqp_linear_ineq_init :603-618
    3: [1e-4, 1e-6, 1.6, 0.95, 5, 1e4, 25, 3, 1 + 1.0 / 100, 1e-4, 1e3],     # ADMM_bqp_linear_eq_and_uneq_init :620-634
}


def dot(a, b):
    if len(a) > FSUM_MAX:
        return float(np.dot(a, b))
    return math.fsum((a * b).tolist())


def total(a):
    if len(a) > FSUM_MAX:
        return float(np.sum(a))
    return math.fsum(np.asarray(a, float).tolist())


def norm(a):
    return math.sqrt(dot(a, a))


def csr(M, rows, cols):
    p, i, v = M
    return sp.csr_matrix((np.asarray(v, float), np.asarray(i), np.asarray(p)), shape=(rows, cols))


def col_sq(M):
    """Sum of squares of the nonzero values of every column (Csq_diag / Esq_diag, SEGcpp:1515-1527, :1536-1547)."""
    Mc = M.tocsc()
    out = np.zeros(M.shape[1])
    for j in range(M.shape[1]):
        v = Mc.data[Mc.indptr[j]:Mc.indptr[j + 1]]
        v = v[v != 0.0]
        if len(v):
            out[j] = total(v * v)
    return out


def inv_diag(d):
    """Eigen::DiagonalPreconditioner::compute: 1 / diagonal, 1 where the diagonal is zero."""
    out = np.ones_like(d)
    nz = d != 0
    out[nz] = 1.0 / d[nz]
    return out


def project_box(t):  # SEGcpp:539-551: > 1 -> 1, < 0 -> 0, anything else (NaN included) unchanged
    return np.where(t > 1, 1.0, np.where(t < 0, 0.0, t))


def project_sphere(t, n):  # SEGcpp:553-558 with p = 2
    s = t - 0.5
    return s * math.pow(n, 1.0 / 2) / (2 * norm(s)) + 0.5


def cost(x, A, b):  # compute_cost SEGcpp:560-572
    return dot(x, A @ x) + dot(b, x)


def std_obj(hist):  # compute_std_obj / std_dev SEGcpp:488-507, :574-584, on the last history_size values
    h = np.asarray(hist, float)
    mean = total(h) / len(h)
    var = total((h - mean) * (h - mean)) / (len(h) - 1)
    s = 0.0 if var == 0 else math.pow(var, 1.0 / 2)
    return s / abs(h[-1])


def pcg(matvec, invdiag, rhs, x, tol, maxiters, curv=None):
    """_conjugate_gradient SEGcpp:415-485 (and its single-matrix twin :272-342).  Returns the iteration count; x is updated in place.
    curv: a list that receives every p.Mp (negative where the operator is indefinite along p)."""
    r = rhs - matvec(x)
    rhs2 = dot(rhs, rhs)
    if rhs2 == 0:
        x[:] = 0
        return 0
    thr = max(tol * tol * rhs2, np.finfo(float).tiny)
    if dot(r, r) < thr:
        return 0
    p = invdiag * r
    abs_new = dot(r, p)
    i = 0
    while i < maxiters:
        tmp = matvec(p)
        pmp = dot(p, tmp)
        if curv is not None:
            curv.append(pmp)
        alpha = abs_new / pmp
        x += alpha * p
        r = r - alpha * tmp
        if dot(r, r) < thr:
            i += 1
            break
        z = invdiag * r
        abs_old = abs_new
        abs_new = dot(r, z)
        p = z + (abs_new / abs_old) * p
        i += 1
    return i


class NumpyBqp:
    """ADMM_bqp (SEGcpp:1384-1832).  problem: dict(n, A=(rowptr, colidx, vals), b, x0[, C=(...), d][, E=(...), f]), A storing every
    diagonal entry.  The problem type follows from C / E as in lpbox_bqp: 0 unconstrained, 1 equality, 2 inequality, 3 both; `preset`
    picks the hyper-parameters of a *_init (default: the type's own), `params` overrides them with an 11-value list."""

    def __init__(self, problem, preset=None, params=None):
        n = self.n = int(problem["n"])
        self.A = csr(problem["A"], n, n)
        self.b = np.asarray(problem["b"], float)
        self.x0 = np.asarray(problem["x0"], float)
        self.eq = problem.get("C") is not None
        self.ineq = problem.get("E") is not None
        if self.eq:
            self.d = np.asarray(problem["d"], float)
            self.C = csr(problem["C"], len(self.d), n)
        if self.ineq:
            self.f = np.asarray(problem["f"], float)
            self.E = csr(problem["E"], len(self.f), n)
        self.ptype = (1 if self.eq else 0) | (2 if self.ineq else 0)
        p = list(PRESETS[self.ptype if preset is None else int(preset)] if params is None else params)
        (self.stop_threshold, self.std_threshold, self.gamma0, self.gamma_factor, rho_step, max_iters, self.initial_rho,
         history, self.learning_fact, self.pcg_tol, pcg_maxiters) = p
        self.rho_change_step, self.max_iters, self.history_size, self.pcg_maxiters = int(rho_step), int(max_iters), int(history), int(pcg_maxiters)
        # SolverInstruction of the four entry points (:1845-1850, :1898-1907, :1969-1974, :2041-2046)
        self.update_y3 = self.update_z4 = self.update_rho4 = self.ineq
        self.update_z3 = self.eq
        self.update_rho3 = self.ptype == 3

    def solve(self, record=False):
        """The whole loop; returns the `iter` it ended on.  record=True keeps a snapshot of the state after every iteration in
        self.trace (list of dicts), each with that iteration's PCG count."""
        n, A, b = self.n, self.A, self.b
        lf = self.learning_fact
        x = self.x0.copy()
        z1, z2 = np.zeros(n), np.zeros(n)
        rho1 = rho2 = rho3 = rho4 = float(self.initial_rho)
        prev_rho1, prev_rho2, prev_rho3, prev_rho4 = rho1, rho2, rho3, rho4
        gamma = float(self.gamma0)
        rho_updated = True
        rcr = None
        obj_list = []
        std = 1.0
        z3 = np.zeros(len(self.d)) if self.update_z3 else None
        z4 = np.zeros(len(self.f)) if self.update_z4 else None
        y3 = None
        # 2A + (rho1 + rho2) I, the diagonal held apart so that it is updated in place as Eigen does (:1486-1487, :1624)
        M = (2 * A).tocsr()
        diag = M.diagonal().copy()
        diag = diag + (rho1 + rho2)
        offd = (M - sp.diags(M.diagonal())).tocsr()
        r3Ct = r4Et = None
        pdiag = diag.copy()                                      # preconditioner_diag_mat (:1489-1501)
        if self.eq:
            Ct = self.C.T.tocsr()
            r3Ct = (rho3 * Ct).tocsr()
            Csq = col_sq(self.C)
            pdiag = pdiag + rho3 * Csq
        if self.ineq:
            Et = self.E.T.tocsr()
            r4Et = (rho4 * Et).tocsr()
            Esq = col_sq(self.E)
            pdiag = pdiag + rho4 * Esq

        def matvec(v):                                           # calculate_mat_expr_multiplication :361-408
            out = offd @ v + diag * v
            if self.eq:
                out = out + r3Ct @ (self.C @ v)
            if self.ineq:
                out = out + r4Et @ (self.E @ v)
            return out
        y1, y2 = x.copy(), x.copy()
        if self.update_y3:
            y3 = self.f - self.E @ x
        best_sol = x.copy()
        best_bin_obj = cost(x, A, b)
        self.trace = []
        self.pcg = []
        self.min_curvature = []
        self.stop = 0
        cvg1 = cvg2 = obj_val = cur_obj = float("nan")
        invdiag = None
        it = 0
        while it < self.max_iters:
            y1 = project_box(x + z1 / rho1)                                      # :1600-1603
            y2 = project_sphere(x + z2 / rho2, n)                                # :1605-1608
            if self.update_y3:                                                   # :1610-1614
                t = (self.f - self.E @ x) - z4 / rho4
                y3 = np.where(t < 0, 0.0, t)
            if it != 0 and rho_updated:                                          # :1619-1638
                diag = diag + rcr * (prev_rho1 + prev_rho2)
                if self.ptype != 0:
                    pdiag = pdiag + rcr * (prev_rho1 + prev_rho2)
                if self.update_rho3:
                    pdiag = pdiag + (rcr * prev_rho3) * Csq
                    r3Ct = (lf * r3Ct).tocsr()
                if self.update_rho4:
                    pdiag = pdiag + (rcr * prev_rho4) * Esq
                    r4Et = (lf * r4Et).tocsr()
            rhs = (rho1 * y1 + rho2 * y2) - ((b + z1) + z2)                      # :1645-1684
            if self.eq:
                rhs = rhs + r3Ct @ self.d
                rhs = rhs - Ct @ z3
            if self.ineq:
                rhs = rhs + r4Et @ (self.f - y3)
                rhs = rhs - Et @ z4
            if rho_updated:                                                      # :1688-1695
                invdiag = inv_diag(pdiag if self.ptype != 0 else diag)
                rho_updated = False
            x = y1.copy()                                                        # :1697-1700
            curv = []
            k = pcg(matvec, invdiag, rhs, x, self.pcg_tol, self.pcg_maxiters, curv)
            self.pcg.append(k)
            self.min_curvature.append(min(curv, default=float("inf")))
            z1 = z1 + (gamma * rho1) * (x - y1)                                  # :1707-1715
            z2 = z2 + (gamma * rho2) * (x - y2)
            if self.update_z3:
                z3 = z3 + (gamma * rho3) * (self.C @ x - self.d)
            if self.update_z4:
                z4 = z4 + (gamma * rho4) * ((self.E @ x + y3) - self.f)
            temp0 = max(norm(x), 2.2204e-16)                                     # :1718-1727
            cvg1 = norm(x - y1) / temp0
            cvg2 = norm(x - y2) / temp0
            done = 0
            if cvg1 <= self.stop_threshold and cvg2 <= self.stop_threshold:
                done = 1
            else:
                if (it + 1) % self.rho_change_step == 0:                         # :1729-1748
                    prev_rho1, prev_rho2 = rho1, rho2
                    rho1, rho2 = lf * rho1, lf * rho2
                    if self.update_rho3:
                        prev_rho3, rho3 = rho3, lf * rho3
                    if self.update_rho4:
                        prev_rho4, rho4 = rho4, lf * rho4
                    gamma = max(gamma * self.gamma_factor, 1.0)
                    rho_updated = True
                    rcr = lf - 1.0
                obj_val = cost(x, A, b)                                          # :1750-1761
                obj_list.append(obj_val)
                if len(obj_list) >= self.history_size:
                    std = std_obj(obj_list[-self.history_size:])
                if std <= self.std_threshold:
                    done = 2
                else:
                    cur_obj = cost((x >= 0.5).astype(float), A, b)               # :1763-1770
                    if best_bin_obj >= cur_obj:
                        best_bin_obj = cur_obj
                        best_sol = x.copy()
            if record:
                snap = dict(x=x.copy(), y1=y1.copy(), y2=y2.copy(), z1=z1.copy(), z2=z2.copy(), best_sol=best_sol.copy(),
                            rho1=rho1, rho3=rho3, rho4=rho4, gamma=gamma, std_obj=std, cvg1=cvg1, cvg2=cvg2,
                            best_bin_obj=best_bin_obj, obj_val=obj_val, cur_obj=cur_obj, pcg=k)
                for name, v in (("z3", z3), ("z4", z4), ("y3", y3)):
                    if v is not None:
                        snap[name] = v.copy()
                self.trace.append(snap)
            if done:
                self.stop = done
                break
            it += 1
        self.iters = it
        self.state = dict(x=x, y1=y1, y2=y2, z1=z1, z2=z2, best_sol=best_sol, rho1=rho1, rho3=rho3, rho4=rho4, gamma=gamma,
                          std_obj=std, cvg1=cvg1, cvg2=cvg2, best_bin_obj=best_bin_obj, obj_val=obj_val, cur_obj=cur_obj)
        for name, v in (("z3", z3), ("z4", z4), ("y3", y3)):
            if v is not None:
                self.state[name] = v
        return it


class NumpySeg:
    """The segmentation flavour: solver state of ADMM_bqp_unconstrained_init (SEGcpp:658-810) on a given problem
    P = dict(n, rowptr, colidx, vals, b, c) -- A_ptr = A / 2 as the cost builder leaves it (:750-758) -- then l2f windows
    (:917-1195) or the legacy loop (:1200-1380).  Hyper-parameters: the unconstrained preset unless `params` is given."""

    def __init__(self, P, params=None):
        p = list(PRESETS[0] if params is None else params)
        (self.stop_threshold, self.std_threshold, self.gamma0, self.gamma_factor, rho_step, max_iters, self.initial_rho,
         history, self.learning_fact, self.pcg_tol, pcg_maxiters) = p
        self.rho_change_step, self.max_iters, self.history_size, self.pcg_maxiters = int(rho_step), int(max_iters), int(history), int(pcg_maxiters)
        self.org_n = self.n = int(P["n"])
        self.A = sp.csr_matrix((np.asarray(P["vals"], float), np.asarray(P["colidx"]), np.asarray(P["rowptr"])), shape=(self.n, self.n))
        self.A.sort_indices()
        self.b = np.asarray(P["b"], float).copy()
        self.c = float(P["c"])
        # members with in-class initialisers (SEGh:197-207): set once per object, not by the init
        self.rho_updated = True
        self.std = 1.0
        self.rcr = 1.0
        self.obj_list = []

    def _set_temp_mat(self):  # temp_mat = 2 A + (rho1 + rho2) I (:784-786, :1054-1057)
        M = (2 * self.A).tocsr()
        self.diag = M.diagonal() + (self.rho1 + self.rho2)
        self.offd = (M - sp.diags(M.diagonal())).tocsr()

    def solve_init(self):  # :778-806
        n = self.n
        self.gamma = float(self.gamma0)
        self.x = np.zeros(n)
        self.z1, self.z2 = np.zeros(n), np.zeros(n)
        self.rho1 = self.rho2 = float(self.initial_rho)
        self.prev_rho1, self.prev_rho2 = self.rho1, self.rho2
        self._set_temp_mat()
        self.y1, self.y2 = self.x.copy(), self.x.copy()
        self.best_sol = self.x.copy()
        self.best_bin_obj = cost(self.x, self.A, self.b)
        self.left_idx = np.arange(n)
        self.fixed_idx = np.zeros(0, int)
        self.fixed_val = np.zeros(0)
        self.pcg = []
        self.cvg1 = self.cvg2 = self.obj_val = self.cur_obj = float("nan")
        self.invdiag = None
        return 1

    def _iteration(self, it):
        """One iteration of the body shared by the l2f (:1068-1173) and legacy (:1223-1336) loops; 1 when a stop test fired."""
        n = self.n
        self.y1 = project_box(self.x + self.z1 / self.rho1)
        self.y2 = project_sphere(self.x + self.z2 / self.rho2, n)
        if it != 0 and self.rho_updated:
            self.diag = self.diag + (self.prev_rho1 + self.prev_rho2) * self.rcr
        rhs = (self.rho1 * self.y1 + self.rho2 * self.y2) - ((self.b + self.z1) + self.z2)
        if self.rho_updated:
            if len(self.diag) != n:
                raise NotImplementedError("a fix while the preconditioner is stale: the reference's Eigen sizes disagree here")
            self.invdiag = inv_diag(self.diag)
            self.rho_updated = False
        x = self.y1.copy()
        offd, diag = self.offd, self.diag
        self.pcg.append(pcg(lambda v: offd @ v + diag * v, self.invdiag, rhs, x, self.pcg_tol, self.pcg_maxiters))
        self.x = x
        if self.x_iters is not None:
            self.x_iters[:, self.cc] = x
            self.cc += 1
        g = self.gamma
        self.z1 = self.z1 + (g * self.rho1) * (x - self.y1)
        self.z2 = self.z2 + (g * self.rho2) * (x - self.y2)
        temp0 = max(norm(x), 2.2204e-16)
        self.cvg1 = norm(x - self.y1) / temp0
        self.cvg2 = norm(x - self.y2) / temp0
        if self.cvg1 <= self.stop_threshold and self.cvg2 <= self.stop_threshold:
            self.last_stop = 1
            return 1
        if (it + 1) % self.rho_change_step == 0:
            self.prev_rho1, self.prev_rho2 = self.rho1, self.rho2
            self.rho1, self.rho2 = self.learning_fact * self.rho1, self.learning_fact * self.rho2
            self.gamma = max(self.gamma * self.gamma_factor, 1.0)
            self.rho_updated = True
            self.rcr = self.learning_fact - 1.0
        self.obj_val = cost(x, self.A, self.b)
        self.obj_list.append(self.obj_val)
        if len(self.obj_list) >= self.history_size:
            self.std = std_obj(self.obj_list[-self.history_size:])
        if self.std <= self.std_threshold:
            self.last_stop = 2
            return 1
        self.cur_obj = cost((x >= 0.5).astype(float), self.A, self.b)
        if self.best_bin_obj >= self.cur_obj:
            self.best_bin_obj = self.cur_obj
            self.best_sol = x.copy()
        return 0

    def _fix(self, vec, fix_num):  # :927-1058
        n = self.n
        vec = np.asarray(vec, float)[:n]
        fixed = (vec == 1) | (vec == 0)
        if int(fixed.sum()) != fix_num:
            raise ValueError("fix_num does not match the vector")
        keep = ~fixed
        self.fixed_idx = np.concatenate([self.fixed_idx, self.left_idx[fixed]])
        self.fixed_val = np.concatenate([self.fixed_val, vec[fixed]])
        self.left_idx = self.left_idx[keep]
        if n - fix_num == 0:
            self.n = 0
            return 1
        Ma = self.A[keep][:, keep]
        Mb = self.A[keep][:, fixed]
        self.x, self.y1, self.y2 = self.x[keep], self.y1[keep], self.y2[keep]
        self.z1, self.z2 = self.z1[keep], self.z2[keep]
        self.b = 2 * (Mb @ vec[fixed]) + self.b[keep]
        self.n = n - fix_num
        self.A = Ma.tocsr()
        self._set_temp_mat()
        return 0

    def solve_iter_l2f(self, it_start, it_end, vec, fix_num):
        """ADMM_bqp_unconstrained_l2f: returns ret (1 when a stop test fired or nothing is left)."""
        self.x_iters = np.zeros((self.n - fix_num, 10))
        self.cc = 0
        ret = 0
        if fix_num != 0 and self._fix(vec, fix_num):
            ret, it_end = 1, it_start
        for it in range(it_start, it_end):
            if self._iteration(it):
                ret = 1
                break
        return ret

    def solve_iter(self):
        """ADMM_bqp_unconstrained_legacy: returns int(cur_obj + c) of the final binary labelling."""
        self.x_iters = None
        self.last_stop = 0
        it = 0
        while it < self.max_iters:
            if self._iteration(it):
                break
            it += 1
        self.legacy_iter_plus1 = it + 1
        self.cur_obj = cost((self.x >= 0.5).astype(float), self.A, self.b)
        e = self.cur_obj + self.c           # (int)energy (:1379): truncated while it fits an int, INT_MIN otherwise (x86-64's cast)
        return int(e) if -2147483649.0 < e < 2147483648.0 else -2147483648

    def get_x_sol(self):
        out = np.zeros(self.org_n)
        out[self.fixed_idx] = self.fixed_val
        if self.n:
            out[self.left_idx] = (self.x >= 0.5).astype(float)
        return out

    def get_x_iters_2d(self, ws):
        return self.x_iters[:, :ws]
