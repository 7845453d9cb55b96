"""Second, independent CPU restatement of the reference's LP path in numpy.  TEST INFRASTRUCTURE ONLY.

Written from the reference source, not from oracle/lpbox_oracle.c, so that the two can pin each other
(the reference ships no golden vectors -- SURVEY.md section 8c):
  LPcpp = LinerProgramming/LinearProgramming/cython_solver/LPboxADMMsolver.cpp
Every product with E runs over the stored entries (scipy's sparse products in float64, segment sums in long double; never a dense
matrix); dot products use numpy's own (pairwise) summation,
i.e. a THIRD association besides Eigen's and the GPU tree; agreement with the C oracle is therefore to rounding, not bitwise.

Three constructor arguments turn one restatement into a family of independent roundings of the same arithmetic:
  vals   the stored values of E in the order of rowidx (default ones);
  dtype  np.float64 or np.longdouble: the number format of every vector, scalar and sum;
  perm   (pv, pr): internal variable i is original variable pv[i], internal row r is original row pr[r].  The whole problem is
         permuted at construction, so every sum over variables / rows / the entries of a row or column runs in another order;
         natural() / from_natural() translate to and from the original order.

Step-locked mode (lock()): the next solve_iter / solve_iter_l2f call runs the restatement's own loop, except that x, z1, z2, z4 are
overwritten with a subject's values before the window's first iteration, and that the PCG of every iteration of the window runs exactly
the subject's iteration count, recording residualNorm2 / threshold after every PCG iteration (pcg_ratios).  Everything else -- rho,
prev_rho, gamma, dI, the rho4 E^T scale, the preconditioner diagonal, rhoUpdated, f / b / left_idx / sum_fix_obj after fixes, the
objective history, std_obj, cur_obj, best_bin_obj and the stop decision -- stays the restatement's own and is never read from a subject
(DESIGN.md section 22).

`mutant` (tests only) swaps one expression for a plausible misreading; see MUTANTS.
"""
import numpy as np
import scipy.sparse as sp

MUTANTS = ("pd_rho4", "drop_pending", "gamma_late", "z4_restart_l2f", "y3_noclamp", "sphere_org_n", "esq_count")


def _segsum(prod, ptr, dtype):
    """Sums of the consecutive segments prod[ptr[i]:ptr[i+1]] (empty segments give 0)."""
    out = np.zeros(len(ptr) - 1, dtype)
    ne = ptr[1:] > ptr[:-1]
    if prod.size and ne.any():
        out[ne] = np.add.reduceat(prod, ptr[:-1][ne])
    return out


class NumpyLpBox:
    def __init__(self, n, l, colptr, rowidx, b, f=None, x_update="pcg", vals=None, dtype=np.float64, perm=None, mutant=None):
        # x_update "direct": the HIP kernels' opt-in exact x-update (no reference counterpart), here as a plain dense solve of
        # (dI I + rho4 E^T E) x = rhs -- none of the Woodbury algebra of the kernel / the C oracle's mirror, so it pins their math
        assert mutant is None or mutant in MUTANTS
        self.x_update, self.dt, self.mutant = x_update, dtype, mutant
        n, l = int(n), int(l)
        colptr, rowidx = np.asarray(colptr, np.int64), np.asarray(rowidx, np.int64)
        pv, pr = (np.arange(n), np.arange(l)) if perm is None else (np.asarray(perm[0], np.int64), np.asarray(perm[1], np.int64))
        assert sorted(pv) == list(range(n)) and sorted(pr) == list(range(l))
        self.pv, self.pr = pv, pr
        ipv, ipr = np.empty(n, np.int64), np.empty(l, np.int64)
        ipv[pv], ipr[pr] = np.arange(n), np.arange(l)
        col = ipv[np.repeat(np.arange(n), np.diff(colptr))]
        row = ipr[rowidx]
        val = np.ones(len(rowidx), dtype) if vals is None else np.asarray(vals, dtype)
        self.l = l
        self._set_entries(n, row, col, val)
        self.b = np.asarray(b, dtype)[pv]
        self.f = (np.ones(l, dtype) if f is None else np.asarray(f, dtype))[pr]
        self._lock_state = self._lock_counts = self._rank_of = None

    # ---- E as its stored entries: once sorted by column (E^T w), once by row (E v) ----
    def _set_entries(self, n, row, col, val):
        o = np.lexsort((row, col))
        self.c_row, self.c_col, self.c_val = row[o], col[o], val[o]
        self.c_ptr = np.searchsorted(self.c_col, np.arange(n + 1))
        o = np.lexsort((self.c_col, self.c_row))
        self.r_row, self.r_col, self.r_val = self.c_row[o], self.c_col[o], self.c_val[o]
        self.r_ptr = np.searchsorted(self.r_row, np.arange(self.l + 1))
        self._EtE = None                             # dense E^T E of the direct x-update, built on first use
        if self.dt is np.float64:                    # float64: scipy's sparse products over the same stored entries
            self.Em = sp.csc_matrix((self.c_val, self.c_row, self.c_ptr), shape=(self.l, n))
            self.Etm = self.Em.T.tocsc()

    def _E(self, v):          # E v
        if self.dt is np.float64:
            return self.Em @ v
        return _segsum(self.r_val * v[self.r_col], self.r_ptr, self.dt)

    def _Et(self, w):         # E^T w
        if self.dt is np.float64:
            return self.Etm @ w
        return _segsum(self.c_val * w[self.c_row], self.c_ptr, self.dt)

    def dense_E(self):
        M = np.zeros((self.l, len(self.c_ptr) - 1))
        np.add.at(M, (self.c_row, self.c_col), self.c_val.astype(np.float64))
        return M

    # ---- original order <-> internal order (live variables in ascending original index; rows in original order) ----
    def _rank(self):
        if self._rank_of is not self.left_idx:
            self._rank_of, self._rank_val = self.left_idx, np.searchsorted(np.sort(self.left_idx), self.left_idx)
        return self._rank_val

    def from_natural(self, name, v):
        v = np.asarray(v, self.dt)
        return v[self.pr] if name in ("z4", "y3", "f") else v[self._rank()]

    def natural(self, name):
        v = np.asarray(getattr(self, name), np.float64)
        out = np.empty_like(v)
        if name in ("z4", "y3", "f"):
            out[self.pr] = v
        else:
            out[self._rank()] = v
        return out

    def lock(self, state=None, counts=None):
        """Step-lock the next solve_iter / solve_iter_l2f call.  state: dict(x, z1, z2, z4) of the subject after the previous iteration
        (live variables in ascending original index, rows in original order), or None to keep the restatement's own; counts: the
        subject's PCG iteration count of every iteration of the window."""
        self._lock_state = state
        self._lock_counts = None if counts is None else [int(k) for k in counts]

    def _inject(self):
        if self._lock_state is not None:
            for name in ("x", "z1", "z2", "z4"):
                v = self.from_natural(name, self._lock_state[name])
                assert v.shape == getattr(self, name).shape, name
                setattr(self, name, v.copy())
            self._lock_state = None

    # ADMM_lp_iters_init LPcpp:489-763
    def solve_init(self):
        dt = self.dt
        self.stop_threshold = 1e-4
        self.gamma_val = dt(1.6)
        self.gamma_factor = dt(0.95)
        self.rho_change_step = 25
        self.learning_fact = dt(1 + 1.0 / 100)
        self.pcg_tol = dt(1e-3)
        self.pcg_maxiters = 1000
        self.std_threshold = 1e-12
        self.history_size = 10
        n, l = len(self.c_ptr) - 1, self.l
        self.n, self.org_n = n, n
        self.x = np.ones(n, dt)
        self.y1 = self.x.copy()
        self.y2 = self.x.copy()
        self.z1 = np.zeros(n, dt)
        self.z2 = np.zeros(n, dt)
        self.z4 = np.zeros(l, dt)
        self.y3 = self.f - self._E(self.x)
        self.rho1 = self.rho2 = self.rho4 = dt(25.0)
        self.prev_rho1 = self.prev_rho2 = self.prev_rho4 = dt(25.0)
        self.rhoUpdated = True
        self.std_obj = dt(1.0)
        self.cur_obj = dt(0.0)
        self.obj_list = []
        self.best_bin_obj = self.b @ self.x
        self.left_idx = self.pv.copy()               # original index of every live variable, internal order
        self.fixed_idx = np.zeros(0, int)
        self.fixed_val = np.zeros(0, dt)
        self.sum_fix_obj = dt(0.0)
        self.iter = 0
        self.pcg_trace = []
        self.pcg_ratios = []                         # per iteration: residualNorm2 / threshold after 0, 1, .. k PCG iterations (None: rhs = 0)
        self.x_iters = None
        self.stop = None
        self.ret = 0
        self._drop = False
        self.invdiag = np.zeros(0, dt)
        return 1

    # update_expression LPcpp:2289-2404
    def _update_expression(self):
        self.r4Et_scale = self.rho4          # rho4_E_transpose = rho4 * E^T (LPcpp:2293), kept as its scalar: every product multiplies it in
        self.dI = self.dt(0.0) + (self.rho1 + self.rho2)
        sq = np.ones_like(self.c_val) if self.mutant == "esq_count" else self.c_val * self.c_val       # LPcpp:2382-2390
        self.Esq = _segsum(sq, self.c_ptr, self.dt)
        if self.dt is np.float64 and self.mutant != "esq_count":
            self.Esq = np.asarray(self.Em.multiply(self.Em).sum(axis=0)).ravel()
        self.pd = self.dI + self.rho4 * self.Esq

    def _matvec(self, v):  # calculate_mat_expr_multiplication LPcpp:115-162
        return self.dI * v + self.r4Et_scale * self._Et(self._E(v))

    def _pcg(self, rhs, x, force=None):  # LPcpp:251-335; force: run exactly that many iterations and record the exit ratios
        r = rhs - self._matvec(x)
        rhsNorm2 = rhs @ rhs
        if rhsNorm2 == 0:
            x[:] = 0
            self.pcg_ratios.append(None)
            return 1, 0
        thr = max(self.pcg_tol * self.pcg_tol * rhsNorm2, np.finfo(float).tiny)
        r2 = r @ r
        ratios = [r2 / thr]
        self.pcg_ratios.append(ratios)
        if (r2 < thr) if force is None else (force == 0):
            return 1, 0
        p = self.invdiag * r
        absNew = r @ p
        i = 0
        while i < (self.pcg_maxiters if force is None else force):
            tmp = self._matvec(p)
            alpha = absNew / (p @ tmp)
            if alpha < 0 and force is None:
                return -1, i
            x += alpha * p
            r -= alpha * tmp
            r2 = r @ r
            ratios.append(r2 / thr)
            if force is None and r2 < thr:
                i += 1
                break
            z = self.invdiag * r
            absOld = absNew
            absNew = r @ z
            p = z + (absNew / absOld) * p
            i += 1
        return 1, i

    def _iteration(self, it, it_start, l2f):
        dt = self.dt
        # y1, y2, y3  LPcpp:806-828
        self.y1 = np.clip(self.x + self.z1 / self.rho1, 0.0, 1.0)
        t = (self.x + self.z2 / self.rho2) - 0.5
        radius_n = self.org_n if self.mutant == "sphere_org_n" else self.n
        self.y2 = t * np.power(dt(radius_n), dt(0.5)) / (2 * np.sqrt(t @ t)) + 0.5
        self.y3 = self.f - self._E(self.x) - self.z4 / self.rho4
        if self.mutant != "y3_noclamp":
            self.y3 = np.maximum(self.y3, 0.0)
        if it == 0:
            self._update_expression()
        if it != 0 and self.rhoUpdated and not self._drop:  # LPcpp:851-866
            rcr = self.learning_fact - 1.0
            self.dI = self.dI + rcr * (self.prev_rho1 + self.prev_rho2)
            self.pd = self.pd + rcr * (self.prev_rho1 + self.prev_rho2)
            self.pd = self.pd + (rcr * (self.rho4 if self.mutant == "pd_rho4" else self.prev_rho4)) * self.Esq
            self.r4Et_scale = self.learning_fact * self.r4Et_scale
        self._drop = False
        rhs = (self.rho1 * self.y1 + self.rho2 * self.y2) - ((self.b + self.z1) + self.z2)  # LPcpp:872-878
        rhs = rhs + self.r4Et_scale * self._Et(self.f - self.y3)
        rhs = rhs - self._Et(self.z4)
        if self.rhoUpdated or len(self.invdiag) != self.n:
            # a fix while no rho update is pending leaves the reference with a preconditioner of the old length (LPcpp:1427-1435 is
            # skipped; undefined behaviour there): the project defines that case as "recompute" 
            self.invdiag = np.where(self.pd != 0, 1.0 / self.pd, dt(1.0))
            self.rhoUpdated = False
        force = None
        if self._lock_counts is not None:
            force = self._lock_counts.pop(0)
        xt = self.y1.copy()
        if self.x_update == "direct":
            if self._EtE is None:
                Ed = self.dense_E()
                self._EtE = Ed.T @ Ed
            M = float(self.dI) * np.eye(self.n) + float(self.r4Et_scale) * self._EtE
            xt = np.linalg.solve(M, rhs.astype(np.float64)).astype(dt)
            self.pcg_ratios.append(None)
            cg, k = 1, 0
        else:
            cg, k = self._pcg(rhs, xt, force)
        self.pcg_trace.append(k)
        if l2f and cg == -1:
            self.stop = "pcg_alpha_negative"
            return 2
        self.x = xt
        if l2f:
            self.x_iters[:, self.cc] = self.x
            self.cc += 1
        g = self.gamma_val
        self.z1 = self.z1 + (g * self.rho1) * (self.x - self.y1)
        self.z2 = self.z2 + (g * self.rho2) * (self.x - self.y2)
        upd = (g * self.rho4) * ((self._E(self.x) + self.y3) - self.f)
        restart = (not l2f or self.mutant == "z4_restart_l2f") and it == it_start
        self.z4 = upd if restart else self.z4 + upd
        t0 = max(np.sqrt(self.x @ self.x), 2.2204e-16)
        d1 = self.x - self.y1
        d2 = self.x - self.y2
        self.cvg1 = c1 = np.sqrt(d1 @ d1) / t0
        self.cvg2 = c2 = np.sqrt(d2 @ d2) / t0
        if c1 <= self.stop_threshold and c2 <= self.stop_threshold and (l2f or it != it_start):
            self.stop = "y1_y2"
            if l2f:
                self.ret = 1
            return 1
        late = self.mutant == "gamma_late"
        if late and it != 0 and it % self.rho_change_step == 0:
            self.gamma_val = max(self.gamma_val * self.gamma_factor, dt(1.0))
        if (it + 1) % self.rho_change_step == 0:  # LPcpp:951-970
            self.prev_rho1, self.prev_rho2, self.prev_rho4 = self.rho1, self.rho2, self.rho4
            self.rho1 = self.rho1 * self.learning_fact
            self.rho2 = self.rho2 * self.learning_fact
            self.rho4 = self.rho4 * self.learning_fact
            if not late:
                self.gamma_val = max(self.gamma_val * self.gamma_factor, dt(1.0))
            self.rhoUpdated = True
        self.obj_val = self.b @ self.x
        self.obj_list.append(self.obj_val)
        if len(self.obj_list) >= self.history_size:
            h = np.array(self.obj_list[-self.history_size:], dt)
            mean = h.sum() / len(h)
            var = ((h - mean) ** 2).sum() / (len(h) - 1)
            self.std_obj = (dt(0.0) if var == 0 else np.sqrt(var)) / abs(h[-1])
        if self.std_obj <= self.std_threshold:
            self.ret = 1
            self.stop = "obj_std"
            return 1
        self.cur_obj = self.b @ (self.x >= 0.5).astype(dt)
        if self.best_bin_obj >= self.cur_obj:
            self.best_bin_obj = self.cur_obj
        return 0

    def solve_iter(self, it_start, it_end):  # ADMM_lp_iters LPcpp:766-1095
        self.ret = 0
        self.stop = None
        self._inject()
        it = it_start
        while it < it_end:
            if self._iteration(it, it_start, False):
                break
            it += 1
        self.last_plain_iter_plus1 = it + 1
        self._lock_counts = None
        return self.ret

    def solve_iter_l2f(self, it_start, it_end, vec, fix_num):  # ADMM_lp_iters_l2f LPcpp:1098-1574
        """vec: one entry per live variable in ascending original index (1 / 0 fix, anything else leave)."""
        self.ret = 0
        self.stop = None
        self._inject()
        n = self.n
        self.x_iters = np.zeros((n - fix_num, 500), self.dt)
        self.cc = 0
        if fix_num != 0:
            vec = np.asarray(vec)[:n][self._rank()]
            fixed = (vec == 1) | (vec == 0)
            assert fixed.sum() == fix_num
            keep = ~fixed
            x2 = vec[fixed].astype(self.dt)
            self.fixed_idx = np.concatenate([self.fixed_idx, self.left_idx[fixed]])
            self.fixed_val = np.concatenate([self.fixed_val, x2])
            self.left_idx = self.left_idx[keep]
            if n - fix_num == 0:
                self.ret = 1
                self.stop = "all_fixed"
                self.n = 0
                it_end = it_start
            else:
                self.x = self.x[keep]
                if np.sqrt(self.x @ self.x) < 1e-3:
                    self.ret = 1
                self.y1, self.y2, self.z1, self.z2 = self.y1[keep], self.y2[keep], self.z1[keep], self.z2[keep]
                b2 = self.b[fixed]
                self.b = self.b[keep]
                self.sum_fix_obj = self.sum_fix_obj + b2 @ x2
                xfull = np.zeros(n, self.dt)
                xfull[fixed] = x2
                self.f = self.f - self._E(xfull)                                   # f -= E2 x2 (LPcpp:1278, :1299-1300)
                self.n = n - fix_num
                newcol = np.cumsum(keep) - 1
                e = keep[self.c_col]
                self._set_entries(self.n, self.c_row[e], newcol[self.c_col[e]], self.c_val[e])
                self._update_expression()                                          # LPcpp:1329
                self._drop = self.mutant == "drop_pending"
        self.iter = it_start
        while self.iter < it_end:
            rc = self._iteration(self.iter, it_start, True)
            if rc == 2:
                self._lock_counts = None
                return 1
            if rc:
                break
            self.iter += 1
        self._lock_counts = None
        return self.ret

    def get_x_sol(self):
        out = np.zeros(self.org_n)
        out[self.fixed_idx] = self.fixed_val
        if self.n != 0:
            out[self.left_idx] = (self.x >= 0.5).astype(float)
        return out

    def cal_obj(self):
        return self.sum_fix_obj + self.cur_obj if self.n != 0 else self.sum_fix_obj
