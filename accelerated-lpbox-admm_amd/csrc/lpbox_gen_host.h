// lpbox_gen_host.h -- host-side pieces shared by the two front ends of the GENERIC constrained binary-QP path: the one-problem handle
// (lpbox_gen_capi.hip, lpbox_bqp_*) and the batch of small problems (lpbox_genb_capi.hip, lpbox_bqp_batch_*).  One validation, one set
// of messages, one preset table (SEGcpp:587-672).  Not part of the C-ABI.
#pragma once
#include "../../include/lpbox_hip.h"
#include "lpbox_gen.h"
#include "lpbox_capi_internal.h"

#include <cmath>
#include <vector>

// c1 = pow(n, 1/p), p = 2 (SEGcpp:556) through libm's pow, as the reference and the oracle call it: with the literal exponent the compiler
// may turn the call into sqrt, and glibc's pow is not correctly rounded (n = 2921, 3541: one ulp apart; as ref_c1 of lpbox_big_capi.hip).
// Reference order only, for both front ends; the default order keeps the expression it has always had.
inline double gen_ref_c1(int n) {
    volatile double e = 1.0 / 2;
    return std::pow((double)n, e);
}

struct GenHostCsr { int rows = 0, cols = 0; std::vector<int> ptr, idx; std::vector<double> val; };

struct GenHostProblem {
    int n = 0, m = 0, l = 0;
    GenHostCsr A, C, Ct, E, Et;
    std::vector<int> adiag;
    std::vector<double> b, x0, d, f;
};

inline int gen_load_csr(GenHostCsr &M, int rows, int cols, const int *ptr, const int *idx, const double *val, const char *what) {
    if (!ptr || ptr[0] != 0) return lpbox_fail(LPBOX_E_BADARG, "%s: bad row pointer", what);
    for (int i = 0; i < rows; i++) {
        if (ptr[i + 1] < ptr[i]) return lpbox_fail(LPBOX_E_BADARG, "%s: row pointer not monotone", what);
        if (ptr[i + 1] > ptr[i] && (!idx || !val)) return lpbox_fail(LPBOX_E_BADARG, "%s: index or value array missing", what);
        for (int k = ptr[i]; k < ptr[i + 1]; k++) {
            if (idx[k] < 0 || idx[k] >= cols) return lpbox_fail(LPBOX_E_BADARG, "%s: column index out of range", what);
            if (k > ptr[i] && idx[k] <= idx[k - 1]) return lpbox_fail(LPBOX_E_BADARG, "%s: columns must ascend inside a row", what);
            if (!std::isfinite(val[k])) return lpbox_fail(LPBOX_E_BADARG, "%s has a non-finite stored value (row %d, column %d)", what, i, idx[k]);
        }
    }
    M.rows = rows; M.cols = cols;
    M.ptr.assign(ptr, ptr + rows + 1); M.idx.assign(idx, idx + ptr[rows]); M.val.assign(val, val + ptr[rows]);
    return LPBOX_OK;
}

inline void gen_transpose(const GenHostCsr &S, GenHostCsr &Tt) {   // rows of the result = columns of S, entries in ascending original row order
    Tt.rows = S.cols; Tt.cols = S.rows;
    Tt.ptr.assign((size_t)S.cols + 1, 0);
    for (int c : S.idx) Tt.ptr[c + 1]++;
    for (int j = 0; j < S.cols; j++) Tt.ptr[j + 1] += Tt.ptr[j];
    Tt.idx.resize(S.idx.size()); Tt.val.resize(S.val.size());
    std::vector<int> cur(Tt.ptr.begin(), Tt.ptr.end() - 1);
    for (int i = 0; i < S.rows; i++)
        for (int k = S.ptr[i]; k < S.ptr[i + 1]; k++) { const int p = cur[S.idx[k]]++; Tt.idx[p] = i; Tt.val[p] = S.val[k]; }
}

inline int gen_preset(GenParams &p, int type) {
    switch (type) {
    case 0:      // ADMM_bqp_unconstrained_init SEGcpp:658-672
        p.std_threshold = 1e-6; p.gamma_val = 1.0; p.gamma_factor = 0.99; p.initial_rho = 5; p.learning_fact = 1 + 3.0 / 100; p.history_size = 5;
        p.rho_change_step = 5; p.stop_threshold = 1e-3; p.max_iters = (int)1e4; p.pcg_tol = 1e-3; p.pcg_maxiters = (int)1e3; return LPBOX_OK;
    case 1:      // ADMM_bqp_linear_eq_init :587-601
        p.stop_threshold = 1e-4; p.std_threshold = 1e-6; p.gamma_val = 1.6; p.gamma_factor = 0.95; p.rho_change_step = 5; p.max_iters = (int)5e3;
        p.initial_rho = 1; p.history_size = 3; p.learning_fact = 1 + 5.0 / 100; p.pcg_tol = 1e-4; p.pcg_maxiters = (int)1e3; return LPBOX_OK;
    case 2:      // ADMM_bqp_linear_ineq_init :603-617
    case 3:      // ADMM_bqp_linear_eq_and_uneq_init :620-634
        p.stop_threshold = 1e-4; p.std_threshold = 1e-6; p.gamma_val = 1.6; p.gamma_factor = 0.95; p.rho_change_step = 5; p.max_iters = (int)1e4;
        p.initial_rho = 25; p.history_size = 3; p.learning_fact = 1 + 1.0 / 100; p.pcg_tol = 1e-4; p.pcg_maxiters = (int)1e3; return LPBOX_OK;
    }
    return lpbox_fail(LPBOX_E_BADARG, "preset %d: 0 unconstrained, 1 equality, 2 inequality, 3 both", type);
}

// A NaN in any vector makes every PCG exit test false: max_iters x pcg_maxiters PCG iterations of halt-and-resume chains before the call
// returns (the reference accepts it and computes garbage; the same deliberate deviation as the LP path's, DESIGN.md sections 24 and 26).
inline int gen_check_finite(const double *v, int len, const char *what) {
    for (int i = 0; i < len; i++)
        if (!std::isfinite(v[i])) return lpbox_fail(LPBOX_E_BADARG, "%s has a non-finite entry (index %d)", what, i);
    return LPBOX_OK;
}

inline int gen_set_params(GenParams &p, const double *p11) {
    static const char *const names[11] = {"stop_threshold", "std_threshold", "gamma_val", "gamma_factor", "rho_change_step", "max_iters",
                                          "initial_rho", "history_size", "learning_fact", "pcg_tol", "pcg_maxiters"};
    for (int i = 0; i < 11; i++)      // before anything is written (and before a NaN reaches an int cast): a rejected call changes nothing
        if (!std::isfinite(p11[i])) return lpbox_fail(LPBOX_E_BADARG, "params has a non-finite entry (index %d, %s)", i, names[i]);
    p.stop_threshold = p11[0]; p.std_threshold = p11[1]; p.gamma_val = p11[2]; p.gamma_factor = p11[3]; p.rho_change_step = (int)p11[4];
    p.max_iters = (int)p11[5]; p.initial_rho = p11[6]; p.history_size = (int)p11[7]; p.learning_fact = p11[8]; p.pcg_tol = p11[9];
    p.pcg_maxiters = (int)p11[10];
    if (p.history_size < 2 || p.history_size > GEN_HIST_MAX) return lpbox_fail(LPBOX_E_BADARG, "history_size must be in [2,%d]", GEN_HIST_MAX);
    if (p.rho_change_step < 1 || p.max_iters < 0 || p.pcg_maxiters < 1) return lpbox_fail(LPBOX_E_BADARG, "bad iteration parameters");
    return LPBOX_OK;
}

// The argument list of lpbox_bqp_set_problem, validated and copied (with the transposes of C and E) into `h`.
inline int gen_load_problem(GenHostProblem &h, int n, const int *Ap, const int *Ai, const double *Av, const double *b, const double *x0,
                            int m, const int *Cp, const int *Ci, const double *Cv, const double *d,
                            int l, const int *Ep, const int *Ei, const double *Ev, const double *f) {
    if (n <= 0 || !b || !x0 || m < 0 || l < 0) return lpbox_fail(LPBOX_E_BADARG, "bad problem arguments");
    int rc = gen_load_csr(h.A, n, n, Ap, Ai, Av, "A");
    if (rc < 0) return rc;
    if ((rc = gen_check_finite(b, n, "b")) < 0 || (rc = gen_check_finite(x0, n, "x0")) < 0) return rc;
    h.adiag.assign(n, -1);
    for (int i = 0; i < n; i++) {
        for (int k = Ap[i]; k < Ap[i + 1]; k++) if (Ai[k] == i) h.adiag[i] = k;
        if (h.adiag[i] < 0)      // `.diagonal() +=` on a compressed sparse matrix needs the entry to exist (SEGcpp:1483): store explicit zeros
            return lpbox_fail(LPBOX_E_BADARG, "A has no stored diagonal entry in row %d", i);
    }
    if (m > 0) {
        if (!d) return lpbox_fail(LPBOX_E_BADARG, "d missing");
        if ((rc = gen_load_csr(h.C, m, n, Cp, Ci, Cv, "C")) < 0 || (rc = gen_check_finite(d, m, "d")) < 0) return rc;
        gen_transpose(h.C, h.Ct); h.d.assign(d, d + m);
    }
    if (l > 0) {
        if (!f) return lpbox_fail(LPBOX_E_BADARG, "f missing");
        if ((rc = gen_load_csr(h.E, l, n, Ep, Ei, Ev, "E")) < 0 || (rc = gen_check_finite(f, l, "f")) < 0) return rc;
        gen_transpose(h.E, h.Et); h.f.assign(f, f + l);
    }
    h.n = n; h.m = m; h.l = l;
    h.b.assign(b, b + n); h.x0.assign(x0, x0 + n);
    return LPBOX_OK;
}
