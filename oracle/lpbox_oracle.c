/*
 * lpbox_oracle.c -- CPU ORACLE (test infrastructure, NOT product code).  See lpbox_oracle.h.
 *
 * Restates, without Eigen, the LP path of the reference:
 *   LPcpp = LinerProgramming/LinearProgramming/cython_solver/LPboxADMMsolver.cpp
 *   LPh   = LinerProgramming/LinearProgramming/cython_solver/LPboxADMMsolver.h
 *
 * Eigen 3.3.8 primitives restated here (the library is not vendored by the reference):
 *   - SparseMatrix<double,ColMajor> * dense vector  (SparseDenseProduct.h, ColMajor branch):
 *       res = 0; for each column j: rhs_j = 1.0 * v[j]; for each stored (i,j): res[i] += val * rhs_j
 *   - dot / squaredNorm / sum   (Core/Redux.h, LinearVectorizedTraversal, SSE2 Packet2d, NoUnrolling):
 *       two packet accumulators walking the vector 4 doubles at a time, see redux_sum_eigen()
 *   - DiagonalPreconditioner::compute/solve (IterativeLinearSolvers/BasicPreconditioners.h):
 *       invdiag[j] = (diag[j] != 0) ? 1/diag[j] : 1 ;  solve(b) = invdiag .* b
 *   - setFromTriplets: column-major, row indices ascending inside a column, duplicates summed
 *
 * Build: gcc -O3 -ffp-contract=off (the reference's flags are plain -O3, LP/cython_solver/Makefile:9,34;
 * x86-64 baseline has no FMA so contraction never happens there either).
 */
#define _POSIX_C_SOURCE 200809L   /* clock_gettime */
#include "lpbox_oracle.h"

#include <float.h>
#include <math.h>
#include <time.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* ------------------------------------------------------------------------------------------ */
/* sparse matrix, column-major (Eigen::SparseMatrix<double, ColMajor>, LPh:17)                 */
/* ------------------------------------------------------------------------------------------ */
typedef struct {
    int rows, cols, nnz;
    int *ptr;    /* cols+1 */
    int *idx;    /* row index of each stored entry, ascending inside a column */
    double *val;
} csc_t;

static void csc_free(csc_t *m) {
    free(m->ptr); free(m->idx); free(m->val);
    memset(m, 0, sizeof(*m));
}

static void csc_alloc(csc_t *m, int rows, int cols, int nnz) {
    m->rows = rows; m->cols = cols; m->nnz = nnz;
    m->ptr = (int *)calloc((size_t)cols + 1, sizeof(int));
    m->idx = (int *)malloc(sizeof(int) * (size_t)(nnz > 0 ? nnz : 1));
    m->val = (double *)malloc(sizeof(double) * (size_t)(nnz > 0 ? nnz : 1));
}

static void csc_copy(csc_t *dst, const csc_t *src) {
    csc_free(dst);
    csc_alloc(dst, src->rows, src->cols, src->nnz);
    memcpy(dst->ptr, src->ptr, sizeof(int) * ((size_t)src->cols + 1));
    if (src->nnz) {
        memcpy(dst->idx, src->idx, sizeof(int) * (size_t)src->nnz);
        memcpy(dst->val, src->val, sizeof(double) * (size_t)src->nnz);
    }
}

/* E_transpose = E.transpose() evaluated into a ColMajor matrix (LPcpp:2292): sorted inner indices. */
static void csc_transpose(csc_t *dst, const csc_t *src) {
    csc_free(dst);
    csc_alloc(dst, src->cols, src->rows, src->nnz);
    int *cnt = (int *)calloc((size_t)src->rows + 1, sizeof(int));
    for (int k = 0; k < src->nnz; k++) cnt[src->idx[k] + 1]++;
    for (int i = 0; i < src->rows; i++) cnt[i + 1] += cnt[i];
    memcpy(dst->ptr, cnt, sizeof(int) * ((size_t)src->rows + 1));
    for (int j = 0; j < src->cols; j++) {
        for (int k = src->ptr[j]; k < src->ptr[j + 1]; k++) {
            int i = src->idx[k];
            int p = cnt[i]++;
            dst->idx[p] = j;          /* j ascending => sorted */
            dst->val[p] = src->val[k];
        }
    }
    free(cnt);
}

typedef struct { int r, c; double v; } trip_t;

/* SparseMatrix::setFromTriplets (LPcpp:1172,1180,2443): sorted, duplicates summed (in input order). */
static void csc_from_triplets(csc_t *m, int rows, int cols, trip_t *t, int nt) {
    trip_t *s = (trip_t *)malloc(sizeof(trip_t) * (size_t)(nt > 0 ? nt : 1));
    /* counting sort by column then insertion by row keeps duplicates in input order */
    int *cnt = (int *)calloc((size_t)cols + 1, sizeof(int));
    for (int k = 0; k < nt; k++) cnt[t[k].c + 1]++;
    for (int j = 0; j < cols; j++) cnt[j + 1] += cnt[j];
    int *pos = (int *)malloc(sizeof(int) * ((size_t)cols + 1));
    memcpy(pos, cnt, sizeof(int) * ((size_t)cols + 1));
    for (int k = 0; k < nt; k++) s[pos[t[k].c]++] = t[k];
    for (int j = 0; j < cols; j++) {             /* stable insertion sort by row inside a column */
        for (int a = cnt[j] + 1; a < cnt[j + 1]; a++) {
            trip_t key = s[a];
            int b = a - 1;
            while (b >= cnt[j] && s[b].r > key.r) { s[b + 1] = s[b]; b--; }
            s[b + 1] = key;
        }
    }
    int nnz = 0;
    for (int k = 0; k < nt; k++)
        if (k == 0 || s[k].c != s[k - 1].c || s[k].r != s[k - 1].r) nnz++;
    csc_free(m);
    csc_alloc(m, rows, cols, nnz);
    int p = -1;
    for (int k = 0; k < nt; k++) {
        if (k == 0 || s[k].c != s[k - 1].c || s[k].r != s[k - 1].r) {
            p++;
            m->idx[p] = s[k].r;
            m->val[p] = s[k].v;
            m->ptr[s[k].c + 1]++;
        } else {
            m->val[p] += s[k].v;
        }
    }
    for (int j = 0; j < cols; j++) m->ptr[j + 1] += m->ptr[j];
    free(s); free(cnt); free(pos);
}

/* mat_mul_vec (LPcpp:102-108) -> Eigen ColMajor sparse * dense: res zeroed, then column scatter. */
static void spmv(const csc_t *m, const double *v, double *res) {
    for (int i = 0; i < m->rows; i++) res[i] = 0.0;
    for (int j = 0; j < m->cols; j++) {
        double rhs_j = 1.0 * v[j];
        for (int k = m->ptr[j]; k < m->ptr[j + 1]; k++) res[m->idx[k]] += m->val[k] * rhs_j;
    }
}

struct lpo;
static void spmv_E(struct lpo *o, const double *v, double *res);

/* ------------------------------------------------------------------------------------------ */
/* the solver object (members of class LPboxADMMsolver, LPh:111-290)                           */
/* ------------------------------------------------------------------------------------------ */
struct lpo {
    int print_info, verbose;
    int order_mode, T;

    /* LPh:111-148 hyper-parameters */
    double stop_threshold, std_threshold, initial_rho, gamma_val, learning_fact, history_size;
    double projection_lp, gamma_factor, pcg_tol, rel_tol;
    int max_iters, rho_change_step, pcg_maxiters;

    /* LPh:199-262 */
    csc_t E, orgE, Et, r4Et;       /* *E_ptr, *org_E_ptr, E_transpose, rho4_E_transpose */
    double r4s;                    /* the scalar of rho4_E_transpose as the kernels carry it: rho4 at update_expression, times learning_fact per update */
    double *b, *f;                 /* *b_ptr, *f_ptr (current problem) */
    int n, l, org_n;
    double *x, *y1, *y2, *z1, *z2, *y3, *z4;
    int x_len;                     /* x_sol.rows() (differs from n only after an all-fixed call) */
    double *temp_vec, *temp_cg, *temp_mm; /* temp_vec, temp_vec_for_cg, temp_vec_for_mat_mul */
    double *fy, *x_try;            /* temporaries Eigen materialises: (f - y3) LPcpp:874, x_sol_try :1439 */
    double *Dd;                    /* diagonal of _2A_plus_rho1_rho2 (LPcpp:2339-2343) */
    double *pd;                    /* diagonal of preconditioner_diag_mat */
    double *Esq;                   /* Esq_diag */
    double *invdiag; int invdiag_len; /* DiagonalPreconditioner::m_invdiag */
    double cur_obj; int rhoUpdated;
    double rho1, rho2, rho3, rho4, prev_rho1, prev_rho2, prev_rho3, prev_rho4;
    double *obj_list; int obj_n, obj_cap;
    double std_obj, cvg1, cvg2, rho_change_ratio, best_bin_obj, prev_obj, prev_sum, obj_val;
    double *best_sol;

    /* early fix bookkeeping LPh:238-262 */
    double *x_iters; int xi_rows, xi_cols;  /* column-major (rows x 500), LPcpp:1113 */
    int fix_sum;
    int *left_idx;                 /* length n: original index of each live variable */
    int *ret_idx_prev; double *ret_val_prev; int ret_prev_len;
    int *ret_idx; double *ret_val; int ret_len;
    double fix_obj, sum_fix_obj;
    int iter;                      /* member iter, LPh:279 (advanced by l2f only) */

    /* inspection */
    int last_plain_iter_plus1, last_pcg_iters, last_stop;
    long total_pcg, total_outer, pow_sqrt_mismatch;
    int *pcg_trace; int trace_n, trace_cap;
    double *full;                  /* scratch, org_n + padding, for the GPU reduction order */
    int *gpu_pos; int gpu_pos_n;   /* storage position of each original variable in the kernels (NULL = identity) */
    int gpu_npos;                  /* number of storage positions (>= org_n; holes contribute +0.0) */
    int gpu_chunk;                 /* > 0: two-level order of the large-instance kernels (workgroup partials of `chunk` positions) */
    int pcg_lean, lean_row_chunk;  /* the large-instance kernels' opt-in comm-lean PCG (NOT the reference's arithmetic): p.Mp = dI (p.p) + r4Et (q.q),
                                      q = E p; q.q summed over the rows in workgroup chunks of lean_row_chunk rows (lpo_set_pcg_lean) */
    double *lean_buf;
    int gpu_ranks;                 /* > 1: the variable-sharded run (lpbox_big_*): contiguous blocks of variables per rank, every sum over
                                      variables = per-rank sums (each in the order above, positions counted from the rank's first variable)
                                      added in rank order p0 + p1 + p2 ... */
    int *row_G;                    /* GPU order: lanes that share row i of E (1,2,4,8); NULL = 1 */
    int *col_own, *col_help;       /* GPU order: split of the sum over column j of E (by ORIGINAL variable): own[j] leading entries,
                                      then chunks of help[4j+q] entries by quad lane q; NULL = unsplit */
    double *valT; int *curT;       /* scratch of spmv_Et */
    FILE *log_fp;                  /* does_log (LPh:148, default ON in the reference): the per-iteration text log of ADMM_lp_iters */
    int *orgEr_ptr, *orgEr_col; double *orgEr_val;   /* CSR view of org_E (rows in ascending column order) */
    double *full_v;                /* scratch: a live vector expanded to the original variable order */
    int x_update;                  /* 0 = the reference's PCG (default); 1 = the kernels' opt-in DIRECT x-update (no reference counterpart) */
    double *H; int H_valid, H_ld;  /* direct mode: (c I + E E^T)^-1 over the rows of E, row pitch H_ld */
    double *dt, *du, *dsig, *dw, *dq; /* direct mode scratch and W */
    int *dir_g, *dgrow, nG;        /* direct mode: dense index of each G row (-1 = D row), its inverse map */
    int has_problem, inited;
};

/* first variable of rank rk when `total` variables are dealt in contiguous blocks to `world` ranks (lpbox_hip/dist.py shard_range) */
static int rank_lo(int total, int world, int rk) {
    const int base = total / world, extra = total % world;
    return rk * base + (rk < extra ? rk : extra);
}

/* GPU order of a row of E (lpbox_lp_kernels.hip rows_gather): the kernels never compact E -- a fixed variable contributes
 * +0.0 -- and G = row_G[i] lanes share row i: lane g adds entries g, g+G, g+2G, ... (ascending column) starting from +0.0,
 * the G partials are combined by an xor butterfly.  full_v = the multiplied vector in ORIGINAL variable order. */
static void spmv_orgE_split(lpo_t *o, const double *full_v, double *res) {
    if (o->gpu_ranks > 1) {        /* every rank sums its own columns of the row (ascending), the rank partials are added in rank order */
        const int W = o->gpu_ranks;
        for (int i = 0; i < o->orgE.rows; i++) {
            double total = 0.0;
            int k = o->orgEr_ptr[i];
            for (int rk = 0; rk < W; rk++) {
                const int hi = rank_lo(o->org_n, W, rk + 1);
                double part = 0.0;
                for (; k < o->orgEr_ptr[i + 1] && o->orgEr_col[k] < hi; k++) part = part + o->orgEr_val[k] * (1.0 * full_v[o->orgEr_col[k]]);
                total = rk == 0 ? part : total + part;
            }
            res[i] = total;
        }
        return;
    }
    for (int i = 0; i < o->orgE.rows; i++) {
        const int G = o->row_G ? o->row_G[i] : 1;
        double part[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        int e = 0;
        for (int k = o->orgEr_ptr[i]; k < o->orgEr_ptr[i + 1]; k++, e++)
            part[e % G] = part[e % G] + o->orgEr_val[k] * (1.0 * full_v[o->orgEr_col[k]]);
        for (int stride = 1; stride < G; stride <<= 1)
            for (int g = 0; g < G; g += 2 * stride) part[g] = part[g] + part[g + stride];
        res[i] = part[0];
    }
}

/* Mt * w with Mt = E^T (scaled or not), a vector over the rows of E (LPcpp:102-108 on E_transpose / rho4_E_transpose).
 * Eigen's column-major product accumulates res[j] over the rows of E in ascending order from 0 -- per j that is the sequential
 * sum below with no split.  GPU order (lp_window_kernel cols_gather): the own lane adds the first own[j] entries, the rest
 * goes in consecutive chunks to the lanes q = 0..3 of the variable's quad; res[j] = own + ((h0 + h1) + (h2 + h3)). */
static void spmv_Et(struct lpo *o, const csc_t *Mt, const double *w, double *res) {
    if (o->order_mode != LPO_ORDER_GPU || !o->col_own) { spmv(Mt, w, res); return; }
    const csc_t *E = &o->E;
    const int n = E->cols;
    o->valT = (double *)realloc(o->valT, sizeof(double) * (size_t)(E->nnz + 1));
    o->curT = (int *)realloc(o->curT, sizeof(int) * (size_t)(n + 1));
    for (int j = 0; j < n; j++) o->curT[j] = E->ptr[j];
    for (int i = 0; i < Mt->cols; i++)                     /* values of Mt re-ordered like the entries of E (both ascend in i) */
        for (int k = Mt->ptr[i]; k < Mt->ptr[i + 1]; k++) o->valT[o->curT[Mt->idx[k]]++] = Mt->val[k];
    for (int j = 0; j < n; j++) {
        const int oj = o->left_idx[j];
        const int b = E->ptr[j], e = E->ptr[j + 1];
        int own = o->col_own[oj];
        if (own > e - b) own = e - b;
        double acc = 0.0;
        int k = b;
        for (; k < b + own; k++) acc = acc + o->valT[k] * (1.0 * w[E->idx[k]]);
        if (k < e) {
            double h[4] = {0.0, 0.0, 0.0, 0.0};
            for (int q = 0; q < 4; q++)
                for (int c = 0; c < o->col_help[4 * oj + q] && k < e; c++, k++) h[q] = h[q] + o->valT[k] * (1.0 * w[E->idx[k]]);
            acc = acc + ((h[0] + h[1]) + (h[2] + h[3]));
        }
        res[j] = acc;
    }
}

/* E * v for a vector over the current live variables (LPcpp:102-108 on *E_ptr) */
static void spmv_E(lpo_t *o, const double *v, double *res) {
    if (o->order_mode != LPO_ORDER_GPU) { spmv(&o->E, v, res); return; }
    for (int j = 0; j < o->org_n; j++) o->full_v[j] = 0.0;
    for (int i = 0; i < o->n; i++) o->full_v[o->left_idx[i]] = v[i];
    spmv_orgE_split(o, o->full_v, res);
}

lpo_t *lpo_create(int print_info) {
    lpo_t *o = (lpo_t *)calloc(1, sizeof(lpo_t));
    o->print_info = print_info;   /* LPcpp:477-480 */
    o->order_mode = LPO_ORDER_EIGEN;
    o->T = 512;
    o->rhoUpdated = 1;            /* LPh:214 */
    o->std_obj = 1;               /* LPh:219 */
    o->cur_obj = 0;               /* LPh:213 */
    return o;
}

static void free_state(lpo_t *o) {
    free(o->x); free(o->y1); free(o->y2); free(o->z1); free(o->z2); free(o->y3); free(o->z4);
    free(o->temp_vec); free(o->temp_cg); free(o->temp_mm); free(o->Dd); free(o->pd); free(o->Esq); free(o->lean_buf); o->lean_buf = NULL;
    free(o->invdiag); free(o->obj_list); free(o->best_sol); free(o->x_iters); free(o->left_idx);
    free(o->ret_idx_prev); free(o->ret_val_prev); free(o->ret_idx); free(o->ret_val);
    free(o->pcg_trace); free(o->full); free(o->fy); free(o->x_try); free(o->full_v);
    o->fy = o->x_try = o->full_v = NULL;
    o->x = o->y1 = o->y2 = o->z1 = o->z2 = o->y3 = o->z4 = NULL;
    o->temp_vec = o->temp_cg = o->temp_mm = o->Dd = o->pd = o->Esq = o->invdiag = NULL;
    o->obj_list = o->best_sol = o->x_iters = NULL;
    o->left_idx = o->ret_idx_prev = o->ret_idx = NULL;
    o->ret_val_prev = o->ret_val = NULL;
    o->pcg_trace = NULL; o->full = NULL;
}

void lpo_destroy(lpo_t *o) {
    if (!o) return;
    free_state(o);
    csc_free(&o->E); csc_free(&o->orgE); csc_free(&o->Et); csc_free(&o->r4Et);
    if (o->log_fp) fclose(o->log_fp);
    free(o->b); free(o->f); free(o->gpu_pos); free(o->row_G); free(o->col_own); free(o->col_help); free(o->valT); free(o->curT);
    free(o->orgEr_ptr); free(o->orgEr_col); free(o->orgEr_val);
    free(o->H); free(o->dt); free(o->du); free(o->dsig); free(o->dw); free(o->dq); free(o->dir_g); free(o->dgrow);
    free(o);
}

void lpo_set_order(lpo_t *o, int mode, int T) {
    o->order_mode = mode;
    if (T >= 64 && T % 64 == 0) o->T = T;
}

void lpo_set_verbose(lpo_t *o, int verbose) { o->verbose = verbose; }
void lpo_set_chunk(lpo_t *o, int chunk) { o->gpu_chunk = chunk > 0 ? chunk : 0; }
void lpo_set_ranks(lpo_t *o, int ranks) { o->gpu_ranks = ranks > 1 ? ranks : 0; }
/* Mirror of lpbox_big_set_pcg_mode(LPBOX_PCG_COMM_LEAN) -- no reference counterpart: the step length of the PCG is taken from
 * p.Mp = dI (p.p) + r4Et (q.q) with q = E p instead of the dot product p.(M p) (LPcpp:300), everything else unchanged.  row_chunk = rows per
 * workgroup of the kernel that squares q (one rank: the row-gather kernel's; several ranks: 256, one row per thread of the block sum). */
void lpo_set_pcg_lean(lpo_t *o, int on, int row_chunk) { o->pcg_lean = on != 0; o->lean_row_chunk = row_chunk > 0 ? row_chunk : 256; }
void lpo_set_x_update(lpo_t *o, int mode) { o->x_update = mode == 1 ? 1 : 0; o->H_valid = 0; }
void lpo_set_direct_rows(lpo_t *o, const int *gidx_of_row, int l) {
    free(o->dir_g);
    o->dir_g = (int *)malloc(sizeof(int) * (size_t)(l + 1));
    memcpy(o->dir_g, gidx_of_row, sizeof(int) * (size_t)l);
    o->H_valid = 0;
}

void lpo_set_positions(lpo_t *o, const int *pos_of_var, int n, int npos) {
    free(o->gpu_pos);
    o->gpu_pos = NULL; o->gpu_pos_n = 0; o->gpu_npos = 0;
    if (pos_of_var && n > 0) {
        o->gpu_pos = (int *)malloc(sizeof(int) * (size_t)n);
        memcpy(o->gpu_pos, pos_of_var, sizeof(int) * (size_t)n);
        o->gpu_pos_n = n;
        o->gpu_npos = npos > n ? npos : n;
        for (int i = 0; i < n; i++) if (pos_of_var[i] >= o->gpu_npos) o->gpu_npos = pos_of_var[i] + 1;
    }
}

void lpo_set_row_split(lpo_t *o, const int *lanes_of_row, int l) {
    free(o->row_G);
    o->row_G = NULL;
    if (lanes_of_row && l > 0) {
        o->row_G = (int *)malloc(sizeof(int) * (size_t)l);
        memcpy(o->row_G, lanes_of_row, sizeof(int) * (size_t)l);
    }
}

void lpo_set_col_split(lpo_t *o, const int *own, const int *help4, int n) {
    free(o->col_own); free(o->col_help);
    o->col_own = o->col_help = NULL;
    if (own && help4 && n > 0) {
        o->col_own = (int *)malloc(sizeof(int) * (size_t)n);
        o->col_help = (int *)malloc(sizeof(int) * 4 * (size_t)n);
        memcpy(o->col_own, own, sizeof(int) * (size_t)n);
        memcpy(o->col_help, help4, sizeof(int) * 4 * (size_t)n);
    }
}

/* ------------------------------------------------------------------------------------------ */
/* reductions                                                                                  */
/* ------------------------------------------------------------------------------------------ */

/* Eigen 3.3.8 Core/Redux.h, redux_impl<scalar_sum_op, Evaluator, LinearVectorizedTraversal, NoUnrolling>,
 * PacketSize = 2 (SSE2 Packet2d, the default for g++ -O3 on x86-64), alignedStart = 0. */
static double redux_sum_eigen(const double *a, int size) {
    if (size <= 0) return 0.0; /* Eigen asserts size>0; the reference never reduces an empty vector */
    const int P = 2;
    const int alignedSize2 = (size / (2 * P)) * (2 * P);
    const int alignedSize = (size / P) * P;
    const int alignedEnd2 = alignedSize2, alignedEnd = alignedSize;
    double res;
    if (alignedSize) {
        double p0a = a[0], p0b = a[1];
        if (alignedSize > P) {
            double p1a = a[2], p1b = a[3];
            for (int index = 2 * P; index < alignedEnd2; index += 2 * P) {
                p0a = p0a + a[index];     p0b = p0b + a[index + 1];
                p1a = p1a + a[index + 2]; p1b = p1b + a[index + 3];
            }
            p0a = p0a + p1a; p0b = p0b + p1b;
            if (alignedEnd > alignedEnd2) { p0a = p0a + a[alignedEnd2]; p0b = p0b + a[alignedEnd2 + 1]; }
        }
        res = p0a + p0b; /* predux(Packet2d) */
        for (int index = alignedEnd; index < size; ++index) res = res + a[index];
    } else {
        res = a[0];
        for (int index = 1; index < size; ++index) res = res + a[index];
    }
    return res;
}

/* The HIP kernels' fixed reduction tree (accelerated-lpbox-admm_amd/csrc/lpbox_lp_kernels.hip, block_sum):
 * value of ORIGINAL variable position pos is owned by thread pos % T, slot pos / T; a thread adds its slots in
 * ascending order starting from +0.0 (fixed / out-of-range positions contribute +0.0); a 64-lane wavefront
 * combines lane l with l^32, then l^16, then pairs, quads, 8, 16 inside a row of 16 lanes (lpbox_dev_common.h); the W = T/64 wave
 * partials by a balanced tree over the wave index. */
static double redux_sum_gpu_full(const double *full, int len, int T) {
    double local[1024];
    for (int t = 0; t < T; t++) local[t] = 0.0;
    for (int pos = 0; pos < len; pos++) { int t = pos % T; local[t] = local[t] + full[pos]; }
    int W = T / 64;
    double part[16];
    for (int w = 0; w < W; w++) {
        double *a = local + 64 * w;
        for (int i = 0; i < 32; i++) a[i] = a[i] + a[i + 32];              /* halves first (v_permlane32_swap) */
        for (int i = 0; i < 16; i++) a[i] = a[i] + a[i + 16];              /* then the row pairs (v_permlane16_swap) */
        for (int stride = 1; stride < 16; stride <<= 1)                    /* then pairs, quads, 8, 16 inside a row of 16 lanes (DPP) */
            for (int i = 0; i < 16; i += 2 * stride) a[i] = a[i] + a[i + stride];
        part[w] = a[0];
    }
    for (int stride = 1; stride < W; stride <<= 1)          /* wave partials: a second balanced tree (block_sum) */
        for (int i = 0; i < W; i += 2 * stride) part[i] = part[i] + part[i + stride];
    return part[0];
}

/* sum of a[0..cnt) where compact element i sits at original position map[i] */
static double reduce(lpo_t *o, const double *a, int cnt, const int *map) {
    if (o->order_mode == LPO_ORDER_EIGEN) return redux_sum_eigen(a, cnt);
    const int use_pos = o->gpu_pos && o->gpu_pos_n == o->org_n;
    const int npos = use_pos ? o->gpu_npos : o->org_n;
    for (int i = 0; i < npos; i++) o->full[i] = 0.0;
    if (use_pos)
        for (int i = 0; i < cnt; i++) o->full[o->gpu_pos[map[i]]] = a[i];
    else
        for (int i = 0; i < cnt; i++) o->full[map[i]] = a[i];
    if (o->gpu_chunk > 0) {        /* lpbox_big_kernels.hip: block tree per chunk, then the same tree over the chunk partials */
        const int CH = o->gpu_chunk, W = o->gpu_ranks > 1 ? o->gpu_ranks : 1;
        double total = 0.0;
        for (int rk = 0; rk < W; rk++) {
            const int lo = rank_lo(npos, W, rk), hi = rank_lo(npos, W, rk + 1), nloc = hi - lo, Gn = (nloc + CH - 1) / CH;
            double *part = o->full + npos;
            for (int g = 0; g < Gn; g++) {
                int len = nloc - g * CH; if (len > CH) len = CH;
                part[g] = redux_sum_gpu_full(o->full + lo + (size_t)g * CH, len, o->T);
            }
            const double pr = redux_sum_gpu_full(part, Gn, o->T);
            total = rk == 0 ? pr : total + pr;
        }
        return total;
    }
    return redux_sum_gpu_full(o->full, npos, o->T);
}

static double dot_live(lpo_t *o, const double *a, const double *b) { /* a.dot(b) over the live variables */
    for (int i = 0; i < o->n; i++) o->temp_cg[i + o->n] = a[i] * b[i];
    return reduce(o, o->temp_cg + o->n, o->n, o->left_idx);
}

static double sqnorm_live(lpo_t *o, const double *a) { return dot_live(o, a, a); }

/* std::pow(v, 1.0/2) as the reference writes it (LPcpp:376); sqrt() is what the GPU uses -- count mismatches */
static double pow_half(lpo_t *o, double v) {
    if (o->order_mode == LPO_ORDER_GPU) return sqrt(v);   /* GPU order = the kernels' numerics, which use sqrt */
    double p = pow(v, 1.0 / 2);
    if (p != sqrt(v) && !(p != p)) o->pow_sqrt_mismatch++;
    return p;
}

/* ------------------------------------------------------------------------------------------ */
/* problem input                                                                               */
/* ------------------------------------------------------------------------------------------ */
int lpo_set_problem(lpo_t *o, int n, int l, int nnz, const int *colptr, const int *rowidx,
                    const double *vals, const double *b, const double *f) {
    if (n <= 0 || l <= 0 || nnz < 0) return -1;
    csc_free(&o->E);
    csc_alloc(&o->E, l, n, nnz);
    memcpy(o->E.ptr, colptr, sizeof(int) * ((size_t)n + 1));
    for (int k = 0; k < nnz; k++) { o->E.idx[k] = rowidx[k]; o->E.val[k] = vals ? vals[k] : 1.0; }
    for (int j = 0; j < n; j++)
        for (int k = colptr[j]; k < colptr[j + 1]; k++) {
            if (rowidx[k] < 0 || rowidx[k] >= l) return -2;
            if (k > colptr[j] && rowidx[k] <= rowidx[k - 1]) return -3;
        }
    csc_copy(&o->orgE, &o->E);                 /* LPcpp:2526-2529 */
    {   /* CSR view of org_E for the GPU-order row sums */
        csc_t tr; memset(&tr, 0, sizeof(tr));
        csc_transpose(&tr, &o->orgE);
        free(o->orgEr_ptr); free(o->orgEr_col); free(o->orgEr_val);
        o->orgEr_ptr = tr.ptr; o->orgEr_col = tr.idx; o->orgEr_val = tr.val;
    }
    free(o->b); free(o->f);
    o->b = (double *)malloc(sizeof(double) * (size_t)n);
    o->f = (double *)malloc(sizeof(double) * (size_t)l);
    memcpy(o->b, b, sizeof(double) * (size_t)n);
    memcpy(o->f, f, sizeof(double) * (size_t)l);
    o->n = n; o->l = l;
    o->has_problem = 1; o->inited = 0;
    return 0;
}

/* readSparseMat LPcpp:2416-2444, readDenseVec :2407-2414, readFile :2446-2545 */
int lpo_read_files(lpo_t *o, const char *path_C, const char *path_b, int k) {
    FILE *fc = fopen(path_C, "r");
    if (!fc) return -1;
    int cap = 1024, nt = 0, row, col, max_row = 0, max_col = 0;
    double val;
    trip_t *t = (trip_t *)malloc(sizeof(trip_t) * (size_t)cap);
    while (fscanf(fc, "%d,%d,%lf\n", &row, &col, &val) == 3) {
        if (row > max_row) max_row = row;
        if (col > max_col) max_col = col;
        if (nt == cap) { cap *= 2; t = (trip_t *)realloc(t, sizeof(trip_t) * (size_t)cap); }
        t[nt].r = row - 1; t[nt].c = col - 1;
        t[nt].v = (k == 2) ? -1.0 * val : val;          /* LPcpp:2436-2439 */
        nt++;
    }
    fclose(fc);
    if (max_row == 0 || max_col == 0) { free(t); return -2; }
    csc_t E; memset(&E, 0, sizeof(E));
    csc_from_triplets(&E, max_row, max_col, t, nt);      /* LPcpp:2441-2443 */
    free(t);
    FILE *fb = fopen(path_b, "r");
    if (!fb) { csc_free(&E); return -3; }
    double *b = (double *)malloc(sizeof(double) * (size_t)max_col);
    for (int i = 0; i < max_col; i++) {
        if (fscanf(fb, "%lf\n", &b[i]) != 1) { fclose(fb); free(b); csc_free(&E); return -4; } /* LPcpp:2409-2412 exit(-1) */
        b[i] = -1.0 * b[i];                               /* LPcpp:2520 */
    }
    fclose(fb);
    double *f = (double *)malloc(sizeof(double) * (size_t)max_row);
    for (int i = 0; i < max_row; i++) f[i] = 1.0;         /* LPcpp:2522 */
    int rc = lpo_set_problem(o, max_col, max_row, E.nnz, E.ptr, E.idx, E.val, b, f);
    free(b); free(f); csc_free(&E);
    return rc;
}

/* ------------------------------------------------------------------------------------------ */
/* update_expression  LPcpp:2289-2404                                                          */
/* ------------------------------------------------------------------------------------------ */
static void update_expression(lpo_t *o) {
    const int n = o->n;
    csc_transpose(&o->Et, &o->E);                          /* :2292 */
    csc_copy(&o->r4Et, &o->Et);                            /* :2293 rho4_E_transpose = rho4 * E_transpose */
    for (int k = 0; k < o->r4Et.nnz; k++) o->r4Et.val[k] = o->rho4 * o->Et.val[k];
    o->r4s = o->rho4;
    for (int j = 0; j < n; j++) {                          /* :2336-2343 zero triplets, diagonal += rho1+rho2 */
        double d = 0.0;
        d += o->rho1 + o->rho2;
        o->Dd[j] = d;
        o->pd[j] = d;                                      /* :2352 preconditioner_diag_mat = _2A_plus_rho1_rho2 */
    }
    for (int j = 0; j < n; j++) {                          /* :2378-2390 */
        double e = 0.0;
        for (int k = o->E.ptr[j]; k < o->E.ptr[j + 1]; k++)
            if (o->E.val[k] != 0.0) e += o->E.val[k] * o->E.val[k];
        o->Esq[j] = e;
    }
    for (int j = 0; j < n; j++) o->pd[j] += o->rho4 * o->Esq[j]; /* :2391 */
}

/* calculate_mat_expr_multiplication LPcpp:115-162 with the expression list of :2368-2376:
 *   result = D * x  +  rho4_E_transpose * (E * x)                                   */
static void mat_expr_mul(lpo_t *o, const double *x, double *result) {
    const int n = o->n, l = o->l;
    for (int j = 0; j < n; j++) { result[j] = 0.0; result[j] += o->Dd[j] * (1.0 * x[j]); } /* diagonal sparse * vec */
    double *t1 = o->temp_mm;             /* temp_vec_for_mat_mul: E*x (length l) ... */
    double *t2 = o->temp_mm + l;         /* ... then rho4Et*(.) (length n); Eigen evaluates the aliased product into a temporary */
    spmv_E(o, x, t1);
    spmv_Et(o, &o->r4Et, t1, t2);
    for (int j = 0; j < n; j++) result[j] += t2[j];
}

/* q.q over the rows in the order of the large-instance kernels' comm-lean PCG: per rank block (one rank: all rows) the two-level tree --
 * workgroup chunks, then the chunk partials -- and the block totals added in rank order (blocks of ceil(l / W) rows, as the q exchange) */
static double rows_sqsum_gpu(lpo_t *o, const double *q) {
    const int l = o->l, T = o->T, W = o->gpu_ranks > 1 ? o->gpu_ranks : 1;
    if (!o->lean_buf) o->lean_buf = (double *)malloc(sizeof(double) * ((size_t)l + (size_t)l / 64 + 1024));
    double *sq = o->lean_buf, *part = o->lean_buf + l;
    for (int i = 0; i < l; i++) sq[i] = q[i] * q[i];
    const int lb = (l + W - 1) / W, CH = W > 1 ? T : o->lean_row_chunk;
    double total = 0.0;
    for (int rk = 0; rk < W; rk++) {
        const int lo = rk * lb < l ? rk * lb : l, hi = lo + lb < l ? lo + lb : l, nloc = hi - lo, Gn = (nloc + CH - 1) / CH;
        for (int g = 0; g < Gn; g++) {
            int len = nloc - g * CH; if (len > CH) len = CH;
            part[g] = redux_sum_gpu_full(sq + lo + (size_t)g * CH, len, T);
        }
        const double pr = redux_sum_gpu_full(part, Gn, T);
        total = rk == 0 ? pr : total + pr;
    }
    return total;
}

/* _conjugate_gradient, the int-returning overload LPcpp:251-335 (verbatim Eigen CG + Jacobi) */
static int conjugate_gradient(lpo_t *o, const double *rhs, double *x, int *iters_io, double *tol_io) {
    const int n = o->n;
    double tol = *tol_io;
    int maxIters = *iters_io;
    double *residual = o->temp_cg + 2 * (size_t)n; /* scratch layout: temp_cg[0..n) Mx, [n..2n) products, then r,p,z,tmp */
    double *p = residual + n, *z = p + n, *tmp = z + n;

    mat_expr_mul(o, x, o->temp_cg);                               /* :267 */
    for (int i = 0; i < n; i++) residual[i] = rhs[i] - o->temp_cg[i]; /* :268 */
    double rhsNorm2 = sqnorm_live(o, rhs);                        /* :271 */
    if (rhsNorm2 == 0) {                                          /* :273-278 */
        for (int i = 0; i < n; i++) x[i] = 0.0;
        *iters_io = 0; *tol_io = 0;
        return 1;
    }
    const double considerAsZero = DBL_MIN;                        /* :280 */
    double threshold = tol * tol * rhsNorm2;                      /* :281 */
    if (threshold < considerAsZero) threshold = considerAsZero;   /* numext::maxi(a,b) = (a<b) ? b : a */
    double residualNorm2 = sqnorm_live(o, residual);              /* :282 */
    if (residualNorm2 < threshold) {                              /* :284-289 */
        *iters_io = 0; *tol_io = sqrt(residualNorm2 / rhsNorm2);
        return 1;
    }
    for (int i = 0; i < n; i++) p[i] = o->invdiag[i] * residual[i]; /* :291 precond.solve */
    double absNew = dot_live(o, residual, p);                     /* :294 */
    int i = 0;
    while (i < maxIters) {                                        /* :296 */
        mat_expr_mul(o, p, tmp);                                  /* :298 */
        double pMp;
        if (o->pcg_lean) {                                        /* opt-in, not the reference's: see lpo_set_pcg_lean */
            const double pp = dot_live(o, p, p), qq = rows_sqsum_gpu(o, o->temp_mm);   /* temp_mm[0..l) = E p, left there by mat_expr_mul */
            const double r4 = o->r4Et.nnz > 0 ? o->r4Et.val[0] / o->Et.val[0] : o->rho4;   /* the scalar the kernels carry (entries of E are 1) */
            pMp = o->Dd[0] * pp + r4 * qq;
        } else pMp = dot_live(o, p, tmp);
        double alpha = absNew / pMp;                              /* :300 */
        if (alpha < 0) { *iters_io = i; return -1; }              /* :301 */
        for (int k = 0; k < n; k++) x[k] += alpha * p[k];         /* :302 */
        for (int k = 0; k < n; k++) residual[k] -= alpha * tmp[k];/* :304 */
        residualNorm2 = sqnorm_live(o, residual);                 /* :305 */
        if (residualNorm2 < threshold) { i++; break; }            /* :309-312 */
        for (int k = 0; k < n; k++) z[k] = o->invdiag[k] * residual[k]; /* :314 */
        double absOld = absNew;
        absNew = dot_live(o, residual, z);                        /* :317 */
        double beta = absNew / absOld;                            /* :318 */
        for (int k = 0; k < n; k++) p[k] = z[k] + beta * p[k];    /* :319 */
        i++;
    }
    *tol_io = sqrt(residualNorm2 / rhsNorm2);                     /* :322 */
    *iters_io = i;
    return 1;
}


/* ------------------------------------------------------------------------------------------ */
/* DIRECT x-update -- NOT the reference's algorithm.  The HIP LP kernel offers it as an opt-in  */
/* (lpbox_set_x_update): instead of running Jacobi-PCG to 1e-3 on         */
/*   (a I + r E^T E) x = rhs,  a = rho1 + rho2, r = rho4     (the system of LPcpp:872-894)      */
/* it solves the system exactly.  The rows of E are split into a set D of rows with pairwise    */
/* disjoint columns (the XOR "dummy item" rows of a combinatorial auction) and the rest G:      */
/*   a I + r E_D^T E_D  is block diagonal with blocks a I + r 1 1^T, inverted in closed form:   */
/*       its inverse is Q / a,  Q v = v - E_D^T W E_D v,  W = diag(1 / (c + m_i)),  c = a / r,  */
/*       m_i = live variables in row i;                                                         */
/*   the Woodbury identity over the G rows then gives                                           */
/*       x = Q (rhs - E_G^T H E_G Q rhs) / a,      H = (c I + E_G Q E_G^T)^-1   (|G| x |G|).     */
/* c is constant while rho1, rho2, rho4 are scaled together (LPcpp:951-970), so H and W are     */
/* built at the first x-update after init or after a fix -- and again at a rho update that      */
/* moves c (only after the double count of a fix with a pending update, see admm_iteration) --, */
/* H by in-place Gauss-Jordan without pivoting (the matrix is SPD).  This restatement follows   */
/* the kernel's operation order so that kernel and oracle agree bit for bit; the reference has  */
/* nothing to compare it with.                                                                  */
/* ------------------------------------------------------------------------------------------ */
static void direct_Q(lpo_t *o, const double *v, double *out) {       /* out = Q v (vectors over the live variables) */
    const int l = o->l, n = o->n;
    double *sig = o->dsig, *cs = o->temp_mm + l;
    spmv_E(o, v, sig);
    for (int i = 0; i < l; i++) sig[i] = o->dir_g[i] < 0 ? o->dw[i] * sig[i] : 0.0;
    spmv_Et(o, &o->Et, sig, cs);
    for (int j = 0; j < n; j++) out[j] = v[j] - cs[j];
}

static void direct_build(lpo_t *o) {
    const int l = o->l, n = o->n;
    if (!o->dir_g) {                 /* no split given: every row is a G row */
        o->dir_g = (int *)malloc(sizeof(int) * (size_t)(l + 1));
        for (int i = 0; i < l; i++) o->dir_g[i] = i;
    }
    int nG = 0;
    for (int i = 0; i < l; i++) if (o->dir_g[i] >= 0) nG++;
    o->nG = nG;
    const int ld = o->H_ld = nG + 2;
    o->H = (double *)realloc(o->H, sizeof(double) * (size_t)ld * (size_t)(nG > 0 ? nG : 1));
    o->dt = (double *)realloc(o->dt, sizeof(double) * (size_t)(l + 1));
    o->du = (double *)realloc(o->du, sizeof(double) * (size_t)(l + 1));
    o->dsig = (double *)realloc(o->dsig, sizeof(double) * (size_t)(l + 1));
    o->dw = (double *)realloc(o->dw, sizeof(double) * (size_t)(l + 1));
    o->dq = (double *)realloc(o->dq, sizeof(double) * (size_t)(2 * n + 2));
    o->dgrow = (int *)realloc(o->dgrow, sizeof(int) * (size_t)(nG + 1));
    for (int i = 0; i < l; i++) if (o->dir_g[i] >= 0) o->dgrow[o->dir_g[i]] = i;
    double *H = o->H, *wv = o->dq, *qw = o->dq + n;
    const double c = o->Dd[0] / o->r4s;                              /* the kernel's dI / r4Et */
    for (int j = 0; j < n; j++) wv[j] = 1.0;
    spmv_E(o, wv, o->dsig);                                          /* m_i: live variables of row i */
    for (int i = 0; i < l; i++) o->dw[i] = 1.0 / (c + o->dsig[i]);
    for (int b = 0; b < nG; b++) {                                   /* column b of c I + E_G Q E_G^T */
        for (int i = 0; i < l; i++) o->dt[i] = 0.0;
        o->dt[o->dgrow[b]] = 1.0;
        spmv_Et(o, &o->Et, o->dt, wv);
        direct_Q(o, wv, qw);
        spmv_E(o, qw, o->du);
        for (int gi = 0; gi < nG; gi++) H[(size_t)gi * ld + b] = gi == b ? o->du[o->dgrow[gi]] + c : o->du[o->dgrow[gi]];
    }
    /* Gauss-Jordan, step k: row k scaled by the reciprocal pivot; every other element G[i][j] -= G[i][k] * G[k][j]; column k last */
    for (int k = 0; k < nG; k++) {
        const double piv = 1.0 / H[(size_t)k * ld + k];
        for (int j = 0; j < nG; j++) if (j != k) H[(size_t)k * ld + j] = H[(size_t)k * ld + j] * piv;
        for (int i = 0; i < nG; i++) {
            if (i == k) continue;
            const double fik = H[(size_t)i * ld + k];
            for (int j = 0; j < nG; j++) if (j != k) H[(size_t)i * ld + j] = H[(size_t)i * ld + j] - fik * H[(size_t)k * ld + j];
        }
        for (int i = 0; i < nG; i++) if (i != k) H[(size_t)i * ld + k] = -(H[(size_t)i * ld + k] * piv);
        H[(size_t)k * ld + k] = piv;
    }
    o->H_valid = 1;
}

static void direct_solve(lpo_t *o, const double *rhs, double *x) {
    const int l = o->l, n = o->n, ld = o->H_ld, nG = o->nG;
    double *q1 = o->dq, *y = o->dq + n, *v = o->temp_mm + l;
    direct_Q(o, rhs, q1);
    spmv_E(o, q1, o->dt);                                            /* t = E_G Q rhs (the D rows of the product are not used) */
    /* u = H t: the four lanes of a quad share a row, lane q adds the columns j = q, q + 4, ... (ascending); (p0 + p1) + (p2 + p3) */
    for (int i = 0; i < l; i++) o->du[i] = 0.0;
    for (int gi = 0; gi < nG; gi++) {
        double part[4] = {0.0, 0.0, 0.0, 0.0};
        for (int j = 0; j < nG; j++) part[j & 3] = part[j & 3] + o->H[(size_t)gi * ld + j] * o->dt[o->dgrow[j]];
        o->du[o->dgrow[gi]] = (part[0] + part[1]) + (part[2] + part[3]);
    }
    spmv_Et(o, &o->Et, o->du, v);
    for (int j = 0; j < n; j++) y[j] = rhs[j] - v[j];
    direct_Q(o, y, q1);
    for (int j = 0; j < n; j++) x[j] = q1[j] / o->Dd[0];
}

/* std_dev LPcpp:358-377 */
static double std_dev(lpo_t *o, const double *arr, size_t begin, size_t end) {
    double mean = 0, std_deviation = 0;
    size_t size = end - begin;
    for (size_t i = begin; i < end; i++) mean += arr[i];
    mean /= size;
    for (size_t i = 0; i < size; i++) std_deviation += (arr[begin + i] - mean) * (arr[begin + i] - mean);
    std_deviation /= size - 1;
    if (std_deviation == 0) return 0;
    return pow_half(o, std_deviation);
}

/* compute_std_obj LPcpp:459-469 */
static double compute_std_obj(lpo_t *o, int history_size) {
    size_t s = (size_t)o->obj_n;
    double std_obj;
    if (s <= (size_t)history_size) std_obj = std_dev(o, o->obj_list, 0, s);
    else std_obj = std_dev(o, o->obj_list, s - (size_t)history_size, s);
    return std_obj / fabs(o->obj_list[s - 1]);
}

static void obj_push(lpo_t *o, double v) {
    if (o->obj_n == o->obj_cap) {
        o->obj_cap = o->obj_cap ? 2 * o->obj_cap : 1024;
        o->obj_list = (double *)realloc(o->obj_list, sizeof(double) * (size_t)o->obj_cap);
    }
    o->obj_list[o->obj_n++] = v;
}

static void trace_push(lpo_t *o, int v) {
    if (o->trace_n == o->trace_cap) {
        o->trace_cap = o->trace_cap ? 2 * o->trace_cap : 1024;
        o->pcg_trace = (int *)realloc(o->pcg_trace, sizeof(int) * (size_t)o->trace_cap);
    }
    o->pcg_trace[o->trace_n++] = v;
}

/* ------------------------------------------------------------------------------------------ */
/* ADMM_lp_iters_init  LPcpp:489-763                                                           */
/* ------------------------------------------------------------------------------------------ */
int lpo_init(lpo_t *o) {
    if (!o->has_problem) return -1;
    o->stop_threshold = 1e-4;                 /* :491 */
    o->std_threshold = 1e-6;
    o->gamma_val = 1.6;                       /* :493 */
    o->gamma_factor = 0.95;
    o->rho_change_step = 25;
    o->max_iters = (int)2e4;
    o->initial_rho = 25;
    o->history_size = 3;
    o->learning_fact = 1 + 1.0 / 100;         /* :499 */
    o->pcg_tol = 1e-3;
    o->pcg_maxiters = (int)1e3;
    o->rel_tol = 5e-5;
    o->projection_lp = 2;
    o->std_threshold = 1e-12;                 /* :506 */
    o->history_size = 10;                     /* :507 */

    const int n = o->E.cols, l = o->E.rows;   /* :537-539 */
    o->n = n; o->l = l;
    if (n == l) return -6;                    /* quirk Q6 (LPcpp:103-107,150): the reference's aliased product breaks; no golden depends on it */
    free_state(o);
    size_t nn = (size_t)n, ll = (size_t)l;
    o->x = (double *)calloc(nn, sizeof(double));
    o->y1 = (double *)calloc(nn, sizeof(double));
    o->y2 = (double *)calloc(nn, sizeof(double));
    o->z1 = (double *)calloc(nn, sizeof(double));
    o->z2 = (double *)calloc(nn, sizeof(double));
    o->best_sol = (double *)calloc(nn, sizeof(double));
    o->temp_vec = (double *)calloc(nn, sizeof(double));
    o->temp_cg = (double *)calloc(6 * nn, sizeof(double));
    o->temp_mm = (double *)calloc(nn + ll, sizeof(double));
    o->fy = (double *)calloc(ll, sizeof(double));
    o->x_try = (double *)calloc(nn, sizeof(double));
    o->Dd = (double *)calloc(nn, sizeof(double));
    o->pd = (double *)calloc(nn, sizeof(double));
    o->Esq = (double *)calloc(nn, sizeof(double));
    o->invdiag = (double *)calloc(nn, sizeof(double));
    o->invdiag_len = 0;
    o->left_idx = (int *)malloc(sizeof(int) * nn);
    o->full = (double *)calloc(nn + 8192, sizeof(double));
    o->full_v = (double *)calloc(nn, sizeof(double));
    o->ret_idx_prev = NULL; o->ret_val_prev = NULL; o->ret_prev_len = 0;
    o->ret_idx = (int *)malloc(sizeof(int) * nn);
    o->ret_val = (double *)malloc(sizeof(double) * nn);
    o->ret_len = n;
    for (int i = 0; i < n; i++) {             /* :583-586, :591-592 */
        o->left_idx[i] = i;
        o->x[i] = 1;
        o->ret_idx[i] = -1; o->ret_val[i] = -1;
    }
    o->x_len = n;
    o->org_n = n;                             /* :588 */
    o->fix_sum = 0;
    o->fix_obj = 0; o->sum_fix_obj = 0;       /* :593-594 */
    /* z1 = z2 = 0 (:616-617) via calloc */
    o->rho1 = o->rho2 = o->rho3 = o->rho4 = o->initial_rho;       /* :623-630 */
    o->prev_rho1 = o->rho1; o->prev_rho2 = o->rho2; o->prev_rho3 = o->rho3; o->prev_rho4 = o->rho4;
    o->y3 = (double *)calloc(ll, sizeof(double));
    o->z4 = (double *)calloc(ll, sizeof(double));                 /* :646-650 */
    for (int i = 0; i < n; i++) { o->y1[i] = o->x[i]; o->y2[i] = o->x[i]; } /* :713-714 */
    spmv_E(o, o->x, o->temp_mm);                                  /* :720 y3 = f - E*x */
    for (int i = 0; i < l; i++) o->y3[i] = o->f[i] - o->temp_mm[i];
    for (int i = 0; i < n; i++) o->best_sol[i] = o->x[i];         /* :725 */
    o->best_bin_obj = dot_live(o, o->b, o->x);                    /* :727 compute_cost_lp(x_sol, b) = b.dot(x) */
    /* members that keep their in-class initialisers (LPh:213-219,279): only valid for a fresh object */
    o->H_valid = 0;
    o->inited = 1;
    return 1;
}

/* ------------------------------------------------------------------------------------------ */
/* one ADMM iteration, shared by ADMM_lp_iters (LPcpp:796-1068) and _l2f (:1341-1564)          */
/* returns 0 = continue, 1 = break, 2 = return 1 immediately (PCG alpha<0 in l2f, :1450-1454) */
/* ------------------------------------------------------------------------------------------ */
static int admm_iteration(lpo_t *o, int iter, int iter_start, int l2f, int *ret, int *cc) {
    const int n = o->n, l = o->l;
    double *tv = o->temp_vec;

    /* y1  :806-809 / :1350-1353, project_box :409-421 */
    for (int i = 0; i < n; i++) tv[i] = o->x[i] + o->z1[i] / o->rho1;
    for (int i = 0; i < n; i++) o->y1[i] = tv[i] > 1 ? 1 : (tv[i] < 0 ? 0 : tv[i]);

    /* y2  :815-818 / :1359-1362, project_shifted_Lp_ball :423-428 (p = 2) */
    for (int i = 0; i < n; i++) tv[i] = o->x[i] + o->z2[i] / o->rho2;
    for (int i = 0; i < n; i++) o->y2[i] = tv[i] - 0.5;
    {
        double normp_shift = sqrt(sqnorm_live(o, o->y2));
        double c1 = pow((double)n, 1.0 / (int)o->projection_lp);
        double c2 = 2 * normp_shift;
        for (int i = 0; i < n; i++) o->y2[i] = o->y2[i] * c1 / c2 + 0.5;
    }

    /* y3  :824-828 / :1369-1373, project_vec_less_than(y3,y3,0,0) :386-391 */
    spmv_E(o, o->x, o->temp_mm);
    for (int i = 0; i < l; i++) {
        double v = o->f[i] - o->temp_mm[i] - o->z4[i] / o->rho4;
        o->y3[i] = v < 0 ? 0 : v;
    }

    if (iter == 0) update_expression(o);                      /* :831-842 / :1390-1391 */

    if (iter != 0 && o->rhoUpdated) {                         /* :851-866 / :1393-1406 */
        const double c_before = (o->x_update == 1 && n > 0) ? o->Dd[0] / o->r4s : 0.0;
        double inc = o->rho_change_ratio * (o->prev_rho1 + o->prev_rho2);
        for (int j = 0; j < n; j++) o->Dd[j] += inc;
        for (int j = 0; j < n; j++) o->pd[j] += inc;
        double inc4 = o->rho_change_ratio * o->prev_rho4;
        for (int j = 0; j < n; j++) o->pd[j] += inc4 * o->Esq[j];
        for (int k = 0; k < o->r4Et.nnz; k++) o->r4Et.val[k] = o->learning_fact * o->r4Et.val[k];
        o->r4s = o->learning_fact * o->r4s;
        if (o->x_update == 1 && n > 0) {
            /* direct mode: H and W hold for c = dI / r4Et.  The schedule scales both by learning_fact, so c moves by rounding only --
             * except after a fix made while a rho update was pending (the double count): from then on dI carries an offset
             * that is not scaled, c changes with every update (1e-4 relative at the first), and the saved inverse would solve another
             * system.  Rebuilt when c moved by more than 1e-9 relative; the same rule and the same scalars as the kernel.  (The plain
             * schedule moves c by at most 2.3e-16 relative per update over the 800 updates of a 20 000-iteration run:
             * tests/test_direct_x_update.py::test_plain_schedule_keeps_c_far_below_the_rebuild_threshold.) */
            const double c_after = o->Dd[0] / o->r4s;
            if (fabs(c_after - c_before) > 1e-9 * c_before) o->H_valid = 0;
        }
    }

    /* rhs  :872-878 / :1413-1422 */
    for (int i = 0; i < n; i++)
        tv[i] = (o->rho1 * o->y1[i] + o->rho2 * o->y2[i]) - ((o->b[i] + o->z1[i]) + o->z2[i]);
    {
        double *fy = o->fy;                   /* (*f_ptr - y3) is evaluated into a temporary vector first */
        double *t = o->temp_mm + l;
        for (int i = 0; i < l; i++) fy[i] = o->f[i] - o->y3[i];
        spmv_Et(o, &o->r4Et, fy, t);
        for (int i = 0; i < n; i++) tv[i] += t[i];
        spmv_Et(o, &o->Et, o->z4, t);
        for (int i = 0; i < n; i++) tv[i] -= t[i];
    }

    if (o->rhoUpdated) {                                       /* :883-890 / :1428-1436 DiagonalPreconditioner.compute */
        for (int j = 0; j < n; j++) o->invdiag[j] = (o->pd[j] != 0.0) ? 1.0 / o->pd[j] : 1.0;
        o->invdiag_len = n;
        o->rhoUpdated = 0;
    }
    if (o->invdiag_len != n) {
        /* The reference would now use a stale DiagonalPreconditioner of the wrong length (Eigen assertion /
         * undefined behaviour): a fix applied while no rho update is pending.  Defined here as: recompute. */
        for (int j = 0; j < n; j++) o->invdiag[j] = (o->pd[j] != 0.0) ? 1.0 / o->pd[j] : 1.0;
        o->invdiag_len = n;
    }

    double tol = o->pcg_tol;
    int maxiter = o->pcg_maxiters;
    int cg = 1;
    if (o->x_update == 1) {                                    /* opt-in direct x-update (no reference counterpart), see direct_build */
        if (!o->H_valid) direct_build(o);
        direct_solve(o, tv, o->x);
        maxiter = 0;
        if (l2f) {
            for (int i = 0; i < n; i++) o->x_iters[(size_t)(*cc) * (size_t)o->xi_rows + (size_t)i] = o->x[i];
            (*cc)++;
        }
    } else if (!l2f) {
        for (int i = 0; i < n; i++) o->x[i] = o->y1[i];         /* :892 x_sol = y1 */
        cg = conjugate_gradient(o, tv, o->x, &maxiter, &tol);   /* :894 (return value ignored) */
        if (cg == -1) o->last_stop = 3;
    } else {
        double *x_try = o->x_try;
        for (int i = 0; i < n; i++) x_try[i] = o->y1[i];        /* :1439 x_sol_try = y1 */
        cg = conjugate_gradient(o, tv, x_try, &maxiter, &tol);  /* :1447 */
        if (cg == -1) {                                         /* :1450-1454 */
            o->last_pcg_iters = maxiter; o->total_pcg += maxiter;
            o->last_stop = 3;
            return 2;
        }
        for (int i = 0; i < n; i++) o->x[i] = x_try[i];         /* :1468 */
        for (int i = 0; i < n; i++) o->x_iters[(size_t)(*cc) * (size_t)o->xi_rows + (size_t)i] = o->x[i]; /* :1472-1475 */
        (*cc)++;
    }
    o->last_pcg_iters = maxiter; o->total_pcg += maxiter; o->total_outer++;
    trace_push(o, maxiter);

    /* duals :917-924 / :1487-1491 */
    {
        double g1 = o->gamma_val * o->rho1, g2 = o->gamma_val * o->rho2, g4 = o->gamma_val * o->rho4;
        for (int i = 0; i < n; i++) o->z1[i] = o->z1[i] + g1 * (o->x[i] - o->y1[i]);
        for (int i = 0; i < n; i++) o->z2[i] = o->z2[i] + g2 * (o->x[i] - o->y2[i]);
        spmv_E(o, o->x, o->temp_mm);
        if (!l2f && iter == iter_start)
            for (int i = 0; i < l; i++) o->z4[i] = g4 * ((o->temp_mm[i] + o->y3[i]) - o->f[i]);           /* :920-921 */
        else
            for (int i = 0; i < l; i++) o->z4[i] = o->z4[i] + g4 * ((o->temp_mm[i] + o->y3[i]) - o->f[i]); /* :923 / :1490 */
    }

    /* convergence  :931-949 / :1501-1511 */
    {
        double xn = sqrt(sqnorm_live(o, o->x));
        double temp0 = (xn < 2.2204e-16) ? 2.2204e-16 : xn;  /* std::max(a,b) = (a<b)?b:a */
        for (int i = 0; i < n; i++) tv[i] = o->x[i] - o->y1[i];
        o->cvg1 = sqrt(sqnorm_live(o, tv)) / temp0;
        for (int i = 0; i < n; i++) tv[i] = o->x[i] - o->y2[i];
        o->cvg2 = sqrt(sqnorm_live(o, tv)) / temp0;
        if (o->cvg1 <= o->stop_threshold && o->cvg2 <= o->stop_threshold && (l2f || iter != iter_start)) {
            if (l2f) *ret = 1;                                   /* :1505 (the plain loop leaves ret = 0) */
            if (o->verbose)
                printf(l2f ? "Stop becuase y1_y2. iter: %d, stop_threshold: %.6f\n"
                           : "Stop because y1_y2. iter: %d, stop_threshold: %.6f\n",
                       iter, o->cvg1 > o->cvg2 ? o->cvg1 : o->cvg2);
            o->last_stop = 1;
            return 1;
        }
    }

    /* rho schedule :951-970 / :1515-1533 */
    if ((iter + 1) % o->rho_change_step == 0) {
        o->prev_rho1 = o->rho1; o->prev_rho2 = o->rho2;
        o->rho1 = o->learning_fact * o->rho1;
        o->rho2 = o->learning_fact * o->rho2;
        o->prev_rho4 = o->rho4;                                  /* instruction.update_rho4 = 1 (:527) */
        o->rho4 = o->learning_fact * o->rho4;
        {
            double g = o->gamma_val * o->gamma_factor;
            o->gamma_val = g < 1.0 ? 1.0 : g;                    /* std::max(g, 1.0) */
        }
        o->rhoUpdated = 1;
        o->rho_change_ratio = o->learning_fact - 1.0;
    }

    /* objective history :972-995 / :1535-1547 */
    o->obj_val = dot_live(o, o->b, o->x);
    obj_push(o, o->obj_val);
    if ((double)o->obj_n >= o->history_size) o->std_obj = compute_std_obj(o, (int)o->history_size);
    if (o->std_obj <= o->std_threshold) {
        *ret = 1;
        if (o->verbose)
            printf(l2f ? "Stop because std_obj. iter: %d, std_threshold: %.6f\n"
                       : "Stop because obj_std. iter: %d, std_threshold: %.6f\n", iter, o->std_obj);
        o->last_stop = 2;
        return 1;
    }

    /* binarise + best tracking :1001-1011 / :1555-1562 */
    for (int i = 0; i < n; i++) tv[i] = o->x[i] >= 0.5 ? 1.0 : 0.0;
    o->cur_obj = dot_live(o, o->b, tv);
    if (o->best_bin_obj >= o->cur_obj) {
        o->best_bin_obj = o->cur_obj;
        for (int i = 0; i < n; i++) o->best_sol[i] = o->x[i];
    }
    return 0;
}

/* the reference's per-iteration log block (LPcpp:1013-1067; `does_log`, LPh:148, is ON by default and not switchable from the pyx):
 * six vector norms that nothing else needs + ten fprintf.  It does not feed back into the iteration; the oracle writes it only on
 * request (lpo_set_log) so that the cost of what ./test really does can be timed beside the bare solve. */
static double norm_eigen(const double *a, int n, double *scratch) {
    for (int i = 0; i < n; i++) scratch[i] = a[i] * a[i];
    return sqrt(redux_sum_eigen(scratch, n));
}
static void log_iteration(lpo_t *o, int iter, double secs) {
    double *t = o->temp_mm;
    FILE *fp = o->log_fp;
    fprintf(fp, "norm of x_sol: %.9lf\n", norm_eigen(o->x, o->n, t));
    fprintf(fp, "norm of y1: %.9lf\n", norm_eigen(o->y1, o->n, t));
    fprintf(fp, "norm of y2: %.9lf\n", norm_eigen(o->y2, o->n, t));
    fprintf(fp, "norm of y3: %.9lf\n", norm_eigen(o->y3, o->l, t));
    fprintf(fp, "norm of z1: %.9lf\n", norm_eigen(o->z1, o->n, t));
    fprintf(fp, "norm of z2: %.9lf\n", norm_eigen(o->z2, o->n, t));
    fprintf(fp, "For z4\nnorm of z4: %.9lf\n", norm_eigen(o->z4, o->l, t));
    fprintf(fp, "LongkangIter: %d;  x_sol: %lf; dou_obj:%lf; bin_obj: %lf\n", iter + 1, norm_eigen(o->x, o->n, t), o->obj_val, o->cur_obj);
    fprintf(fp, "Time elapsed: %lfs\n", secs);
    fprintf(fp, "-------------------------------------------------\n");
}
int lpo_set_log(lpo_t *o, const char *path) {
    if (o->log_fp) { fclose(o->log_fp); o->log_fp = NULL; }
    if (path && *path) { o->log_fp = fopen(path, "a+"); if (!o->log_fp) return -1; }     /* "a+" as LPcpp:772 */
    return 0;
}

/* ADMM_lp_iters LPcpp:766-1095 */
int lpo_iters(lpo_t *o, int iter_start, int iter_end) {
    if (!o->inited) return -1;
    int ret = 0, iter, cc = 0;
    o->trace_n = 0; o->last_stop = 0;
    struct timespec t0, t1;
    if (o->log_fp) clock_gettime(CLOCK_MONOTONIC, &t0);
    for (iter = iter_start; iter < iter_end; iter++) {
        if (o->log_fp) fprintf(o->log_fp, "Iteration: %d\n", iter);                       /* :789 */
        int rc = admm_iteration(o, iter, iter_start, 0, &ret, &cc);
        if (rc) break;
        if (o->log_fp) {
            fprintf(o->log_fp, "Conjugate gradient stops after %d iterations\n", o->last_pcg_iters);   /* :898-901 */
            clock_gettime(CLOCK_MONOTONIC, &t1);
            log_iteration(o, iter, (double)((long)((t1.tv_sec - t0.tv_sec) * 1000 + (t1.tv_nsec - t0.tv_nsec) / 1000000)) / 1000.0);
        }
    }
    o->last_plain_iter_plus1 = iter + 1;   /* :1081 */
    return ret;
}

/* ADMM_lp_iters_l2f LPcpp:1098-1574 */
int lpo_iters_l2f(lpo_t *o, int iter_start, int iter_end, const double *vec, int fix_num) {
    if (!o->inited) return -1;
    int ret = 0, cc = 0;
    o->trace_n = 0; o->last_stop = 0;
    int n = o->n;
    if (fix_num < 0 || fix_num > n) return -2;
    if (iter_end - iter_start > 500) return -3;           /* x_iters has 500 columns (:1113) */
    if (fix_num != 0) {
        int cnt = 0;
        for (int i = 0; i < n; i++) if (vec[i] == 1 || vec[i] == 0) cnt++;
        if (cnt != fix_num) return -4;                     /* the reference would index out of bounds (:1135-1149) */
    }

    free(o->x_iters);                                       /* :1113 */
    o->xi_rows = n - fix_num; o->xi_cols = 500;
    o->x_iters = (double *)calloc((size_t)(o->xi_rows > 0 ? o->xi_rows : 1) * 500, sizeof(double));

    if (fix_num != 0) {                                     /* :1124-1335 */
        o->fix_sum += fix_num;
        int nk = n - fix_num;
        int *fix_idx = (int *)malloc(sizeof(int) * (size_t)(fix_num));
        int *non_fix_idx = (int *)malloc(sizeof(int) * (size_t)(nk > 0 ? nk : 1));
        double *org_fix_val = (double *)malloc(sizeof(double) * (size_t)fix_num);
        trip_t *efix = (trip_t *)malloc(sizeof(trip_t) * (size_t)(o->E.nnz > 0 ? o->E.nnz : 1));
        trip_t *enonfix = (trip_t *)malloc(sizeof(trip_t) * (size_t)(o->E.nnz > 0 ? o->E.nnz : 1));
        int nef = 0, nen = 0, j = 0, k = 0;
        for (int i = 0; i < n; i++) {                       /* :1135-1165 */
            int fixed;
            if (vec[i] == 1) { fix_idx[j] = i; org_fix_val[j] = 1; j++; fixed = 1; }
            else if (vec[i] == 0) { fix_idx[j] = i; org_fix_val[j] = 0; j++; fixed = 1; }
            else { non_fix_idx[k] = i; k++; fixed = 0; }
            for (int q = o->E.ptr[i]; q < o->E.ptr[i + 1]; q++) {
                if (!fixed) { enonfix[nen].r = o->E.idx[q]; enonfix[nen].c = k - 1; enonfix[nen].v = o->E.val[q]; nen++; }
                else { efix[nef].r = o->E.idx[q]; efix[nef].c = j - 1; efix[nef].v = o->E.val[q]; nef++; }
            }
        }
        csc_t E1, E2; memset(&E1, 0, sizeof(E1)); memset(&E2, 0, sizeof(E2));
        csc_from_triplets(&E1, o->E.rows, k, enonfix, nen); /* :1170-1173 */
        csc_from_triplets(&E2, o->E.rows, j, efix, nef);    /* :1179-1181 */
        free(efix); free(enonfix);

        int *org_fix_idx = (int *)malloc(sizeof(int) * (size_t)fix_num);      /* :1192-1194 */
        int *new_left = (int *)malloc(sizeof(int) * (size_t)(nk > 0 ? nk : 1));
        for (int q = 0; q < fix_num; q++) org_fix_idx[q] = o->left_idx[fix_idx[q]];
        for (int q = 0; q < nk; q++) new_left[q] = o->left_idx[non_fix_idx[q]];

        int new_len = o->ret_prev_len + fix_num;            /* :1201-1206 */
        int *ri = (int *)malloc(sizeof(int) * (size_t)new_len);
        double *rv = (double *)malloc(sizeof(double) * (size_t)new_len);
        for (int q = 0; q < o->ret_prev_len; q++) { ri[q] = o->ret_idx_prev[q]; rv[q] = o->ret_val_prev[q]; }
        for (int q = 0; q < fix_num; q++) { ri[o->ret_prev_len + q] = org_fix_idx[q]; rv[o->ret_prev_len + q] = org_fix_val[q]; }
        free(o->ret_idx_prev); free(o->ret_val_prev);
        o->ret_idx_prev = ri; o->ret_val_prev = rv; o->ret_prev_len = new_len;
        free(o->ret_idx); free(o->ret_val);
        o->ret_idx = (int *)malloc(sizeof(int) * (size_t)o->org_n);
        o->ret_val = (double *)malloc(sizeof(double) * (size_t)o->org_n);
        memcpy(o->ret_idx, ri, sizeof(int) * (size_t)new_len);
        memcpy(o->ret_val, rv, sizeof(double) * (size_t)new_len);
        o->ret_len = new_len;

        if (nk == 0) {                                      /* :1212-1217 */
            ret = 1;
            o->n = 0;
            iter_end = iter_start;
            o->last_stop = 4;
            /* left_idx = org_non_fix_idx (empty) (:1194) */
            free(new_left);
        } else {
            /* reductions over the compacted vectors use the new live map */
            double *b2 = (double *)malloc(sizeof(double) * (size_t)fix_num);
            for (int q = 0; q < fix_num; q++) b2[q] = o->b[fix_idx[q]];
            /* fix_obj = compute_cost_lp(x2, b2) = b2.dot(x2) (:1237), reduced over the just-fixed set */
            {
                double *prod = (double *)malloc(sizeof(double) * (size_t)fix_num);
                for (int q = 0; q < fix_num; q++) prod[q] = b2[q] * org_fix_val[q];
                o->fix_obj = reduce(o, prod, fix_num, org_fix_idx);
                free(prod);
            }
            /* x_sol = x_sol(non_fix_idx) etc. (:1222-1231) */
            for (int q = 0; q < nk; q++) {
                int s = non_fix_idx[q];
                o->x[q] = o->x[s]; o->y1[q] = o->y1[s]; o->y2[q] = o->y2[s];
                o->z1[q] = o->z1[s]; o->z2[q] = o->z2[s];
                o->temp_vec[q] = o->b[s];
            }
            for (int q = 0; q < nk; q++) o->b[q] = o->temp_vec[q];   /* b1 */
            o->x_len = nk;
            memcpy(o->left_idx, new_left, sizeof(int) * (size_t)nk);
            free(new_left);
            o->n = nk;                                       /* (:1295; moved up so the norm below runs on the live set) */
            o->H_valid = 0;                                  /* direct mode: E changed */
            if (sqrt(sqnorm_live(o, o->x)) < 1e-3) ret = 1;  /* :1223 */
            o->prev_sum = o->sum_fix_obj;                    /* :1247-1250 */
            o->sum_fix_obj += o->fix_obj;
            o->prev_obj = o->cur_obj;
            {                                                /* :1276-1278 f1 = f - E2*x2 */
                double *t = (double *)malloc(sizeof(double) * (size_t)o->l);
                if (o->order_mode == LPO_ORDER_GPU) {
                    for (int jj = 0; jj < o->org_n; jj++) o->full_v[jj] = 0.0;
                    for (int q = 0; q < fix_num; q++) o->full_v[org_fix_idx[q]] = org_fix_val[q];
                    spmv_orgE_split(o, o->full_v, t);
                } else
                    spmv(&E2, org_fix_val, t);
                for (int i = 0; i < o->l; i++) o->f[i] = o->f[i] - t[i];
                free(t);
            }
            csc_copy(&o->E, &E1);                            /* :1297-1298 */
            update_expression(o);                            /* :1329 */
            free(b2);
        }
        if (o->print_info == 1 || o->verbose)
            printf("Iter: %d; Fixed %d Elements; Totally Fixed %d Elements; Left %d Elements; Sum_fix_obj: %f\n",
                   iter_start, fix_num, o->fix_sum, nk, o->sum_fix_obj);   /* :1333-1334 */
        csc_free(&E1); csc_free(&E2);
        free(fix_idx); free(non_fix_idx); free(org_fix_val); free(org_fix_idx);
    }

    for (o->iter = iter_start; o->iter < iter_end; o->iter++) {  /* :1341 */
        int rc = admm_iteration(o, o->iter, iter_start, 1, &ret, &cc);
        if (rc == 2) return 1;
        if (rc) break;
    }
    return ret;
}

/* ------------------------------------------------------------------------------------------ */
/* getters                                                                                     */
/* ------------------------------------------------------------------------------------------ */
int lpo_get_n(const lpo_t *o) { return o->n; }
int lpo_get_org_n(const lpo_t *o) { return o->org_n; }
int lpo_get_l(const lpo_t *o) { return o->l; }
int lpo_get_iter(const lpo_t *o) { return o->iter; }
int lpo_get_x_iters_rows(const lpo_t *o) { return o->x_iters ? o->xi_rows : 0; }

int lpo_get_x_iters(const lpo_t *o, int ws, double *out) {   /* :1616-1627 */
    if (!o->x_iters || ws < 0 || ws > o->xi_cols) return -1;
    int rows = o->xi_rows;
    for (int i = 0; i < rows; i++)
        for (int j = 0; j < ws; j++) out[(size_t)i * (size_t)ws + (size_t)j] = o->x_iters[(size_t)j * (size_t)rows + (size_t)i];
    return rows;
}

int lpo_get_x_sol(lpo_t *o, double *out) {                    /* :1648-1665 */
    if (o->n != 0) {
        int len = o->ret_prev_len + o->n;
        for (int q = 0; q < o->ret_prev_len; q++) { o->ret_idx[q] = o->ret_idx_prev[q]; o->ret_val[q] = o->ret_val_prev[q]; }
        for (int q = 0; q < o->n; q++) {
            o->ret_idx[o->ret_prev_len + q] = o->left_idx[q];
            o->ret_val[o->ret_prev_len + q] = o->x[q] >= 0.5 ? 1.0 : 0.0;
        }
        o->ret_len = len;
    }
    for (int i = 0; i < o->ret_len; i++) {
        int index = o->ret_idx[i];
        if (index >= 0 && index < o->org_n) out[index] = o->ret_val[i];
    }
    return o->ret_len;
}

int lpo_get_final_x_sol(const lpo_t *o, double *out) {        /* :1668-1685 */
    for (int i = 0; i < o->x_len; i++) out[i] = o->x[i];
    return o->x_len;
}

double lpo_cal_obj(const lpo_t *o) {                          /* :1630-1642 */
    if (o->n != 0) return o->sum_fix_obj + o->cur_obj;
    return o->sum_fix_obj;
}

double lpo_cur_bin_obj(const lpo_t *o) { return o->cur_obj; } /* :1644-1646 */

int lpo_check_infeasible_lpbox(lpo_t *o) {                    /* :1577-1591 */
    if (o->n == 0) return 0;
    int inf = 0;
    spmv(&o->E, o->x, o->temp_mm);
    for (int i = 0; i < o->E.rows; i++) if (!(o->temp_mm[i] <= 1.0)) inf++;
    return inf;
}

int lpo_check_infeasible_l2f(lpo_t *o) {                      /* :1593-1612 */
    double *sol = (double *)calloc((size_t)o->org_n, sizeof(double));
    double *t = (double *)calloc((size_t)o->orgE.rows, sizeof(double));
    lpo_get_x_sol(o, sol);
    spmv(&o->orgE, sol, t);
    int inf = 0;
    for (int i = 0; i < o->orgE.rows; i++) if (!(t[i] <= 1.0)) inf++;
    free(sol); free(t);
    return inf;
}

int  lpo_last_plain_iter_plus1(const lpo_t *o) { return o->last_plain_iter_plus1; }
long lpo_total_pcg_iters(const lpo_t *o) { return o->total_pcg; }
long lpo_total_outer_iters(const lpo_t *o) { return o->total_outer; }
int  lpo_last_pcg_iters(const lpo_t *o) { return o->last_pcg_iters; }
int  lpo_last_stop_reason(const lpo_t *o) { return o->last_stop; }

int lpo_get_vec(const lpo_t *o, const char *name, double *out, int cap) {
    const double *src = NULL; int len = 0;
    if (!strcmp(name, "x")) { src = o->x; len = o->x_len; }
    else if (!strcmp(name, "y1")) { src = o->y1; len = o->n; }
    else if (!strcmp(name, "y2")) { src = o->y2; len = o->n; }
    else if (!strcmp(name, "y3")) { src = o->y3; len = o->l; }
    else if (!strcmp(name, "z1")) { src = o->z1; len = o->n; }
    else if (!strcmp(name, "z2")) { src = o->z2; len = o->n; }
    else if (!strcmp(name, "z4")) { src = o->z4; len = o->l; }
    else if (!strcmp(name, "b")) { src = o->b; len = o->n; }
    else if (!strcmp(name, "f")) { src = o->f; len = o->l; }
    else if (!strcmp(name, "pd")) { src = o->pd; len = o->n; }
    else if (!strcmp(name, "left_idx")) {
        len = o->n;
        if (len > cap) return -len;
        for (int i = 0; i < len; i++) out[i] = (double)o->left_idx[i];
        return len;
    } else return -1;
    if (len > cap) return -len;
    for (int i = 0; i < len; i++) out[i] = src[i];
    return len;
}

double lpo_get_scalar(const lpo_t *o, const char *name) {
    if (!strcmp(name, "rho1")) return o->rho1;
    if (!strcmp(name, "rho2")) return o->rho2;
    if (!strcmp(name, "rho4")) return o->rho4;
    if (!strcmp(name, "prev_rho1")) return o->prev_rho1;
    if (!strcmp(name, "prev_rho4")) return o->prev_rho4;
    if (!strcmp(name, "gamma")) return o->gamma_val;
    if (!strcmp(name, "dI")) return o->n > 0 ? o->Dd[0] : 0.0;
    if (!strcmp(name, "rho4Et")) return o->r4Et.nnz > 0 ? o->r4Et.val[0] / (o->Et.val[0]) : 0.0;
    if (!strcmp(name, "std_obj")) return o->std_obj;
    if (!strcmp(name, "cur_obj")) return o->cur_obj;
    if (!strcmp(name, "sum_fix_obj")) return o->sum_fix_obj;
    if (!strcmp(name, "best_bin_obj")) return o->best_bin_obj;
    if (!strcmp(name, "cvg1")) return o->cvg1;
    if (!strcmp(name, "cvg2")) return o->cvg2;
    if (!strcmp(name, "obj_val")) return o->obj_val;
    if (!strcmp(name, "rhoUpdated")) return (double)o->rhoUpdated;
    if (!strcmp(name, "pow_sqrt_mismatch")) return (double)o->pow_sqrt_mismatch;
    return NAN;
}

int lpo_get_pcg_trace(const lpo_t *o, int *out, int cap) {
    int c = o->trace_n < cap ? o->trace_n : cap;
    for (int i = 0; i < c; i++) out[i] = o->pcg_trace[i];
    return c;
}

/* ---- stand-alone kernels of the iteration, for known-answer tests ---- */
/* project_box LPcpp:409-421 */
void lpo_project_box(int n, const double *x, double *y) {
    for (int i = 0; i < n; i++) y[i] = x[i] > 1 ? 1 : (x[i] < 0 ? 0 : x[i]);
}
/* project_shifted_Lp_ball LPcpp:423-428 with p = 2 (Eigen reduction order) */
void lpo_project_shifted_lp_ball(int n, const double *x, double *y) {
    double *t = (double *)malloc(sizeof(double) * (size_t)(n > 0 ? n : 1));
    for (int i = 0; i < n; i++) { y[i] = x[i] - 0.5; t[i] = y[i] * y[i]; }
    double normp_shift = sqrt(redux_sum_eigen(t, n));
    double c1 = pow((double)n, 1.0 / 2), c2 = 2 * normp_shift;
    for (int i = 0; i < n; i++) y[i] = y[i] * c1 / c2 + 0.5;
    free(t);
}
