// lpbox_genb_kernels.hip -- gfx950 kernels of the BATCH of small generic constrained binary QPs (ADMM_bqp, SEGcpp:1384-1832; see
// lpbox_genb.h).  One persistent workgroup of 256 threads per problem runs the whole loop that lpbox_gen_kernels.hip cuts into
//   prep -> y -> rhs_cols -> rows(y1) -> resid -> K x { rows(p) -> pcg_cols -> pcg_upd } -> post -> rows(x) -> dual
// with the grid-wide dependencies replaced by workgroup barriers.  The expressions are those of that file (the shared ones live in
// lpbox_gen_dev.h), and every sum keeps its association:
//   * element j belongs to thread j % 256, slot j / 256; a chunk of 512 elements is two slots, summed (0.0 + even) + odd per thread,
//     then through the 64-lane tree and (w0+w1)+(w2+w3) of block_sum<256>; the <= 4 chunk totals combine as (c0+c1)+(c2+c3).  A chunk
//     past the end of a problem contributes +0.0, which leaves the bits alone (no partial of a chain started at +0.0 is -0.0).
//   * the chunk trees of one reduction share their butterflies: the NV x chunks partials go through block_sum four at a time (the
//     reduce-scatter steps of lpbox_dev_common.h), whose per-value tree is the one-value tree.
//   * rows and columns are summed by one lane in ascending index order, res = 0 + 1.0 * tmp (Eigen's RowMajor sparse * dense).
// Placement: the gathered vectors (the PCG direction / y1 / x, C v, E v) live in LDS; the PCG state of a thread's elements (x, r, p,
// 1/diag, M p, z) in registers; the ADMM state between outer iterations and all matrices in the problem's slice of the pooled global
// arrays, where each element is read and written by its owner thread only (L2 traffic once per outer iteration, not per PCG step).
// REF = true (lpbox_bqp_batch_set_order(LPBOX_ORDER_REFERENCE)): the same kernels with every sum over a
// problem's n elements in the reference's order instead -- Eigen's redux over the n terms in index order (lpbox_eigen_redux.h): the
// terms go to staging rows in LDS between the gathered vector and C v, and four lanes per value walk them.  Rows, columns and every other
// expression are shared with the default order, whose code is what it was (the `if constexpr (!REF)` branches).
#include "lpbox_genb.h"
#include "lpbox_dev_common.h"
#include "lpbox_gen_dev.h"
#include "lpbox_eigen_redux.h"

#include <float.h>

namespace {

constexpr int T = GEN_T;

__device__ __forceinline__ double csr_dot(const GenCsr &c, const double *vals, int j, const double *q) {
    return gen_sparse_dot(c.idx, vals, c.ptr[j], c.ptr[j + 1], [q](int i) { return q[i]; });
}

// N per-thread partials -> workgroup totals in every thread, four values per butterfly
template <int N>
__device__ __forceinline__ void sum_all(double (&f)[N], double *red, int &parity) {
    constexpr int FULL = N / 4, REM = N % 4;
#pragma unroll
    for (int q = 0; q < FULL; q++) {
        double t[4] = {f[4 * q], f[4 * q + 1], f[4 * q + 2], f[4 * q + 3]};
        block_sum<T, 4>(t, red, parity);
        f[4 * q] = t[0]; f[4 * q + 1] = t[1]; f[4 * q + 2] = t[2]; f[4 * q + 3] = t[3];
    }
    if constexpr (REM > 0) {
        double t[REM];
#pragma unroll
        for (int k = 0; k < REM; k++) t[k] = f[4 * FULL + k];
        block_sum<T, REM>(t, red, parity);
#pragma unroll
        for (int k = 0; k < REM; k++) f[4 * FULL + k] = t[k];
    }
}
// NV values x GC chunk partials -> out[k] = the two-level tree of the one-problem path: (c0 + c1) + (c2 + c3)
template <int NV, int GC>
__device__ __forceinline__ void reduce_chunks(double (&part)[NV * GC], double (&out)[NV], double *red, int &parity) {
    sum_all<NV * GC>(part, red, parity);
#pragma unroll
    for (int k = 0; k < NV; k++) {
        if constexpr (GC == 1) out[k] = part[k];
        else if constexpr (GC == 2) out[k] = part[2 * k] + part[2 * k + 1];
        else out[k] = (part[4 * k] + part[4 * k + 1]) + (part[4 * k + 2] + part[4 * k + 3]);
    }
}

// C v and E v for the rows this thread owns (rows tid, tid + 256, ...), v gathered from `src`
template <typename F>
__device__ __forceinline__ void for_rows(int rows, F f) { for (int i = threadIdx.x; i < rows; i += T) f(i); }

// ---- SEGcpp:1430-1560: x = y1 = y2 = best = x0, the matrix 2A + (rho1+rho2) I, the scaled transposes, the Jacobi diagonal, cost(x0)
template <int SL, bool REF>
__global__ void __launch_bounds__(T) genb_init_kernel(const GenbProb *probs, GenState *states) {
    extern __shared__ double lds[];                          // REF: [res ER_RES][2 staging rows of er_stride(n)]; otherwise none
    __shared__ double red[2 * RED_MAXV * RED_MAXW];
    constexpr int GC = SL / 2;
    [[maybe_unused]] int parity = 0;
    const int tid = threadIdx.x;
    const GenbProb P = probs[blockIdx.x];
    const double rho = P.prm.initial_rho;
    const double *x0 = P.x0;
    [[maybe_unused]] double *const stage = lds + ER_RES;
    [[maybe_unused]] const int sst = er_stride(P.n);
    [[maybe_unused]] double pc[2 * GC];
#pragma unroll
    for (int k = 0; k < 2 * GC; k++) pc[k] = 0.0;
#pragma unroll
    for (int s = 0; s < SL; s++) {
        const int j = s * T + tid;
        double c0 = 0.0, c1v = 0.0;
        if (j < P.n) {
            const double xj = x0[j];
            P.x[j] = xj; P.y1[j] = xj; P.y2[j] = xj; P.best[j] = xj; P.z1[j] = 0.0; P.z2[j] = 0.0;
            for (int k = P.aptr[j]; k < P.aptr[j + 1]; k++) P.tmval[k] = 2 * P.aval[k];                 // 2 * A (:1482)
            P.tmval[P.adiag[j]] += rho + rho;                                                          // diagonal += rho1 + rho2 (:1483)
            double pd = P.tmval[P.adiag[j]];
            if (P.eq) {                                                                                // Csq_diag (:1513-1526)
                double sq = 0;
                for (int k = P.Cc.ptr[j]; k < P.Cc.ptr[j + 1]; k++) { const double v = P.Cc.val[k]; if (v != 0.0) sq += v * v; P.Cc_sv[k] = rho * v; }
                P.Csq[j] = sq; pd += rho * sq;
            }
            if (P.ineq) {                                                                              // Esq_diag (:1535-1548)
                double sq = 0;
                for (int k = P.Ec.ptr[j]; k < P.Ec.ptr[j + 1]; k++) { const double v = P.Ec.val[k]; if (v != 0.0) sq += v * v; P.Ec_sv[k] = rho * v; }
                P.Esq[j] = sq; pd += rho * sq;
            }
            P.pdiag[j] = pd; P.dinv[j] = 1.0;
            const double ax = gen_sparse_dot(P.aidx, P.aval, P.aptr[j], P.aptr[j + 1], [x0](int c) { return x0[c]; });   // best_bin_obj = cost(x0) (:1560)
            c0 = xj * ax; c1v = P.b[j] * xj;
            if constexpr (REF) { stage[j] = c0; stage[sst + j] = c1v; }
        }
        if constexpr (!REF) { pc[s / 2] = pc[s / 2] + c0; pc[GC + s / 2] = pc[GC + s / 2] + c1v; }
    }
    double o[2];
    if constexpr (REF) er_reduce<2>(stage, sst, P.n, lds, o);
    else reduce_chunks<2, GC>(pc, o, red, parity);
    if (P.eq) for_rows(P.m, [&](int i) { P.z3[i] = 0.0; });
    if (P.ineq) for_rows(P.l, [&](int i) { P.z4[i] = 0.0; P.y3[i] = 0.0; P.fy[i] = 0.0; P.Ex[i] = csr_dot(P.Er, P.Er.val, i, x0); });   // E x0 for the first y3
    if (tid == 0) {
        GenState *s = states + blockIdx.x;
        memset(s, 0, sizeof(GenState));
        s->rho1 = s->rho2 = s->rho3 = s->rho4 = s->prev_rho1 = s->prev_rho2 = s->prev_rho3 = s->prev_rho4 = rho;
        s->gamma_val = P.prm.gamma_val; s->std_obj = 1.0; s->rhoUpdated = 1; s->c1 = P.c1;
        s->best_bin_obj = o[0] + o[1];
        if (P.prm.max_iters <= 0) s->halt = GEN_HALT_END;
    }
}

// ---- at most `window` outer iterations of ADMM_bqp (SEGcpp:1596-1794) for the problem of this workgroup
template <int SL, bool REF>
__global__ void __launch_bounds__(T) genb_window_kernel(const GenbProb *probs, GenState *states, int window, int npad, int mmax) {
    extern __shared__ double lds[];
    __shared__ double red[2 * RED_MAXV * RED_MAXW];
    __shared__ GenState S;
    constexpr int GC = SL / 2;
    [[maybe_unused]] int parity = 0;
    const int tid = threadIdx.x;
    GenState *gst = states + blockIdx.x;
    if (gst->halt) return;                                   // a halted problem is not touched again
    const GenbProb P = probs[blockIdx.x];
    const GenParams &prm = P.prm;
    // REF: the totals and ER_MAXV staging rows sit between g and C v
    [[maybe_unused]] double *const res = lds + npad, *const stage = res + ER_RES;
    [[maybe_unused]] const int sst = er_stride(npad);
    double *g = lds, *qC = REF ? stage + ER_MAXV * sst : lds + npad, *qE = qC + mmax;
    const int n = P.n, type = (P.eq ? 1 : 0) | (P.ineq ? 2 : 0);
    const bool rows = P.eq || P.ineq;
    if (tid == 0) S = *gst;
    __syncthreads();

    // C v and E v of the vector in g
    auto rows_of_g = [&]() {
        if (P.eq) for_rows(P.m, [&](int i) { qC[i] = csr_dot(P.Cr, P.Cr.val, i, g); });
        if (P.ineq) for_rows(P.l, [&](int i) { qE[i] = csr_dot(P.Er, P.Er.val, i, g); });
    };
    // (2A + (rho1+rho2) I) v + (rho3 C')(C v) + (rho4 E')(E v) for element j, the terms in the order A, C, E (SEGcpp:361-411)
    auto expr_row = [&](int j) {
        double Mv = gen_sparse_dot(P.aidx, P.tmval, P.aptr[j], P.aptr[j + 1], [g](int c) { return g[c]; });
        if (P.eq) Mv += csr_dot(P.Cc, P.Cc_sv, j, qC);
        if (P.ineq) Mv += csr_dot(P.Ec, P.Ec_sv, j, qE);
        return Mv;
    };

    for (int w = 0; w < window; w++) {
        if (S.halt) break;
        const double rho1 = S.rho1, rho2 = S.rho2, rho3 = S.rho3, rho4 = S.rho4, gamma = S.gamma_val, c1 = S.c1;
        const int it = S.iter, rhoUpdated = S.rhoUpdated, copy_best = S.copy_best;
        const bool refresh = it != 0 && rhoUpdated;
        const double inc = S.rcr * (S.prev_rho1 + S.prev_rho2), s3 = S.rcr * S.prev_rho3, s4 = S.rcr * S.prev_rho4;

        // ---- ||x + z2/rho2 - 1/2||^2 (:1603-1606, :553-558)
        double c2;
        {
            [[maybe_unused]] double pa[GC];
            double o[1];
#pragma unroll
            for (int k = 0; k < GC; k++) pa[k] = 0.0;
#pragma unroll
            for (int s = 0; s < SL; s++) {
                const int j = s * T + tid;
                double c = 0.0;
                if (j < n) { const double u = gen_y2_centre(P.x[j], P.z2[j], rho2); c = u * u; if constexpr (REF) stage[j] = c; }
                if constexpr (!REF) pa[s / 2] = pa[s / 2] + c;
            }
            if constexpr (REF) er_reduce<1>(stage, sst, n, res, o);
            else reduce_chunks<1, GC>(pa, o, red, parity);
            c2 = 2 * sqrt(o[0]);
        }

        // ---- y1, y2, y3, matrix / preconditioner refresh (:1619-1650), rhs base (:1656), preconditioner (:1711-1718), best_sol (:1792)
        double rhs[SL], dv[SL];
#pragma unroll
        for (int s = 0; s < SL; s++) {
            const int j = s * T + tid;
            rhs[s] = 0.0; dv[s] = 1.0;
            if (j >= n) continue;
            const double x = P.x[j], z1 = P.z1[j], z2 = P.z2[j];
            if (copy_best) P.best[j] = x;
            const double y1 = gen_y1(x, z1, rho1);                               // :1598-1601
            const double y2 = gen_y2(gen_y2_centre(x, z2, rho2), c1, c2);
            P.y1[j] = y1; P.y2[j] = y2;
            double pd = P.pdiag[j];
            if (refresh) {
                P.tmval[P.adiag[j]] += inc;                                      // :1623
                if (type != 0) pd += inc;                                        // :1626
                if (type == 3) pd += s3 * P.Csq[j];                              // :1629-1632, update_rho3 only
                if (P.ineq) pd += s4 * P.Esq[j];                                 // :1646
                P.pdiag[j] = pd;
            }
            if (rhoUpdated) {                                                    // :1711-1718
                const double dg = type == 0 ? P.tmval[P.adiag[j]] : pd;
                P.dinv[j] = (dg != 0.0) ? 1.0 / dg : 1.0;
            }
            dv[s] = P.dinv[j];
            rhs[s] = gen_rhs_base(rho1, y1, rho2, y2, P.b[j], z1, z2);              // :1656
            g[j] = y1;                                                            // x_sol = y1 (:1721)
        }
        if (refresh) {                                                            // the scaled transposes (:1643, :1648)
            if (type == 3) for (int k = tid; k < P.Cnnz; k += T) P.Cc_sv[k] = prm.learning_fact * P.Cc_sv[k];
            if (P.ineq) for (int k = tid; k < P.Ennz; k += T) P.Ec_sv[k] = prm.learning_fact * P.Ec_sv[k];
        }
        if (P.ineq)
            for_rows(P.l, [&](int i) {
                const double f = P.f[i];
                const double y3 = gen_y3(f, P.Ex[i], P.z4[i], rho4);              // :1609-1613
                P.y3[i] = y3; P.fy[i] = f - y3;
            });
        __syncthreads();                                                          // g = y1, fy, the scaled transposes, the diagonal of tmval

        // ---- rhs (:1663-1706), C y1 and E y1
        if (rows) {
#pragma unroll
            for (int s = 0; s < SL; s++) {
                const int j = s * T + tid;
                if (j >= n) continue;
                double r_ = rhs[s];
                if (P.eq) { r_ += csr_dot(P.Cc, P.Cc_sv, j, P.d); r_ -= csr_dot(P.Cc, P.Cc.val, j, P.z3); }
                if (P.ineq) { r_ += csr_dot(P.Ec, P.Ec_sv, j, P.fy); r_ -= csr_dot(P.Ec, P.Ec.val, j, P.z4); }
                rhs[s] = r_;
            }
            rows_of_g();
            __syncthreads();
        }

        // ---- the PCG on the matrix expression from x = y1 (:415-469)
        double xt[SL], r[SL], p[SL], Mp[SL], z[SL];
        double threshold = 0.0, absNew = 0.0;
        bool done = false;
        {
            [[maybe_unused]] double pb[3 * GC];
            double o[3];
#pragma unroll
            for (int k = 0; k < 3 * GC; k++) pb[k] = 0.0;
#pragma unroll
            for (int s = 0; s < SL; s++) {
                const int j = s * T + tid;
                double c0 = 0.0, c1r = 0.0, c2r = 0.0;
                xt[s] = 0.0; r[s] = 0.0; p[s] = 0.0; Mp[s] = 0.0; z[s] = 0.0;
                if (j < n) {
                    const double Mx = expr_row(j);
                    const double rr = rhs[s] - Mx;
                    const double pp = dv[s] * rr;
                    xt[s] = g[j]; r[s] = rr; p[s] = pp;
                    c0 = rhs[s] * rhs[s]; c1r = rr * rr; c2r = rr * pp;
                    if constexpr (REF) { stage[j] = c0; stage[sst + j] = c1r; stage[2 * sst + j] = c2r; }
                }
                if constexpr (!REF) { pb[s / 2] = pb[s / 2] + c0; pb[GC + s / 2] = pb[GC + s / 2] + c1r; pb[2 * GC + s / 2] = pb[2 * GC + s / 2] + c2r; }
            }
            if constexpr (REF) er_reduce<3>(stage, sst, n, res, o);
            else reduce_chunks<3, GC>(pb, o, red, parity);
            if (o[0] == 0) {                                                      // rhs == 0: x := 0 (:424-430)
                done = true;
#pragma unroll
                for (int s = 0; s < SL; s++) xt[s] = 0.0;
            } else {
                double thr = prm.pcg_tol * prm.pcg_tol * o[0];                    // :433
                if (thr < DBL_MIN) thr = DBL_MIN;
                threshold = thr;
                if (o[1] < thr) done = true;                                      // :435
                absNew = o[2];
            }
        }
        int k = 0;
        while (!done) {
            // (every read of g, qC, qE of the previous step lies before the barriers of the reductions since)
#pragma unroll
            for (int s = 0; s < SL; s++) { const int j = s * T + tid; if (j < n) g[j] = p[s]; }
            __syncthreads();
            if (rows) { rows_of_g(); __syncthreads(); }
            double o1[1], o2[2];
            {
                [[maybe_unused]] double pc[GC];
#pragma unroll
                for (int q = 0; q < GC; q++) pc[q] = 0.0;
#pragma unroll
                for (int s = 0; s < SL; s++) {                                    // tmp = M p, p.tmp (:447-448)
                    const int j = s * T + tid;
                    double c = 0.0;
                    if (j < n) { Mp[s] = expr_row(j); c = p[s] * Mp[s]; if constexpr (REF) stage[j] = c; }
                    if constexpr (!REF) pc[s / 2] = pc[s / 2] + c;
                }
                if constexpr (REF) er_reduce<1>(stage, sst, n, res, o1);
                else reduce_chunks<1, GC>(pc, o1, red, parity);
            }
            const double alpha = absNew / o1[0];
            {
                [[maybe_unused]] double pd2[2 * GC];
#pragma unroll
                for (int q = 0; q < 2 * GC; q++) pd2[q] = 0.0;
#pragma unroll
                for (int s = 0; s < SL; s++) {                                    // :448-462
                    const int j = s * T + tid;
                    double a = 0.0, b2 = 0.0;
                    if (j < n) {
                        double x = xt[s], rr = r[s];
                        x += alpha * p[s];
                        rr -= alpha * Mp[s];
                        const double zz = dv[s] * rr;
                        xt[s] = x; r[s] = rr; z[s] = zz;
                        a = rr * rr; b2 = rr * zz;
                        if constexpr (REF) { stage[j] = a; stage[sst + j] = b2; }
                    }
                    if constexpr (!REF) { pd2[s / 2] = pd2[s / 2] + a; pd2[GC + s / 2] = pd2[GC + s / 2] + b2; }
                }
                if constexpr (REF) er_reduce<2>(stage, sst, n, res, o2);
                else reduce_chunks<2, GC>(pd2, o2, red, parity);
            }
            k++;
            if (o2[0] < threshold || k >= prm.pcg_maxiters) done = true;         // :453-456, :445
            else {
                const double absOld = absNew; absNew = o2[1];                     // :460-463
                const double beta = absNew / absOld;
#pragma unroll
                for (int s = 0; s < SL; s++) p[s] = z[s] + beta * p[s];           // p = z + beta p (:464)
            }
        }

        // ---- commit x, duals z1 z2 (:1733-1734), the seven sums of :1742-1793
        const double g1 = gamma * rho1, g2 = gamma * rho2;
#pragma unroll
        for (int s = 0; s < SL; s++) {
            const int j = s * T + tid;
            if (j >= n) continue;
            const double x = xt[s];
            P.x[j] = x;
            P.z1[j] = P.z1[j] + g1 * (x - P.y1[j]);
            P.z2[j] = P.z2[j] + g2 * (x - P.y2[j]);
            g[j] = x;
        }
        __syncthreads();
        double o[7];
        {
            [[maybe_unused]] double e[7 * GC];
            [[maybe_unused]] double late[SL][3];                                   // REF: the terms of sums 4..6, staged in a second round
#pragma unroll
            for (int q = 0; q < 7 * GC; q++) e[q] = 0.0;
#pragma unroll
            for (int s = 0; s < SL; s++) {
                const int j = s * T + tid;
                double v[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                if (j < n) {
                    const double x = xt[s], y1 = P.y1[j], y2 = P.y2[j], b = P.b[j];
                    const double ax = gen_sparse_dot(P.aidx, P.aval, P.aptr[j], P.aptr[j + 1], [g](int c) { return g[c]; });      // compute_cost (:560-572)
                    const double axb = gen_sparse_dot(P.aidx, P.aval, P.aptr[j], P.aptr[j + 1], [g](int c) { return g[c] >= 0.5 ? 1.0 : 0.0; });
                    const double d1 = x - y1, d2 = x - y2, xb = x >= 0.5 ? 1.0 : 0.0;
                    v[0] = x * x; v[1] = d1 * d1; v[2] = d2 * d2; v[3] = x * ax; v[4] = b * x; v[5] = xb * axb; v[6] = b * xb;
                }
                if constexpr (REF) {
                    if (j < n) { stage[j] = v[0]; stage[sst + j] = v[1]; stage[2 * sst + j] = v[2]; stage[3 * sst + j] = v[3]; }
                    late[s][0] = v[4]; late[s][1] = v[5]; late[s][2] = v[6];
                } else {
#pragma unroll
                    for (int q = 0; q < 7; q++) e[q * GC + s / 2] = e[q * GC + s / 2] + v[q];
                }
            }
            if constexpr (REF) {                                                    // seven sums, ER_MAXV rows: two rounds
                er_reduce<4>(stage, sst, n, res, o);
#pragma unroll
                for (int s = 0; s < SL; s++) {
                    const int j = s * T + tid;
                    if (j < n) { stage[j] = late[s][0]; stage[sst + j] = late[s][1]; stage[2 * sst + j] = late[s][2]; }
                }
                er_reduce<3>(stage, sst, n, res, o + 4);
            } else reduce_chunks<7, GC>(e, o, red, parity);
        }
        // ---- z3 += gamma rho3 (C x - d) (:1736), z4 += gamma rho4 (E x + y3 - f) (:1739); Ex = E x for the next y3
        const double g3 = gamma * rho3, g4 = gamma * rho4;
        if (P.eq) for_rows(P.m, [&](int i) { P.z3[i] = P.z3[i] + g3 * (csr_dot(P.Cr, P.Cr.val, i, g) - P.d[i]); });
        if (P.ineq)
            for_rows(P.l, [&](int i) {
                const double Ex = csr_dot(P.Er, P.Er.val, i, g);
                P.Ex[i] = Ex;
                P.z4[i] = P.z4[i] + g4 * ((Ex + P.y3[i]) - P.f[i]);
            });

        // ---- the stop tests, the rho / gamma schedule, the objective history (:1742-1794)
        if (tid == 0) {
            GenState *s = &S;
            s->rhoUpdated = 0; s->copy_best = 0;
            s->last_pcg = k; s->pcg_total += k; s->outer_total++;
            if (k > s->pcg_max) s->pcg_max = k;
            gen_finish_iteration(s, prm, o, it, P.eq, P.ineq);
            if (!s->halt && s->iter >= prm.max_iters) s->halt = GEN_HALT_END;
        }
        __syncthreads();
    }

    // best_sol = x_sol of the last improving iteration (:1792) is copied by the NEXT iteration; if the loop ended right after an
    // improvement, do it here (x is not touched after the halt)
    const bool trailing = S.halt && S.copy_best;
    if (trailing) {
#pragma unroll
        for (int s = 0; s < SL; s++) { const int j = s * T + tid; if (j < n) P.best[j] = P.x[j]; }
    }
    __syncthreads();
    if (tid == 0) { if (trailing) S.copy_best = 0; *gst = S; }
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
static inline int genb_pad(int n) { return (n + 1) & ~1; }

// default order: the gathered vectors.  Reference order: also the totals and ER_MAXV staging rows of the largest n
size_t genb_lds_bytes(int nmax, int mmax, int lmax, bool ref) {
    size_t d = (size_t)genb_pad(nmax) + (size_t)mmax + (size_t)lmax;
    if (ref) d += ER_RES + (size_t)ER_MAXV * er_stride(genb_pad(nmax));
    return sizeof(double) * d;
}

// above 64 KB of dynamic LDS a launch needs the function attribute (reference order with a large n + m + l only)
template <typename K>
static hipError_t genb_allow_lds(K kernel, size_t lds) {
    if (lds <= 64 * 1024) return hipSuccess;
    return hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

hipError_t genb_launch_init(const GenbProb *probs, GenState *st, int count, int slots, int nmax, bool ref, hipStream_t s) {
    if (ref) {
        const size_t lds = sizeof(double) * (ER_RES + (size_t)2 * er_stride(nmax));       // at most 33 KB
        if (slots == 2) hipLaunchKernelGGL((genb_init_kernel<2, true>), dim3(count), dim3(T), lds, s, probs, st);
        else if (slots == 4) hipLaunchKernelGGL((genb_init_kernel<4, true>), dim3(count), dim3(T), lds, s, probs, st);
        else hipLaunchKernelGGL((genb_init_kernel<8, true>), dim3(count), dim3(T), lds, s, probs, st);
        return hipGetLastError();
    }
    if (slots == 2) hipLaunchKernelGGL((genb_init_kernel<2, false>), dim3(count), dim3(T), 0, s, probs, st);
    else if (slots == 4) hipLaunchKernelGGL((genb_init_kernel<4, false>), dim3(count), dim3(T), 0, s, probs, st);
    else hipLaunchKernelGGL((genb_init_kernel<8, false>), dim3(count), dim3(T), 0, s, probs, st);
    return hipGetLastError();
}

hipError_t genb_launch_window(const GenbProb *probs, GenState *st, int count, int slots, int window, int nmax, int mmax, int lmax, bool ref,
                              hipStream_t s) {
    const size_t lds = genb_lds_bytes(nmax, mmax, lmax, ref);
    const int npad = genb_pad(nmax);
    if (ref) {
        hipError_t e = slots == 2 ? genb_allow_lds(genb_window_kernel<2, true>, lds) : slots == 4 ? genb_allow_lds(genb_window_kernel<4, true>, lds)
                                                                                                   : genb_allow_lds(genb_window_kernel<8, true>, lds);
        if (e != hipSuccess) return e;
        if (slots == 2) hipLaunchKernelGGL((genb_window_kernel<2, true>), dim3(count), dim3(T), lds, s, probs, st, window, npad, mmax);
        else if (slots == 4) hipLaunchKernelGGL((genb_window_kernel<4, true>), dim3(count), dim3(T), lds, s, probs, st, window, npad, mmax);
        else hipLaunchKernelGGL((genb_window_kernel<8, true>), dim3(count), dim3(T), lds, s, probs, st, window, npad, mmax);
        return hipGetLastError();
    }
    if (slots == 2) hipLaunchKernelGGL((genb_window_kernel<2, false>), dim3(count), dim3(T), lds, s, probs, st, window, npad, mmax);
    else if (slots == 4) hipLaunchKernelGGL((genb_window_kernel<4, false>), dim3(count), dim3(T), lds, s, probs, st, window, npad, mmax);
    else hipLaunchKernelGGL((genb_window_kernel<8, false>), dim3(count), dim3(T), lds, s, probs, st, window, npad, mmax);
    return hipGetLastError();
}
