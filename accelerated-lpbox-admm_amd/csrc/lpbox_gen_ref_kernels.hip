// lpbox_gen_ref_kernels.hip -- gfx950 kernels of the GENERIC constrained binary-QP chain in the REFERENCE's summation order
// (lpbox_bqp_set_order(LPBOX_ORDER_REFERENCE); specification: oracle/bqp_oracle.c in ORDER_EIGEN).
// The chain is the one of lpbox_gen_kernels.hip, launch for launch.  What differs:
//   * a kernel that fed a reduction (init, prep, resid, pcg_cols, pcg_upd, post) writes the term of element j to GenRef::stage at
//     row slot, column j (this path never removes a variable: the staging index is j itself) and sums nothing;
//   * genref_k_walk, in the place of gen_k_fin, adds the n staged terms of up to seven rows up in Eigen's redux association and
//     writes GenDev::red[slot], where the consumers read it as they always have.
// gen_k_y, gen_k_rhs_cols, gen_k_rows, gen_k_dual and the state kernels feed no reduction and sum every row and column by one lane in
// ascending order from +0.0: they serve this order as they are.  The element-wise expressions and the end-of-iteration state machine
// are those of lpbox_gen_dev.h; what this file restates of lpbox_gen_kernels.hip is listed in DESIGN.md section 14.3.
// No FMA contraction; IEEE divide / sqrt.
#include "lpbox_gen.h"
#include "lpbox_gen_dev.h"

#include <float.h>

namespace {

constexpr int T = GEN_T;
#define LEADER (blockIdx.x == 0 && threadIdx.x == 0)

__device__ __forceinline__ void forward_state(const GenDev &d, int in, int out) {
    if (LEADER) d.st[out] = d.st[in];
}
__device__ __forceinline__ double *stg(const GenDev &d, const GenRef &rf, int slot) { return rf.stage + (size_t)slot * d.n; }

// A x for row j with x read through `ld` (ascending columns, diagonal included)
template <typename LD>
__device__ __forceinline__ double a_row(const GenDev &d, int j, const double *vals, LD ld) {
    return gen_sparse_dot(d.aidx, vals, d.aptr[j], d.aptr[j + 1], ld);
}
// (scaled transpose row j) . q = sum over the column's entries in ascending row order
__device__ __forceinline__ double col_dot(const GenCsr &c, const double *vals, int j, const double *q) {
    return gen_sparse_dot(c.idx, vals, c.ptr[j], c.ptr[j + 1], [q](int i) { return q[i]; });
}

// ---- the walker: Eigen 3.3.8 redux (SSE2 packets) over the n staged terms of up to GEN_REF_NSTAGE rows at once ----
// Lane 4 v + c of wave 0 walks chain c of value v: a[c], + a[c + 4], + a[c + 8], ... over the part of the vector that is a multiple of
// four long.  The whole workgroup brings the operands in: tile t + 1 is loaded (coalesced) into registers before tile t is walked from
// LDS and stored to the other LDS buffer after it, so the dependent chain is the addition alone.  Lane v then combines
// (p0a + p1a) + (p0b + p1b), the left-over pair and the final odd element; sizes 1-3 take the short branches.  Nothing is padded and
// nothing beyond the n staged terms is read.
// sidx: the GenState the producer of these terms wrote.  A producer that fell through (halt; a converged PCG) staged nothing: the
// walk is skipped and red[] keeps what it holds -- what the reduction launch of the default order recomputes from stale partials --
// so a resumed PCG finds the sums of its last update.
constexpr int WMAXV = GEN_REF_NSTAGE, WTILE = 1024, WROW = WTILE + 4, WU = WTILE / T;   // row pitch + 4: the chains of different values start on different banks
__global__ void __launch_bounds__(T) genref_k_walk(GenDev d, GenRef rf, int nv, int slot0, int sidx, int pcg) {
    __shared__ double tile[2][WMAXV][WROW];
    __shared__ double fin[WMAXV][4];
    if (sidx >= 0) {
        const GenState *si = d.st + sidx;
        if (si->halt || (pcg && si->pcg_done)) return;
    }
    const int size = d.n;
    const int aS2 = (size / 4) * 4, aS = (size / 2) * 2;
    const double *base = stg(d, rf, slot0);
    const int ntiles = (aS2 + WTILE - 1) / WTILE;
    const int lane = threadIdx.x, wv = lane >> 2, wc = lane & 3;
    const bool walker = lane < nv * 4;
    double acc = 0.0, pre[WMAXV][WU];
    auto load = [&](int t) {
#pragma unroll
        for (int v = 0; v < WMAXV; v++)
#pragma unroll
            for (int u = 0; u < WU; u++) {
                const int idx = t * WTILE + u * T + lane;
                pre[v][u] = (v < nv && idx < aS2) ? base[(size_t)v * size + idx] : 0.0;
            }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int v = 0; v < WMAXV; v++)
#pragma unroll
            for (int u = 0; u < WU; u++) if (v < nv) tile[buf][v][u * T + lane] = pre[v][u];
    };
    if (ntiles > 0) { load(0); store(0); }
    __syncthreads();
    for (int t = 0; t < ntiles; t++) {
        if (t + 1 < ntiles) load(t + 1);
        if (walker) {
            const double *tp = tile[t & 1][wv] + wc;
            const int left = aS2 - t * WTILE;
            const int cnt = (left < WTILE ? left : WTILE) / 4;
            int i = 0;
            if (t == 0) { acc = tp[0]; i = 1; }
#pragma unroll 8
            for (; i < cnt; i++) acc = acc + tp[4 * i];
        }
        if (t + 1 < ntiles) store((t + 1) & 1);
        __syncthreads();
    }
    if (walker) fin[wv][wc] = acc;
    __syncthreads();
    if (lane < nv) {
        const double *a = base + (size_t)lane * size;
        double res = 0.0;
        if (size > 0) {
            if (aS) {
                double p0a, p0b;
                if (aS > 2) {
                    p0a = fin[lane][0] + fin[lane][2]; p0b = fin[lane][1] + fin[lane][3];
                    if (aS > aS2) { p0a = p0a + a[aS2]; p0b = p0b + a[aS2 + 1]; }
                } else { p0a = a[0]; p0b = a[1]; }
                res = p0a + p0b;
                for (int idx = aS; idx < size; idx++) res = res + a[idx];
            } else res = a[0];
        }
        d.red[slot0 + lane] = res;
    }
}

// ---- producers (lpbox_gen_kernels.hip, with the workgroup sums replaced by the staged terms) ----
__global__ void __launch_bounds__(T) genref_k_init(GenDev d, GenRef rf, double c1, const double *x0) {     // SEGcpp:1430-1560
    const GenParams &P = d.prm;
    const double rho = P.initial_rho;
    double *s0 = stg(d, rf, 0), *s1 = stg(d, rf, 1);
    if (blockIdx.x < d.G)
        for (int s = 0; s < d.EPT; s++) {
            const int j = blockIdx.x * (T * d.EPT) + s * T + threadIdx.x;
            if (j < d.n) {
                const double xj = x0[j];
                d.x[j] = xj; d.xt[j] = xj; d.y1[j] = xj; d.y2[j] = xj; d.best[j] = xj; d.gsrc[j] = xj;
                d.z1[j] = 0.0; d.z2[j] = 0.0; d.r[j] = 0.0; d.z[j] = 0.0; d.tmp[j] = 0.0; d.p0[j] = 0.0; d.p1[j] = 0.0; d.rhs[j] = 0.0;
                d.zp[j] = make_double2(0.0, 0.0);
                for (int k = d.aptr[j]; k < d.aptr[j + 1]; k++) d.tmval[k] = 2 * d.aval[k];            // 2 * A (:1482)
                d.tmval[d.adiag[j]] += rho + rho;                                                          // diagonal += rho1 + rho2 (:1483)
                double pd = d.tmval[d.adiag[j]];
                if (d.eq) {                                                                                // Csq_diag (:1513-1526)
                    double sq = 0;
                    for (int k = d.Cc.ptr[j]; k < d.Cc.ptr[j + 1]; k++) { const double v = d.Cc.val[k]; if (v != 0.0) sq += v * v; d.Cc_sv[k] = rho * v; }
                    d.Csq[j] = sq; pd += rho * sq;
                }
                if (d.ineq) {                                                                              // Esq_diag (:1535-1548)
                    double sq = 0;
                    for (int k = d.Ec.ptr[j]; k < d.Ec.ptr[j + 1]; k++) { const double v = d.Ec.val[k]; if (v != 0.0) sq += v * v; d.Ec_sv[k] = rho * v; }
                    d.Esq[j] = sq; pd += rho * sq;
                }
                d.pdiag[j] = pd; d.dinv[j] = 1.0;
                const double ax = a_row(d, j, d.aval, [x0](int c) { return x0[c]; });                       // best_bin_obj = cost(x0) (:1560)
                s0[j] = xj * ax; s1[j] = d.b[j] * xj;
            }
        }
    if (blockIdx.x < d.Gm) for (int s = 0; s < d.EPTm; s++) { const int i = blockIdx.x * (T * d.EPTm) + s * T + threadIdx.x; if (i < d.m) { d.z3[i] = 0.0; d.qC[i] = 0.0; } }
    if (blockIdx.x < d.Gl) for (int s = 0; s < d.EPTl; s++) { const int i = blockIdx.x * (T * d.EPTl) + s * T + threadIdx.x; if (i < d.l) { d.z4[i] = 0.0; d.y3[i] = 0.0; d.fy[i] = 0.0; d.Ex[i] = 0.0; d.qE[i] = 0.0; } }
    if (LEADER) {
        GenState *s = d.st;
        memset(s, 0, sizeof(GenState));
        s->rho1 = s->rho2 = s->rho3 = s->rho4 = s->prev_rho1 = s->prev_rho2 = s->prev_rho3 = s->prev_rho4 = rho;
        s->gamma_val = P.gamma_val; s->std_obj = 1.0; s->rhoUpdated = 1; s->c1 = c1;
        d.st[1] = d.st[0];
    }
}

// finalise the previous iteration from red[0..7) (gen_finish_iteration), then the terms of ||x + z2/rho2 - 1/2||^2 for the next one
__global__ void __launch_bounds__(T) genref_k_prep(GenDev d, GenRef rf, int in, int out, int do_prep) {
    const GenState *si = d.st + in;
    const GenParams &P = d.prm;
    const int halt0 = si->halt, have_prev = si->have_prev, it = si->iter;
    double rho2 = si->rho2;
    const bool fin = !halt0 && have_prev;
    bool will_stop = false;
    if (fin) {       // every thread needs to know whether the loop goes on (and the rho2 of the next iteration)
        const double xn = sqrt(d.red[0]);
        const double t0 = (xn < 2.2204e-16) ? 2.2204e-16 : xn;
        if (sqrt(d.red[1]) / t0 <= P.stop_threshold && sqrt(d.red[2]) / t0 <= P.stop_threshold) will_stop = true;
        else if ((it + 1) % P.rho_change_step == 0) rho2 = P.learning_fact * rho2;
    }
    if (LEADER) {
        d.st[out] = *si;
        GenState *s = d.st + out;
        if (fin) {
            s->have_prev = 0;
            gen_finish_iteration(s, P, d.red, it, d.eq, d.ineq);
        }
        if (!s->halt && s->iter >= P.max_iters) s->halt = GEN_HALT_END;
        if (!s->halt && do_prep) s->phase = 1;
    }
    // (the std stop is only known to the leader; terms staged for an iteration that does not come are never walked: the leader halts)
    const int next_iter = (fin && !will_stop) ? it + 1 : it;
    if (!do_prep || halt0 || will_stop || next_iter >= P.max_iters || blockIdx.x >= d.G) return;
    double *s0 = stg(d, rf, 0);
    for (int q = 0; q < d.EPT; q++) {
        const int j = blockIdx.x * (T * d.EPT) + q * T + threadIdx.x;
        if (j < d.n) { const double u = gen_y2_centre(d.x[j], d.z2[j], rho2); s0[j] = u * u; }
    }
}

__global__ void __launch_bounds__(T) genref_k_resid(GenDev d, GenRef rf, int in, int out) {       // :419-441
    const GenState *si = d.st + in;
    if (si->halt || si->phase != 1) { forward_state(d, in, out); return; }
    const double *gs = d.gsrc;
    double *s0 = stg(d, rf, 0), *s1 = stg(d, rf, 1), *s2 = stg(d, rf, 2);
    for (int q = 0; q < d.EPT; q++) {
        const int j = blockIdx.x * (T * d.EPT) + q * T + threadIdx.x;
        if (j < d.n) {
            double Mx = a_row(d, j, d.tmval, [gs](int c) { return gs[c]; });
            if (d.eq) Mx += col_dot(d.Cc, d.Cc_sv, j, d.qC);
            if (d.ineq) Mx += col_dot(d.Ec, d.Ec_sv, j, d.qE);
            const double rhs = d.rhs[j];
            const double r = rhs - Mx;
            const double p = d.dinv[j] * r;
            d.xt[j] = d.y1[j]; d.r[j] = r; d.p0[j] = p;
            s0[j] = rhs * rhs; s1[j] = r * r; s2[j] = r * p;
        }
    }
    if (LEADER) { d.st[out] = *si; d.st[out].pcg_k = 0; d.st[out].pcg_done = 0; d.st[out].pcg_first = 0; d.st[out].phase = 2; }
}

__global__ void __launch_bounds__(T) genref_k_pcg_cols(GenDev d, GenRef rf, int in, int out) {    // tmp = M p, terms of p.tmp (:447-448)
    const GenState *si = d.st + in;
    if (si->halt || si->phase != 2) { forward_state(d, in, out); return; }
    if (si->pcg_done) {
        if (si->pcg_first)                                                       // rhs == 0: x := 0 (:424-430)
            for (int q = 0; q < d.EPT; q++) { const int j = blockIdx.x * (T * d.EPT) + q * T + threadIdx.x; if (j < d.n) d.xt[j] = 0.0; }
        if (LEADER) { d.st[out] = *si; d.st[out].pcg_first = 0; }
        return;
    }
    const int k = si->pcg_k;
    const double beta = si->beta;
    const bool first = k == 0;
    const double *pold = ((k - 1) & 1) ? d.p1 : d.p0;
    double *pnew = (k & 1) ? d.p1 : d.p0;
    const double *p0 = d.p0;
    const double2 *zp = d.zp;
    double *s0 = stg(d, rf, 0);
    for (int q = 0; q < d.EPT; q++) {
        const int j = blockIdx.x * (T * d.EPT) + q * T + threadIdx.x;
        if (j < d.n) {
            double pj, Mp;
            if (first) { pj = p0[j]; Mp = a_row(d, j, d.tmval, [p0](int c2) { return p0[c2]; }); }
            else {
                pj = d.z[j] + beta * pold[j];                                     // p = z + beta p (:464)
                pnew[j] = pj;
                Mp = a_row(d, j, d.tmval, [zp, beta](int c2) { const double2 v = zp[c2]; return v.x + beta * v.y; });
            }
            if (d.eq) Mp += col_dot(d.Cc, d.Cc_sv, j, d.qC);
            if (d.ineq) Mp += col_dot(d.Ec, d.Ec_sv, j, d.qE);
            d.tmp[j] = Mp;
            s0[j] = pj * Mp;
        }
    }
    forward_state(d, in, out);
}

__global__ void __launch_bounds__(T) genref_k_pcg_upd(GenDev d, GenRef rf, int in, int out) {     // :448-462
    const GenState *si = d.st + in;
    if (si->halt || si->phase != 2 || si->pcg_done) { forward_state(d, in, out); return; }
    const int k = si->pcg_k;
    const double alpha = si->absNew / d.red[0];
    const double *p = (k & 1) ? d.p1 : d.p0;
    double *s0 = stg(d, rf, 0), *s1 = stg(d, rf, 1);
    for (int q = 0; q < d.EPT; q++) {
        const int j = blockIdx.x * (T * d.EPT) + q * T + threadIdx.x;
        if (j < d.n) {
            double x = d.xt[j], r = d.r[j];
            const double pj = p[j];
            x += alpha * pj;
            r -= alpha * d.tmp[j];
            const double z = d.dinv[j] * r;
            d.xt[j] = x; d.r[j] = r; d.z[j] = z;
            d.zp[j] = make_double2(z, pj);
            s0[j] = r * r; s1[j] = r * z;
        }
    }
    if (LEADER) { d.st[out] = *si; d.st[out].pcg_k = k + 1; }
}

// after the PCG: commit x, duals z1 z2 (:1733-1734), the terms of the seven sums (:1742-1793)
__global__ void __launch_bounds__(T) genref_k_post(GenDev d, GenRef rf, int in, int out) {
    const GenState *si = d.st + in;
    if (si->halt || si->phase != 2) { forward_state(d, in, out); return; }
    const GenParams &P = d.prm;
    const int k = si->pcg_k;
    if (!si->pcg_done) {                      // the exit test of the last update is still pending
        if (!(k >= 1 && (d.red[0] < si->threshold || k >= P.pcg_maxiters))) {
            if (LEADER) { d.st[out] = *si; d.st[out].halt = GEN_HALT_PCG_MORE; }
            return;
        }
    }
    const double g1 = si->gamma_val * si->rho1, g2 = si->gamma_val * si->rho2;
    const double *xt = d.xt;
    double *s0 = stg(d, rf, 0), *s1 = stg(d, rf, 1), *s2 = stg(d, rf, 2), *s3 = stg(d, rf, 3), *s4 = stg(d, rf, 4), *s5 = stg(d, rf, 5),
           *s6 = stg(d, rf, 6);
    for (int q = 0; q < d.EPT; q++) {
        const int j = blockIdx.x * (T * d.EPT) + q * T + threadIdx.x;
        if (j < d.n) {
            const double x = xt[j], y1 = d.y1[j], y2 = d.y2[j], b = d.b[j];
            d.x[j] = x;
            d.z1[j] = d.z1[j] + g1 * (x - y1);
            d.z2[j] = d.z2[j] + g2 * (x - y2);
            d.gsrc[j] = x;
            const double ax = a_row(d, j, d.aval, [xt](int c) { return xt[c]; });                       // compute_cost (:560-572)
            const double axb = a_row(d, j, d.aval, [xt](int c) { return xt[c] >= 0.5 ? 1.0 : 0.0; });
            const double d1 = x - y1, d2 = x - y2, xb = x >= 0.5 ? 1.0 : 0.0;
            s0[j] = x * x; s1[j] = d1 * d1; s2[j] = d2 * d2; s3[j] = x * ax; s4[j] = b * x; s5[j] = xb * axb; s6[j] = b * xb;
        }
    }
    if (LEADER) {
        d.st[out] = *si;
        GenState *s = d.st + out;
        s->pcg_done = 1; s->last_pcg = k; s->pcg_total += k; s->outer_total++;
        if (k > s->pcg_max) s->pcg_max = k;
        s->phase = 3;
    }
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
#define REF_LAUNCH(kernel, grid, ...)                                                                         \
    do {                                                                                                      \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(T), 0, s, d, rf, *parity, *parity ^ 1, ##__VA_ARGS__);    \
        *parity ^= 1;                                                                                         \
    } while (0)

static inline int gmax3(int a, int b, int c) { int m = a > b ? a : b; return m > c ? m : c; }

hipError_t genref_launch_walk(const GenDev &d, const GenRef &rf, int nv, int slot0, int sidx, int pcg, hipStream_t s) {
    if (nv < 1 || slot0 < 0 || slot0 + nv > GEN_REF_NSTAGE || !rf.stage) return hipErrorInvalidValue;
    hipLaunchKernelGGL(genref_k_walk, dim3(1), dim3(T), 0, s, d, rf, nv, slot0, sidx, pcg);
    return hipGetLastError();
}
hipError_t genref_launch_init(const GenDev &d, const GenRef &rf, double c1, const double *x0, hipStream_t s) {
    if (!rf.stage) return hipErrorInvalidValue;
    hipLaunchKernelGGL(genref_k_init, dim3(gmax3(d.G, d.Gm, d.Gl)), dim3(T), 0, s, d, rf, c1, x0);
    return genref_launch_walk(d, rf, 2, 0, -1, 0, s);
}
hipError_t genref_launch_prep(const GenDev &d, const GenRef &rf, int do_prep, int *parity, hipStream_t s) { REF_LAUNCH(genref_k_prep, d.G, do_prep); return hipGetLastError(); }
hipError_t genref_launch_resid(const GenDev &d, const GenRef &rf, int *parity, hipStream_t s) { REF_LAUNCH(genref_k_resid, d.G); return hipGetLastError(); }
hipError_t genref_launch_pcg_cols(const GenDev &d, const GenRef &rf, int *parity, hipStream_t s) { REF_LAUNCH(genref_k_pcg_cols, d.G); return hipGetLastError(); }
hipError_t genref_launch_pcg_upd(const GenDev &d, const GenRef &rf, int *parity, hipStream_t s) { REF_LAUNCH(genref_k_pcg_upd, d.G); return hipGetLastError(); }
hipError_t genref_launch_post(const GenDev &d, const GenRef &rf, int *parity, hipStream_t s) { REF_LAUNCH(genref_k_post, d.G); return hipGetLastError(); }
