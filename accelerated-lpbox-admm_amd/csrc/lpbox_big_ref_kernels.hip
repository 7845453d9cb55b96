// lpbox_big_ref_kernels.hip -- gfx950 kernels of the large-instance LP path in the REFERENCE's summation order
// (lpbox_big_set_order(LPBOX_ORDER_REFERENCE), one rank; specification: oracle/lpbox_oracle.c in LPO_ORDER_EIGEN).
// The chain is the one of lpbox_big_kernels.hip, launch for launch.  What differs:
//   * a kernel that fed a reduction writes its per-variable terms into BigRef::stage at the variable's live rank (bigref_k_rank) and
//     sums nothing; bigref_k_walk, in the place of big_k_fin, adds them up in Eigen's redux association and writes BigDev::red, which
//     the consumers read as they do on the route with a reduction launch (BigDev::fold is off);
//   * VALUED instantiations multiply by the stored values of E and carry rho4_E_transpose per entry (r4v) instead of the scalar r4Et.
// Kernels that neither feed a reduction nor touch a value (big_k_y, big_k_rhs_cols, big_k_rows with one column slice, big_k_fix3,
// big_k_z4, the state kernels) serve the unit instance as they are: they already sum every row and column by one lane in ascending
// order from +0.0.  No FMA contraction; IEEE divide / sqrt.
#include "lpbox_big.h"

#include <float.h>

namespace {

constexpr int T = BIG_T;
#define LEADER (blockIdx.x == 0 && threadIdx.x == 0)

__device__ __forceinline__ void forward_state(const BigDev &d, int in, int out) {
    if (LEADER) d.st[out] = d.st[in];
}
template <int PHASE>
__device__ __forceinline__ double *stg(const BigDev &d, const BigRef &rf, int v) {
    return rf.stage + (size_t)(big_ref_stage_off(PHASE) + v) * d.n_loc;
}
__device__ __forceinline__ double red_of(const BigDev &d, int phase, int v) { return d.red[phase * BIG_NPART + v]; }

// ---- live rank: one workgroup, a block prefix sum per chunk of T * RE variables with a carried offset ----
constexpr int RE = 4;
__global__ void __launch_bounds__(T) bigref_k_rank(BigDev d, BigRef rf, int mode) {
    __shared__ int wsum[T / 64 + 1];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int *out = mode == 1 ? rf.frank : rf.rank;
    int carried = 0;
    for (int base = 0; base < d.n_loc; base += T * RE) {
        int keep[RE], c = 0;
#pragma unroll
        for (int k = 0; k < RE; k++) {
            const int j = base + threadIdx.x * RE + k;
            keep[k] = 0;
            if (j < d.n_loc) {
                const int lv = d.live[j], nf = d.newfix[j];
                keep[k] = mode == 0 ? (lv != 0) : (mode == 1 ? (nf != 0) : (lv != 0 && nf == 0));
            }
            c += keep[k];
        }
        int v = c;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) { const int t = __shfl_up(v, off, 64); if (lane >= off) v += t; }
        if (lane == 63) wsum[w + 1] = v;
        __syncthreads();
        if (threadIdx.x == 0) { wsum[0] = 0; for (int k = 1; k <= T / 64; k++) wsum[k] += wsum[k - 1]; }
        __syncthreads();
        int pos = carried + wsum[w] + v - c;
        const int total = wsum[T / 64];
#pragma unroll
        for (int k = 0; k < RE; k++) {
            const int j = base + threadIdx.x * RE + k;
            if (j < d.n_loc) out[j] = keep[k] ? pos++ : -1;
        }
        carried += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) rf.cnt[mode == 1 ? 1 : 0] = carried;
}

// ---- the walker: Eigen 3.3.8 redux (SSE2 packets) over the staged terms of up to BIG_REF_MAXV values at once ----
// Lane 4 v + c of wave 0 walks chain c of value v: a[c], + a[c + 4], + a[c + 8], ... over the part of the vector that is a multiple of
// four long.  The whole workgroup brings the operands in: tile t + 1 is loaded (coalesced) into registers before tile t is walked from
// LDS and stored to the other LDS buffer after it, so the dependent chain is the addition alone.  Lane v then combines
// (p0a + p1a) + (p0b + p1b), the left-over pair and the final odd element; sizes 1-3 take the short branches.
constexpr int WTILE = 1024, WROW = WTILE + 4, WU = WTILE / T;    // row pitch + 4: the chains of different values start on different banks
__global__ void __launch_bounds__(T) bigref_k_walk(BigDev d, BigRef rf, int nv, int soff, int roff, int which, int sidx, int pcg) {
    __shared__ double tile[2][BIG_REF_MAXV][WROW];
    __shared__ double fin[BIG_REF_MAXV][4];
    if (sidx >= 0) {
        const BigState *si = d.st + sidx;
        if (si->halt || (pcg && si->pcg_done)) return;          // the producer fell through: red[] keeps what it holds
    }
    int size = rf.cnt[which];
    if (size > d.n_loc) size = d.n_loc;
    const int aS2 = (size / 4) * 4, aS = (size / 2) * 2;
    const double *base = rf.stage + (size_t)soff * d.n_loc;
    const int ntiles = (aS2 + WTILE - 1) / WTILE;
    const int lane = threadIdx.x, wv = lane >> 2, wc = lane & 3;
    const bool walker = lane < nv * 4;
    double acc = 0.0, pre[BIG_REF_MAXV][WU];
    auto load = [&](int t) {
#pragma unroll
        for (int v = 0; v < BIG_REF_MAXV; v++)
#pragma unroll
            for (int u = 0; u < WU; u++) {
                const int idx = t * WTILE + u * T + lane;
                pre[v][u] = (v < nv && idx < aS2) ? base[(size_t)v * d.n_loc + idx] : 0.0;
            }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int v = 0; v < BIG_REF_MAXV; v++)
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
        const double *a = base + (size_t)lane * d.n_loc;
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
        d.red[roff + lane] = res;
    }
}

// ---- producers (lpbox_big_kernels.hip, with the workgroup sums replaced by the staged terms) ----
__global__ void __launch_bounds__(T) bigref_k_init(BigDev d, BigRef rf, double c1) {          // ADMM_lp_iters_init LPcpp:489-763
    double *sx = stg<BIG_PH_X>(d, rf, 0);
    for (int s = 0; s < d.EPT; s++) {
        const int j = blockIdx.x * (T * d.EPT) + s * T + threadIdx.x;
        if (j < d.n_loc) {
            d.x[j] = 1.0; d.z1[j] = 0.0; d.z2[j] = 0.0; d.pd[j] = 0.0; d.dinv[j] = 1.0;
            d.y1[j] = 1.0; d.y2[j] = 1.0; d.gsrc[j] = 1.0; d.xt[j] = 1.0; d.live[j] = 1;
            d.r[j] = 0.0; d.z[j] = 0.0; d.tmp[j] = 0.0; d.p0[j] = 0.0; d.p1[j] = 0.0; d.rhs[j] = 0.0;
            sx[j] = d.b[j] * 1.0;                                                // best_bin_obj = b.dot(x0) (:727); every variable is live
        }
    }
    for (int s = 0; s < d.EPTl; s++) {
        const int i = blockIdx.x * (T * d.EPTl) + s * T + threadIdx.x;
        if (i < d.l) { d.z4[i] = 0.0; d.y3[i] = 0.0; d.fz[i] = make_double2(0.0, 0.0); d.Ex[i] = 0.0; }
    }
    if (LEADER) {
        BigState *s = d.st;
        memset(s, 0, sizeof(BigState));
        s->rho1 = s->rho2 = s->rho4 = s->prev_rho1 = s->prev_rho2 = s->prev_rho4 = LP_RHO0;
        s->gamma_val = LP_GAMMA0; s->std_obj = 1.0; s->rhoUpdated = 1; s->c1 = c1;
        s->n_live_lo = (int)(d.n_glob & 0x7fffffff); s->n_live_hi = (int)(d.n_glob >> 31);
        d.st[1] = d.st[0];
    }
}

__global__ void __launch_bounds__(T) bigref_k_prep(BigDev d, BigRef rf, int in, int out, int do_prep) {
    const BigState *si = d.st + in;
    const int halt0 = si->halt, have_prev = si->have_prev, it = si->iter, iter_end = si->iter_end;
    double rho2 = si->rho2;
    const bool fin = !halt0 && have_prev;
    if (fin && (it + 1) % LP_RHO_STEP == 0) rho2 = LP_LEARNING_FACT * rho2;
    const int next_iter = fin ? it + 1 : it;
    const bool will_prep = do_prep && !halt0 && next_iter < iter_end;
    if (LEADER) {
        double e5[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        if (fin) for (int k = 0; k < 5; k++) e5[k] = red_of(d, BIG_PH_E, k);
        d.st[out] = *si;
        BigState *s = d.st + out;
        if (fin) {
            s->have_prev = 0;
            const double xn = sqrt(e5[0]);
            const double t0 = (xn < 2.2204e-16) ? 2.2204e-16 : xn;
            s->cvg1 = sqrt(e5[1]) / t0; s->cvg2 = sqrt(e5[2]) / t0;            // :931-933
            bool stopped = false;
            if (s->cvg1 <= LP_STOP_THRESHOLD && s->cvg2 <= LP_STOP_THRESHOLD && (s->l2f || it != s->iter_start)) {   // :934 / :1503
                if (s->l2f) s->ret = 1;
                s->stop = LP_STOP_Y1Y2; stopped = true;
            } else {
                if ((it + 1) % LP_RHO_STEP == 0) {                                // :951-970
                    s->prev_rho1 = s->rho1; s->prev_rho2 = s->rho2; s->prev_rho4 = s->rho4;
                    s->rho1 = LP_LEARNING_FACT * s->rho1; s->rho2 = LP_LEARNING_FACT * s->rho2; s->rho4 = LP_LEARNING_FACT * s->rho4;
                    const double g = s->gamma_val * LP_GAMMA_FACTOR;
                    s->gamma_val = g < 1.0 ? 1.0 : g;
                    s->rhoUpdated = 1; s->rcr = LP_LEARNING_FACT - 1.0;
                }
                s->obj_val = e5[3];                                               // :972
                int hn = s->hist_n;
                if (hn < LP_HIST) s->hist[hn] = s->obj_val;
                else { for (int k = 0; k < LP_HIST - 1; k++) s->hist[k] = s->hist[k + 1]; s->hist[LP_HIST - 1] = s->obj_val; }
                if (hn < 0x3fffffff) hn++;
                s->hist_n = hn;
                if (hn >= LP_HIST) {                                              // :459-469, :358-377
                    double mean = 0;
                    for (int k = 0; k < LP_HIST; k++) mean += s->hist[k];
                    mean /= (double)LP_HIST;
                    double dev = 0;
                    for (int k = 0; k < LP_HIST; k++) dev += (s->hist[k] - mean) * (s->hist[k] - mean);
                    dev /= (double)(LP_HIST - 1);
                    const double sd = (dev == 0) ? 0.0 : sqrt(dev);               // the reference: pow(v, 1/2)
                    s->std_obj = sd / fabs(s->hist[LP_HIST - 1]);
                }
                if (s->std_obj <= LP_STD_THRESHOLD) { s->ret = 1; s->stop = LP_STOP_OBJSTD; stopped = true; }   // :977
                else {
                    s->cur_obj = e5[4];                                           // :1001-1003
                    if (s->best_bin_obj >= s->cur_obj) s->best_bin_obj = s->cur_obj;
                }
            }
            if (stopped) { s->halt = BIG_HALT_STOP; s->plain_iter_p1 = it + 1; }
            else s->iter = it + 1;
        }
        if (!s->halt && s->iter >= s->iter_end) { s->halt = BIG_HALT_WINDOW; s->plain_iter_p1 = s->iter + 1; }
        if (!s->halt && do_prep) s->phase = 1;
    }
    if (!will_prep || blockIdx.x >= d.G) return;
    double *sa = stg<BIG_PH_A>(d, rf, 0);
    for (int q = 0; q < d.EPT; q++) {
        const int j = blockIdx.x * (T * d.EPT) + q * T + threadIdx.x;
        if (j < d.n_loc && d.live[j]) { const double u = (d.x[j] + d.z2[j] / rho2) - 0.5; sa[rf.rank[j]] = u * u; }
    }
}

// VALUED only: big_k_y with Esq_diag = the sum of val^2 down the column and rho4_E_transpose kept per entry
__global__ void __launch_bounds__(T) bigref_k_y_v(BigDev d, BigRef rf, int in, int out) {
    const BigState *si = d.st + in;
    if (si->halt || si->phase != 1) { forward_state(d, in, out); return; }
    const double rho1 = si->rho1, rho2 = si->rho2, rho4 = si->rho4, c1 = si->c1;
    const int it = si->iter, rhoUpdated = si->rhoUpdated;
    double dI = si->dI, r4Et = si->r4Et;
    const bool first = it == 0, refresh = it != 0 && rhoUpdated;
    const double inc = si->rcr * (si->prev_rho1 + si->prev_rho2), inc4 = si->rcr * si->prev_rho4;
    if (first) { dI = 0.0; dI += rho1 + rho2; r4Et = rho4; }                     // update_expression(0) :2289-2404
    if (refresh) { dI += inc; r4Et = LP_LEARNING_FACT * r4Et; }                  // :851-866
    const double c2 = 2 * sqrt(red_of(d, BIG_PH_A, 0));
    if (blockIdx.x < d.G)
        for (int q = 0; q < d.EPT; q++) {
            const int j = blockIdx.x * (T * d.EPT) + q * T + threadIdx.x;
            if (j >= d.n_loc) continue;
            const double x = d.x[j], z1 = d.z1[j], z2 = d.z2[j];
            const double t = x + z1 / rho1;
            const double y1 = t > 1 ? 1 : (t < 0 ? 0 : t);                       // :806-809
            double y2 = (x + z2 / rho2) - 0.5;                                   // :815-818
            y2 = y2 * c1 / c2 + 0.5;
            d.y1[j] = y1; d.y2[j] = y2;
            double pd = d.pd[j];
            const int k0 = d.cptr[j], k1 = d.cptr[j + 1];
            if (first || refresh) {
                double Esq = 0.0;
                for (int k = k0; k < k1; k++) { const double v = rf.vcsc[k]; Esq += v * v; }     // :2378-2390
                if (first) { pd = dI; pd += rho4 * Esq; for (int k = k0; k < k1; k++) rf.r4v[k] = rho4 * rf.vcsc[k]; }   // :2293, :2391
                if (refresh) { pd += inc; pd += inc4 * Esq; for (int k = k0; k < k1; k++) rf.r4v[k] = LP_LEARNING_FACT * rf.r4v[k]; }
            }
            d.pd[j] = pd;
            if (rhoUpdated) d.dinv[j] = (pd != 0.0) ? 1.0 / pd : 1.0;            // :883-890
            d.rhs[j] = (rho1 * y1 + rho2 * y2) - ((d.b[j] + z1) + z2);            // :872
            d.gsrc[j] = d.live[j] ? y1 : 0.0;
        }
    if (blockIdx.x < d.Gl)
        for (int q = 0; q < d.EPTl; q++) {
            const int i = blockIdx.x * (T * d.EPTl) + q * T + threadIdx.x;
            if (i >= d.l) continue;
            const double f = d.f[i];
            const double z4 = d.z4[i];
            const double v = f - d.Ex[i] - z4 / rho4;                             // :824-828
            const double y3 = v < 0 ? 0 : v;
            d.y3[i] = y3; d.fz[i] = make_double2(f - y3, z4);
        }
    if (LEADER) {
        d.st[out] = *si;
        BigState *s = d.st + out;
        s->dI = dI; s->r4Et = r4Et; s->rhoUpdated = 0; s->expr_ready = 1;
    }
}

__global__ void __launch_bounds__(T) bigref_k_rhs_cols_v(BigDev d, BigRef rf, int in, int out) {   // :874-877
    const BigState *si = d.st + in;
    if (si->halt || si->phase != 1) { forward_state(d, in, out); return; }
    for (int q = 0; q < d.EPT; q++) {
        const int j = blockIdx.x * (T * d.EPT) + q * T + threadIdx.x;
        if (j >= d.n_loc) continue;
        double tA = 0.0, tB = 0.0;
        const int k1 = d.cptr[j + 1];
        int k = d.cptr[j];
        for (; k + 4 <= k1; k += 4) {                      // 4 gathers in flight, additions in column order
            double2 e[4]; double a[4], v[4];
#pragma unroll
            for (int u = 0; u < 4; u++) { e[u] = d.fz[d.crow[k + u]]; a[u] = rf.r4v[k + u]; v[u] = rf.vcsc[k + u]; }
#pragma unroll
            for (int u = 0; u < 4; u++) { tA += a[u] * e[u].x; tB += v[u] * e[u].y; }
        }
        for (; k < k1; k++) { const double2 e = d.fz[d.crow[k]]; tA += rf.r4v[k] * e.x; tB += rf.vcsc[k] * e.y; }
        double r_ = d.rhs[j];
        r_ += tA;
        r_ -= tB;
        d.rhs[j] = r_;
    }
    forward_state(d, in, out);
}

// VALUED only: big_k_rows for one column slice, acc += val * v_j
__global__ void __launch_bounds__(T) bigref_k_rows_v(BigDev d, BigRef rf, int in, int out, int mode) {
    const BigState *si = d.st + in;
    if (si->halt) { forward_state(d, in, out); return; }
    double beta = 0.0;
    bool first = false;
    if (mode == 1) {
        if (si->phase != 2 || si->pcg_done) { forward_state(d, in, out); return; }
        const int k = si->pcg_k;
        double threshold = si->threshold, absNew = si->absNew, rhsNorm2 = si->rhsNorm2;
        bool done = false; int zero_x = 0;
        first = k == 0;
        if (first) {
            const double b0 = red_of(d, BIG_PH_B, 0), b1 = red_of(d, BIG_PH_B, 1), b2 = red_of(d, BIG_PH_B, 2);
            rhsNorm2 = b0;
            if (rhsNorm2 == 0) { done = true; zero_x = 1; }                      // :273-278
            else {
                double thr = LP_PCG_TOL * LP_PCG_TOL * rhsNorm2;                 // :281
                if (thr < DBL_MIN) thr = DBL_MIN;
                threshold = thr;
                if (b1 < thr) done = true;                                       // :284
                absNew = b2;
            }
        } else {
            const double d0 = red_of(d, BIG_PH_D, 0), d1 = red_of(d, BIG_PH_D, 1);
            if (d0 < threshold || k >= LP_PCG_MAXITERS) done = true;             // :309-312, :296
            else { const double absOld = absNew; absNew = d1; beta = absNew / absOld; }   // :316-318
        }
        if (LEADER) {
            d.st[out] = *si;
            BigState *s = d.st + out;
            s->threshold = threshold; s->absNew = absNew; s->rhsNorm2 = rhsNorm2; s->beta = beta;
            s->pcg_done = done ? 1 : 0; s->pcg_first = zero_x;
        }
        if (done) return;
    } else forward_state(d, in, out);
    if ((int)blockIdx.x >= d.Gl) return;
    for (int s = 0; s < d.EPTl; s++) {
        const int i = blockIdx.x * (T * d.EPTl) + s * T + threadIdx.x;
        if (i >= d.l) continue;
        double acc = 0.0;
        const int k1 = d.rptr[i + 1];
        int k = d.rptr[i];
        if (mode == 0 || first) {
            const double *src = mode == 0 ? d.gsrc : d.p0;
            for (; k + 8 <= k1; k += 8) {
                double v[8], a[8];
#pragma unroll
                for (int u = 0; u < 8; u++) { v[u] = src[d.rcol[k + u]]; a[u] = rf.vcsr[k + u]; }
#pragma unroll
                for (int u = 0; u < 8; u++) acc += a[u] * v[u];
            }
            for (; k < k1; k++) acc += rf.vcsr[k] * src[d.rcol[k]];
        } else {
            for (; k + 8 <= k1; k += 8) {
                double2 v[8]; double a[8];
#pragma unroll
                for (int u = 0; u < 8; u++) { v[u] = d.zp[d.rcol[k + u]]; a[u] = rf.vcsr[k + u]; }
#pragma unroll
                for (int u = 0; u < 8; u++) acc += a[u] * (v[u].x + beta * v[u].y);
            }
            for (; k < k1; k++) { const double2 v = d.zp[d.rcol[k]]; acc += rf.vcsr[k] * (v.x + beta * v.y); }
        }
        d.q[i] = acc;
    }
}

// t = sum over column j of rho4_E_transpose * q, rows ascending from +0.0
template <bool VALUED>
__device__ __forceinline__ double col_r4_q(const BigDev &d, const BigRef &rf, int j, double r4Et) {
    double t = 0.0;
    const int k1 = d.cptr[j + 1];
    int k = d.cptr[j];
    for (; k + 4 <= k1; k += 4) {
        const double v0 = d.q[d.crow[k]], v1 = d.q[d.crow[k + 1]], v2 = d.q[d.crow[k + 2]], v3 = d.q[d.crow[k + 3]];
        if constexpr (VALUED) {
            const double a0 = rf.r4v[k], a1 = rf.r4v[k + 1], a2 = rf.r4v[k + 2], a3 = rf.r4v[k + 3];
            t += a0 * v0; t += a1 * v1; t += a2 * v2; t += a3 * v3;
        } else { t += r4Et * v0; t += r4Et * v1; t += r4Et * v2; t += r4Et * v3; }
    }
    for (; k < k1; k++) {
        if constexpr (VALUED) t += rf.r4v[k] * d.q[d.crow[k]];
        else t += r4Et * d.q[d.crow[k]];
    }
    return t;
}

template <bool VALUED>
__global__ void __launch_bounds__(T) bigref_k_resid(BigDev d, BigRef rf, int in, int out) {       // :267-294
    const BigState *si = d.st + in;
    if (si->halt || si->phase != 1) { forward_state(d, in, out); return; }
    const double dI = si->dI, r4Et = si->r4Et;
    double *s0 = stg<BIG_PH_B>(d, rf, 0), *s1 = stg<BIG_PH_B>(d, rf, 1), *s2 = stg<BIG_PH_B>(d, rf, 2);
    for (int q = 0; q < d.EPT; q++) {
        const int j = blockIdx.x * (T * d.EPT) + q * T + threadIdx.x;
        if (j >= d.n_loc) continue;
        const double t = col_r4_q<VALUED>(d, rf, j, r4Et);
        const double y1 = d.y1[j];
        double Mx = 0.0;
        Mx += dI * (1.0 * y1);
        Mx += t;
        const double rhs = d.rhs[j];
        const double r = rhs - Mx;
        const double p = d.dinv[j] * r;
        const bool lv = d.live[j];
        d.xt[j] = y1; d.r[j] = r; d.p0[j] = lv ? p : 0.0;
        if (lv) { const int rk = rf.rank[j]; s0[rk] = rhs * rhs; s1[rk] = r * r; s2[rk] = r * p; }
    }
    if (LEADER) { d.st[out] = *si; d.st[out].pcg_k = 0; d.st[out].pcg_done = 0; d.st[out].pcg_first = 0; d.st[out].phase = 2; }
}

template <bool VALUED>
__global__ void __launch_bounds__(T) bigref_k_pcg_cols(BigDev d, BigRef rf, int in, int out) {    // tmp = M p, terms of p.tmp (:298-300)
    const BigState *si = d.st + in;
    if (si->halt || si->phase != 2) { forward_state(d, in, out); return; }
    if (si->pcg_done) {
        if (si->pcg_first)                                                       // rhs == 0: x := 0 (:273-278)
            for (int q = 0; q < d.EPT; q++) { const int j = blockIdx.x * (T * d.EPT) + q * T + threadIdx.x; if (j < d.n_loc) d.xt[j] = 0.0; }
        if (LEADER) { d.st[out] = *si; d.st[out].pcg_first = 0; }
        return;
    }
    const int k = si->pcg_k;
    const double dI = si->dI, r4Et = si->r4Et, beta = si->beta;
    const bool first = k == 0;
    const double *pold = ((k - 1) & 1) ? d.p1 : d.p0;
    double *pnew = (k & 1) ? d.p1 : d.p0;
    double *sc = stg<BIG_PH_C>(d, rf, 0);
    for (int q = 0; q < d.EPT; q++) {
        const int j = blockIdx.x * (T * d.EPT) + q * T + threadIdx.x;
        if (j >= d.n_loc) continue;
        double pj;
        if (first) pj = d.p0[j];
        else { pj = d.z[j] + beta * pold[j]; pnew[j] = pj; }                     // p = z + beta p (:319)
        const double t = col_r4_q<VALUED>(d, rf, j, r4Et);
        double Mp = 0.0;
        Mp += dI * (1.0 * pj);
        Mp += t;
        d.tmp[j] = Mp;
        if (d.live[j]) sc[rf.rank[j]] = pj * Mp;
    }
    forward_state(d, in, out);
}

__global__ void __launch_bounds__(T) bigref_k_pcg_upd(BigDev d, BigRef rf, int in, int out) {     // :300-317
    const BigState *si = d.st + in;
    if (si->halt || si->phase != 2 || si->pcg_done) { forward_state(d, in, out); return; }
    const int k = si->pcg_k;
    const double alpha = si->absNew / red_of(d, BIG_PH_C, 0);
    const bool fail = alpha < 0;
    const double *p = (k & 1) ? d.p1 : d.p0;
    double *s0 = stg<BIG_PH_D>(d, rf, 0), *s1 = stg<BIG_PH_D>(d, rf, 1);
    if (!fail)
        for (int q = 0; q < d.EPT; q++) {
            const int j = blockIdx.x * (T * d.EPT) + q * T + threadIdx.x;
            if (j >= d.n_loc) continue;
            double x = d.xt[j], r = d.r[j];
            x += alpha * p[j];
            r -= alpha * d.tmp[j];
            const double z = d.dinv[j] * r;
            const bool lv = d.live[j];
            d.xt[j] = x; d.r[j] = r; d.z[j] = lv ? z : 0.0;
            d.zp[j] = make_double2(lv ? z : 0.0, p[j]);
            if (lv) { const int rk = rf.rank[j]; s0[rk] = r * r; s1[rk] = r * z; }
        }
    if (LEADER) {
        d.st[out] = *si;
        if (fail) { d.st[out].pcg_done = 1; d.st[out].stop = LP_STOP_PCG; }
        else d.st[out].pcg_k = k + 1;
    }
}

__global__ void __launch_bounds__(T) bigref_k_post(BigDev d, BigRef rf, int in, int out) {
    const BigState *si = d.st + in;
    if (si->halt || si->phase != 2) { forward_state(d, in, out); return; }
    const int k = si->pcg_k;
    if (!si->pcg_done) {                      // the exit test of the last update is still pending
        const double d0 = k >= 1 ? red_of(d, BIG_PH_D, 0) : 0.0;
        if (!(k >= 1 && (d0 < si->threshold || k >= LP_PCG_MAXITERS))) {
            if (LEADER) { d.st[out] = *si; d.st[out].halt = BIG_HALT_PCG_MORE; }
            return;
        }
    }
    if (si->l2f && si->stop == LP_STOP_PCG) {   // alpha < 0 inside the l2f loop: return 1, x_sol untouched (:1450-1454)
        if (LEADER) { d.st[out] = *si; BigState *s = d.st + out; s->ret = 1; s->halt = BIG_HALT_STOP; s->pcg_done = 1; s->last_pcg = k; s->pcg_total += k; }
        return;
    }
    const double g1 = si->gamma_val * si->rho1, g2 = si->gamma_val * si->rho2;
    double *xh = ((si->l2f || si->rec) && d.xhist && si->cc < d.ws_cap) ? d.xhist + (size_t)si->cc * d.n_loc : nullptr;
    double *s0 = stg<BIG_PH_E>(d, rf, 0), *s1 = stg<BIG_PH_E>(d, rf, 1), *s2 = stg<BIG_PH_E>(d, rf, 2), *s3 = stg<BIG_PH_E>(d, rf, 3),
           *s4 = stg<BIG_PH_E>(d, rf, 4);
    for (int q = 0; q < d.EPT; q++) {
        const int j = blockIdx.x * (T * d.EPT) + q * T + threadIdx.x;
        if (j >= d.n_loc) continue;
        const bool lv = d.live[j];
        const double x = lv ? d.xt[j] : d.x[j], y1 = d.y1[j], y2 = d.y2[j], b = d.b[j];
        d.x[j] = x;
        if (xh) xh[j] = x;                                                    // x_iters column (:1472-1475)
        d.z1[j] = d.z1[j] + g1 * (x - y1);
        d.z2[j] = d.z2[j] + g2 * (x - y2);
        d.gsrc[j] = lv ? x : 0.0;
        const double d1 = x - y1, d2 = x - y2, xb = x >= 0.5 ? 1.0 : 0.0;
        if (lv) { const int rk = rf.rank[j]; s0[rk] = x * x; s1[rk] = d1 * d1; s2[rk] = d2 * d2; s3[rk] = b * x; s4[rk] = b * xb; }
    }
    if (LEADER) {
        d.st[out] = *si;
        BigState *s = d.st + out;
        s->pcg_done = 1; s->last_pcg = k; s->pcg_total += k; s->outer_total++;
        if (si->l2f || si->rec) s->cc = si->cc + 1;
        if (k > s->pcg_max) s->pcg_max = k;
        s->phase = 3;
    }
}

// ---- early fixing: the terms of b2.x2 at the rank among the newly fixed (:1237), of |x_live|^2 at the NEW live rank (:1223) ----
__global__ void __launch_bounds__(T) bigref_k_fix1(BigDev d, BigRef rf) {
    double *sx = stg<BIG_PH_X>(d, rf, 0);
    for (int q = 0; q < d.EPT; q++) {
        const int j = blockIdx.x * (T * d.EPT) + q * T + threadIdx.x;
        if (j >= d.n_loc) continue;
        const int nf = d.newfix[j];
        const double val = nf == 2 ? 1.0 : 0.0;
        d.gsrc[j] = nf ? val : 0.0;
        if (nf) sx[rf.frank[j]] = d.b[j] * val;
    }
}

__global__ void __launch_bounds__(T) bigref_k_fix2(BigDev d, BigRef rf, int in, int out) {   // red[0] = fix_obj, q = E2*x2; rank = the new live rank
    if (blockIdx.x < d.Gl)
        for (int s = 0; s < d.EPTl; s++) {
            const int i = blockIdx.x * (T * d.EPTl) + s * T + threadIdx.x;
            if (i < d.l) d.f[i] = d.f[i] - d.q[i];                                  // f1 = f - E2*x2 (:1278)
        }
    if (LEADER) { d.st[out] = d.st[in]; d.st[out].fix_obj = red_of(d, BIG_PH_X, 0); }
    if (blockIdx.x >= d.G) return;
    double *sx = stg<BIG_PH_X>(d, rf, 0);
    for (int q = 0; q < d.EPT; q++) {
        const int j = blockIdx.x * (T * d.EPT) + q * T + threadIdx.x;
        if (j >= d.n_loc) continue;
        const int nf = d.newfix[j];
        if (nf) { d.live[j] = 0; d.x[j] = nf == 2 ? 1.0 : 0.0; }
        else if (d.live[j]) { const double x = d.x[j]; sx[rf.rank[j]] = x * x; }
    }
}

// VALUED only: big_k_fix3 with update_expression on the stored values (:1329 -> :2289-2404)
__global__ void __launch_bounds__(T) bigref_k_fix3_v(BigDev d, BigRef rf, int in, int out, long n_live_new, double c1_new) {
    const BigState *si = d.st + in;
    const double rho1 = si->rho1, rho2 = si->rho2, rho4 = si->rho4;
    if (LEADER) {
        d.st[out] = *si;
        BigState *s = d.st + out;
        s->n_live_lo = (int)(n_live_new & 0x7fffffff); s->n_live_hi = (int)(n_live_new >> 31);
        if (n_live_new == 0) { s->ret = 1; s->stop = LP_STOP_ALLFIXED; s->halt = BIG_HALT_STOP; }
        else {
            if (sqrt(red_of(d, BIG_PH_X, 0)) < 1e-3) s->ret = 1;                                    // :1223
            s->prev_sum = s->sum_fix_obj; s->sum_fix_obj += s->fix_obj; s->prev_obj = s->cur_obj;   // :1247-1250
            s->c1 = c1_new;
            double dI = 0.0; dI += rho1 + rho2;
            s->dI = dI; s->r4Et = rho4; s->expr_ready = 1;
        }
    }
    if (n_live_new == 0) return;
    double dI = 0.0; dI += rho1 + rho2;
    for (int q = 0; q < d.EPT; q++) {
        const int j = blockIdx.x * (T * d.EPT) + q * T + threadIdx.x;
        if (j >= d.n_loc) continue;
        double Esq = 0.0;
        for (int k = d.cptr[j]; k < d.cptr[j + 1]; k++) { const double v = rf.vcsc[k]; Esq += v * v; rf.r4v[k] = rho4 * v; }
        double pd = dI;
        pd += rho4 * Esq;
        d.pd[j] = pd;
        d.dinv[j] = (pd != 0.0) ? 1.0 / pd : 1.0;
        d.gsrc[j] = d.live[j] ? d.x[j] : 0.0;
    }
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
#define REF_LAUNCH(kernel, grid, ...)                                                                         \
    do {                                                                                                      \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(T), 0, s, d, rf, *parity, *parity ^ 1, ##__VA_ARGS__);    \
        *parity ^= 1;                                                                                         \
    } while (0)

hipError_t bigref_launch_rank(const BigDev &d, const BigRef &rf, int mode, hipStream_t s) {
    hipLaunchKernelGGL(bigref_k_rank, dim3(1), dim3(T), 0, s, d, rf, mode);
    return hipGetLastError();
}
hipError_t bigref_launch_walk(const BigDev &d, const BigRef &rf, int nv, int phase, int which, int sidx, hipStream_t s) {
    if (nv < 1 || nv > BIG_REF_MAXV) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bigref_k_walk, dim3(1), dim3(T), 0, s, d, rf, nv, big_ref_stage_off(phase), phase * BIG_NPART, which, sidx,
                       (phase == BIG_PH_C || phase == BIG_PH_D) ? 1 : 0);
    return hipGetLastError();
}
hipError_t bigref_launch_init(const BigDev &d, const BigRef &rf, double c1, hipStream_t s) {
    hipLaunchKernelGGL(bigref_k_init, dim3(d.G > d.Gl ? d.G : d.Gl), dim3(T), 0, s, d, rf, c1);
    return hipGetLastError();
}
hipError_t bigref_launch_fix1(const BigDev &d, const BigRef &rf, hipStream_t s) {
    hipLaunchKernelGGL(bigref_k_fix1, dim3(d.G), dim3(T), 0, s, d, rf);
    return hipGetLastError();
}
hipError_t bigref_launch_fix2(const BigDev &d, const BigRef &rf, int *parity, hipStream_t s) { REF_LAUNCH(bigref_k_fix2, (d.G > d.Gl ? d.G : d.Gl)); return hipGetLastError(); }
hipError_t bigref_launch_fix3(const BigDev &d, const BigRef &rf, long n_live_new, double c1_new, int *parity, hipStream_t s) {
    if (!rf.valued) return big_launch_fix3(d, n_live_new, c1_new, parity, s);
    REF_LAUNCH(bigref_k_fix3_v, d.G, n_live_new, c1_new);
    return hipGetLastError();
}
hipError_t bigref_launch_prep(const BigDev &d, const BigRef &rf, int do_prep, int *parity, hipStream_t s) { REF_LAUNCH(bigref_k_prep, d.G, do_prep); return hipGetLastError(); }
hipError_t bigref_launch_y(const BigDev &d, const BigRef &rf, int *parity, hipStream_t s) {
    if (!rf.valued) return big_launch_y(d, parity, s);
    REF_LAUNCH(bigref_k_y_v, (d.G > d.Gl ? d.G : d.Gl));
    return hipGetLastError();
}
hipError_t bigref_launch_rhs_cols(const BigDev &d, const BigRef &rf, int *parity, hipStream_t s) {
    if (!rf.valued) return big_launch_rhs_cols(d, parity, s);
    REF_LAUNCH(bigref_k_rhs_cols_v, d.G);
    return hipGetLastError();
}
hipError_t bigref_launch_rows(const BigDev &d, const BigRef &rf, int mode, int *parity, hipStream_t s) {
    if (!rf.valued) return big_launch_rows(d, mode, parity, s);
    REF_LAUNCH(bigref_k_rows_v, d.Gl, mode);
    return hipGetLastError();
}
hipError_t bigref_launch_resid(const BigDev &d, const BigRef &rf, int *parity, hipStream_t s) {
    if (rf.valued) REF_LAUNCH(bigref_k_resid<true>, d.G); else REF_LAUNCH(bigref_k_resid<false>, d.G);
    return hipGetLastError();
}
hipError_t bigref_launch_pcg_cols(const BigDev &d, const BigRef &rf, int *parity, hipStream_t s) {
    if (rf.valued) REF_LAUNCH(bigref_k_pcg_cols<true>, d.G); else REF_LAUNCH(bigref_k_pcg_cols<false>, d.G);
    return hipGetLastError();
}
hipError_t bigref_launch_pcg_upd(const BigDev &d, const BigRef &rf, int *parity, hipStream_t s) { REF_LAUNCH(bigref_k_pcg_upd, d.G); return hipGetLastError(); }
hipError_t bigref_launch_post(const BigDev &d, const BigRef &rf, int *parity, hipStream_t s) { REF_LAUNCH(bigref_k_post, d.G); return hipGetLastError(); }
