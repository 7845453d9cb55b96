// lpbox_seg_ref_kernels.hip -- gfx950 kernels of the SEGMENTATION flavour in the REFERENCE's summation order
// (lpbox_seg_set_order(LPBOX_ORDER_REFERENCE); specification: oracle/seg_oracle.c with order_mode 0, i.e. Eigen 3.3.8's SSE2 redux over
// the reference's COMPACTED live vector).  DESIGN.md section 33.
//
// The chain is the one of lpbox_seg_kernels.hip with a walker behind every producer of a sum:
//   [prep, walk A]  yrhs  resid, walk B   k x (matvec, walk C, update, walk D)   post, walk E+A   ...   [prep (finalise only)]
//   * a producer writes ONE term per live variable, formed as the oracle's dot() forms it (the rounded product), to
//     stage[row][rank[i]], where rank[i] is the variable's position among the live ones (segr_k_rank: at init and after every fix);
//     it adds nothing: no LDS, no barrier;
//   * the walker (one workgroup per problem) adds the rows up in Eigen's redux association and leaves the totals in red[row]; the
//     consumers read them as scalars where the default order's kernels recompute the second level of their tree (final_sums);
//   * the walker returns at once when its producer fell through (a halted chain, a finished PCG, a stopped member of a batch), so
//     red[] keeps what a resumed PCG needs.
// The state kernels (init, set_window, resume, fix, decide, compact, pack, collect) are those of lpbox_seg_kernels.hip: they sum
// nothing over the variables.  That file is untouched; the row product, the scalar decisions of an iteration (finalise_state,
// close_or_continue) and the per-variable expressions of the six bodies are DUPLICATED here in their generic (one row at a time) form.
#include "lpbox_seg.h"

#include <float.h>

namespace {

constexpr int T = SEG_T;
#define LEADER (blockIdx.x == 0 && threadIdx.x == 0)

__device__ __forceinline__ void forward_state(const SegDev &d, int in, int out) {
    if (LEADER) d.st[out] = d.st[in];
}
__device__ __forceinline__ double *stg(const SegDev &d, const SegRef &rf, int row) { return rf.stage + (size_t)row * (size_t)d.n; }

// ---- the row product of lpbox_seg_kernels.hip (ell_load / ell_sum / tm_row), one row at a time ----
struct EllRow { int len; double tdi; int c[8]; double v[8]; };
__device__ __forceinline__ void ell_load(const SegDev &d, int i, EllRow &R) {
    R.tdi = d.td[i];
    if (d.dia) {
        const unsigned long long pk = d.dpack[i];
        const double aii = d.adiag[i];
        const int other = i ? i - 1 : 1;
        R.len = 7;
#pragma unroll
        for (int k = 0; k < 7; k++) {
            if (k == 3) { R.c[k] = i; R.v[k] = aii; continue; }
            const int s = k < 3 ? k : k - 1;
            const int ci = i + d.doff[k];
            R.c[k] = (unsigned)ci < (unsigned)d.n ? ci : other;
            R.v[k] = -(double)(unsigned)((pk >> (8 * s)) & 255ull);
        }
        R.c[7] = i; R.v[7] = 0.0;
        return;
    }
    R.len = d.rowlen[i];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const bool in = k < d.ell_w;
        R.c[k] = in ? d.ecol[(size_t)k * d.n + i] : i;
        R.v[k] = in ? d.eval[(size_t)k * d.n + i] : 0.0;
    }
}
__device__ __forceinline__ double ell_sum(const EllRow &R, int i, const double (&g)[8]) {
    double tmp = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) if (k < R.len) tmp += ((R.c[k] == i) ? R.tdi : 2 * R.v[k]) * g[k];
    double res = 0.0;
    res += 1.0 * tmp;
    return res;
}
// (2A + (rho1+rho2) I) row i times a gathered vector, ascending columns from +0.0 (SEGcpp:784-786): the oracle's order in both modes
template <typename GET>
__device__ __forceinline__ double tm_row(const SegDev &d, int i, GET get) {
    double tmp = 0;
    if (d.ell_w <= 8) {
        EllRow R;
        ell_load(d, i, R);
        double g[8];
#pragma unroll
        for (int k = 0; k < 8; k++) g[k] = get(R.c[k]);
        return ell_sum(R, i, g);
    } else {
        const int len = d.rowlen[i];
        const double tdi = d.td[i];
        for (int k = 0; k < len; k++) {
            const int c = d.ecol[(size_t)k * d.n + i];
            const double val = (c == i) ? tdi : 2 * d.eval[(size_t)k * d.n + i];
            tmp += val * get(c);
        }
    }
    double res = 0.0;
    res += 1.0 * tmp;
    return res;
}

// ---- live rank: one workgroup per problem, a block prefix sum per chunk of T * RE variables with a carried offset ----
constexpr int RE = 4;
__device__ __forceinline__ void segr_b_rank(const SegDev &d, const SegRef &rf) {
    __shared__ int wsum[T / 64 + 1];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int carried = 0;
    for (int base = 0; base < d.n; base += T * RE) {
        int keep[RE], c = 0;
#pragma unroll
        for (int k = 0; k < RE; k++) {
            const int j = base + threadIdx.x * RE + k;
            keep[k] = (j < d.n && d.live[j]) ? 1 : 0;
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
            if (j < d.n) rf.rank[j] = keep[k] ? pos++ : -1;
        }
        carried += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) rf.cnt[0] = carried;
}

// ---- the walker: Eigen 3.3.8 redux (SSE2 packets) over the staged terms of up to SEG_REF_MAXV rows at once ----
// Lane 4 v + c of wave 0 walks chain c of row v: a[c], + a[c + 4], + a[c + 8], ... over the part of the vector that is a multiple of four
// long.  The whole workgroup brings the operands in: tile t + 1 is loaded (coalesced) into registers before tile t is walked from LDS
// and stored to the other LDS buffer after it.  Lane v then combines (p0a + p1a) + (p0b + p1b), the left-over pair and the odd last
// element; sizes 1-3 take the short branches.  Every walk is bounded by the live count; nothing is padded.
// pcg: the producer was matvec / update (falls through on a finished PCG as well).
constexpr int WTILE = 1024, WROW = WTILE + 4, WU = WTILE / T;
__device__ __forceinline__ void segr_b_walk(const SegDev &d, const SegRef &rf, int nv, int row0, int sidx, int pcg) {
    __shared__ double tile[2][SEG_REF_MAXV][WROW];
    __shared__ double fin[SEG_REF_MAXV][4];
    const SegState *si = d.st + sidx;
    if (si->halt || (pcg && (si->pcg_done || si->phase != 2))) return;      // the producer fell through: red[] keeps what it holds
    int size = rf.cnt[0];
    if (size > d.n) size = d.n;
    const int aS2 = (size / 4) * 4, aS = (size / 2) * 2;
    const double *base = stg(d, rf, row0);
    const int ntiles = (aS2 + WTILE - 1) / WTILE;
    const int lane = threadIdx.x, wv = lane >> 2, wc = lane & 3;
    const bool walker = lane < nv * 4;
    double acc = 0.0, pre[SEG_REF_MAXV][WU];
    auto load = [&](int t) {
#pragma unroll
        for (int v = 0; v < SEG_REF_MAXV; v++)
#pragma unroll
            for (int u = 0; u < WU; u++) {
                const int idx = t * WTILE + u * T + lane;
                pre[v][u] = (v < nv && idx < aS2) ? base[(size_t)v * d.n + idx] : 0.0;
            }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int v = 0; v < SEG_REF_MAXV; v++)
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
        const double *a = base + (size_t)lane * d.n;
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
        rf.red[row0 + lane] = res;
    }
}

// ---- the scalar decisions of an iteration (SEGcpp:1122-1180 / :1277-1376), as in lpbox_seg_kernels.hip; the totals come from red[] ----
__device__ __forceinline__ void finalise_state(SegState *s, const double *e, const double *e2) {
    const int it = s->iter;
    s->have_prev = 0;
    const double xn = sqrt(e[0]);
    const double t0 = xn < 2.2204e-16 ? 2.2204e-16 : xn;
    s->cvg1 = sqrt(e[1]) / t0; s->cvg2 = sqrt(e[2]) / t0;
    const double bin_cost = e2[0] + e2[1];                       // compute_cost(round(x)) (:1167 / :1372)
    bool stopped = false;
    if (s->cvg1 <= SEG_STOP_THRESHOLD && s->cvg2 <= SEG_STOP_THRESHOLD) {   // :1127 / :1282
        if (s->l2f) s->ret = 1;
        s->stop = SEG_STOP_XYY; stopped = true;
    } else {
        if ((it + 1) % SEG_RHO_STEP == 0) {                      // :1137-1145
            s->prev_rho1 = s->rho1; s->prev_rho2 = s->rho2;
            s->rho1 = SEG_LEARNING_FACT * s->rho1; s->rho2 = SEG_LEARNING_FACT * s->rho2;
            const double g = s->gamma_val * SEG_GAMMA_FACTOR;
            s->gamma_val = g < 1.0 ? 1.0 : g;
            s->rhoUpdated = 1; s->rcr = SEG_LEARNING_FACT - 1.0;
        }
        s->obj_val = e[3] + e[4];                                // compute_cost(x) (:1148)
        int hn = s->hist_n;
        if (hn < SEG_HIST) s->hist[hn] = s->obj_val;
        else { for (int k = 0; k < SEG_HIST - 1; k++) s->hist[k] = s->hist[k + 1]; s->hist[SEG_HIST - 1] = s->obj_val; }
        if (hn < 0x3fffffff) hn++;
        s->hist_n = hn;
        if (hn >= SEG_HIST) {
            double mean = 0;
            for (int k = 0; k < SEG_HIST; k++) mean += s->hist[k];
            mean /= (double)SEG_HIST;
            double dev = 0;
            for (int k = 0; k < SEG_HIST; k++) dev += (s->hist[k] - mean) * (s->hist[k] - mean);
            dev /= (double)(SEG_HIST - 1);
            const double sd = dev == 0 ? 0.0 : sqrt(dev);        // the reference's pow(v, 1/2): within 2 ulps (DESIGN.md sections 18, 21)
            s->std_obj = sd / fabs(s->hist[SEG_HIST - 1]);
        }
        if (s->std_obj <= SEG_STD_THRESHOLD) { if (s->l2f) s->ret = 1; s->stop = SEG_STOP_OBJSTD; stopped = true; }
        else {
            s->cur_obj = bin_cost;
            if (s->best_bin_obj >= s->cur_obj) s->best_bin_obj = s->cur_obj;
        }
    }
    if (stopped) {
        s->halt = SEG_HALT_STOP;
        if (!s->l2f) { s->cur_obj = bin_cost; s->legacy_iter_p1 = it + 1; }   // legacy epilogue (:1371-1376)
    } else s->iter = it + 1;
}
__device__ __forceinline__ void close_or_continue(SegState *s, int do_prep) {
    if (!s->halt && s->iter >= s->iter_end) { s->halt = SEG_HALT_WINDOW; if (!s->l2f) s->legacy_iter_p1 = s->iter + 1; }
    if (!s->halt && do_prep) s->phase = 1;
}

#define SEGR_ROWS(i)                                                                  \
    for (int q_ = 0, i; q_ < d.EPT; q_++)                                             \
        if ((i = blockIdx.x * (T * d.EPT) + q_ * T + threadIdx.x) < d.n && d.live[i])

// prep: finalise the previous iteration if that is pending (thread 0 of workgroup 0, from red[]), then the terms of ||x+z2/rho2-1/2||^2
__device__ __forceinline__ void segr_b_prep(const SegDev &d, const SegRef &rf, int in, int out, int do_prep) {
    const SegState *si = d.st + in;
    const int halt0 = si->halt, have_prev = si->have_prev, it = si->iter, iter_end = si->iter_end;
    double rho2 = si->rho2;
    const bool fin = !halt0 && have_prev;
    if (fin && (it + 1) % SEG_RHO_STEP == 0) rho2 = SEG_LEARNING_FACT * rho2;
    const int next_iter = fin ? it + 1 : it;
    const bool will_prep = do_prep && !halt0 && next_iter < iter_end;
    if (LEADER) {
        d.st[out] = *si;
        SegState *s = d.st + out;
        if (fin) finalise_state(s, rf.red + SEG_REF_E, rf.red + SEG_REF_E + 5);
        close_or_continue(s, do_prep);
    }
    if (!will_prep) return;
    double *sa = stg(d, rf, SEG_REF_A);
    SEGR_ROWS(i) { const double u = (d.x[i] + d.z2[i] / rho2) - 0.5; sa[rf.rank[i]] = u * u; }
}

__device__ __forceinline__ void segr_b_yrhs(const SegDev &d, const SegRef &rf, int in, int out) {
    const SegState *si = d.st + in;
    if (si->halt) { forward_state(d, in, out); return; }
    // inside a batch of iterations the previous one is still to be finalised: every workgroup does that for itself from the same
    // totals, on a copy of the state in LDS; workgroup 0 publishes it
    __shared__ SegState fst;
    if (si->have_prev) {                                                     // uniform over the grid
        if (threadIdx.x == 0) { fst = *si; finalise_state(&fst, rf.red + SEG_REF_E, rf.red + SEG_REF_E + 5); close_or_continue(&fst, 1); }
        __syncthreads();
        si = &fst;
        if (si->halt) { if (LEADER) d.st[out] = fst; return; }
    }
    const double rho1 = si->rho1, rho2 = si->rho2, c1 = si->c1;
    const int rhoUpdated = si->rhoUpdated, stale = si->dinv_stale;
    const bool refresh = si->iter != 0 && rhoUpdated;
    const double inc = (si->prev_rho1 + si->prev_rho2) * si->rcr;            // :1086
    const double c2 = 2 * sqrt(rf.red[SEG_REF_A]);
    SEGR_ROWS(i) {
        const double x = d.x[i], z1 = d.z1[i], z2 = d.z2[i];
        const double t = x + z1 / rho1;
        const double y1 = t > 1 ? 1 : (t < 0 ? 0 : t);
        double y2 = (x + z2 / rho2) - 0.5;
        y2 = y2 * c1 / c2 + 0.5;
        d.y1[i] = y1; d.y2[i] = y2;
        double td = d.td[i];
        if (refresh) { td += inc; d.td[i] = td; }
        if (rhoUpdated || stale) d.dinv[i] = td != 0.0 ? 1.0 / td : 1.0;    // DiagonalPreconditioner::compute (:1098-1101)
        d.rhs[i] = (rho1 * y1 + rho2 * y2) - ((d.b[i] + z1) + z2);           // :1091
        d.x[i] = y1;                                                         // x_sol = y1 (:1104)
    }
    if (LEADER) { d.st[out] = *si; d.st[out].rhoUpdated = 0; d.st[out].dinv_stale = 0; }
}

__device__ __forceinline__ void segr_b_resid(const SegDev &d, const SegRef &rf, int in, int out) {
    const SegState *si = d.st + in;
    if (si->halt) { forward_state(d, in, out); return; }
    const double *x = d.x;
    double *s0 = stg(d, rf, SEG_REF_B), *s1 = s0 + d.n, *s2 = s1 + d.n;
    SEGR_ROWS(i) {
        const double Mx = tm_row(d, i, [x](int c) { return x[c]; });
        const double rhs = d.rhs[i];
        const double r = rhs - Mx;                                            // :263
        const double p = d.dinv[i] * r;                                       // :286
        d.r[i] = r; d.p0[i] = p;
        const int k = rf.rank[i];
        s0[k] = rhs * rhs; s1[k] = r * r; s2[k] = r * p;
    }
    if (LEADER) { d.st[out] = *si; d.st[out].pcg_k = 0; d.st[out].pcg_done = 0; d.st[out].phase = 2; }
}

// tmp = M p with the search-direction update of the previous PCG iteration folded in
__device__ __forceinline__ void segr_b_matvec(const SegDev &d, const SegRef &rf, int in, int out) {
    const SegState *si = d.st + in;
    if (si->halt || si->pcg_done || si->phase != 2) { forward_state(d, in, out); return; }
    const int pcg_k = si->pcg_k;
    double threshold = si->threshold, absNew = si->absNew, rhsNorm2 = si->rhsNorm2;
    double beta = 0.0;
    const bool first = pcg_k == 0;
    bool done = false, zero_x = false;
    const double *pold = ((pcg_k - 1) & 1) ? d.p1 : d.p0;
    const double *zz = d.z;
    if (first) {
        const double *b3 = rf.red + SEG_REF_B;
        rhsNorm2 = b3[0];
        if (rhsNorm2 == 0) { done = true; zero_x = true; }                   // :265-271
        else {
            double thr = SEG_PCG_TOL * SEG_PCG_TOL * rhsNorm2;               // :274
            if (thr < DBL_MIN) thr = DBL_MIN;
            threshold = thr;
            if (b3[1] < thr) done = true;                                     // :277
            absNew = b3[2];
        }
    } else {
        const double *d2 = rf.red + SEG_REF_D;
        if (d2[0] < threshold || pcg_k >= SEG_PCG_MAXITERS) done = true;     // :304-307
        else { const double absOld = absNew; absNew = d2[1]; beta = absNew / absOld; }   // :311-313
    }
    if (LEADER) {
        d.st[out] = *si;
        SegState *s = d.st + out;
        s->threshold = threshold; s->absNew = absNew; s->rhsNorm2 = rhsNorm2; s->pcg_done = done ? 1 : 0;
    }
    if (done) {
        if (zero_x)
            for (int q = 0; q < d.EPT; q++) { const int i = blockIdx.x * (T * d.EPT) + q * T + threadIdx.x; if (i < d.n) d.x[i] = 0.0; }
        return;
    }
    double *pnew = (pcg_k & 1) ? d.p1 : d.p0;
    double *sc = stg(d, rf, SEG_REF_C);
    SEGR_ROWS(i) {
        double Mp, pi;
        if (first) {
            pi = d.p0[i];
            const double *p0 = d.p0;
            Mp = tm_row(d, i, [p0](int c2) { return p0[c2]; });
        } else {
            pi = zz[i] + beta * pold[i];                                       // p = z + beta p (:314)
            Mp = tm_row(d, i, [zz, pold, beta](int c2) { return zz[c2] + beta * pold[c2]; });
            pnew[i] = pi;
        }
        d.tmp[i] = Mp;
        sc[rf.rank[i]] = pi * Mp;
    }
}

__device__ __forceinline__ void segr_b_update(const SegDev &d, const SegRef &rf, int in, int out) {
    const SegState *si = d.st + in;
    if (si->halt || si->pcg_done || si->phase != 2) { forward_state(d, in, out); return; }
    const int pcg_k = si->pcg_k;
    const double *p = (pcg_k & 1) ? d.p1 : d.p0;
    const double alpha = si->absNew / rf.red[SEG_REF_C];                      // :295
    double *s0 = stg(d, rf, SEG_REF_D), *s1 = s0 + d.n;
    SEGR_ROWS(i) {
        double x = d.x[i], r = d.r[i];
        x += alpha * p[i];                                                    // :297
        r -= alpha * d.tmp[i];                                                // :299
        const double z = d.dinv[i] * r;                                       // :309
        d.x[i] = x; d.r[i] = r; d.z[i] = z;
        const int k = rf.rank[i];
        s0[k] = r * r; s1[k] = r * z;
    }
    if (LEADER) { d.st[out] = *si; d.st[out].pcg_k = pcg_k + 1; }
}

__device__ __forceinline__ void segr_b_post(const SegDev &d, const SegRef &rf, int in, int out) {
    const SegState *si = d.st + in;
    if (si->halt || si->phase != 2) { forward_state(d, in, out); return; }
    const int pcg_k = si->pcg_k, rec = si->rec, cc = si->cc;
    if (!si->pcg_done) {                   // the exit test of the last update is still pending
        const double *d2 = rf.red + SEG_REF_D;
        if (!(pcg_k >= 1 && (d2[0] < si->threshold || pcg_k >= SEG_PCG_MAXITERS))) {
            if (LEADER) { d.st[out] = *si; d.st[out].halt = SEG_HALT_PCG_MORE; }
            return;
        }
    }
    const double g1 = si->gamma_val * si->rho1, g2 = si->gamma_val * si->rho2;
    const double rho2n = (si->iter + 1) % SEG_RHO_STEP == 0 ? SEG_LEARNING_FACT * si->rho2 : si->rho2;   // the rho2 of the NEXT iteration
    const double *x = d.x;
    double *xh = (rec && cc < d.ws_cap) ? d.xhist + (size_t)cc * d.n : nullptr;
    double *se = stg(d, rf, SEG_REF_E), *sa = stg(d, rf, SEG_REF_A);
    const size_t n = (size_t)d.n;
    SEGR_ROWS(i) {
        const double xi = x[i], y1 = d.y1[i], y2 = d.y2[i], bi = d.b[i];
        d.z1[i] = d.z1[i] + g1 * (xi - y1);                               // :1119-1120
        const double z2n = d.z2[i] + g2 * (xi - y2);
        d.z2[i] = z2n;
        const double u = (xi + z2n / rho2n) - 0.5;                         // next iteration's ||x + z2/rho2 - 1/2||^2 (:1075-1080)
        if (xh) xh[i] = xi;                                               // x_iters column (:1113-1116)
        // A x and A round(x) in one pass over the row (compute_cost :568-572, A_ptr restricted to the live variables)
        double t1 = 0, t2 = 0;
        if (d.ell_w <= 8) {
            EllRow Rr;
            ell_load(d, i, Rr);
            double xc[8];
#pragma unroll
            for (int k = 0; k < 8; k++) xc[k] = x[Rr.c[k]];
#pragma unroll
            for (int k = 0; k < 8; k++) if (k < Rr.len) { t1 += Rr.v[k] * xc[k]; t2 += Rr.v[k] * (xc[k] >= 0.5 ? 1.0 : 0.0); }
        } else {
            const int len = d.rowlen[i];
            for (int k = 0; k < len; k++) {
                const int c = d.ecol[(size_t)k * d.n + i];
                const double xc = x[c], a = d.eval[(size_t)k * d.n + i];
                t1 += a * xc;
                t2 += a * (xc >= 0.5 ? 1.0 : 0.0);                       // fixed variables hold x = 0
            }
        }
        double Ax = 0.0; Ax += 1.0 * t1;
        double Axb = 0.0; Axb += 1.0 * t2;
        const double xb = xi >= 0.5 ? 1.0 : 0.0;
        const double d1 = xi - y1, d2 = xi - y2;
        const int k = rf.rank[i];
        se[k] = xi * xi; se[n + k] = d1 * d1; se[2 * n + k] = d2 * d2; se[3 * n + k] = xi * Ax; se[4 * n + k] = bi * xi;
        se[5 * n + k] = xb * Axb; se[6 * n + k] = bi * xb;
        sa[k] = u * u;
    }
    if (LEADER) {
        d.st[out] = *si;
        SegState *s = d.st + out;
        s->pcg_done = 1; s->last_pcg = pcg_k; s->pcg_total += pcg_k; s->outer_total++;
        if (pcg_k > s->pcg_max) s->pcg_max = pcg_k;
        if (rec) s->cc = cc + 1;
        s->have_prev = 1; s->phase = 0;
    }
}

// entry points: one problem (descriptors by value) / a batch in lockstep (descriptor arrays, blockIdx.y = member; workgroups beyond a
// member's own count leave at once; one walker and one rank pass per member, grid (1, B))
#define KB_MEMBER                                     \
    const SegDev &d = devs[blockIdx.y];               \
    if ((int)blockIdx.x >= d.G) return;               \
    const SegRef &rf = refs[blockIdx.y]
__global__ void __launch_bounds__(T) segr_k_rank(SegDev d, SegRef rf) { segr_b_rank(d, rf); }
__global__ void __launch_bounds__(T) segr_kb_rank(const SegDev *devs, const SegRef *refs) { segr_b_rank(devs[blockIdx.y], refs[blockIdx.y]); }
__global__ void __launch_bounds__(T) segr_k_walk(SegDev d, SegRef rf, int nv, int row0, int sidx, int pcg) { segr_b_walk(d, rf, nv, row0, sidx, pcg); }
__global__ void __launch_bounds__(T) segr_kb_walk(const SegDev *devs, const SegRef *refs, int nv, int row0, int sidx, int pcg) { segr_b_walk(devs[blockIdx.y], refs[blockIdx.y], nv, row0, sidx, pcg); }
__global__ void __launch_bounds__(T) segr_k_prep(SegDev d, SegRef rf, int in, int out, int do_prep) { segr_b_prep(d, rf, in, out, do_prep); }
__global__ void __launch_bounds__(T) segr_kb_prep(const SegDev *devs, const SegRef *refs, int in, int out, int do_prep) { KB_MEMBER; segr_b_prep(d, rf, in, out, do_prep); }
__global__ void __launch_bounds__(T) segr_k_yrhs(SegDev d, SegRef rf, int in, int out) { segr_b_yrhs(d, rf, in, out); }
__global__ void __launch_bounds__(T) segr_kb_yrhs(const SegDev *devs, const SegRef *refs, int in, int out) { KB_MEMBER; segr_b_yrhs(d, rf, in, out); }
__global__ void __launch_bounds__(T) segr_k_resid(SegDev d, SegRef rf, int in, int out) { segr_b_resid(d, rf, in, out); }
__global__ void __launch_bounds__(T) segr_kb_resid(const SegDev *devs, const SegRef *refs, int in, int out) { KB_MEMBER; segr_b_resid(d, rf, in, out); }
__global__ void __launch_bounds__(T) segr_k_matvec(SegDev d, SegRef rf, int in, int out) { segr_b_matvec(d, rf, in, out); }
__global__ void __launch_bounds__(T) segr_kb_matvec(const SegDev *devs, const SegRef *refs, int in, int out) { KB_MEMBER; segr_b_matvec(d, rf, in, out); }
__global__ void __launch_bounds__(T) segr_k_update(SegDev d, SegRef rf, int in, int out) { segr_b_update(d, rf, in, out); }
__global__ void __launch_bounds__(T) segr_kb_update(const SegDev *devs, const SegRef *refs, int in, int out) { KB_MEMBER; segr_b_update(d, rf, in, out); }
__global__ void __launch_bounds__(T) segr_k_post(SegDev d, SegRef rf, int in, int out) { segr_b_post(d, rf, in, out); }
__global__ void __launch_bounds__(T) segr_kb_post(const SegDev *devs, const SegRef *refs, int in, int out) { KB_MEMBER; segr_b_post(d, rf, in, out); }

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
// a producer flips the ping-pong index *parity; a walk flips nothing, and its state index is the parity where it is enqueued, i.e. the
// state its producer has just written
#define SEGR_LAUNCH(kernel, ...)                                                                             \
    do {                                                                                                     \
        hipLaunchKernelGGL(kernel, dim3(d.G), dim3(T), 0, s, d, rf, *parity, *parity ^ 1, ##__VA_ARGS__);    \
        *parity ^= 1;                                                                                        \
    } while (0)
#define SEGR_WALK(nv, row0, pcg) hipLaunchKernelGGL(segr_k_walk, dim3(1), dim3(T), 0, s, d, rf, nv, row0, *parity, pcg)

hipError_t segr_launch_rank(const SegDev &d, const SegRef &rf, hipStream_t s) {
    hipLaunchKernelGGL(segr_k_rank, dim3(1), dim3(T), 0, s, d, rf);
    return hipGetLastError();
}
hipError_t segr_enqueue_prep(const SegDev &d, const SegRef &rf, int *parity, hipStream_t s) {
    SEGR_LAUNCH(segr_k_prep, 1);
    SEGR_WALK(1, SEG_REF_A, 0);
    return hipGetLastError();
}
static void segr_pcg_pairs(const SegDev &d, const SegRef &rf, int pairs, int *parity, hipStream_t s) {
    for (int k = 0; k < pairs; k++) {
        SEGR_LAUNCH(segr_k_matvec);
        SEGR_WALK(1, SEG_REF_C, 1);
        SEGR_LAUNCH(segr_k_update);
        SEGR_WALK(2, SEG_REF_D, 1);
    }
    SEGR_LAUNCH(segr_k_post);
    SEGR_WALK(8, SEG_REF_E, 0);                      // the seven sums of the iteration and the sphere norm of the next one
}
hipError_t segr_enqueue_iterations(const SegDev &d, const SegRef &rf, int iters, int kmax, int *parity, hipStream_t s) {
    for (int it = 0; it < iters; it++) {
        SEGR_LAUNCH(segr_k_yrhs);
        SEGR_LAUNCH(segr_k_resid);
        SEGR_WALK(3, SEG_REF_B, 0);
        segr_pcg_pairs(d, rf, kmax, parity, s);
    }
    return hipGetLastError();
}
hipError_t segr_enqueue_pcg_more(const SegDev &d, const SegRef &rf, int pairs, int *parity, hipStream_t s) {
    hipError_t e = seg_launch_copy(d, 0, parity, s);           // SEG_HALT_PCG_MORE -> none
    if (e != hipSuccess) return e;
    segr_pcg_pairs(d, rf, pairs, parity, s);
    return hipGetLastError();
}
hipError_t segr_enqueue_finalize(const SegDev &d, const SegRef &rf, int *parity, hipStream_t s) {
    SEGR_LAUNCH(segr_k_prep, 0);
    return hipGetLastError();
}

// ---- the same launch sequences for a batch in lockstep ----
#define SEGRB_LAUNCH(kernel, ...)                                                                                  \
    do {                                                                                                           \
        hipLaunchKernelGGL(kernel, dim3(Gmax, B), dim3(T), 0, s, devs, refs, *parity, *parity ^ 1, ##__VA_ARGS__);  \
        *parity ^= 1;                                                                                              \
    } while (0)
#define SEGRB_WALK(nv, row0, pcg) hipLaunchKernelGGL(segr_kb_walk, dim3(1, B), dim3(T), 0, s, devs, refs, nv, row0, *parity, pcg)

hipError_t segrb_launch_rank(const SegDev *devs, const SegRef *refs, int B, hipStream_t s) {
    hipLaunchKernelGGL(segr_kb_rank, dim3(1, B), dim3(T), 0, s, devs, refs);
    return hipGetLastError();
}
hipError_t segrb_enqueue_prep(const SegDev *devs, const SegRef *refs, int B, int Gmax, int *parity, hipStream_t s) {
    SEGRB_LAUNCH(segr_kb_prep, 1);
    SEGRB_WALK(1, SEG_REF_A, 0);
    return hipGetLastError();
}
static void segrb_pcg_pairs(const SegDev *devs, const SegRef *refs, int B, int Gmax, int pairs, int *parity, hipStream_t s) {
    for (int k = 0; k < pairs; k++) {
        SEGRB_LAUNCH(segr_kb_matvec);
        SEGRB_WALK(1, SEG_REF_C, 1);
        SEGRB_LAUNCH(segr_kb_update);
        SEGRB_WALK(2, SEG_REF_D, 1);
    }
    SEGRB_LAUNCH(segr_kb_post);
    SEGRB_WALK(8, SEG_REF_E, 0);
}
hipError_t segrb_enqueue_iterations(const SegDev *devs, const SegRef *refs, int B, int Gmax, int iters, int kmax, int *parity, hipStream_t s) {
    for (int it = 0; it < iters; it++) {
        SEGRB_LAUNCH(segr_kb_yrhs);
        SEGRB_LAUNCH(segr_kb_resid);
        SEGRB_WALK(3, SEG_REF_B, 0);
        segrb_pcg_pairs(devs, refs, B, Gmax, kmax, parity, s);
    }
    return hipGetLastError();
}
hipError_t segrb_enqueue_pcg_more(const SegDev *devs, const SegRef *refs, int B, int Gmax, int pairs, int *parity, hipStream_t s) {
    hipError_t e = segb_launch_copy(devs, B, 0, parity, s);
    if (e != hipSuccess) return e;
    segrb_pcg_pairs(devs, refs, B, Gmax, pairs, parity, s);
    return hipGetLastError();
}
hipError_t segrb_enqueue_finalize(const SegDev *devs, const SegRef *refs, int B, int Gmax, int *parity, hipStream_t s) {
    SEGRB_LAUNCH(segr_kb_prep, 0);
    return hipGetLastError();
}
