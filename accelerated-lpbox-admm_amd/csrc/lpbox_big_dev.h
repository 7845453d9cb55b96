// lpbox_big_dev.h -- the kernel BODIES of the large-instance LP chain, once for both summation orders: lpbox_big_kernels.hip (default
// order, one problem and the lockstep batch) and lpbox_big_ref_kernels.hip (the reference's order) hold entries and nothing of the
// arithmetic.  One definition per expression keeps the orders from drifting apart.  Same arithmetic as lp_window_kernel (LPcpp:766-1095,
// ADMM_lp_iters), cut into kernels at the grid-wide dependencies:
//   prep -> [fin] -> y -> rhs_cols -> rows -> [AR q] -> resid -> [fin] ->
//   K x { rows(p) -> [AR q] -> pcg_cols -> [fin] -> pcg_upd -> [fin] } -> post -> [fin] -> rows(x) -> [AR q] -> z4
// ([fin] = reduce the workgroup partials to red[]; on more than one rank the host all-reduces red[] / q after it.)
// The PCG search direction p = z + beta p is recomputed on the fly for the gathered columns inside rows(p) (bit-identical
// expression), so a PCG iteration needs no separate p-update launch.  Rows and columns are summed by one lane in ascending
// index order; no FMA contraction; IEEE divide / sqrt.
//
// A body is parametrised at compile time on two things:
//   S       where the terms of the phase's sums go (below): WgSums here, Staged in lpbox_big_ref_kernels.hip;
//   VALUED  the stored values of E and rho4_E_transpose per entry (sp.rf.vcsr / vcsc / r4v) instead of 1 and the scalar r4Et.
// Instantiated: (WgSums, unit), (Staged, unit), (Staged, valued).  The host refuses folded totals, the comm-lean PCG, column-sliced rows
// and more than one rank in the reference order, so those branches exist under S::wg_sums only.
#pragma once
#include "lpbox_big.h"
#include "lpbox_dev_common.h"

#include <float.h>

namespace {

constexpr int T = BIG_T;
#define LEADER (blockIdx.x == 0 && threadIdx.x == 0)

// Streamed once per launch (index lists, pointers, the n-vectors a column owns).  Measured: the non-temporal hint on these makes
// the chain SLOWER (1.52 -> 1.83 ms per iteration at n = 1e6: a lane's index run shares its 128-byte line with its neighbours'
// and with its own next loads, which the hint gives up), so it is a diagnostic knob only (LPBOX_BIG_NT).
#ifndef LPBOX_BIG_NT
template <typename V> __device__ __forceinline__ V ld_stream(const V *p) { return *p; }
template <typename V> __device__ __forceinline__ void st_stream(V *p, V v) { *p = v; }
#else
template <typename V> __device__ __forceinline__ V ld_stream(const V *p) { return __builtin_nontemporal_load(p); }
template <typename V> __device__ __forceinline__ void st_stream(V *p, V v) { __builtin_nontemporal_store(v, p); }
#endif

__device__ __forceinline__ void forward_state(const BigDev &d, int in, int out) {
    if (LEADER) d.st[out] = d.st[in];
}

// the extent of a problem's own launch (big_launch_*), per kernel: what a lockstep batch's entries (big_kb_*, bigref_kb_*) test blockIdx.x against
__device__ __forceinline__ int ext_cols(const BigDev &d) { return d.G; }
__device__ __forceinline__ int ext_y(const BigDev &d) { return d.G > d.Gl ? d.G : d.Gl; }
__device__ __forceinline__ int ext_rows(const BigDev &d) { return d.P > 1 ? d.Glr : d.Gl; }
__device__ __forceinline__ int ext_z4(const BigDev &d) { return d.Gl; }

// Workgroup partials of NV values -> d.part; big_k_fin reduces them to d.red in a launch of its own.  Measured alternative: the
// workgroup that arrives last (ticket counter, __threadfence before and after) reduces them inside the producing kernel -- 41
// launches per iteration fewer, but 3.05 instead of 1.52 ms per iteration at n = 1e6: a device-scope fence per workgroup writes the
// XCD's L2 back each time.  Dropped.
__device__ __forceinline__ double *part_ptr(const BigDev &d, int phase) { return d.part + (size_t)phase * BIG_NPART * d.Gs; }

template <int NV>
__device__ __forceinline__ void store_partials(const BigDev &d, int phase, double (&v)[NV], double *red, int &parity) {
    block_sum<T, NV>(v, red, parity);
    if (threadIdx.x == 0) {
        double *pp = part_ptr(d, phase);
#pragma unroll
        for (int k = 0; k < NV; k++) pp[(size_t)k * d.Gs + blockIdx.x] = v[k];
    }
}

// ---- where the terms of a phase's sums go ----
// A body that feeds a reduction of NV values opens `Sums<S, NV> acc(d, sp, phase)`, calls `acc.add(j, live, t0, ...)` once per step of
// its loop over the variables -- for a dead or out-of-range j with live == false and zero terms -- and ends with the uniform call
// `acc.flush(d, red, parity)`.  WgSums, the default order: NV per-thread partials from +0.0, every term added (the zeros too), the
// workgroup tree and one partial per workgroup and value (store_partials).  wg_sums also marks what only this order has.
template <class S, int NV> using Sums = typename S::template Acc<NV>;

struct WgSums {
    static constexpr bool wg_sums = true;
    template <int NV> struct Acc {
        double v[NV];
        const int phase;
        __device__ __forceinline__ Acc(const BigDev &, const WgSums &, int ph) : phase(ph) {
#pragma unroll
            for (int k = 0; k < NV; k++) v[k] = 0.0;
        }
        template <typename... D> __device__ __forceinline__ void add(int, bool, D... t) {
            static_assert(sizeof...(D) == NV, "one term per value");
            const double a[NV] = {t...};
#pragma unroll
            for (int k = 0; k < NV; k++) v[k] = v[k] + a[k];
        }
        __device__ __forceinline__ void flush(const BigDev &d, double *red, int &parity) { store_partials<NV>(d, phase, v, red, parity); }
    };
};

// The totals of the first NV of the NVP values a phase holds, for every thread of the calling workgroup (a uniform call: it contains
// barriers).  Route with a reduction launch (and the reference order, whose walker writes d.red): big_k_fin (+ the cross-rank sum) has
// left them in d.red.  Folded route: this workgroup adds the partials up itself -- per rank the order of big_k_fin (thread t: partials
// t, t + T, ... ascending, then the block tree), the rank totals in rank order like big_k_rank_sum -- so both routes give the same
// bits.  All loads of a rank are issued before the first addition.
template <class S, int NV, int NVP>
__device__ __forceinline__ void get_red(const BigDev &d, int phase, double (&out)[NV], double *red, int &parity) {
    static_assert(NV <= NVP, "a phase holds NVP values");
    if (!S::wg_sums || !d.fold) {
#pragma unroll
        for (int k = 0; k < NV; k++) out[k] = d.red[phase * BIG_NPART + k];
        return;
    }
    const int W = d.gathered ? d.W : 1;
    for (int r = 0; r < W; r++) {
        const double *base = d.gathered ? d.gpart + ((size_t)phase * W * BIG_NPART + (size_t)r * NVP) * d.Gs : part_ptr(d, phase);
        const int G = d.gathered ? d.Gr[r] : d.G;
        double t[NV][BIG_FOLD_U];
#pragma unroll
        for (int k = 0; k < NV; k++)
#pragma unroll
            for (int u = 0; u < BIG_FOLD_U; u++) { const int e = threadIdx.x + u * T; t[k][u] = e < G ? base[(size_t)k * d.Gs + e] : 0.0; }
        double a[NV];
#pragma unroll
        for (int k = 0; k < NV; k++) {
            double acc = 0.0;
#pragma unroll
            for (int u = 0; u < BIG_FOLD_U; u++) acc = (int)threadIdx.x + u * T < G ? acc + t[k][u] : acc;
            a[k] = acc;
        }
        block_sum<T, NV>(a, red, parity);
#pragma unroll
        for (int k = 0; k < NV; k++) out[k] = r == 0 ? a[k] : out[k] + a[k];
    }
}

template <class S>
__device__ __forceinline__ void big_b_init(const BigDev &d, const S &sp, double c1) {          // ADMM_lp_iters_init LPcpp:489-763
    __shared__ double red[2 * RED_MAXV * RED_MAXW];
    int parity = 0;
    Sums<S, 1> acc(d, sp, BIG_PH_X);
    for (int s = 0; s < d.EPT; s++) {
        const int j = blockIdx.x * (T * d.EPT) + s * T + threadIdx.x;
        double c = 0.0;
        if (j < d.n_loc) {
            d.x[j] = 1.0; d.z1[j] = 0.0; d.z2[j] = 0.0; d.pd[j] = 0.0; d.dinv[j] = 1.0;   // :583-586, :616-617
            d.y1[j] = 1.0; d.y2[j] = 1.0; d.gsrc[j] = 1.0; d.xt[j] = 1.0; d.live[j] = 1;
            d.r[j] = 0.0; d.z[j] = 0.0; d.tmp[j] = 0.0; d.p0[j] = 0.0; d.p1[j] = 0.0; d.rhs[j] = 0.0;
            c = d.b[j] * 1.0;                                                    // best_bin_obj = b.dot(x0) (:727); every variable is live
        }
        acc.add(j, j < d.n_loc, c);
    }
    if (blockIdx.x < d.G) acc.flush(d, red, parity);
    for (int s = 0; s < d.EPTl; s++) {
        const int i = blockIdx.x * (T * d.EPTl) + s * T + threadIdx.x;
        if (i < d.l) { d.z4[i] = 0.0; d.y3[i] = 0.0; d.fz[i] = make_double2(0.0, 0.0); d.Ex[i] = 0.0; }   // :650
    }
    if (LEADER) {
        BigState *s = d.st;
        memset(s, 0, sizeof(BigState));
        s->rho1 = s->rho2 = s->rho4 = s->prev_rho1 = s->prev_rho2 = s->prev_rho4 = LP_RHO0;   // :623-630
        s->gamma_val = LP_GAMMA0; s->std_obj = 1.0; s->rhoUpdated = 1; s->c1 = c1;
        s->n_live_lo = (int)(d.n_glob & 0x7fffffff); s->n_live_hi = (int)(d.n_glob >> 31);
        d.st[1] = d.st[0];
    }
}

// The end of outer iteration `it` from e5 = x.x, |x-y1|^2, |x-y2|^2, b.x, b.round(x): the stop test on cvg1 / cvg2, the rho / gamma
// schedule, the objective history with its standard-deviation stop, the best binary objective.  Halts on a stop, otherwise advances iter.
__device__ __forceinline__ void big_finish_iteration(BigState *s, const double (&e5)[5], int it) {
    s->have_prev = 0;
    const double xn = sqrt(e5[0]);
    const double t0 = (xn < 2.2204e-16) ? 2.2204e-16 : xn;
    s->cvg1 = sqrt(e5[1]) / t0; s->cvg2 = sqrt(e5[2]) / t0;            // :931-933
    bool stopped = false;
    if (s->cvg1 <= LP_STOP_THRESHOLD && s->cvg2 <= LP_STOP_THRESHOLD && (s->l2f || it != s->iter_start)) {   // :934 / :1503
        if (s->l2f) s->ret = 1;                                          // :1505 (plain loop: ret stays 0)
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

// finalise the previous iteration from red[0..5) (x.x, |x-y1|^2, |x-y2|^2, b.x, b.round(x)), then the terms of ||x+z2/rho2-1/2||^2
template <class S>
__device__ __forceinline__ void big_b_prep(const BigDev &d, const S &sp, int in, int out, int do_prep) {
    __shared__ double red[2 * RED_MAXV * RED_MAXW];
    int parity = 0;
    const BigState *si = d.st + in;
    const int halt0 = si->halt, have_prev = si->have_prev, it = si->iter, iter_end = si->iter_end;
    double rho2 = si->rho2;
    const bool fin = !halt0 && have_prev;
    if (fin && (it + 1) % LP_RHO_STEP == 0) rho2 = LP_LEARNING_FACT * rho2;
    const int next_iter = fin ? it + 1 : it;
    const bool will_prep = do_prep && !halt0 && next_iter < iter_end;
    double e5[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (blockIdx.x == 0 && fin) get_red<S, 5, 5>(d, BIG_PH_E, e5, red, parity);    // uniform over workgroup 0
    if (LEADER) {
        d.st[out] = *si;
        BigState *s = d.st + out;
        if (fin) big_finish_iteration(s, e5, it);
        if (!s->halt && s->iter >= s->iter_end) { s->halt = BIG_HALT_WINDOW; s->plain_iter_p1 = s->iter + 1; }
        if (!s->halt && do_prep) s->phase = 1;
    }
    if (!will_prep || blockIdx.x >= d.G) return;
    Sums<S, 1> acc(d, sp, BIG_PH_A);
    for (int q = 0; q < d.EPT; q++) {
        const int j = blockIdx.x * (T * d.EPT) + q * T + threadIdx.x;
        const bool lv = j < d.n_loc && d.live[j];
        double c = 0.0;
        if (lv) { const double u = (d.x[j] + d.z2[j] / rho2) - 0.5; c = u * u; }
        acc.add(j, lv, c);
    }
    acc.flush(d, red, parity);
}

// y1, y2, expression refresh (:831-866), rhs base, PCG start x0 = y1; for the rows: y3 = max(0, f - Ex - z4/rho4), fz = (f - y3, z4).
// VALUED: Esq_diag = the sum of val^2 down the column, and rho4_E_transpose is kept per entry (r4v).
template <class S, bool VALUED>
__device__ __forceinline__ void big_b_y(const BigDev &d, const S &sp, int in, int out) {
    __shared__ double red[2 * RED_MAXV * RED_MAXW];
    int parity = 0;
    const BigState *si = d.st + in;
    if (si->halt || si->phase != 1) { forward_state(d, in, out); return; }
    const double rho1 = si->rho1, rho2 = si->rho2, rho4 = si->rho4, c1 = si->c1;
    const int it = si->iter, rhoUpdated = si->rhoUpdated;
    double dI = si->dI, r4Et = si->r4Et;
    const bool first = it == 0, refresh = it != 0 && rhoUpdated;
    const double inc = si->rcr * (si->prev_rho1 + si->prev_rho2), inc4 = si->rcr * si->prev_rho4;
    if (first) { dI = 0.0; dI += rho1 + rho2; r4Et = rho4; }                     // update_expression(0) :2289-2404
    if (refresh) { dI += inc; r4Et = LP_LEARNING_FACT * r4Et; }                  // :851-866
    double a1[1];
    get_red<S, 1, 1>(d, BIG_PH_A, a1, red, parity);
    const double c2 = 2 * sqrt(a1[0]);
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
            double Esq = (double)(k1 - k0);
            if constexpr (VALUED) {
                Esq = 0.0;
                if (first || refresh) for (int k = k0; k < k1; k++) { const double v = sp.rf.vcsc[k]; Esq += v * v; }     // :2378-2390
            }
            if (first) { pd = dI; pd += rho4 * Esq; }
            if (refresh) { pd += inc; pd += inc4 * Esq; }
            if constexpr (VALUED) {
                if (first) for (int k = k0; k < k1; k++) sp.rf.r4v[k] = rho4 * sp.rf.vcsc[k];                             // :2293, :2391
                if (refresh) for (int k = k0; k < k1; k++) sp.rf.r4v[k] = LP_LEARNING_FACT * sp.rf.r4v[k];
            }
            d.pd[j] = pd;
            if (rhoUpdated) d.dinv[j] = (pd != 0.0) ? 1.0 / pd : 1.0;            // :883-890
            d.rhs[j] = (rho1 * y1 + rho2 * y2) - ((d.b[j] + z1) + z2);            // :872
            d.gsrc[j] = d.live[j] ? y1 : 0.0;                                     // x_sol = y1 (:892); fixed columns are gone from E
        }
    if (blockIdx.x < d.Gl)
        for (int q = 0; q < d.EPTl; q++) {
            const int i = blockIdx.x * (T * d.EPTl) + q * T + threadIdx.x;
            if (i >= d.l) continue;
            const double f = d.f[i];
            const double z4 = d.z4[i];
            const double v = f - d.Ex[i] - z4 / rho4;                             // :824-828
            const double y3 = v < 0 ? 0 : v;
            d.y3[i] = y3; d.fz[i] = make_double2(f - y3, z4);                     // what rhs_cols gathers per entry: ONE 16-byte element
        }
    if (LEADER) {
        d.st[out] = *si;
        BigState *s = d.st + out;
        s->dI = dI; s->r4Et = r4Et; s->rhoUpdated = 0; s->expr_ready = 1;
    }
}

template <class S, bool VALUED>
__device__ __forceinline__ void big_b_rhs_cols(const BigDev &d, const S &sp, int in, int out) {   // :874-877
    const BigState *si = d.st + in;
    if (si->halt || si->phase != 1) { forward_state(d, in, out); return; }
    const double r4Et = si->r4Et;
    for (int q = 0; q < d.EPT; q++) {
        const int j = blockIdx.x * (T * d.EPT) + q * T + threadIdx.x;
        if (j >= d.n_loc) continue;
        double tA = 0.0, tB = 0.0;
        const int k1 = d.cptr[j + 1];
        int k = d.cptr[j];
        for (; k + 4 <= k1; k += 4) {                      // 4 gathers in flight, additions in column order
            const int i0 = d.crow[k], i1 = d.crow[k + 1], i2 = d.crow[k + 2], i3 = d.crow[k + 3];
            const double2 e0 = d.fz[i0], e1 = d.fz[i1], e2 = d.fz[i2], e3 = d.fz[i3];     // (f - y3, z4) of the row
            if constexpr (VALUED) {
                const double a0 = sp.rf.r4v[k], a1 = sp.rf.r4v[k + 1], a2 = sp.rf.r4v[k + 2], a3 = sp.rf.r4v[k + 3];
                const double v0 = sp.rf.vcsc[k], v1 = sp.rf.vcsc[k + 1], v2 = sp.rf.vcsc[k + 2], v3 = sp.rf.vcsc[k + 3];
                tA += a0 * e0.x; tB += v0 * e0.y; tA += a1 * e1.x; tB += v1 * e1.y; tA += a2 * e2.x; tB += v2 * e2.y; tA += a3 * e3.x; tB += v3 * e3.y;
            } else { tA += r4Et * e0.x; tB += e0.y; tA += r4Et * e1.x; tB += e1.y; tA += r4Et * e2.x; tB += e2.y; tA += r4Et * e3.x; tB += e3.y; }
        }
        for (; k < k1; k++) {
            const double2 e = d.fz[d.crow[k]];
            if constexpr (VALUED) { tA += sp.rf.r4v[k] * e.x; tB += sp.rf.vcsc[k] * e.y; }
            else { tA += r4Et * e.x; tB += e.y; }
        }
        double r_ = d.rhs[j];
        r_ += tA;
        r_ -= tB;
        d.rhs[j] = r_;
    }
    forward_state(d, in, out);
}

// Row i of E[:, shard] * v when the table being gathered does not fit an XCD's L2 (n_loc * 16 B > the slice size, i.e. the
// single-GPU run of a 1e6-variable LP): the entries are stored SLICE-major -- slice ph holds the columns [ph * SW, (ph + 1) * SW),
// and inside a slice the rows follow each other, each with its entries in ascending column order (d.rptr[ph * l + i] is the start
// of the run of (slice ph, row i); the runs are consecutive, so the next pointer is its end).  Every thread walks the slices in
// order, which is still the ascending column order of its row: the sum is bit for bit the one of the unsliced loop.  What
// changes is WHEN a column is touched: all workgroups of the launch are co-resident and progress at the same pace, so at any
// time the whole chip gathers from ONE slice of (z, p) -- 1-2 MB, resident in every XCD's 4 MB L2 -- instead of drawing random
// 128-byte lines of a 16 MB table from the Infinity Cache at 12 % utilisation.  Runs are short (~1.5 entries), so the loop is
// software-pipelined over the slices: pointers two slices ahead, indices one slice ahead, gathers of the current slice.
constexpr int SLU = 6;   // entries of a run handled without a loop (longer runs: remainder loop)
template <bool ZP>
__device__ __forceinline__ double row_sum_sliced(const BigDev &d, int i, const double *src, const double2 *zp, double beta) {
    const int P = d.P;
    const size_t l = (size_t)d.l;
    const int *sp = d.rptr + i;
    double acc = 0.0;
    int ka = sp[0], kae = sp[1];                       // current slice
    int kb = 0, kbe = 0;                               // next slice
    if (P > 1) { kb = sp[l]; kbe = sp[l + 1]; }
    int c[SLU];
#pragma unroll
    for (int u = 0; u < SLU; u++) c[u] = ka + u < kae ? ld_stream(d.rcol + ka + u) : -1;
    for (int ph = 0; ph < P; ph++) {
        double vx[SLU], vy[SLU];
#pragma unroll
        for (int u = 0; u < SLU; u++) {
            vx[u] = 0.0; vy[u] = 0.0;
            if (c[u] >= 0) {
                if constexpr (ZP) { const double2 t = zp[c[u]]; vx[u] = t.x; vy[u] = t.y; }
                else vx[u] = src[c[u]];
            }
        }
        int cn[SLU];
#pragma unroll
        for (int u = 0; u < SLU; u++) cn[u] = kb + u < kbe ? ld_stream(d.rcol + kb + u) : -1;      // ph + 1 < P, else the run is empty
        int kc = 0, kce = 0;
        if (ph + 2 < P) { kc = sp[(size_t)(ph + 2) * l]; kce = sp[(size_t)(ph + 2) * l + 1]; }
#pragma unroll
        for (int u = 0; u < SLU; u++) {
            if constexpr (ZP) { const double t = vx[u] + beta * vy[u]; acc = c[u] >= 0 ? acc + t : acc; }
            else acc = c[u] >= 0 ? acc + vx[u] : acc;
        }
        for (int k = ka + SLU; k < kae; k++) {         // rare: a run longer than SLU entries
            const int cc = d.rcol[k];
            if constexpr (ZP) { const double2 t = zp[cc]; acc += t.x + beta * t.y; }
            else acc += src[cc];
        }
#pragma unroll
        for (int u = 0; u < SLU; u++) c[u] = cn[u];
        ka = kb; kae = kbe; kb = kc; kbe = kce;
    }
    return acc;
}

// The head of rows(p), PCG iteration k = si->pcg_k: the start of the PCG from the totals of resid (k == 0), else the exit test and beta
// of the previous iteration from those of pcg_upd (LPcpp:296-319).  The leader writes the state; true: the PCG is over, nothing to gather.
template <class S>
__device__ __forceinline__ bool big_pcg_control(const BigDev &d, const BigState *si, int out, double *red, int &parity, double &beta, bool &first) {
    const int k = si->pcg_k;
    double threshold = si->threshold, absNew = si->absNew, rhsNorm2 = si->rhsNorm2;
    bool done = false; int zero_x = 0;
    first = k == 0;
    if (first) {
        double b3[3];
        get_red<S, 3, 3>(d, BIG_PH_B, b3, red, parity);
        rhsNorm2 = b3[0];
        if (rhsNorm2 == 0) { done = true; zero_x = 1; }                      // :273-278
        else {
            double thr = LP_PCG_TOL * LP_PCG_TOL * rhsNorm2;                 // :281
            if (thr < DBL_MIN) thr = DBL_MIN;
            threshold = thr;
            if (b3[1] < thr) done = true;                                    // :284
            absNew = b3[2];
        }
    } else {
        double d2[2];
        get_red<S, 2, 2>(d, BIG_PH_D, d2, red, parity);
        if (d2[0] < threshold || k >= LP_PCG_MAXITERS) done = true;          // :309-312, :296
        else { const double absOld = absNew; absNew = d2[1]; beta = absNew / absOld; }   // :316-318
    }
    if (LEADER) {
        d.st[out] = *si;
        BigState *s = d.st + out;
        s->threshold = threshold; s->absNew = absNew; s->rhsNorm2 = rhsNorm2; s->beta = beta;
        s->pcg_done = done ? 1 : 0; s->pcg_first = zero_x;
    }
    return done;
}

// q_part = E[:, shard] * v over this rank's columns.  mode 0: v = gsrc.  mode 1: v = the PCG search direction (big_pcg_control first).
// VALUED: acc += val * v_j.
template <class S, bool VALUED>
__device__ __forceinline__ void big_b_rows(const BigDev &d, const S &sp, int in, int out, int mode) {
    __shared__ double red[2 * RED_MAXV * RED_MAXW];
    int parity = 0;
    const BigState *si = d.st + in;
    if (si->halt) { forward_state(d, in, out); return; }
    double beta = 0.0;
    bool first = false;
    if (mode == 1) {
        if (si->phase != 2 || si->pcg_done) { forward_state(d, in, out); return; }
        if (big_pcg_control<S>(d, si, out, red, parity, beta, first)) return;
    } else forward_state(d, in, out);
    const double *gs = d.gsrc, *p0 = d.p0;
    int rowgrid = d.Gl;
    bool lean_qq = false;
    double qq[1] = {0.0};
    if constexpr (S::wg_sums) {
        const bool lean = d.lean && mode == 1;
        if (d.P > 1) rowgrid = d.Glr;
        if (lean && (int)blockIdx.x < d.G) {
            // comm-lean PCG: the search direction p = z + beta p of this iteration for the workgroup's own variables (what pcg_cols does in the
            // default mode) and the workgroup partial of p.p, which rides with the q exchange
            const int k = si->pcg_k;
            const double *pold = ((k - 1) & 1) ? d.p1 : d.p0;
            double *pnew = (k & 1) ? d.p1 : d.p0;
            double pp[1] = {0.0};
            for (int q = 0; q < d.EPT; q++) {
                const int j = blockIdx.x * (T * d.EPT) + q * T + threadIdx.x;
                double c = 0.0;
                if (j < d.n_loc) {
                    double pj;
                    if (first) pj = p0[j];
                    else { pj = d.z[j] + beta * pold[j]; pnew[j] = pj; }                // p = z + beta p (:319)
                    c = d.live[j] ? pj * pj : 0.0;
                }
                pp[0] = pp[0] + c;
            }
            block_sum<T, 1>(pp, red, parity);
            if (threadIdx.x == 0) d.lsmall[blockIdx.x] = pp[0];
        }
        if ((int)blockIdx.x >= rowgrid) return;
        lean_qq = lean && !d.gathered;               // no exchange: q is final here, so its squares are summed here too
        if (d.P > 1) {                               // column-sliced rows (see row_sum_sliced): one row per thread
            const int i = blockIdx.x * T + threadIdx.x;
            if (i < d.l) {
                double qi;
                if (mode == 0 || first) qi = row_sum_sliced<false>(d, i, mode == 0 ? gs : p0, nullptr, 0.0);
                else qi = row_sum_sliced<true>(d, i, nullptr, d.zp, beta);
                d.q[i] = qi;
                qq[0] = qq[0] + qi * qi;
            }
            if (lean_qq) { block_sum<T, 1>(qq, red, parity); if (threadIdx.x == 0) d.lsmall[d.Gs + blockIdx.x] = qq[0]; }
            return;
        }
    } else if ((int)blockIdx.x >= rowgrid) return;
    for (int s = 0; s < d.EPTl; s++) {
        const int i = blockIdx.x * (T * d.EPTl) + s * T + threadIdx.x;
        if (i >= d.l) continue;
        double acc = 0.0;
        const int k1 = d.rptr[i + 1];
        int k = d.rptr[i];
        // the row is summed in ascending column order by this one lane; the gathers of 8 entries are issued together so that
        // their latencies overlap (the additions stay sequential: same rounding as the one-at-a-time loop)
        if (mode == 0 || first) {
            const double *src = mode == 0 ? gs : p0;
            for (; k + 8 <= k1; k += 8) {
                int c[8]; double v[8];
#pragma unroll
                for (int u = 0; u < 8; u++) c[u] = d.rcol[k + u];
#pragma unroll
                for (int u = 0; u < 8; u++) v[u] = src[c[u]];
                if constexpr (VALUED) {
                    double a[8];
#pragma unroll
                    for (int u = 0; u < 8; u++) a[u] = sp.rf.vcsr[k + u];
#pragma unroll
                    for (int u = 0; u < 8; u++) acc += a[u] * v[u];
                } else {
#pragma unroll
                    for (int u = 0; u < 8; u++) acc += v[u];
                }
            }
            for (; k < k1; k++) {
                if constexpr (VALUED) acc += sp.rf.vcsr[k] * src[d.rcol[k]];
                else acc += src[d.rcol[k]];
            }
        } else {
            for (; k + 8 <= k1; k += 8) {
                int c[8]; double2 v[8];
#pragma unroll
                for (int u = 0; u < 8; u++) c[u] = d.rcol[k + u];
#pragma unroll
                for (int u = 0; u < 8; u++) v[u] = d.zp[c[u]];
                if constexpr (VALUED) {
                    double a[8];
#pragma unroll
                    for (int u = 0; u < 8; u++) a[u] = sp.rf.vcsr[k + u];
#pragma unroll
                    for (int u = 0; u < 8; u++) acc += a[u] * (v[u].x + beta * v[u].y);
                } else {
#pragma unroll
                    for (int u = 0; u < 8; u++) acc += v[u].x + beta * v[u].y;
                }
            }
            for (; k < k1; k++) {
                const double2 v = d.zp[d.rcol[k]];
                if constexpr (VALUED) acc += sp.rf.vcsr[k] * (v.x + beta * v.y);
                else acc += v.x + beta * v.y;
            }
        }
        d.q[i] = acc;
        if constexpr (S::wg_sums) qq[0] = qq[0] + acc * acc;
    }
    if constexpr (S::wg_sums)
        if (lean_qq) { block_sum<T, 1>(qq, red, parity); if (threadIdx.x == 0) d.lsmall[d.Gs + blockIdx.x] = qq[0]; }
}

// t = sum over column j of rho4_E_transpose * q, rows ascending from +0.0; 4 gathers in flight, additions in column order
template <bool VALUED, class S>
__device__ __forceinline__ double big_col_r4_q(const BigDev &d, const S &sp, int j, double r4Et) {
    double t = 0.0;
    const int k1 = d.cptr[j + 1];
    int k = d.cptr[j];
    for (; k + 4 <= k1; k += 4) {
        const int r0 = ld_stream(d.crow + k), r1 = ld_stream(d.crow + k + 1), r2 = ld_stream(d.crow + k + 2), r3 = ld_stream(d.crow + k + 3);
        const double v0 = d.q[r0], v1 = d.q[r1], v2 = d.q[r2], v3 = d.q[r3];
        if constexpr (VALUED) {
            const double a0 = sp.rf.r4v[k], a1 = sp.rf.r4v[k + 1], a2 = sp.rf.r4v[k + 2], a3 = sp.rf.r4v[k + 3];
            t += a0 * v0; t += a1 * v1; t += a2 * v2; t += a3 * v3;
        } else { t += r4Et * v0; t += r4Et * v1; t += r4Et * v2; t += r4Et * v3; }
    }
    for (; k < k1; k++) {
        if constexpr (VALUED) t += sp.rf.r4v[k] * d.q[ld_stream(d.crow + k)];
        else t += r4Et * d.q[ld_stream(d.crow + k)];
    }
    return t;
}

template <class S, bool VALUED>
__device__ __forceinline__ void big_b_resid(const BigDev &d, const S &sp, int in, int out) {       // :267-294
    __shared__ double red[2 * RED_MAXV * RED_MAXW];
    int parity = 0;
    const BigState *si = d.st + in;
    if (si->halt || si->phase != 1) { forward_state(d, in, out); return; }
    const double dI = si->dI, r4Et = si->r4Et;
    Sums<S, 3> acc(d, sp, BIG_PH_B);
    for (int q = 0; q < d.EPT; q++) {
        const int j = blockIdx.x * (T * d.EPT) + q * T + threadIdx.x;
        double c0 = 0.0, c1 = 0.0, c2 = 0.0;
        bool lv = false;
        if (j < d.n_loc) {
            const double t = big_col_r4_q<VALUED>(d, sp, j, r4Et);
            const double y1 = d.y1[j];
            double Mx = 0.0;
            Mx += dI * (1.0 * y1);
            Mx += t;
            const double rhs = d.rhs[j];
            const double r = rhs - Mx;
            const double p = d.dinv[j] * r;
            lv = d.live[j];
            d.xt[j] = y1; d.r[j] = r; d.p0[j] = lv ? p : 0.0;
            if (lv) { c0 = rhs * rhs; c1 = r * r; c2 = r * p; }
        }
        acc.add(j, lv, c0, c1, c2);
    }
    acc.flush(d, red, parity);
    if (LEADER) { d.st[out] = *si; d.st[out].pcg_k = 0; d.st[out].pcg_done = 0; d.st[out].pcg_first = 0; d.st[out].phase = 2; }
}

// pcg_cols / pcg_lean behind a finished PCG: nothing to do but x := 0 when the right-hand side was zero (:273-278).  true: handled.
__device__ __forceinline__ bool big_pcg_finished(const BigDev &d, const BigState *si, int out) {
    if (!si->pcg_done) return false;
    if (si->pcg_first)
        for (int q = 0; q < d.EPT; q++) { const int j = blockIdx.x * (T * d.EPT) + q * T + threadIdx.x; if (j < d.n_loc) d.xt[j] = 0.0; }
    if (LEADER) { d.st[out] = *si; d.st[out].pcg_first = 0; }
    return true;
}

template <class S, bool VALUED>
__device__ __forceinline__ void big_b_pcg_cols(const BigDev &d, const S &sp, int in, int out) {    // tmp = M p, terms of p.tmp (:298-300)
    __shared__ double red[2 * RED_MAXV * RED_MAXW];
    int parity = 0;
    const BigState *si = d.st + in;
    if (si->halt || si->phase != 2) { forward_state(d, in, out); return; }
    if (big_pcg_finished(d, si, out)) return;
    const int k = si->pcg_k;
    const double dI = si->dI, r4Et = si->r4Et, beta = si->beta;
    const bool first = k == 0;
    const double *pold = ((k - 1) & 1) ? d.p1 : d.p0;
    double *pnew = (k & 1) ? d.p1 : d.p0;
    Sums<S, 1> acc(d, sp, BIG_PH_C);
    for (int q = 0; q < d.EPT; q++) {
        const int j = blockIdx.x * (T * d.EPT) + q * T + threadIdx.x;
        double c = 0.0;
        bool lv = false;
        if (j < d.n_loc) {
            double pj;
            if (first) pj = ld_stream(d.p0 + j);
            else { pj = ld_stream(d.z + j) + beta * ld_stream(pold + j); st_stream(pnew + j, pj); }   // p = z + beta p (:319)
            const double t = big_col_r4_q<VALUED>(d, sp, j, r4Et);
            double Mp = 0.0;
            Mp += dI * (1.0 * pj);
            Mp += t;
            st_stream(d.tmp + j, Mp);
            lv = d.live[j];
            c = lv ? pj * Mp : 0.0;
        }
        acc.add(j, lv, c);
    }
    acc.flush(d, red, parity);
    forward_state(d, in, out);
}

// x += alpha p (:302), r -= alpha M p (:304), z = r / diag (:314) for variable j, and (z, p) packed for the gather of the next search
// direction z + beta p in rows(); the terms of r.r and r.z of a live variable
__device__ __forceinline__ void big_pcg_step(const BigDev &d, int j, double alpha, double pj, double Mp, bool &lv, double &rr, double &rz) {
    double x = d.xt[j], r = d.r[j];
    x += alpha * pj;
    r -= alpha * Mp;
    const double z = d.dinv[j] * r;
    lv = d.live[j];
    d.xt[j] = x; d.r[j] = r; d.z[j] = lv ? z : 0.0;
    d.zp[j] = make_double2(lv ? z : 0.0, pj);
    if (lv) { rr = r * r; rz = r * z; }
}

template <class S>
__device__ __forceinline__ void big_b_pcg_upd(const BigDev &d, const S &sp, int in, int out) {     // :300-317
    __shared__ double red[2 * RED_MAXV * RED_MAXW];
    int parity = 0;
    const BigState *si = d.st + in;
    if (si->halt || si->phase != 2 || si->pcg_done) { forward_state(d, in, out); return; }
    const int k = si->pcg_k;
    double c1v[1];
    get_red<S, 1, 1>(d, BIG_PH_C, c1v, red, parity);
    const double alpha = si->absNew / c1v[0];
    // (alpha < 0 -> the plain loop ignores the PCG's -1 return, LPcpp:894; x keeps the updates made so far, which is what
    //  happens here too because the remaining pairs fall through once pcg_done is set)
    const bool fail = alpha < 0;
    const double *p = (k & 1) ? d.p1 : d.p0;
    if (!fail) {
        Sums<S, 2> acc(d, sp, BIG_PH_D);
        for (int q = 0; q < d.EPT; q++) {
            const int j = blockIdx.x * (T * d.EPT) + q * T + threadIdx.x;
            double a = 0.0, b2 = 0.0;
            bool lv = false;
            if (j < d.n_loc) big_pcg_step(d, j, alpha, p[j], d.tmp[j], lv, a, b2);
            acc.add(j, lv, a, b2);
        }
        acc.flush(d, red, parity);
    }
    if (LEADER) {
        d.st[out] = *si;
        if (fail) { d.st[out].pcg_done = 1; d.st[out].stop = LP_STOP_PCG; }
        else d.st[out].pcg_k = k + 1;
    }
}

// after the PCG: duals z1, z2 (:917-918), the five terms (:931-1003), gsrc = x for the E*x that feeds z4 and the next y3
template <class S>
__device__ __forceinline__ void big_b_post(const BigDev &d, const S &sp, int in, int out) {
    __shared__ double red[2 * RED_MAXV * RED_MAXW];
    int parity = 0;
    const BigState *si = d.st + in;
    if (si->halt || si->phase != 2) { forward_state(d, in, out); return; }
    const int k = si->pcg_k;
    if (!si->pcg_done) {                      // the exit test of the last update is still pending
        double d1[1] = {0.0};
        if (k >= 1) get_red<S, 1, 2>(d, BIG_PH_D, d1, red, parity);
        if (!(k >= 1 && (d1[0] < si->threshold || k >= LP_PCG_MAXITERS))) {
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
    Sums<S, 5> acc(d, sp, BIG_PH_E);
    for (int q = 0; q < d.EPT; q++) {
        const int j = blockIdx.x * (T * d.EPT) + q * T + threadIdx.x;
        double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0, v4 = 0.0;
        bool lv = false;
        if (j < d.n_loc) {
            lv = d.live[j];
            const double x = lv ? d.xt[j] : d.x[j], y1 = d.y1[j], y2 = d.y2[j], b = d.b[j];   // commit: fixed variables keep their value
            d.x[j] = x;
            if (xh) xh[j] = x;                                                // x_iters column (:1472-1475)
            d.z1[j] = d.z1[j] + g1 * (x - y1);
            d.z2[j] = d.z2[j] + g2 * (x - y2);
            d.gsrc[j] = lv ? x : 0.0;
            const double d1 = x - y1, d2 = x - y2, xb = x >= 0.5 ? 1.0 : 0.0;
            if (lv) { v0 = x * x; v1 = d1 * d1; v2 = d2 * d2; v3 = b * x; v4 = b * xb; }
        }
        acc.add(j, lv, v0, v1, v2, v3, v4);
    }
    acc.flush(d, red, parity);
    if (LEADER) {
        d.st[out] = *si;
        BigState *s = d.st + out;
        s->pcg_done = 1; s->last_pcg = k; s->pcg_total += k; s->outer_total++;
        if (si->l2f || si->rec) s->cc = si->cc + 1;
        if (k > s->pcg_max) s->pcg_max = k;
        s->phase = 3;
    }
}

// ---- early fixing (LPcpp:1124-1335) as a mask; three passes cut at the two reductions it needs ----
template <class S>
__device__ __forceinline__ void big_b_fix1(const BigDev &d, const S &sp) {          // x2 = the newly fixed values; terms of fix_obj = b2.x2 (:1237)
    __shared__ double red[2 * RED_MAXV * RED_MAXW];
    int parity = 0;
    Sums<S, 1> acc(d, sp, BIG_PH_X);
    for (int q = 0; q < d.EPT; q++) {
        const int j = blockIdx.x * (T * d.EPT) + q * T + threadIdx.x;
        double c = 0.0;
        bool nfx = false;
        if (j < d.n_loc) {
            const int nf = d.newfix[j];
            const double val = nf == 2 ? 1.0 : 0.0;
            d.gsrc[j] = nf ? val : 0.0;
            if (nf) { c = d.b[j] * val; nfx = true; }
        }
        acc.add(j, nfx, c);
    }
    acc.flush(d, red, parity);
}

template <class S>
__device__ __forceinline__ void big_b_fix2(const BigDev &d, const S &sp, int in, int out) {   // red[0] = fix_obj, q = E2*x2 (all ranks); terms of |x_live|^2 (:1223)
    __shared__ double red[2 * RED_MAXV * RED_MAXW];
    int parity = 0;
    if (blockIdx.x < d.Gl)
        for (int s = 0; s < d.EPTl; s++) {
            const int i = blockIdx.x * (T * d.EPTl) + s * T + threadIdx.x;
            if (i < d.l) d.f[i] = d.f[i] - d.q[i];                                  // f1 = f - E2*x2 (:1278)
        }
    if (LEADER) { d.st[out] = d.st[in]; d.st[out].fix_obj = d.red[BIG_PH_X * BIG_NPART]; }
    if (blockIdx.x >= d.G) return;
    Sums<S, 1> acc(d, sp, BIG_PH_X);
    for (int q = 0; q < d.EPT; q++) {
        const int j = blockIdx.x * (T * d.EPT) + q * T + threadIdx.x;
        double c = 0.0;
        bool lv = false;
        if (j < d.n_loc) {
            const int nf = d.newfix[j];
            if (nf) { d.live[j] = 0; d.x[j] = nf == 2 ? 1.0 : 0.0; }
            else if (d.live[j]) { const double x = d.x[j]; c = x * x; lv = true; }
        }
        acc.add(j, lv, c);
    }
    acc.flush(d, red, parity);
}

// red[0] = |x_live|^2.  n_live_new == 0: everything is fixed (:1212-1217, nothing else is updated).
template <class S, bool VALUED>
__device__ __forceinline__ void big_b_fix3(const BigDev &d, const S &sp, int in, int out, long n_live_new, double c1_new) {
    const BigState *si = d.st + in;
    const double rho1 = si->rho1, rho2 = si->rho2, rho4 = si->rho4;
    if (LEADER) {
        d.st[out] = *si;
        BigState *s = d.st + out;
        s->n_live_lo = (int)(n_live_new & 0x7fffffff); s->n_live_hi = (int)(n_live_new >> 31);
        if (n_live_new == 0) { s->ret = 1; s->stop = LP_STOP_ALLFIXED; s->halt = BIG_HALT_STOP; }
        else {
            if (sqrt(d.red[BIG_PH_X * BIG_NPART]) < 1e-3) s->ret = 1;                                 // :1223
            s->prev_sum = s->sum_fix_obj; s->sum_fix_obj += s->fix_obj; s->prev_obj = s->cur_obj;   // :1247-1250
            s->c1 = c1_new;
            double dI = 0.0; dI += rho1 + rho2;                                      // update_expression (:1329 -> :2289-2404)
            s->dI = dI; s->r4Et = rho4; s->expr_ready = 1;
        }
    }
    if (n_live_new == 0) return;
    double dI = 0.0; dI += rho1 + rho2;
    for (int q = 0; q < d.EPT; q++) {
        const int j = blockIdx.x * (T * d.EPT) + q * T + threadIdx.x;
        if (j >= d.n_loc) continue;
        double Esq = (double)(d.cptr[j + 1] - d.cptr[j]);
        if constexpr (VALUED) {
            Esq = 0.0;
            for (int k = d.cptr[j]; k < d.cptr[j + 1]; k++) { const double v = sp.rf.vcsc[k]; Esq += v * v; sp.rf.r4v[k] = rho4 * v; }
        }
        double pd = dI;
        pd += rho4 * Esq;
        d.pd[j] = pd;
        d.dinv[j] = (pd != 0.0) ? 1.0 / pd : 1.0;        // the preconditioner always mirrors pd (a stale one is UB in the reference)
        d.gsrc[j] = d.live[j] ? d.x[j] : 0.0;            // for E*x of the first iteration's y3
    }
}

}  // namespace
