// lpbox_big_kernels.hip -- gfx950 kernels of the LARGE-instance LP path (one LP, n up to ~1e6, variable-sharded) in the DEFAULT summation
// order: the entries of the chain's bodies (lpbox_big_dev.h, where the chain and its arithmetic are described) for one problem (big_k_*)
// and for a batch in lockstep (big_kb_*), every body with workgroup sums and unit values; the kernels only this order has (the reduction
// launch big_k_fin, the comm-lean PCG, the rank-ordered sums); the state kernels and z4, which no order changes; and the launch helpers
// of BOTH orders -- a helper that is given a BigRef launches the staged entry of lpbox_big_ref_kernels.hip over the same grid.
#include "lpbox_big_dev.h"

#include <algorithm>

namespace {

// red[v] = tree over the G workgroup partials of value v (second level of the fixed reduction order)
__global__ void __launch_bounds__(T) big_k_fin(BigDev d, int nv, int phase) {
    __shared__ double red[2 * RED_MAXV * RED_MAXW];
    int parity = 0;
    fin_reduce<T>(part_ptr(d, phase), d.G, nv, d.red + phase * BIG_NPART, red, parity, d.Gs);
}

__global__ void big_k_init2(BigDev d) {       // after the partial of b.x0 has been reduced: best_bin_obj (:727)
    d.st[0].best_bin_obj = d.red[BIG_PH_X * BIG_NPART];
    d.st[1].best_bin_obj = d.red[BIG_PH_X * BIG_NPART];
}

__device__ __forceinline__ void big_b_set_window(const BigDev &d, int in, int out, int iter_start, int iter_end, int l2f) {
    d.st[out] = d.st[in];
    BigState *s = d.st + out;
    s->iter = iter_start; s->iter_start = iter_start; s->iter_end = iter_end; s->ret = 0; s->stop = LP_STOP_NONE; s->halt = BIG_HALT_NONE;
    s->l2f = l2f & 1; s->rec = (l2f >> 1) & 1; s->cc = 0;
}

__device__ __forceinline__ void big_b_resume(const BigDev &d, int in, int out, int reset_pcg_max) {
    d.st[out] = d.st[in];
    if (d.st[out].halt == BIG_HALT_PCG_MORE) d.st[out].halt = BIG_HALT_NONE;
    if (reset_pcg_max) d.st[out].pcg_max = 0;
}

// COMM-LEAN PCG (opt-in, not the reference's arithmetic): pcg_cols and pcg_upd in one launch.  p.Mp is not summed over the variables but
// taken from p.p and q.q -- both complete once the q exchange is: alpha = absNew / (dI (p.p) + r4Et (q.q)) -- so no exchange separates the
// column product from the vector updates.  Totals: per rank the tree over its workgroup partials, the rank totals in rank order.
constexpr int FOLD_UQ = 8;     // q.q partials per thread (one rank: up to 2048 row workgroups)
__device__ __forceinline__ double lean_total(const BigDev &d, bool qq, double *red, int &parity) {
    const int W = d.W > 1 ? d.W : 1;
    double out = 0.0;
    for (int r = 0; r < W; r++) {
        const double *base = (d.gathered ? d.gsmall + (size_t)r * (d.Gs + d.Gqs) : d.lsmall) + (qq ? d.Gs : 0);
        const int G = qq ? (d.gathered ? d.Gqr[r] : d.Gq) : (d.gathered ? d.Gr[r] : d.G);
        double t[FOLD_UQ];
#pragma unroll
        for (int u = 0; u < FOLD_UQ; u++) { const int e = threadIdx.x + u * T; t[u] = e < G ? base[e] : 0.0; }
        double a[1] = {0.0};
#pragma unroll
        for (int u = 0; u < FOLD_UQ; u++) a[0] = (int)threadIdx.x + u * T < G ? a[0] + t[u] : a[0];
        block_sum<T, 1>(a, red, parity);
        out = r == 0 ? a[0] : out + a[0];
    }
    return out;
}

__global__ void __launch_bounds__(T) big_k_pcg_lean(BigDev d, int in, int out) {
    __shared__ double red[2 * RED_MAXV * RED_MAXW];
    int parity = 0;
    const BigState *si = d.st + in;
    if (si->halt || si->phase != 2) { forward_state(d, in, out); return; }
    if (big_pcg_finished(d, si, out)) return;
    const int k = si->pcg_k;
    const double dI = si->dI, r4Et = si->r4Et;
    const double pp = lean_total(d, false, red, parity), qq = lean_total(d, true, red, parity);
    const double pMp = dI * pp + r4Et * qq;
    const double alpha = si->absNew / pMp;
    const bool fail = alpha < 0;
    const double *p = (k & 1) ? d.p1 : d.p0;
    double pd2[2] = {0.0, 0.0};
    if (!fail)
        for (int q = 0; q < d.EPT; q++) {
            const int j = blockIdx.x * (T * d.EPT) + q * T + threadIdx.x;
            double a = 0.0, b2 = 0.0;
            if (j < d.n_loc) {
                const double pj = p[j];
                double Mp = 0.0;
                Mp += dI * (1.0 * pj);
                Mp += big_col_r4_q<false>(d, WgSums{}, j, r4Et);                   // tmp = M p (:298)
                bool lv;
                big_pcg_step(d, j, alpha, pj, Mp, lv, a, b2);
            }
            pd2[0] = pd2[0] + a; pd2[1] = pd2[1] + b2;
        }
    if (!fail) store_partials<2>(d, BIG_PH_D, pd2, red, parity);
    if (LEADER) {
        d.st[out] = *si;
        if (fail) { d.st[out].pcg_done = 1; d.st[out].stop = LP_STOP_PCG; }
        else d.st[out].pcg_k = k + 1;
    }
}

// rank-ordered sum of this rank's block of E*v (as big_k_rank_sum) and, for the comm-lean PCG, the workgroup partials of q.q over the block:
// one row per thread, 256 rows per workgroup
__global__ void __launch_bounds__(T) big_k_rank_sum_qq(const double *g, int W, long count, long stride, double *out, double *qq_part) {
    __shared__ double red[2 * RED_MAXV * RED_MAXW];
    int parity = 0;
    const long i = (long)blockIdx.x * T + threadIdx.x;
    double c[1] = {0.0};
    if (i < count) {
        double acc = g[i];
        for (int r = 1; r < W; r++) acc = acc + g[(long)r * stride + i];
        out[i] = acc;
        c[0] = c[0] + acc * acc;
    }
    block_sum<T, 1>(c, red, parity);
    if (threadIdx.x == 0) qq_part[blockIdx.x] = c[0];
}

// Ex = q (= E*x, already all-reduced), z4 dual update (:919-924; the plain loop OVERWRITES z4 on the first iteration of a call)
__device__ __forceinline__ void big_b_z4(const BigDev &d, int in, int out, int init_only) {
    const BigState *si = d.st + in;
    if (init_only) {
        for (int s = 0; s < d.EPTl; s++) { const int i = blockIdx.x * (T * d.EPTl) + s * T + threadIdx.x; if (i < d.l) d.Ex[i] = d.q[i]; }
        forward_state(d, in, out);
        return;
    }
    if (si->halt || si->phase != 3) { forward_state(d, in, out); return; }
    const double g4 = si->gamma_val * si->rho4;
    const bool overwrite = !si->l2f && si->iter == si->iter_start;
    for (int s = 0; s < d.EPTl; s++) {
        const int i = blockIdx.x * (T * d.EPTl) + s * T + threadIdx.x;
        if (i >= d.l) continue;
        const double Ex = d.q[i];
        d.Ex[i] = Ex;
        const double dd = g4 * ((Ex + d.y3[i]) - d.f[i]);
        d.z4[i] = overwrite ? dd : d.z4[i] + dd;
    }
    if (LEADER) { d.st[out] = *si; d.st[out].have_prev = 1; d.st[out].phase = 0; }
}

// out[r*ws + c] = x after iteration c of the r-th LOCAL live variable (get_x_iters_d, LPcpp:1616-1627)
// out[i] = g[0][i] + g[1][i] + ... + g[W-1][i], added in RANK ORDER: the cross-rank association of every sum over variables of the
// variable-sharded run (each g[r] is the contribution of rank r; every rank runs this on the same gathered data and gets the same bits).
__global__ void big_k_rank_sum(const double *g, int W, long count, long stride, double *out) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (long)gridDim.x * blockDim.x) {
        double acc = g[i];
        for (int r = 1; r < W; r++) acc = acc + g[(long)r * stride + i];
        out[i] = acc;
    }
}

__global__ void big_k_pack_xiters(BigDev d, const int *live_idx, int rows, int ws, double *out) {
    const long total = (long)rows * ws;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int r = (int)(e / ws), c = (int)(e % ws);
        out[e] = c < d.ws_cap ? d.xhist[(size_t)c * d.n_loc + live_idx[r]] : 0.0;
    }
}

// ---- entries.  big_k_*: one problem, the descriptor in the kernel arguments.  big_kb_*: a BATCH of problems in lockstep (one rank each,
// folded reductions, plain windows), grid (X, B): row blockIdx.y of the grid runs problem blockIdx.y through the same body on its own
// descriptor, control state, partials and vectors.  X is the largest extent of that kernel over the batch; a workgroup at or beyond its
// problem's own extent leaves before the first barrier and before any store (the whole workgroup: uniform), so LEADER and every
// reduction see exactly the workgroups the problem's own launch would have had.
__global__ void __launch_bounds__(T) big_k_init(BigDev d, double c1) { big_b_init(d, WgSums{}, c1); }
__global__ void __launch_bounds__(T) big_k_fix1(BigDev d) { big_b_fix1(d, WgSums{}); }
__global__ void __launch_bounds__(T) big_k_fix2(BigDev d, int in, int out) { big_b_fix2(d, WgSums{}, in, out); }
__global__ void __launch_bounds__(T) big_k_fix3(BigDev d, int in, int out, long n_live_new, double c1_new) { big_b_fix3<WgSums, false>(d, WgSums{}, in, out, n_live_new, c1_new); }
__global__ void big_k_set_window(BigDev d, int in, int out, int iter_start, int iter_end, int l2f) { big_b_set_window(d, in, out, iter_start, iter_end, l2f); }
__global__ void big_k_resume(BigDev d, int in, int out, int reset_pcg_max) { big_b_resume(d, in, out, reset_pcg_max); }
__global__ void __launch_bounds__(T) big_k_prep(BigDev d, int in, int out, int do_prep) { big_b_prep(d, WgSums{}, in, out, do_prep); }
__global__ void __launch_bounds__(T) big_k_y(BigDev d, int in, int out) { big_b_y<WgSums, false>(d, WgSums{}, in, out); }
__global__ void __launch_bounds__(T) big_k_rhs_cols(BigDev d, int in, int out) { big_b_rhs_cols<WgSums, false>(d, WgSums{}, in, out); }
__global__ void __launch_bounds__(T) big_k_rows(BigDev d, int in, int out, int mode) { big_b_rows<WgSums, false>(d, WgSums{}, in, out, mode); }
__global__ void __launch_bounds__(T) big_k_resid(BigDev d, int in, int out) { big_b_resid<WgSums, false>(d, WgSums{}, in, out); }
__global__ void __launch_bounds__(T) big_k_pcg_cols(BigDev d, int in, int out) { big_b_pcg_cols<WgSums, false>(d, WgSums{}, in, out); }
__global__ void __launch_bounds__(T) big_k_pcg_upd(BigDev d, int in, int out) { big_b_pcg_upd(d, WgSums{}, in, out); }
__global__ void __launch_bounds__(T) big_k_post(BigDev d, int in, int out) { big_b_post(d, WgSums{}, in, out); }
__global__ void __launch_bounds__(T) big_k_z4(BigDev d, int in, int out, int init_only) { big_b_z4(d, in, out, init_only); }

__global__ void big_kb_set_window(const BigDev *__restrict__ devs, int in, int out, int iter_start, int iter_end) { big_b_set_window(devs[blockIdx.y], in, out, iter_start, iter_end, 0); }
__global__ void big_kb_resume(const BigDev *__restrict__ devs, int in, int out, int reset_pcg_max) { big_b_resume(devs[blockIdx.y], in, out, reset_pcg_max); }
__global__ void __launch_bounds__(T) big_kb_prep(const BigDev *__restrict__ devs, int in, int out, int do_prep) { const BigDev &d = devs[blockIdx.y]; if ((int)blockIdx.x >= ext_cols(d)) return; big_b_prep(d, WgSums{}, in, out, do_prep); }
__global__ void __launch_bounds__(T) big_kb_y(const BigDev *__restrict__ devs, int in, int out) { const BigDev &d = devs[blockIdx.y]; if ((int)blockIdx.x >= ext_y(d)) return; big_b_y<WgSums, false>(d, WgSums{}, in, out); }
__global__ void __launch_bounds__(T) big_kb_rhs_cols(const BigDev *__restrict__ devs, int in, int out) { const BigDev &d = devs[blockIdx.y]; if ((int)blockIdx.x >= ext_cols(d)) return; big_b_rhs_cols<WgSums, false>(d, WgSums{}, in, out); }
__global__ void __launch_bounds__(T) big_kb_rows(const BigDev *__restrict__ devs, int in, int out, int mode) { const BigDev &d = devs[blockIdx.y]; if ((int)blockIdx.x >= ext_rows(d)) return; big_b_rows<WgSums, false>(d, WgSums{}, in, out, mode); }
__global__ void __launch_bounds__(T) big_kb_resid(const BigDev *__restrict__ devs, int in, int out) { const BigDev &d = devs[blockIdx.y]; if ((int)blockIdx.x >= ext_cols(d)) return; big_b_resid<WgSums, false>(d, WgSums{}, in, out); }
__global__ void __launch_bounds__(T) big_kb_pcg_cols(const BigDev *__restrict__ devs, int in, int out) { const BigDev &d = devs[blockIdx.y]; if ((int)blockIdx.x >= ext_cols(d)) return; big_b_pcg_cols<WgSums, false>(d, WgSums{}, in, out); }
__global__ void __launch_bounds__(T) big_kb_pcg_upd(const BigDev *__restrict__ devs, int in, int out) { const BigDev &d = devs[blockIdx.y]; if ((int)blockIdx.x >= ext_cols(d)) return; big_b_pcg_upd(d, WgSums{}, in, out); }
__global__ void __launch_bounds__(T) big_kb_post(const BigDev *__restrict__ devs, int in, int out) { const BigDev &d = devs[blockIdx.y]; if ((int)blockIdx.x >= ext_cols(d)) return; big_b_post(d, WgSums{}, in, out); }
__global__ void __launch_bounds__(T) big_kb_z4(const BigDev *__restrict__ devs, int in, int out) { const BigDev &d = devs[blockIdx.y]; if ((int)blockIdx.x >= ext_z4(d)) return; big_b_z4(d, in, out, 0); }
__global__ void big_kb_collect(const BigDev *__restrict__ devs, int parity, BigState *out) { out[blockIdx.x] = devs[blockIdx.x].st[parity]; }

// ---- early-fixing windows of a batch: the prologue of lpbox_big_iterate_l2f (fix1, fin, rows, fix2, fin, fix3, rows, z4) over (X, members).
// par[blockIdx.y] is the member's record of this window.  A member with apply == 0 falls through: the whole workgroup leaves before the
// first barrier and before any store; in the launches that move the ping-pong parity its leader copies st[in] to st[out], so that one
// parity serves the chain.  A member whose fix leaves nothing live (n_live_new == 0) is halted by fix3 and falls through the two
// launches behind it the same way, as the one-problem call does not enqueue them.
__global__ void big_kb_set_window_l2f(const BigDev *__restrict__ devs, int in, int out, int iter_start, int iter_end) { big_b_set_window(devs[blockIdx.y], in, out, iter_start, iter_end, 1); }
__global__ void __launch_bounds__(T) big_kb_fix1(const BigDev *__restrict__ devs, const BigFixPar *__restrict__ par) {
    if (!par[blockIdx.y].apply) return;
    const BigDev &d = devs[blockIdx.y];
    if ((int)blockIdx.x >= ext_cols(d)) return;
    big_b_fix1(d, WgSums{});
}
__global__ void __launch_bounds__(T) big_kb_fin(const BigDev *__restrict__ devs, const BigFixPar *__restrict__ par, int nv, int phase) {
    __shared__ double red[2 * RED_MAXV * RED_MAXW];
    if (!par[blockIdx.y].apply) return;
    const BigDev &d = devs[blockIdx.y];
    int parity = 0;
    fin_reduce<T>(part_ptr(d, phase), d.G, nv, d.red + phase * BIG_NPART, red, parity, d.Gs);
}
__global__ void __launch_bounds__(T) big_kb_fix_rows(const BigDev *__restrict__ devs, const BigFixPar *__restrict__ par, int in, int out, int after_fix3) {
    const BigDev &d = devs[blockIdx.y];
    const BigFixPar &p = par[blockIdx.y];
    if (!p.apply || (after_fix3 && p.n_live_new == 0)) { forward_state(d, in, out); return; }
    if ((int)blockIdx.x >= ext_rows(d)) return;
    big_b_rows<WgSums, false>(d, WgSums{}, in, out, 0);
}
__global__ void __launch_bounds__(T) big_kb_fix2(const BigDev *__restrict__ devs, const BigFixPar *__restrict__ par, int in, int out) {
    const BigDev &d = devs[blockIdx.y];
    if (!par[blockIdx.y].apply) { forward_state(d, in, out); return; }
    if ((int)blockIdx.x >= ext_y(d)) return;
    big_b_fix2(d, WgSums{}, in, out);
}
__global__ void __launch_bounds__(T) big_kb_fix3(const BigDev *__restrict__ devs, const BigFixPar *__restrict__ par, int in, int out) {
    const BigDev &d = devs[blockIdx.y];
    const BigFixPar &p = par[blockIdx.y];
    if (!p.apply) { forward_state(d, in, out); return; }
    if ((int)blockIdx.x >= ext_cols(d)) return;
    big_b_fix3<WgSums, false>(d, WgSums{}, in, out, p.n_live_new, p.c1_new);
}
__global__ void __launch_bounds__(T) big_kb_z4_init(const BigDev *__restrict__ devs, const BigFixPar *__restrict__ par, int in, int out) {
    const BigDev &d = devs[blockIdx.y];
    const BigFixPar &p = par[blockIdx.y];
    if (!p.apply || p.n_live_new == 0) { forward_state(d, in, out); return; }
    if ((int)blockIdx.x >= ext_z4(d)) return;
    big_b_z4(d, in, out, 1);
}

// x_iters = Zero (LPcpp:1113) for every member: all ws_cap staged columns, as the one-problem call's memset
__global__ void big_kb_clear_xhist(const BigDev *__restrict__ devs) {
    const BigDev &d = devs[blockIdx.y];
    if (!d.xhist) return;
    const size_t total = (size_t)d.ws_cap * d.n_loc;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) d.xhist[e] = 0.0;
}

// The fix decision per packed row q of member y (original index live_idx[q]) -> its newfix code, and the member's counts of fixes to one
// / to zero (integer atomics: the sums do not depend on the order).  scores: deter_fix_2 on the float32 score of row row0 + q, widened to
// double (s > hi -> 1, s < lo -> 0, NaN -> neither); codes: the host's decision, one byte per row (the host-vector form).
__global__ void __launch_bounds__(T) big_kb_decide(const BigDev *__restrict__ devs, const BigFixPar *__restrict__ par, const float *__restrict__ scores,
                                                   const uint8_t *__restrict__ codes, double hi, double lo, int *counts) {
    const BigDev &d = devs[blockIdx.y];
    const BigFixPar &a = par[blockIdx.y];
    uint8_t *newfix = const_cast<uint8_t *>(d.newfix);
    __shared__ int cnt[2];
    if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
    __syncthreads();
    for (int q = blockIdx.x * T + threadIdx.x; q < a.rows; q += gridDim.x * T) {
        int code;
        if (codes) code = codes[(size_t)a.row0 + q];
        else { const double s = (double)scores[(size_t)a.row0 + q]; code = s > hi ? 2 : (s < lo ? 1 : 0); }
        newfix[a.live_idx[q]] = (uint8_t)code;
        if (code) atomicAdd(&cnt[code == 2 ? 0 : 1], 1);
    }
    __syncthreads();
    if (threadIdx.x < 2 && cnt[threadIdx.x]) atomicAdd(&counts[2 * blockIdx.y + threadIdx.x], cnt[threadIdx.x]);
}

// Ordered stream compaction of a member's live list after a fix: the entries whose newfix code is 0 stay, in the same (ascending) order,
// in place; the codes are cleared on the way (every non-zero code sits at an entry of the old list), which is the one-problem call's
// memset.  One workgroup per member walks the list in chunks of BIG_CT * BIG_CE entries: wave64 prefix by shuffles, wave totals through
// LDS, a carried offset; a chunk's writes land at or before its own entries, which were all read before its first write.  A member with
// clear != 0 (codes on the device, but the guard left the fix unapplied) gets its codes cleared and keeps its list.
__global__ void __launch_bounds__(BIG_CT) big_kb_compact(const BigDev *__restrict__ devs, const BigFixPar *__restrict__ par) {
    const BigDev &d = devs[blockIdx.x];
    const BigFixPar &a = par[blockIdx.x];
    if (!a.apply && !a.clear) return;
    const bool move = a.apply != 0;
    uint8_t *newfix = const_cast<uint8_t *>(d.newfix);
    __shared__ int wsum[BIG_CT / 64 + 1];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int carried = 0;
    for (int base = 0; base < a.rows; base += BIG_CT * BIG_CE) {
        int org[BIG_CE], keep[BIG_CE], c = 0;
#pragma unroll
        for (int k = 0; k < BIG_CE; k++) {
            const int q = base + threadIdx.x * BIG_CE + k;
            org[k] = q < a.rows ? a.live_idx[q] : -1;
            keep[k] = 0;
            if (org[k] >= 0) {
                if (newfix[org[k]]) newfix[org[k]] = 0; else keep[k] = 1;
            }
            c += keep[k];
        }
        if (!move) continue;                                                  // uniform over the workgroup
        int v = c;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) { const int t = __shfl_up(v, off, 64); if (lane >= off) v += t; }
        if (lane == 63) wsum[w + 1] = v;
        __syncthreads();
        if (threadIdx.x == 0) { wsum[0] = 0; for (int k = 1; k <= BIG_CT / 64; k++) wsum[k] += wsum[k - 1]; }
        __syncthreads();
        int pos = carried + wsum[w] + v - c;
        const int total = wsum[BIG_CT / 64];
#pragma unroll
        for (int k = 0; k < BIG_CE; k++) if (keep[k]) a.live_idx[pos++] = org[k];
        carried += total;
        __syncthreads();
    }
}

// big_k_pack_xiters per member: member y's (rows x ws) window goes to out + row0 * ws
__global__ void big_kb_pack(const BigDev *__restrict__ devs, const BigFixPar *__restrict__ par, int ws, double *out) {
    const BigDev &d = devs[blockIdx.y];
    const BigFixPar &a = par[blockIdx.y];
    const long total = (long)a.rows * ws;
    double *o = out + (size_t)a.row0 * ws;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int r = (int)(e / ws), c = (int)(e % ws);
        o[e] = c < d.ws_cap ? d.xhist[(size_t)c * d.n_loc + a.live_idx[r]] : 0.0;
    }
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
// One helper per launch of the chain, for both orders: rf == nullptr is the default order; with a BigRef the staged entry runs
// (REF_LAUNCH; a phase without a staged unit entry runs the default one there too) over the same grid.
#define BIG_LAUNCH(kernel, grid, ...)                                                                     \
    do {                                                                                                  \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(T), 0, s, d, *parity, *parity ^ 1, ##__VA_ARGS__);    \
        *parity ^= 1;                                                                                     \
    } while (0)
#define REF_LAUNCH(kernel, grid, ...)                                                                          \
    do {                                                                                                       \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(T), 0, s, d, *rf, *parity, *parity ^ 1, ##__VA_ARGS__);    \
        *parity ^= 1;                                                                                          \
    } while (0)

hipError_t big_launch_init(const BigDev &d, const BigRef *rf, double c1, hipStream_t s) {
    const int grid = d.G > d.Gl ? d.G : d.Gl;
    if (rf) hipLaunchKernelGGL(bigref_k_init, dim3(grid), dim3(T), 0, s, d, *rf, c1);      // the caller ranks and walks
    else {
        hipLaunchKernelGGL(big_k_init, dim3(grid), dim3(T), 0, s, d, c1);
        hipLaunchKernelGGL(big_k_fin, dim3(1), dim3(T), 0, s, d, 1, BIG_PH_X);
    }
    return hipGetLastError();
}
hipError_t big_launch_init2(const BigDev &d, hipStream_t s) {
    hipLaunchKernelGGL(big_k_init2, dim3(1), dim3(1), 0, s, d);
    return hipGetLastError();
}
hipError_t big_launch_fix1(const BigDev &d, const BigRef *rf, hipStream_t s) {
    if (rf) hipLaunchKernelGGL(bigref_k_fix1, dim3(d.G), dim3(T), 0, s, d, *rf);
    else hipLaunchKernelGGL(big_k_fix1, dim3(d.G), dim3(T), 0, s, d);
    return hipGetLastError();
}
hipError_t big_launch_fix2(const BigDev &d, const BigRef *rf, int *parity, hipStream_t s) {
    const int grid = d.G > d.Gl ? d.G : d.Gl;
    if (rf) REF_LAUNCH(bigref_k_fix2, grid); else BIG_LAUNCH(big_k_fix2, grid);
    return hipGetLastError();
}
hipError_t big_launch_fix3(const BigDev &d, const BigRef *rf, long n_live_new, double c1_new, int *parity, hipStream_t s) {
    if (rf && rf->valued) REF_LAUNCH(bigref_k_fix3_v, d.G, n_live_new, c1_new); else BIG_LAUNCH(big_k_fix3, d.G, n_live_new, c1_new);
    return hipGetLastError();
}
hipError_t big_launch_pack_xiters(const BigDev &d, const int *live_idx, int rows, int ws, double *out, hipStream_t s) {
    if (rows <= 0 || ws <= 0) return hipSuccess;
    const long total = (long)rows * ws;
    const int grid = (int)std::min<long>((total + 255) / 256, 65535);
    hipLaunchKernelGGL(big_k_pack_xiters, dim3(grid), dim3(256), 0, s, d, live_idx, rows, ws, out);
    return hipGetLastError();
}
hipError_t big_launch_rank_sum(const double *g, int W, long count, long stride, double *out, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    const int grid = (int)std::min<long>((count + 255) / 256, 4096);
    hipLaunchKernelGGL(big_k_rank_sum, dim3(grid), dim3(256), 0, s, g, W, count, stride, out);
    return hipGetLastError();
}
hipError_t big_launch_set_window(const BigDev &d, int iter_start, int iter_end, int l2f, int *parity, hipStream_t s) {
    hipLaunchKernelGGL(big_k_set_window, dim3(1), dim3(1), 0, s, d, *parity, *parity ^ 1, iter_start, iter_end, l2f);
    *parity ^= 1;
    return hipGetLastError();
}
hipError_t big_launch_resume(const BigDev &d, int reset_pcg_max, int *parity, hipStream_t s) {
    hipLaunchKernelGGL(big_k_resume, dim3(1), dim3(1), 0, s, d, *parity, *parity ^ 1, reset_pcg_max);
    *parity ^= 1;
    return hipGetLastError();
}
hipError_t big_launch_prep(const BigDev &d, const BigRef *rf, int do_prep, int *parity, hipStream_t s) {
    if (rf) REF_LAUNCH(bigref_k_prep, d.G, do_prep); else BIG_LAUNCH(big_k_prep, d.G, do_prep);
    return hipGetLastError();
}
hipError_t big_launch_fin(const BigDev &d, int nv, int phase, hipStream_t s) {
    hipLaunchKernelGGL(big_k_fin, dim3(1), dim3(T), 0, s, d, nv, phase);
    return hipGetLastError();
}
hipError_t big_launch_y(const BigDev &d, const BigRef *rf, int *parity, hipStream_t s) {
    const int grid = d.G > d.Gl ? d.G : d.Gl;
    if (rf && rf->valued) REF_LAUNCH(bigref_k_y_v, grid); else BIG_LAUNCH(big_k_y, grid);
    return hipGetLastError();
}
hipError_t big_launch_rhs_cols(const BigDev &d, const BigRef *rf, int *parity, hipStream_t s) {
    if (rf && rf->valued) REF_LAUNCH(bigref_k_rhs_cols_v, d.G); else BIG_LAUNCH(big_k_rhs_cols, d.G);
    return hipGetLastError();
}
hipError_t big_launch_rows(const BigDev &d, const BigRef *rf, int mode, int *parity, hipStream_t s) {
    const int rowgrid = d.P > 1 ? d.Glr : d.Gl;                                                // reference order: P == 1, no comm-lean PCG
    const int grid = d.lean && mode == 1 && d.G > rowgrid ? d.G : rowgrid;                     // comm-lean: the column workgroups' p.p partials ride along
    if (rf && rf->valued) REF_LAUNCH(bigref_k_rows_v, grid, mode); else BIG_LAUNCH(big_k_rows, grid, mode);
    return hipGetLastError();
}
hipError_t big_launch_pcg_lean(const BigDev &d, int *parity, hipStream_t s) { BIG_LAUNCH(big_k_pcg_lean, d.G); return hipGetLastError(); }
hipError_t big_launch_rank_sum_qq(const double *g, int W, long count, long stride, double *out, double *qq_part, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(big_k_rank_sum_qq, dim3((unsigned)((count + T - 1) / T)), dim3(T), 0, s, g, W, count, stride, out, qq_part);
    return hipGetLastError();
}
hipError_t big_launch_resid(const BigDev &d, const BigRef *rf, int *parity, hipStream_t s) {
    if (!rf) BIG_LAUNCH(big_k_resid, d.G); else if (rf->valued) REF_LAUNCH(bigref_k_resid_v, d.G); else REF_LAUNCH(bigref_k_resid, d.G);
    return hipGetLastError();
}
hipError_t big_launch_pcg_cols(const BigDev &d, const BigRef *rf, int *parity, hipStream_t s) {
    if (!rf) BIG_LAUNCH(big_k_pcg_cols, d.G); else if (rf->valued) REF_LAUNCH(bigref_k_pcg_cols_v, d.G); else REF_LAUNCH(bigref_k_pcg_cols, d.G);
    return hipGetLastError();
}
hipError_t big_launch_pcg_upd(const BigDev &d, const BigRef *rf, int *parity, hipStream_t s) {
    if (rf) REF_LAUNCH(bigref_k_pcg_upd, d.G); else BIG_LAUNCH(big_k_pcg_upd, d.G);
    return hipGetLastError();
}
hipError_t big_launch_post(const BigDev &d, const BigRef *rf, int *parity, hipStream_t s) {
    if (rf) REF_LAUNCH(bigref_k_post, d.G); else BIG_LAUNCH(big_k_post, d.G);
    return hipGetLastError();
}
hipError_t big_launch_z4(const BigDev &d, int init_only, int *parity, hipStream_t s) { BIG_LAUNCH(big_k_z4, d.Gl, init_only); return hipGetLastError(); }

// ---- a batch in lockstep: grid (X, B), X = BigBatchGrid's maximum of that kernel's own extent over the B problems ----
#define BIGB_LAUNCH(kernel, X, ...)                                                                              \
    do {                                                                                                         \
        hipLaunchKernelGGL(kernel, dim3(X, g.B), dim3(T), 0, s, devs, *parity, *parity ^ 1, ##__VA_ARGS__);      \
        *parity ^= 1;                                                                                            \
    } while (0)

hipError_t bigb_launch_set_window(const BigDev *devs, const BigBatchGrid &g, int iter_start, int iter_end, int *parity, hipStream_t s) {
    hipLaunchKernelGGL(big_kb_set_window, dim3(1, g.B), dim3(1), 0, s, devs, *parity, *parity ^ 1, iter_start, iter_end);
    *parity ^= 1;
    return hipGetLastError();
}
hipError_t bigb_launch_resume(const BigDev *devs, const BigBatchGrid &g, int reset_pcg_max, int *parity, hipStream_t s) {
    hipLaunchKernelGGL(big_kb_resume, dim3(1, g.B), dim3(1), 0, s, devs, *parity, *parity ^ 1, reset_pcg_max);
    *parity ^= 1;
    return hipGetLastError();
}
hipError_t bigb_launch_prep(const BigDev *devs, const BigBatchGrid &g, int do_prep, int *parity, hipStream_t s) { BIGB_LAUNCH(big_kb_prep, g.cols, do_prep); return hipGetLastError(); }
hipError_t bigb_enqueue_pcg(const BigDev *devs, const BigBatchGrid &g, int pairs, int *parity, hipStream_t s) {
    for (int k = 0; k < pairs; k++) {
        BIGB_LAUNCH(big_kb_rows, g.rows, 1);
        BIGB_LAUNCH(big_kb_pcg_cols, g.cols);
        BIGB_LAUNCH(big_kb_pcg_upd, g.cols);
    }
    return hipGetLastError();
}
hipError_t bigb_enqueue_tail(const BigDev *devs, const BigBatchGrid &g, int *parity, hipStream_t s) {
    BIGB_LAUNCH(big_kb_post, g.cols);
    BIGB_LAUNCH(big_kb_rows, g.rows, 0);
    BIGB_LAUNCH(big_kb_z4, g.z4);
    return hipGetLastError();
}
hipError_t bigb_launch_z4(const BigDev *devs, const BigBatchGrid &g, int *parity, hipStream_t s) { BIGB_LAUNCH(big_kb_z4, g.z4); return hipGetLastError(); }
hipError_t bigb_enqueue_iterations(const BigDev *devs, const BigBatchGrid &g, int iters, int kmax, int *parity, hipStream_t s) {
    for (int it = 0; it < iters; it++) {
        BIGB_LAUNCH(big_kb_prep, g.cols, 1);
        BIGB_LAUNCH(big_kb_y, g.y);
        BIGB_LAUNCH(big_kb_rhs_cols, g.cols);
        BIGB_LAUNCH(big_kb_rows, g.rows, 0);
        BIGB_LAUNCH(big_kb_resid, g.cols);
        hipError_t e = bigb_enqueue_pcg(devs, g, kmax, parity, s);
        if (e == hipSuccess) e = bigb_enqueue_tail(devs, g, parity, s);
        if (e != hipSuccess) return e;
    }
    return hipGetLastError();
}
hipError_t bigb_collect_states(const BigDev *devs, const BigBatchGrid &g, int parity, BigState *out, hipStream_t s) {
    hipLaunchKernelGGL(big_kb_collect, dim3(g.B), dim3(1), 0, s, devs, parity, out);
    return hipGetLastError();
}

// ---- early-fixing windows of a batch ----
hipError_t bigb_launch_set_window_l2f(const BigDev *devs, const BigBatchGrid &g, int iter_start, int iter_end, int *parity, hipStream_t s) {
    hipLaunchKernelGGL(big_kb_set_window_l2f, dim3(1, g.B), dim3(1), 0, s, devs, *parity, *parity ^ 1, iter_start, iter_end);
    *parity ^= 1;
    return hipGetLastError();
}
#define BIGB_FIX_LAUNCH(kernel, X, ...)                                                                               \
    do {                                                                                                              \
        hipLaunchKernelGGL(kernel, dim3(X, g.B), dim3(T), 0, s, devs, par, *parity, *parity ^ 1, ##__VA_ARGS__);      \
        *parity ^= 1;                                                                                                 \
    } while (0)
hipError_t bigb_enqueue_fix(const BigDev *devs, const BigFixPar *par, const BigBatchGrid &g, int *parity, hipStream_t s) {
    hipLaunchKernelGGL(big_kb_fix1, dim3(g.cols, g.B), dim3(T), 0, s, devs, par);
    hipLaunchKernelGGL(big_kb_fin, dim3(1, g.B), dim3(T), 0, s, devs, par, 1, BIG_PH_X);      // fix_obj = b2.x2
    BIGB_FIX_LAUNCH(big_kb_fix_rows, g.rows, 0);                                               // q = E2 * x2
    BIGB_FIX_LAUNCH(big_kb_fix2, g.y);
    hipLaunchKernelGGL(big_kb_fin, dim3(1, g.B), dim3(T), 0, s, devs, par, 1, BIG_PH_X);      // |x_live|^2
    BIGB_FIX_LAUNCH(big_kb_fix3, g.cols);
    BIGB_FIX_LAUNCH(big_kb_fix_rows, g.rows, 1);                                               // E * x (live columns) for the first y3
    BIGB_FIX_LAUNCH(big_kb_z4_init, g.z4);
    return hipGetLastError();
}
hipError_t bigb_launch_clear_xhist(const BigDev *devs, const BigBatchGrid &g, long max_total, hipStream_t s) {
    if (max_total <= 0) return hipSuccess;
    const int X = (int)std::min<long>((max_total + 1023) / 1024, 1024);
    hipLaunchKernelGGL(big_kb_clear_xhist, dim3(X, g.B), dim3(256), 0, s, devs);
    return hipGetLastError();
}
hipError_t bigb_launch_decide(const BigDev *devs, const BigFixPar *par, const BigBatchGrid &g, int max_rows, const float *scores, const uint8_t *codes,
                              double hi, double lo, int *counts, hipStream_t s) {
    if (max_rows <= 0) return hipSuccess;
    const int X = std::min((max_rows + T - 1) / T, 1024);
    hipLaunchKernelGGL(big_kb_decide, dim3(X, g.B), dim3(T), 0, s, devs, par, scores, codes, hi, lo, counts);
    return hipGetLastError();
}
hipError_t bigb_launch_compact(const BigDev *devs, const BigFixPar *par, const BigBatchGrid &g, hipStream_t s) {
    hipLaunchKernelGGL(big_kb_compact, dim3(g.B), dim3(BIG_CT), 0, s, devs, par);
    return hipGetLastError();
}
hipError_t bigb_launch_pack(const BigDev *devs, const BigFixPar *par, const BigBatchGrid &g, int max_rows, int ws, double *out, hipStream_t s) {
    if (max_rows <= 0 || ws <= 0) return hipSuccess;
    const int X = (int)std::min<long>(((long)max_rows * ws + 255) / 256, 4096);
    hipLaunchKernelGGL(big_kb_pack, dim3(X, g.B), dim3(256), 0, s, devs, par, ws, out);
    return hipGetLastError();
}
