// lpbox_big_ref_kernels.hip -- gfx950 kernels of the large-instance LP path in the REFERENCE's summation order
// (lpbox_big_set_order(LPBOX_ORDER_REFERENCE), one rank; specification: oracle/lpbox_oracle.c in LPO_ORDER_EIGEN).
// The chain is the one of lpbox_big_kernels.hip, launch for launch, and its bodies are the same ones (lpbox_big_dev.h).  What this file
// adds:
//   * the Staged policy: a body that fed a reduction writes its per-variable terms into BigRef::stage at the variable's live rank
//     (bigref_k_rank) and sums nothing; bigref_k_walk, in the place of big_k_fin, adds them up in Eigen's redux association and writes
//     BigDev::red, which the consumers read as they do on the route with a reduction launch (BigDev::fold is off);
//   * the entries of the bodies with that policy (bigref_k_*), and with it and VALUED (bigref_k_*_v): the stored values of E as factors
//     and rho4_E_transpose per entry (r4v) instead of the scalar r4Et;
//   * the same entries for a BATCH of problems in lockstep (bigref_kb_*, grid (X, B); lpbox_big_batch_* with every member in this order),
//     unit and valued members side by side, with one walker per member (bigref_kb_walk), and their launch helpers (bigrefb_*).
// Bodies that neither feed a reduction nor touch a value (y, rhs_cols, rows, fix3; z4 and the state kernels) have no staged unit entry:
// the unit instance runs their default entries, which already sum every row and column by one lane in ascending order from +0.0.
// The entries have external linkage: the launch helpers of both orders are in lpbox_big_kernels.hip.
#include "lpbox_big_dev.h"

namespace {

__device__ __forceinline__ double *stg(const BigDev &d, const BigRef &rf, int phase, int v) {
    return rf.stage + (size_t)(big_ref_stage_off(phase) + v) * d.n_loc;
}

// The terms of a LIVE variable go to stage[phase][k][where the variable stands among the summed ones]; nothing is added, nothing flushed:
// no LDS, no barrier.  AT_RANK: the live rank.  AT_FRANK: the rank among the variables fixed by the current call (fix1).  AT_INDEX: the
// variable's own index (init: every variable is live, and bigref_k_rank runs behind it).
enum StageAt { AT_RANK, AT_FRANK, AT_INDEX };
template <StageAt AT> struct Staged {
    static constexpr bool wg_sums = false;
    const BigRef &rf;
    template <int NV> struct Acc {
        double *const row0;
        const int *const at;
        const size_t pitch;
        __device__ __forceinline__ Acc(const BigDev &d, const Staged &sp, int phase)
            : row0(stg(d, sp.rf, phase, 0)), at(AT == AT_FRANK ? sp.rf.frank : sp.rf.rank), pitch((size_t)d.n_loc) {}
        template <typename... D> __device__ __forceinline__ void add(int j, bool live, D... t) {
            static_assert(sizeof...(D) == NV, "one term per value");
            if (!live) return;
            const int pos = AT == AT_INDEX ? j : at[j];
            const double a[NV] = {t...};
#pragma unroll
            for (int k = 0; k < NV; k++) row0[(size_t)k * pitch + pos] = a[k];
        }
        __device__ __forceinline__ void flush(const BigDev &, double *, int &) {}
    };
};
using AtRank = Staged<AT_RANK>;

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
__device__ __forceinline__ void bigref_b_walk(const BigDev &d, const BigRef &rf, int nv, int soff, int roff, int which, int sidx, int pcg) {
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
__global__ void __launch_bounds__(T) bigref_k_walk(BigDev d, BigRef rf, int nv, int soff, int roff, int which, int sidx, int pcg) { bigref_b_walk(d, rf, nv, soff, roff, which, sidx, pcg); }

// ---- a BATCH in lockstep (lpbox_big_batch_* with every member in the reference order), grid (X, B) as the
// big_kb_* entries of lpbox_big_kernels.hip: row blockIdx.y runs member blockIdx.y's own body on devs[blockIdx.y] and refs[blockIdx.y]; a
// workgroup at or beyond the member's own extent leaves first thing, before any barrier or store.  Unit and valued members share a
// launch: ONE entry per phase with a branch on the member's `valued`, uniform over the workgroup, between the two instantiations the
// member's solo chain picks between on the host -- for rhs_cols and rows that is (AtRank, valued) against the default entry's
// (WgSums, unit) body, which reads d.red because the reference order runs with BigDev::fold off.  The exception is y: with both
// instantiations in one entry it needs 75 VGPRs, one occupancy step below bigref_k_y_v (71: 7 waves per SIMD), so y has one entry per
// kind (72 VGPRs each) over the same grid, each leaving first thing on members of the other kind; the host skips the launch of a kind
// the batch does not have.  No body is touched.
// The walker: one workgroup per member, grid (1, B).  nv, the offsets, which, sidx and pcg are the same for every member of a lockstep
// launch; the early-out, the size (the member's own cnt[which]) and n_loc are the member's own.
#define KB_MEMBER(ext)                                \
    const BigDev &d = devs[blockIdx.y];               \
    if ((int)blockIdx.x >= ext(d)) return;            \
    const BigRef &rf = refs[blockIdx.y]
__global__ void __launch_bounds__(T) bigref_kb_walk(const BigDev *__restrict__ devs, const BigRef *__restrict__ refs, int nv, int soff, int roff, int which, int sidx, int pcg) {
    bigref_b_walk(devs[blockIdx.y], refs[blockIdx.y], nv, soff, roff, which, sidx, pcg);
}
__global__ void __launch_bounds__(T) bigref_kb_prep(const BigDev *__restrict__ devs, const BigRef *__restrict__ refs, int in, int out, int do_prep) { KB_MEMBER(ext_cols); big_b_prep(d, AtRank{rf}, in, out, do_prep); }
__global__ void __launch_bounds__(T) bigref_kb_y_u(const BigDev *__restrict__ devs, const BigRef *__restrict__ refs, int in, int out) {
    KB_MEMBER(ext_y);
    if (rf.valued) return;
    big_b_y<WgSums, false>(d, WgSums{}, in, out);
}
__global__ void __launch_bounds__(T) bigref_kb_y_v(const BigDev *__restrict__ devs, const BigRef *__restrict__ refs, int in, int out) {
    KB_MEMBER(ext_y);
    if (!rf.valued) return;
    big_b_y<AtRank, true>(d, AtRank{rf}, in, out);
}
__global__ void __launch_bounds__(T) bigref_kb_rhs_cols(const BigDev *__restrict__ devs, const BigRef *__restrict__ refs, int in, int out) {
    KB_MEMBER(ext_cols);
    if (rf.valued) big_b_rhs_cols<AtRank, true>(d, AtRank{rf}, in, out); else big_b_rhs_cols<WgSums, false>(d, WgSums{}, in, out);
}
__global__ void __launch_bounds__(T) bigref_kb_rows(const BigDev *__restrict__ devs, const BigRef *__restrict__ refs, int in, int out, int mode) {
    KB_MEMBER(ext_rows);
    if (rf.valued) big_b_rows<AtRank, true>(d, AtRank{rf}, in, out, mode); else big_b_rows<WgSums, false>(d, WgSums{}, in, out, mode);
}
__global__ void __launch_bounds__(T) bigref_kb_resid(const BigDev *__restrict__ devs, const BigRef *__restrict__ refs, int in, int out) {
    KB_MEMBER(ext_cols);
    if (rf.valued) big_b_resid<AtRank, true>(d, AtRank{rf}, in, out); else big_b_resid<AtRank, false>(d, AtRank{rf}, in, out);
}
__global__ void __launch_bounds__(T) bigref_kb_pcg_cols(const BigDev *__restrict__ devs, const BigRef *__restrict__ refs, int in, int out) {
    KB_MEMBER(ext_cols);
    if (rf.valued) big_b_pcg_cols<AtRank, true>(d, AtRank{rf}, in, out); else big_b_pcg_cols<AtRank, false>(d, AtRank{rf}, in, out);
}
__global__ void __launch_bounds__(T) bigref_kb_pcg_upd(const BigDev *__restrict__ devs, const BigRef *__restrict__ refs, int in, int out) { KB_MEMBER(ext_cols); big_b_pcg_upd(d, AtRank{rf}, in, out); }
__global__ void __launch_bounds__(T) bigref_kb_post(const BigDev *__restrict__ devs, const BigRef *__restrict__ refs, int in, int out) { KB_MEMBER(ext_cols); big_b_post(d, AtRank{rf}, in, out); }

}  // namespace

// ---- the staged entries (declared in lpbox_big.h, launched by the helpers in lpbox_big_kernels.hip) ----
__global__ void __launch_bounds__(T) bigref_k_init(BigDev d, BigRef rf, double c1) { big_b_init(d, Staged<AT_INDEX>{rf}, c1); }
__global__ void __launch_bounds__(T) bigref_k_prep(BigDev d, BigRef rf, int in, int out, int do_prep) { big_b_prep(d, AtRank{rf}, in, out, do_prep); }
__global__ void __launch_bounds__(T) bigref_k_y_v(BigDev d, BigRef rf, int in, int out) { big_b_y<AtRank, true>(d, AtRank{rf}, in, out); }
__global__ void __launch_bounds__(T) bigref_k_rhs_cols_v(BigDev d, BigRef rf, int in, int out) { big_b_rhs_cols<AtRank, true>(d, AtRank{rf}, in, out); }
__global__ void __launch_bounds__(T) bigref_k_rows_v(BigDev d, BigRef rf, int in, int out, int mode) { big_b_rows<AtRank, true>(d, AtRank{rf}, in, out, mode); }
__global__ void __launch_bounds__(T) bigref_k_resid(BigDev d, BigRef rf, int in, int out) { big_b_resid<AtRank, false>(d, AtRank{rf}, in, out); }
__global__ void __launch_bounds__(T) bigref_k_resid_v(BigDev d, BigRef rf, int in, int out) { big_b_resid<AtRank, true>(d, AtRank{rf}, in, out); }
__global__ void __launch_bounds__(T) bigref_k_pcg_cols(BigDev d, BigRef rf, int in, int out) { big_b_pcg_cols<AtRank, false>(d, AtRank{rf}, in, out); }
__global__ void __launch_bounds__(T) bigref_k_pcg_cols_v(BigDev d, BigRef rf, int in, int out) { big_b_pcg_cols<AtRank, true>(d, AtRank{rf}, in, out); }
__global__ void __launch_bounds__(T) bigref_k_pcg_upd(BigDev d, BigRef rf, int in, int out) { big_b_pcg_upd(d, AtRank{rf}, in, out); }
__global__ void __launch_bounds__(T) bigref_k_post(BigDev d, BigRef rf, int in, int out) { big_b_post(d, AtRank{rf}, in, out); }
// early fixing: the terms of b2.x2 at the rank among the newly fixed (:1237), of |x_live|^2 at the NEW live rank (:1223): bigref_k_rank
// with modes 1 and 2 has run before these launches
__global__ void __launch_bounds__(T) bigref_k_fix1(BigDev d, BigRef rf) { big_b_fix1(d, Staged<AT_FRANK>{rf}); }
__global__ void __launch_bounds__(T) bigref_k_fix2(BigDev d, BigRef rf, int in, int out) { big_b_fix2(d, AtRank{rf}, in, out); }
__global__ void __launch_bounds__(T) bigref_k_fix3_v(BigDev d, BigRef rf, int in, int out, long n_live_new, double c1_new) { big_b_fix3<AtRank, true>(d, AtRank{rf}, in, out, n_live_new, c1_new); }

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

// ---- the lockstep batch in the reference order: the launches of enqueue_iteration (lpbox_big_capi.hip) with a BigRef, launch for launch ----
#define BIGREFB_LAUNCH(kernel, X, ...)                                                                                 \
    do {                                                                                                               \
        hipLaunchKernelGGL(kernel, dim3(X, g.B), dim3(T), 0, s, devs, refs, *parity, *parity ^ 1, ##__VA_ARGS__);      \
        *parity ^= 1;                                                                                                  \
    } while (0)
// a walk flips no parity; its sidx is the parity where it is enqueued, i.e. the state its producer has just written
#define BIGREFB_WALK(nv, phase)                                                                                                         \
    hipLaunchKernelGGL(bigref_kb_walk, dim3(1, g.B), dim3(T), 0, s, devs, refs, nv, big_ref_stage_off(phase), (phase) * BIG_NPART, 0, *parity, \
                       ((phase) == BIG_PH_C || (phase) == BIG_PH_D) ? 1 : 0)

hipError_t bigrefb_launch_prep(const BigDev *devs, const BigRef *refs, const BigBatchGrid &g, int do_prep, int *parity, hipStream_t s) {
    BIGREFB_LAUNCH(bigref_kb_prep, g.cols, do_prep);
    return hipGetLastError();
}
hipError_t bigrefb_enqueue_pcg(const BigDev *devs, const BigRef *refs, const BigBatchGrid &g, int pairs, int *parity, hipStream_t s) {
    for (int k = 0; k < pairs; k++) {
        BIGREFB_LAUNCH(bigref_kb_rows, g.rows, 1);
        BIGREFB_LAUNCH(bigref_kb_pcg_cols, g.cols);
        BIGREFB_WALK(1, BIG_PH_C);
        BIGREFB_LAUNCH(bigref_kb_pcg_upd, g.cols);
        BIGREFB_WALK(2, BIG_PH_D);
    }
    return hipGetLastError();
}
hipError_t bigrefb_enqueue_tail(const BigDev *devs, const BigRef *refs, const BigBatchGrid &g, int *parity, hipStream_t s) {
    BIGREFB_LAUNCH(bigref_kb_post, g.cols);
    BIGREFB_WALK(5, BIG_PH_E);
    BIGREFB_LAUNCH(bigref_kb_rows, g.rows, 0);
    return bigb_launch_z4(devs, g, parity, s);
}
hipError_t bigrefb_enqueue_iterations(const BigDev *devs, const BigRef *refs, const BigBatchGrid &g, int kinds, int iters, int kmax, int *parity, hipStream_t s) {
    if (!(kinds & (BIGREF_KIND_UNIT | BIGREF_KIND_VALUED))) return hipErrorInvalidValue;
    for (int it = 0; it < iters; it++) {
        BIGREFB_LAUNCH(bigref_kb_prep, g.cols, 1);
        BIGREFB_WALK(1, BIG_PH_A);
        // y: one launch per kind of member in the batch, both on the same (in, out) -- every member's state moves once
        if (kinds & BIGREF_KIND_UNIT) hipLaunchKernelGGL(bigref_kb_y_u, dim3(g.y, g.B), dim3(T), 0, s, devs, refs, *parity, *parity ^ 1);
        if (kinds & BIGREF_KIND_VALUED) hipLaunchKernelGGL(bigref_kb_y_v, dim3(g.y, g.B), dim3(T), 0, s, devs, refs, *parity, *parity ^ 1);
        *parity ^= 1;
        BIGREFB_LAUNCH(bigref_kb_rhs_cols, g.cols);
        BIGREFB_LAUNCH(bigref_kb_rows, g.rows, 0);
        BIGREFB_LAUNCH(bigref_kb_resid, g.cols);
        BIGREFB_WALK(3, BIG_PH_B);
        hipError_t e = bigrefb_enqueue_pcg(devs, refs, g, kmax, parity, s);
        if (e == hipSuccess) e = bigrefb_enqueue_tail(devs, refs, g, parity, s);
        if (e != hipSuccess) return e;
    }
    return hipGetLastError();
}
