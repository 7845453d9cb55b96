// lpbox_lp_ref_kernels.hip -- the opt-in REFERENCE-ORDER LP kernels (lpbox_set_order(LPBOX_ORDER_REFERENCE)).
//
// Same algorithm and same state buffers as lp_window_kernel (LpBatchDev), but every sum is associated the way the reference's Eigen
// path associates it (the specification is oracle/lpbox_oracle.c in LPO_ORDER_EIGEN):
//   * dot / squaredNorm over the live n-vectors: Eigen 3.3.8 SSE2 redux (Core/Redux.h, LinearVectorizedTraversal) -- four packet
//     accumulators started at elements 0..3, each adding every 4th element, then (p0a + p1a) + (p0b + p1b), a left-over pair, a last
//     odd element.  Element k is the k-th LIVE variable in ascending original index (the reference compacts on a fix);
//   * E v: each row summed in ascending column order from +0.0 (one accumulator per row, no lane split);
//   * E^T w and (rho4 E^T) w: each column summed in ascending row order from +0.0 (no helper split).
// Layout: one workgroup of RT threads per instance, variable j at storage position j (identity), row i at row slot i; thread t owns
// variables / rows t, t + RT, ... (EPT slots).  The index sets of E sit in LDS as u16 CSR and CSC.  A reduction scatters its products
// to an LDS staging buffer at the live rank of each variable (a block prefix sum over the live mask, rebuilt at launch and after a fix);
// then four lanes of wave 0 walk the four chains of the redux.  Independent reductions ride on different lane groups of that wave at
// the same time (up to NSTG of them), so they cost one walk.
// VALUED variants (a batch in which some instance stores a value other than 1.0): every entry of a row / column sum
// is val * v, rounded, then added; rho4_E_transpose is an array r4v with one entry per stored entry (CSC order), set to rho4 * val and
// scaled in place by learning_fact exactly as the reference does, kept in global memory between launches.  The values sit in LDS behind
// the carve-up below (VLDS) or stay in global memory.  The unit variants are the code as it was and never touch the values.
// Built with -ffp-contract=off like the rest of the library.  The one known deviation from the reference: the std stop test takes
// sqrt where the reference calls pow(v, 1/2) (glibc pow is not correctly rounded; the oracle counts the disagreements).
#include "lpbox_lp.h"
#include "lpbox_eigen_redux.h"

#include <float.h>

namespace {

constexpr int RT = 512;           // threads per instance
constexpr int RNW = RT / 64;      // wavefronts per instance
constexpr int NSTG = 3;           // staging buffers = reductions walked together

// LDS carve-up shared by the launcher (size) and the kernels (pointers)
struct RefLds {
    size_t rs_ptr, cs_ptr, rs_col, cs_row, gx, gl, stage, res, rank, flag, wsum, total;
    __host__ __device__ RefLds(int NS, int LS, int ZS) {
        size_t o = 0;
        auto take = [&](size_t bytes) { size_t at = o; o += (bytes + 15) & ~size_t(15); return at; };
        rs_ptr = take(sizeof(int) * ((size_t)LS + 1));       // row i: entries rs_ptr[i] .. rs_ptr[i + 1] of rs_col
        cs_ptr = take(sizeof(int) * ((size_t)NS + 1));       // column j: entries cs_ptr[j] .. cs_ptr[j + 1] of cs_row
        rs_col = take(sizeof(uint16_t) * (size_t)ZS);        // column indices of each row, ascending
        cs_row = take(sizeof(uint16_t) * (size_t)ZS);        // row indices of each column, ascending
        gx = take(sizeof(double) * (size_t)NS);              // the n-vector being row-gathered (fixed variables hold +0.0)
        gl = take(sizeof(double) * 2 * (size_t)LS);          // two l-vectors interleaved, gl[2 i + c], being column-gathered
        stage = take(sizeof(double) * NSTG * (size_t)NS);    // products of the reductions, by live rank
        res = take(sizeof(double) * 16);                     // reduction results
        rank = take(sizeof(uint16_t) * (size_t)NS);          // prefix sum of the flags below
        flag = take((size_t)NS);
        wsum = take(sizeof(int) * RNW);
        total = o;
    }
};

// (the walk itself -- Eigen's redux with Packet2d over a[0 .. size), one accumulator per lane of a group of four -- is er_walk of
// lpbox_eigen_redux.h, shared with the BQP batch)

// NR (<= 16) reductions of `size` staged products each (buffer k at stage + k * sst); every thread receives the sums.  The barrier on
// entry publishes the products, the one on exit the results (and frees the staging buffers for the next reduction).
template <int NR>
__device__ __forceinline__ void eigen_reduce(const double *stage, int sst, int size, double *res, double (&out)[NR]) {
    static_assert(NR >= 1 && NR <= NSTG, "staging buffers");
    __syncthreads();
    const int tid = threadIdx.x;
    if (tid < 4 * NR) {
        const int g = tid >> 2;
        const double r = er_walk(stage + (size_t)g * sst, size, tid & 3);
        if ((tid & 3) == 0) res[g] = r;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NR; k++) out[k] = res[k];
}

// acc = (((+0.0 + src[idx[b]]) + src[idx[b + 1]]) + ...) over idx[b .. e), src element i at src[STRIDE * i]
template <int STRIDE>
__device__ __forceinline__ double seq_gather(const uint16_t *idx, int b, int e, const double *src) {
    double acc = 0.0;
    int k = b;
    for (; k + 4 <= e; k += 4) {
        const double v0 = src[STRIDE * idx[k]], v1 = src[STRIDE * idx[k + 1]], v2 = src[STRIDE * idx[k + 2]], v3 = src[STRIDE * idx[k + 3]];
        acc = acc + v0; acc = acc + v1; acc = acc + v2; acc = acc + v3;
    }
    for (; k < e; k++) acc = acc + src[STRIDE * idx[k]];
    return acc;
}

// the same with stored values: acc = ((+0.0 + val[b] * src[idx[b]]) + val[b + 1] * src[idx[b + 1]]) + ..., every product rounded first
template <int STRIDE>
__device__ __forceinline__ double seq_gather_val(const uint16_t *idx, const double *val, int b, int e, const double *src) {
    double acc = 0.0;
    int k = b;
    for (; k + 4 <= e; k += 4) {
        const double p0 = val[k] * src[STRIDE * idx[k]], p1 = val[k + 1] * src[STRIDE * idx[k + 1]];
        const double p2 = val[k + 2] * src[STRIDE * idx[k + 2]], p3 = val[k + 3] * src[STRIDE * idx[k + 3]];
        acc = acc + p0; acc = acc + p1; acc = acc + p2; acc = acc + p3;
    }
    for (; k < e; k++) acc = acc + val[k] * src[STRIDE * idx[k]];
    return acc;
}

// VALUED kernels: rho4_E_transpose = rho4 * E_transpose (LPcpp:2293) and rho4_E_transpose *= learning_fact (:864), entry by entry.  A thread
// keeps the entries of its own columns j = s * RT + tid (cs_ptr[j] .. cs_ptr[j + 1] of the CSC order), the only ones it ever reads, so no
// barrier orders these writes.  (Free functions: a lambda in the window kernel would perturb the code of the unit variants.)
template <int EPT>
__device__ __forceinline__ void r4v_set(double *r4v, const double *vc, const int *cs_ptr, int n, double rho4) {
#pragma unroll
    for (int s = 0; s < EPT; s++) {
        const int j = s * RT + (int)threadIdx.x;
        if (j < n) for (int k = cs_ptr[j]; k < cs_ptr[j + 1]; k++) r4v[k] = rho4 * vc[k];
    }
}
template <int EPT>
__device__ __forceinline__ void r4v_scale(double *r4v, const int *cs_ptr, int n, double fct) {
#pragma unroll
    for (int s = 0; s < EPT; s++) {
        const int j = s * RT + (int)threadIdx.x;
        if (j < n) for (int k = cs_ptr[j]; k < cs_ptr[j + 1]; k++) r4v[k] = fct * r4v[k];
    }
}

// ------------------------------------------------------------------------------------------------
// ADMM_lp_iters_init (LPcpp:489-763): lp_init_kernel with best_bin_obj = b.dot(x0) in Eigen's order
// ------------------------------------------------------------------------------------------------
template <bool VALUED>
__global__ void __launch_bounds__(RT) lp_ref_init_kernel(LpBatchDev bd, const double *f_org, const double *c1_init, const uint8_t *live_init,
                                                         LpRefVals vv) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const RefLds L(bd.NS, bd.LS, bd.ZS);
    double *stage = (double *)(smem + L.stage), *res = (double *)(smem + L.res);
    const int inst = blockIdx.x, tid = threadIdx.x;
    int *isc = bd.isc + (size_t)inst * NI_COUNT;
    double *dsc = bd.dsc + (size_t)inst * ND_COUNT;
    const int n = isc[NI_N], l = isc[NI_L];
    const size_t on = (size_t)inst * bd.NS, ol = (size_t)inst * bd.LS;
    for (int pos = tid; pos < bd.NS; pos += RT) {
        const bool isvar = live_init[on + pos] != 0;   // identity layout: positions 0 .. n-1
        bd.x[on + pos] = isvar ? 1.0 : 0.0;            // :583-586
        bd.z1[on + pos] = 0.0; bd.z2[on + pos] = 0.0;  // :616-617
        bd.pd[on + pos] = 0.0;
        bd.live[on + pos] = isvar ? 1 : 0;
        if (pos < n) stage[pos] = bd.b[on + pos] * 1.0;   // products of b.dot(x0), :727
    }
    for (int i = tid; i < l; i += RT) { bd.z4[ol + i] = 0.0; bd.f[ol + i] = f_org[ol + i]; }   // :650
    if constexpr (VALUED)                                // rho4_E_transpose is built by the first iteration (what ND_R4ET = 0 says below)
        for (int k = tid; k < isc[NI_NNZ]; k += RT) vv.r4v[(size_t)inst * bd.ZS + k] = 0.0;
    double bb[1];
    eigen_reduce<1>(stage, bd.NS, n, res, bb);
    if (tid == 0) {
        dsc[ND_RHO1] = LP_RHO0; dsc[ND_RHO2] = LP_RHO0; dsc[ND_RHO4] = LP_RHO0;             // :623-630
        dsc[ND_PREV_RHO1] = LP_RHO0; dsc[ND_PREV_RHO2] = LP_RHO0; dsc[ND_PREV_RHO4] = LP_RHO0;
        dsc[ND_GAMMA] = LP_GAMMA0;
        dsc[ND_DI] = 0.0; dsc[ND_R4ET] = 0.0; dsc[ND_RCR] = 0.0;
        dsc[ND_STD_OBJ] = 1.0;                       // LPh:219
        dsc[ND_CUR_OBJ] = 0.0;                       // LPh:213
        dsc[ND_BEST_BIN_OBJ] = bb[0];
        dsc[ND_SUM_FIX_OBJ] = 0.0; dsc[ND_FIX_OBJ] = 0.0;   // :593-594
        dsc[ND_C1] = c1_init[inst];                  // pow(n, 1/p), p = 2 (:427,:503)
        dsc[ND_CVG1] = 0.0; dsc[ND_CVG2] = 0.0; dsc[ND_OBJ_VAL] = 0.0;
        dsc[ND_PREV_SUM] = 0.0; dsc[ND_PREV_OBJ] = 0.0;
        isc[NI_NLIVE] = n;
        isc[NI_RHO_UPDATED] = 1;                     // LPh:214
        isc[NI_ITER] = 0; isc[NI_HIST_N] = 0; isc[NI_RET] = 0; isc[NI_STOP] = 0;
        isc[NI_PCG_TOTAL] = 0; isc[NI_OUTER_TOTAL] = 0; isc[NI_LAST_PCG] = 0; isc[NI_PLAIN_ITER_P1] = 0;
        isc[NI_EXPR_READY] = 0; isc[NI_H_VALID] = 0;
        for (int k = 0; k < LP_HIST; k++) bd.hist[(size_t)inst * LP_HIST + k] = 0.0;
    }
}

// ------------------------------------------------------------------------------------------------
// The ADMM window in the reference's order: iterations [iter_start, iter_end) of ADMM_lp_iters (LPcpp:766-1095, mode bit 0 clear) or
// ADMM_lp_iters_l2f (LPcpp:1098-1574, bit 0 set); bit 1 keeps x after every iteration in xhist.  Same phases, same expressions and the
// same saved state as lp_window_kernel; only the sums are associated differently.
// ------------------------------------------------------------------------------------------------
template <int EPT, bool VALUED, bool VLDS>
__global__ void __launch_bounds__(RT) lp_ref_window_kernel(LpBatchDev bd, int iter_start, int iter_end, int mode, LpRefVals vv) {
    const int l2f = mode & 1, rec = mode & 2;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int inst = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int *isc = bd.isc + (size_t)inst * NI_COUNT;
    double *dsc = bd.dsc + (size_t)inst * ND_COUNT;
    if (!isc[NI_ACTIVE]) return;

    const int n = isc[NI_N], l = isc[NI_L], nnz = isc[NI_NNZ];
    const int NS = bd.NS;
    const size_t on = (size_t)inst * NS, ol = (size_t)inst * bd.LS, oz = (size_t)inst * bd.ZS;
    const RefLds L(NS, bd.LS, bd.ZS);
    int *s_rs_ptr = (int *)(smem + L.rs_ptr), *s_cs_ptr = (int *)(smem + L.cs_ptr);
    uint16_t *s_rs_col = (uint16_t *)(smem + L.rs_col), *s_cs_row = (uint16_t *)(smem + L.cs_row);
    double *gx = (double *)(smem + L.gx), *gl = (double *)(smem + L.gl);
    double *stage = (double *)(smem + L.stage), *res = (double *)(smem + L.res);
    uint16_t *s_rank = (uint16_t *)(smem + L.rank);
    uint8_t *s_flag = (uint8_t *)(smem + L.flag);
    int *s_wsum = (int *)(smem + L.wsum);
    // VALUED: the values in CSR and CSC entry order and rho4_E_transpose (CSC entry order), in LDS behind the carve-up or in global memory
    const double *vr = nullptr, *vc = nullptr;
    double *r4v = nullptr;
    if constexpr (VALUED) {
        if constexpr (VLDS) { double *sv = (double *)(smem + L.total); vr = sv; vc = sv + bd.ZS; r4v = sv + 2 * (size_t)bd.ZS; }
        else { vr = vv.vr + oz; vc = vv.vc + oz; r4v = vv.r4v + oz; }
    }

    // ---- stage the index sets of E into LDS ----
    {
        const int *gp = bd.rs_ptr + (size_t)inst * (NS + 1), *gc = bd.cs_ptr + (size_t)inst * (NS + 1);
        for (int i = tid; i <= l; i += RT) s_rs_ptr[i] = gp[i];
        for (int j = tid; j <= n; j += RT) s_cs_ptr[j] = gc[j];
        for (int k = tid; k < nnz; k += RT) { s_rs_col[k] = bd.rs_col[oz + k]; s_cs_row[k] = bd.cs_row[oz + k]; }
        if constexpr (VALUED && VLDS) {
            double *sv = (double *)(smem + L.total);
            for (int k = tid; k < nnz; k += RT) {
                sv[k] = vv.vr[oz + k]; sv[bd.ZS + k] = vv.vc[oz + k]; sv[2 * (size_t)bd.ZS + k] = vv.r4v[oz + k];
            }
        }
    }

    // ---- per-thread state: variables j = s * RT + tid, rows i = s * RT + tid ----
    double x[EPT], z1[EPT], z2[EPT], bv[EPT], pd[EPT], dinv[EPT], esq[EPT];
    double z4[EPT], f[EPT], y3[EPT], Ex[EPT];
    bool live[EPT], rv[EPT];
    int rk[EPT];
#pragma unroll
    for (int s = 0; s < EPT; s++) {
        const int j = s * RT + tid;
        x[s] = bd.x[on + j]; z1[s] = bd.z1[on + j]; z2[s] = bd.z2[on + j]; bv[s] = bd.b[on + j]; pd[s] = bd.pd[on + j];
        live[s] = bd.live[on + j] != 0;
        esq[s] = j < n ? (double)(bd.cmeta[on + j] & 0x7FFF) : 0.0;   // Esq_diag_j = column length (entries are 1.0), LPcpp:2378-2390
        rv[s] = j < l;
        z4[s] = rv[s] ? bd.z4[ol + j] : 0.0;
        f[s] = rv[s] ? bd.f[ol + j] : 0.0;
        y3[s] = 0.0; Ex[s] = 0.0; dinv[s] = 1.0; rk[s] = 0;
    }
    double rho1 = dsc[ND_RHO1], rho2 = dsc[ND_RHO2], rho4 = dsc[ND_RHO4];
    double prev_rho1 = dsc[ND_PREV_RHO1], prev_rho2 = dsc[ND_PREV_RHO2], prev_rho4 = dsc[ND_PREV_RHO4];
    double gamma_val = dsc[ND_GAMMA], dI = dsc[ND_DI], r4Et = dsc[ND_R4ET], rcr = dsc[ND_RCR];
    double std_obj = dsc[ND_STD_OBJ], cur_obj = dsc[ND_CUR_OBJ], best_bin_obj = dsc[ND_BEST_BIN_OBJ];
    double sum_fix_obj = dsc[ND_SUM_FIX_OBJ], fix_obj = dsc[ND_FIX_OBJ], c1 = dsc[ND_C1];
    double cvg1 = dsc[ND_CVG1], cvg2 = dsc[ND_CVG2], obj_val = dsc[ND_OBJ_VAL];
    double prev_sum = dsc[ND_PREV_SUM], prev_obj = dsc[ND_PREV_OBJ];
    int n_live = isc[NI_NLIVE], rhoUpdated = isc[NI_RHO_UPDATED], hist_n = isc[NI_HIST_N];
    int pcg_total = isc[NI_PCG_TOTAL], outer_total = isc[NI_OUTER_TOTAL], last_pcg = isc[NI_LAST_PCG];
    int expr_ready = isc[NI_EXPR_READY];
    double h_reg[LP_HIST];
#pragma unroll
    for (int k = 0; k < LP_HIST; k++) h_reg[k] = bd.hist[(size_t)inst * LP_HIST + k];
    const double learning_fact = LP_LEARNING_FACT;
    int ret = 0, stop = LP_STOP_NONE;

    __syncthreads();   // index sets staged
    if constexpr (VALUED) {                                       // Esq_diag_j = sum of val^2 down column j, rows ascending, from +0.0 (:2378-2390)
#pragma unroll
        for (int s = 0; s < EPT; s++) {
            const int j = s * RT + tid;
            double e = 0.0;
            if (j < n) for (int k = s_cs_ptr[j]; k < s_cs_ptr[j + 1]; k++) e += vc[k] * vc[k];
            esq[s] = e;
        }
    }
    // out[s] = rank of this thread's variable of slot s among the flagged ones (ascending index); returns how many are flagged.
    // Thread t counts the flags of positions t*EPT .. t*EPT+EPT-1, a wave scan and the wave totals give every position its rank.
    auto rank_build = [&](const bool (&fl)[EPT], int (&out)[EPT]) {
#pragma unroll
        for (int s = 0; s < EPT; s++) s_flag[s * RT + tid] = fl[s] ? 1 : 0;
        __syncthreads();
        int cnt = 0;
#pragma unroll
        for (int e = 0; e < EPT; e++) cnt += s_flag[tid * EPT + e];
        int v = cnt;
        for (int off = 1; off < 64; off <<= 1) { const int u = __shfl_up(v, off, 64); if (lane >= off) v += u; }
        if (lane == 63) s_wsum[wv] = v;
        __syncthreads();
        int base = 0, total = 0;
#pragma unroll
        for (int w = 0; w < RNW; w++) { const int t = s_wsum[w]; if (w < wv) base += t; total += t; }
        int ex = base + v - cnt;
#pragma unroll
        for (int e = 0; e < EPT; e++) { s_rank[tid * EPT + e] = (uint16_t)ex; ex += s_flag[tid * EPT + e]; }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < EPT; s++) out[s] = s_rank[s * RT + tid];
        return total;
    };
    // the product of live slot s goes to position rank of staging buffer k
    auto put = [&](int k, int s, double v) { if (live[s]) stage[(size_t)k * NS + rk[s]] = v; };
    // (E gx)_i for this thread's rows; gx must have been published
    auto rows_sum = [&](double (&out)[EPT]) {
#pragma unroll
        for (int s = 0; s < EPT; s++) {
            const int i = s * RT + tid;
            if constexpr (VALUED) out[s] = rv[s] ? seq_gather_val<1>(s_rs_col, vr, s_rs_ptr[i], s_rs_ptr[i + 1], gx) : 0.0;
            else out[s] = rv[s] ? seq_gather<1>(s_rs_col, s_rs_ptr[i], s_rs_ptr[i + 1], gx) : 0.0;
        }
    };
    // (E^T gl[.][c])_j for this thread's variables; gl must have been published.  VALUED: c = 0 multiplies by the entries of
    // rho4_E_transpose (r4v), c = 1 by those of E_transpose (vc)
    auto cols_sum = [&](int c, double (&out)[EPT]) {
#pragma unroll
        for (int s = 0; s < EPT; s++) {
            const int j = s * RT + tid;
            if constexpr (VALUED) out[s] = j < n ? seq_gather_val<2>(s_cs_row, c == 0 ? r4v : vc, s_cs_ptr[j], s_cs_ptr[j + 1], gl + c) : 0.0;
            else out[s] = j < n ? seq_gather<2>(s_cs_row, s_cs_ptr[j], s_cs_ptr[j + 1], gl + c) : 0.0;
        }
    };
    auto publish_x = [&](const double (&v)[EPT]) {
#pragma unroll
        for (int s = 0; s < EPT; s++) gx[s * RT + tid] = live[s] ? v[s] : 0.0;
    };

    // ---- early fixing: apply this call's fix vector (LPcpp:1124-1335); the live ranks shift as the reference's compaction does ----
    bool finished = false, fixed_now = false;
    if (bd.ctl[(size_t)inst * 4 + 0]) {
        const int n_live_new = bd.ctl[(size_t)inst * 4 + 2];
        uint8_t nf[EPT];
        bool isf[EPT];
#pragma unroll
        for (int s = 0; s < EPT; s++) { nf[s] = bd.newfix[on + s * RT + tid]; isf[s] = nf[s] != 0; }
        const int nfix = rank_build(isf, rk);
#pragma unroll
        for (int s = 0; s < EPT; s++) if (isf[s]) stage[rk[s]] = bv[s] * (nf[s] == 2 ? 1.0 : 0.0);
        double fo[1];
        eigen_reduce<1>(stage, NS, nfix, res, fo);                // fix_obj = b2.dot(x2), ascending original index, :1237
        fix_obj = fo[0];
        if (n_live_new == 0) {                                    // :1212-1217 (nothing else is updated)
            ret = 1; stop = LP_STOP_ALLFIXED; n_live = 0; finished = true;
#pragma unroll
            for (int s = 0; s < EPT; s++) if (nf[s]) { live[s] = false; x[s] = nf[s] == 2 ? 1.0 : 0.0; }
        } else {
#pragma unroll
            for (int s = 0; s < EPT; s++) gx[s * RT + tid] = nf[s] == 2 ? 1.0 : 0.0;
            __syncthreads();
            double cnt[EPT];
            rows_sum(cnt);                                        // E2*x2 over the columns fixed now, :1276
#pragma unroll
            for (int s = 0; s < EPT; s++) {
                if (rv[s]) f[s] = f[s] - cnt[s];                  // f1 = f - E2*x2, :1278
                if (nf[s]) { live[s] = false; x[s] = nf[s] == 2 ? 1.0 : 0.0; }
            }
            prev_sum = sum_fix_obj; sum_fix_obj += fix_obj; prev_obj = cur_obj;   // :1247-1250
            n_live = n_live_new;
            c1 = bd.dctl[inst];
            dI = 0.0; dI += rho1 + rho2;                          // update_expression (:1329 -> :2289-2404)
#pragma unroll
            for (int s = 0; s < EPT; s++) { double v = dI; v += rho4 * esq[s]; pd[s] = v; }
            r4Et = rho4;
            if constexpr (VALUED) r4v_set<EPT>(r4v, vc, s_cs_ptr, n, rho4);
            expr_ready = 1;
            fixed_now = true;
        }
    }

    int it = iter_start;
    if (!finished) {
        const int nl = rank_build(live, rk);                      // live ranks = positions in the reference's compacted vectors
        if (fixed_now) {
            double px[1];
#pragma unroll
            for (int s = 0; s < EPT; s++) put(0, s, x[s] * x[s]);
            eigen_reduce<1>(stage, NS, nl, res, px);
            if (sqrt(px[0]) < 1e-3) ret = 1;                      // :1223
        }
        // DiagonalPreconditioner state (LPcpp:883-890) = 1/pd as of the last compute (as lp_window_kernel)
#pragma unroll
        for (int s = 0; s < EPT; s++) dinv[s] = (pd[s] != 0.0) ? 1.0 / pd[s] : 1.0;
        publish_x(x);
        __syncthreads();
        rows_sum(Ex);                                             // E*x for the first iteration's y3

        int cc = 0;
        for (; it < iter_end; ++it) {
            // ---------------- y1 (box), y2 (shifted L2 sphere), y3, LPcpp:806-828 ----------------
            double y1[EPT], y2[EPT];
#pragma unroll
            for (int s = 0; s < EPT; s++) {
                const double t = x[s] + z1[s] / rho1;
                y1[s] = t > 1 ? 1 : (t < 0 ? 0 : t);
                y2[s] = (x[s] + z2[s] / rho2) - 0.5;
                put(0, s, y2[s] * y2[s]);
                if (rv[s]) { const double v = f[s] - Ex[s] - z4[s] / rho4; y3[s] = v < 0 ? 0 : v; }
            }
            double pn[1];
            eigen_reduce<1>(stage, NS, nl, res, pn);
            const double c2 = 2 * sqrt(pn[0]);
#pragma unroll
            for (int s = 0; s < EPT; s++) y2[s] = y2[s] * c1 / c2 + 0.5;
            // ---------------- matrix-expression refresh, LPcpp:831-866 ----------------
            if (it == 0) {
                dI = 0.0; dI += rho1 + rho2;
#pragma unroll
                for (int s = 0; s < EPT; s++) { double v = dI; v += rho4 * esq[s]; pd[s] = v; }
                r4Et = rho4;
                if constexpr (VALUED) r4v_set<EPT>(r4v, vc, s_cs_ptr, n, rho4);
                expr_ready = 1;
            }
            if (it != 0 && rhoUpdated) {
                const double inc = rcr * (prev_rho1 + prev_rho2);
                const double inc4 = rcr * prev_rho4;
                dI += inc;
#pragma unroll
                for (int s = 0; s < EPT; s++) { double v = pd[s]; v += inc; v += inc4 * esq[s]; pd[s] = v; }
                r4Et = learning_fact * r4Et;                      // rho4_E_transpose *= learning_fact (:864)
                if constexpr (VALUED) r4v_scale<EPT>(r4v, s_cs_ptr, n, learning_fact);
            }
            const double r4 = r4Et;
            // ---------------- rhs (:872-878): (rho4 E^T)(f - y3) and E^T z4; every entry of the scaled product adds (rho4 * 1.0) * w_i,
            // the same value for every column of row i, so the row publishes r4 * w_i once.  VALUED: the row publishes w_i itself and
            // every entry multiplies it by its own r4v ----------------
#pragma unroll
            for (int s = 0; s < EPT; s++) {
                const int i = s * RT + tid;
                if constexpr (VALUED) { if (rv[s]) { gl[2 * i] = f[s] - y3[s]; gl[2 * i + 1] = z4[s]; } }
                else { if (rv[s]) { gl[2 * i] = r4 * (f[s] - y3[s]); gl[2 * i + 1] = z4[s]; } }
            }
            __syncthreads();
            double rhs[EPT];
            {
                double tA[EPT], tB[EPT];
                cols_sum(0, tA);
                cols_sum(1, tB);
#pragma unroll
                for (int s = 0; s < EPT; s++) {
                    double r_ = (rho1 * y1[s] + rho2 * y2[s]) - ((bv[s] + z1[s]) + z2[s]);
                    r_ += tA[s];
                    r_ -= tB[s];
                    rhs[s] = r_;
                }
            }
            if (rhoUpdated) {                                     // DiagonalPreconditioner::compute (:883-890)
#pragma unroll
                for (int s = 0; s < EPT; s++) dinv[s] = (pd[s] != 0.0) ? 1.0 / pd[s] : 1.0;
                rhoUpdated = 0;
            }
            // ---------------- PCG (LPcpp:251-335) on (dI*I + rho4 E^T E) x = rhs from x0 = y1 ----------------
            double xt[EPT], r[EPT], p[EPT], tcol[EPT];
            int k_it = 0;
            bool pcg_fail = false;
            publish_x(y1);
            __syncthreads();                                      // (also orders the rhs column reads before gl is rewritten)
            {
                double q[EPT];
                rows_sum(q);
#pragma unroll
                for (int s = 0; s < EPT; s++) if (rv[s]) gl[2 * (s * RT + tid)] = VALUED ? q[s] : r4 * q[s];
            }
            __syncthreads();
            cols_sum(0, tcol);
#pragma unroll
            for (int s = 0; s < EPT; s++) {
                xt[s] = y1[s];
                double Mx = 0.0;
                Mx += dI * (1.0 * xt[s]);
                Mx += tcol[s];
                r[s] = rhs[s] - Mx;                               // :268
                p[s] = dinv[s] * r[s];                            // :291
                put(0, s, rhs[s] * rhs[s]);                       // rhsNorm2 :271
                put(1, s, r[s] * r[s]);                           // residualNorm2 :282
                put(2, s, r[s] * p[s]);                           // absNew :294
            }
            double p3[3];
            eigen_reduce<3>(stage, NS, nl, res, p3);
            const double rhsNorm2 = p3[0];
            double residualNorm2 = p3[1], absNew = p3[2];
            if (rhsNorm2 == 0) {                                  // :273-278
#pragma unroll
                for (int s = 0; s < EPT; s++) xt[s] = 0.0;
            } else {
                double threshold = LP_PCG_TOL * LP_PCG_TOL * rhsNorm2;    // :281
                if (threshold < DBL_MIN) threshold = DBL_MIN;
                if (!(residualNorm2 < threshold)) {               // :284
                    while (k_it < LP_PCG_MAXITERS) {              // :296
                        publish_x(p);
                        __syncthreads();
                        {
                            double q[EPT];
                            rows_sum(q);
#pragma unroll
                            for (int s = 0; s < EPT; s++) if (rv[s]) gl[2 * (s * RT + tid)] = VALUED ? q[s] : r4 * q[s];
                        }
                        __syncthreads();
                        cols_sum(0, tcol);
                        double tmp[EPT];
#pragma unroll
                        for (int s = 0; s < EPT; s++) {           // tmp = M p (:298)
                            double Mp = 0.0;
                            Mp += dI * (1.0 * p[s]);
                            Mp += tcol[s];
                            tmp[s] = Mp;
                            put(0, s, p[s] * tmp[s]);
                        }
                        double p1[1];
                        eigen_reduce<1>(stage, NS, nl, res, p1);
                        const double alpha = absNew / p1[0];      // :300
                        if (alpha < 0) { pcg_fail = true; break; }    // :301
                        double z[EPT];
#pragma unroll
                        for (int s = 0; s < EPT; s++) {
                            xt[s] += alpha * p[s];                // :302
                            r[s] -= alpha * tmp[s];               // :304
                            z[s] = dinv[s] * r[s];                // :314
                            put(0, s, r[s] * r[s]);               // :305
                            put(1, s, r[s] * z[s]);               // :317
                        }
                        double p2[2];
                        eigen_reduce<2>(stage, NS, nl, res, p2);
                        residualNorm2 = p2[0];
                        if (residualNorm2 < threshold) { k_it++; break; }     // :309-312
                        const double absOld = absNew;
                        absNew = p2[1];
                        const double beta = absNew / absOld;      // :318
#pragma unroll
                        for (int s = 0; s < EPT; s++) p[s] = z[s] + beta * p[s];   // :319
                        k_it++;
                    }
                }
            }
            last_pcg = k_it;
            pcg_total += k_it;
            if (pcg_fail) stop = LP_STOP_PCG;
            if (pcg_fail && l2f) { ret = 1; break; }              // :1450-1454: return 1, x_sol untouched
#pragma unroll
            for (int s = 0; s < EPT; s++) x[s] = live[s] ? xt[s] : x[s];
            outer_total++;
            if (rec) {                                            // x_iters column cc (:1472-1475); plain loop: the xiter dump (:903-909)
                double *xh = bd.xhist + ((size_t)inst * bd.ws_cap + cc) * NS;
#pragma unroll
                for (int s = 0; s < EPT; s++) xh[s * RT + tid] = x[s];
                cc++;
            }
            // ---------------- duals (:917-924 / :1487-1491) ----------------
            const double g1 = gamma_val * rho1, g2 = gamma_val * rho2, g4 = gamma_val * rho4;
#pragma unroll
            for (int s = 0; s < EPT; s++) {
                z1[s] = z1[s] + g1 * (x[s] - y1[s]);
                z2[s] = z2[s] + g2 * (x[s] - y2[s]);
            }
            publish_x(x);
            __syncthreads();
            rows_sum(Ex);                                         // E*x: feeds z4 now and y3 of the next iteration
#pragma unroll
            for (int s = 0; s < EPT; s++) {
                if (!rv[s]) continue;
                const double d = g4 * ((Ex[s] + y3[s]) - f[s]);
                z4[s] = (!l2f && it == iter_start) ? d : z4[s] + d;   // :920-923 (plain loop overwrites on its first iteration)
            }
            // ---------------- convergence (:931-949) ----------------
#pragma unroll
            for (int s = 0; s < EPT; s++) {
                const double d1 = x[s] - y1[s], d2 = x[s] - y2[s];
                put(0, s, x[s] * x[s]);
                put(1, s, d1 * d1);
                put(2, s, d2 * d2);
            }
            eigen_reduce<3>(stage, NS, nl, res, p3);
            {
                const double xn = sqrt(p3[0]);
                const double temp0 = (xn < 2.2204e-16) ? 2.2204e-16 : xn;
                cvg1 = sqrt(p3[1]) / temp0;
                cvg2 = sqrt(p3[2]) / temp0;
            }
            if (cvg1 <= LP_STOP_THRESHOLD && cvg2 <= LP_STOP_THRESHOLD && (l2f || it != iter_start)) {
                if (l2f) ret = 1;                                 // :1505 (plain loop: ret stays 0, :934-949)
                stop = LP_STOP_Y1Y2;
                break;
            }
            if ((it + 1) % LP_RHO_STEP == 0) {                    // :951-970
                prev_rho1 = rho1; prev_rho2 = rho2;
                rho1 = learning_fact * rho1;
                rho2 = learning_fact * rho2;
                prev_rho4 = rho4;
                rho4 = learning_fact * rho4;
                const double g = gamma_val * LP_GAMMA_FACTOR;
                gamma_val = g < 1.0 ? 1.0 : g;
                rhoUpdated = 1;
                rcr = learning_fact - 1.0;
            }
            // ---------------- objective history and the binary objective (:972-1011) ----------------
#pragma unroll
            for (int s = 0; s < EPT; s++) {
                const double xb = x[s] >= 0.5 ? 1.0 : 0.0;
                put(0, s, bv[s] * x[s]);
                put(1, s, bv[s] * xb);
            }
            double p2[2];
            eigen_reduce<2>(stage, NS, nl, res, p2);
            obj_val = p2[0];                                      // :972
            if (hist_n < LP_HIST) {
#pragma unroll
                for (int k = 0; k < LP_HIST; k++) if (k == hist_n) h_reg[k] = obj_val;
            } else {
#pragma unroll
                for (int k = 0; k < LP_HIST - 1; k++) h_reg[k] = h_reg[k + 1];
                h_reg[LP_HIST - 1] = obj_val;
            }
            if (hist_n < 0x3fffffff) hist_n++;
            if (hist_n >= LP_HIST) {                              // compute_std_obj :459-469, std_dev :358-377
                double mean = 0;
#pragma unroll
                for (int k = 0; k < LP_HIST; k++) mean += h_reg[k];
                mean /= (double)LP_HIST;
                double dev = 0;
#pragma unroll
                for (int k = 0; k < LP_HIST; k++) dev += (h_reg[k] - mean) * (h_reg[k] - mean);
                dev /= (double)(LP_HIST - 1);
                const double sd = (dev == 0) ? 0.0 : sqrt(dev);   // the reference: pow(dev, 1/2) -- the mode's one known deviation
                std_obj = sd / fabs(h_reg[LP_HIST - 1]);
            }
            if (std_obj <= LP_STD_THRESHOLD) { ret = 1; stop = LP_STOP_OBJSTD; break; }   // :977
            cur_obj = p2[1];                                      // :1001-1003
            if (best_bin_obj >= cur_obj) best_bin_obj = cur_obj;
        }
    }

    // ---- write the state back ----
    if constexpr (VALUED && VLDS) {
        __syncthreads();                                          // every thread's entries of r4v
        for (int k = tid; k < nnz; k += RT) vv.r4v[oz + k] = r4v[k];
    }
#pragma unroll
    for (int s = 0; s < EPT; s++) {
        const int j = s * RT + tid;
        bd.x[on + j] = x[s];
        bd.live[on + j] = live[s] ? 1 : 0;
        bd.z1[on + j] = z1[s]; bd.z2[on + j] = z2[s]; bd.pd[on + j] = pd[s];
        if (rv[s]) { bd.z4[ol + j] = z4[s]; bd.f[ol + j] = f[s]; }
    }
    if (tid == 0) {
        dsc[ND_RHO1] = rho1; dsc[ND_RHO2] = rho2; dsc[ND_RHO4] = rho4;
        dsc[ND_PREV_RHO1] = prev_rho1; dsc[ND_PREV_RHO2] = prev_rho2; dsc[ND_PREV_RHO4] = prev_rho4;
        dsc[ND_GAMMA] = gamma_val; dsc[ND_DI] = dI; dsc[ND_R4ET] = r4Et; dsc[ND_RCR] = rcr;
        dsc[ND_STD_OBJ] = std_obj; dsc[ND_CUR_OBJ] = cur_obj; dsc[ND_BEST_BIN_OBJ] = best_bin_obj;
        dsc[ND_SUM_FIX_OBJ] = sum_fix_obj; dsc[ND_FIX_OBJ] = fix_obj; dsc[ND_C1] = c1;
        dsc[ND_CVG1] = cvg1; dsc[ND_CVG2] = cvg2; dsc[ND_OBJ_VAL] = obj_val;
        dsc[ND_PREV_SUM] = prev_sum; dsc[ND_PREV_OBJ] = prev_obj;
        isc[NI_NLIVE] = n_live; isc[NI_RHO_UPDATED] = rhoUpdated; isc[NI_HIST_N] = hist_n;
        isc[NI_RET] = ret; isc[NI_STOP] = stop;
        isc[NI_PCG_TOTAL] = pcg_total; isc[NI_OUTER_TOTAL] = outer_total; isc[NI_LAST_PCG] = last_pcg;
        isc[NI_EXPR_READY] = expr_ready;
        if (l2f) isc[NI_ITER] = it;                               // member `iter` (LPh:279), advanced by l2f only
        else isc[NI_PLAIN_ITER_P1] = it + 1;                      // LPcpp:1081
        for (int k = 0; k < LP_HIST; k++) bd.hist[(size_t)inst * LP_HIST + k] = h_reg[k];
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
size_t lp_ref_lds_bytes(int NS, int LS, int ZS, bool vals_in_lds) {
    return RefLds(NS, LS, ZS).total + (vals_in_lds ? 3 * sizeof(double) * (size_t)ZS : 0);
}

bool lp_ref_supported(int T, int EPT) { return T == RT && (EPT == 1 || EPT == 2 || EPT == 4); }

hipError_t lp_ref_launch_init(const LpBatchDev &bd, const LpRefVals &vv, size_t lds, const double *f_org, const double *c1_init,
                              const uint8_t *live_init, hipStream_t s) {
    auto kfn = vv.vr ? lp_ref_init_kernel<true> : lp_ref_init_kernel<false>;
    hipError_t e = hipFuncSetAttribute((const void *)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kfn, dim3(bd.B), dim3(RT), lds, s, bd, f_org, c1_init, live_init, vv);
    return hipGetLastError();
}

// vv.vr == nullptr: the unit kernels; else the VALUED ones with the values in LDS (vv.in_lds) or in global memory
hipError_t lp_ref_launch_window(const LpBatchDev &bd, const LpRefVals &vv, int EPT, size_t lds, int iter_start, int iter_end, int mode,
                                hipStream_t s) {
#define CALL_REF(EE, VA, VL)                                                                                   \
    {                                                                                                          \
        auto kfn = lp_ref_window_kernel<EE, VA, VL>;                                                           \
        hipError_t e = hipFuncSetAttribute((const void *)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
        if (e != hipSuccess) return e;                                                                         \
        hipLaunchKernelGGL(kfn, dim3(bd.B), dim3(RT), lds, s, bd, iter_start, iter_end, mode, vv);             \
    }
#define PICK_REF(EE)                                                                                           \
    {                                                                                                          \
        if (!vv.vr) CALL_REF(EE, false, false)                                                                 \
        else if (vv.in_lds) CALL_REF(EE, true, true)                                                           \
        else CALL_REF(EE, true, false)                                                                         \
    }
    if (EPT == 1) PICK_REF(1)
    else if (EPT == 2) PICK_REF(2)
    else if (EPT == 4) PICK_REF(4)
    else return hipErrorInvalidConfiguration;
#undef PICK_REF
#undef CALL_REF
    return hipGetLastError();
}
