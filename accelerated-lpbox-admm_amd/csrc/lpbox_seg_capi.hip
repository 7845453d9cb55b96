// lpbox_seg_capi.hip -- host side of the SEGMENTATION flavour behind the C-ABI: image -> (A, b, c) cost construction
// (SEGcpp:46-248, :705-756), device buffers, the graph-replayed iteration driver, early-fix index bookkeeping and getters.
// All solver arithmetic runs in lpbox_seg_kernels.hip; there is no CPU fallback.  What the launch chains decide (kmax, batches, the resume
// limit) is in lpbox_chain.h; the drivers of the single-problem chain and of the lockstep chain of a batch, the graph cache, the device
// buffer, the timer and the error-check macros are in lpbox_host.h.  This file supplies their launches (SegChainOps, SegBatchOps).
#include "../../include/lpbox_hip.h"
#include "lpbox_capi_internal.h"
#include "lpbox_host.h"
#include "lpbox_seg.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

namespace {
static_assert(SEG_HALT_NONE == CHAIN_HALT_NONE && SEG_HALT_PCG_MORE == CHAIN_HALT_PCG_MORE, "lpbox_chain.h reads SegState::halt");
static_assert(CHAIN_RULES_SEG.pcg_cap == SEG_PCG_MAXITERS, "the resume limit follows the PCG cap of the kernels");
static_assert(CHAIN_RULES_SEG.iters_per_graph % 2 == 0, "an iteration is an odd number of launches: an even count keeps the ping-pong parity");
constexpr int SEG_KMAX_LIMIT = CHAIN_RULES_SEG.kmax_cap;

// the rules of a chain created now: LPBOX_SEG_KMARGIN overrides the spare groups (also for the lockstep chain of a batch)
ChainRules seg_rules() {
    ChainRules r = CHAIN_RULES_SEG;
    if (const char *e = getenv("LPBOX_SEG_KMARGIN")) r.margin = std::max(0, atoi(e));
    return r;
}

// c1 = pow(n_live, 1/p), p = 2 (SEGcpp:557,670) through libm's pow, as the reference and the oracle call it: with the literal exponent
// the compiler turns the call into sqrt, and glibc's pow is not correctly rounded (n = 2921: one ulp apart).  Reference order only; the
// default order keeps the expressions it has always had.
double ref_c1(int n) {
    volatile double e = 1.0 / 2;
    return std::pow((double)n, e);
}
}  // namespace

struct SegSolver {
    int print_info = 0, device = 0;
    int n = 0, nnz = 0, rows = 0, cols = 0;
    double c = 0.0;
    std::vector<int> rowptr, colidx;
    std::vector<double> vals, orgb;
    std::vector<int> left_idx, xi_left_idx;   // original indices of the live variables (ascending)
    int xi_rows = 0;
    bool left_stale = false;     // a batched window fixed on the device: d_left is current, left_idx is refreshed from it on demand
    bool dleft_valid = false;    // d_left holds the live list (false between an init and the first early-fixing window)
    long win_serial = 0;         // inits and early-fixing windows run so far (a batch's packed rows belong to one of them)
    bool has_problem = false, uploaded = false, inited = false, xi_valid = false;
    int G = 0, EPT = 2, parity = 0;
    hipStream_t stream = nullptr;
    StreamTimer timer;
    ChainController chain{seg_rules()};   // kmax; pcg_resumes: SEG_HALT_PCG_MORE seen by the host loops on this handle's state since solve_init
    GraphCache graphs;
    bool use_graph = getenv("LPBOX_SEG_NOGRAPH") == nullptr;     // eager launches (profilers that dislike graphs)
    double kernel_ms = 0.0; long long launches = 0, collectives = 0;   // (no collectives on this path)
    DevBuf<int> d_ecol, d_left;
    DevBuf<uint8_t> d_rowlen;
    int ell_w = 0;
    bool dia = false; int doff[7] = {0, 0, 0, 0, 0, 0, 0};      // diagonal storage of the matrix (SegDev::dia), chosen by upload()
    DevBuf<unsigned long long> d_dpack; DevBuf<double> d_adiag;
    DevBuf<double> d_eval, x, y1, y2, z1, z2, b, rhs, r, z, tmp, dinv, td, p0, p1, part, xhist, xi_out;
    DevBuf<uint8_t> live, fixval, newfix;
    DevBuf<SegState> st;
    int ws_cap = 0, last_ws = 0;
    int record = 0;        // legacy loop keeps x of up to `record` iterations (lpbox_set_record; print_info 1, SEGcpp:1209-1213,1270-1277)
    int rec_cols = 0;      // iterations the last legacy solve recorded
    SegState hst;
    // the reference's summation order (lpbox_seg_set_order; lpbox_seg_ref_kernels.hip): chosen before the problem, so the handle's
    // buffers, launch chain and captured graphs belong to one order for good
    int order = LPBOX_ORDER_DEFAULT;
    DevBuf<int> d_rank, d_cnt;
    DevBuf<double> d_stage, d_red;
    bool ref() const { return order == LPBOX_ORDER_REFERENCE; }
    SegRef rf() const { SegRef r; r.rank = d_rank.p; r.cnt = d_cnt.p; r.stage = d_stage.p; r.red = d_red.p; return r; }
    double c1_of(int n_live) const { return ref() ? ref_c1(n_live) : std::pow((double)n_live, 1.0 / 2); }

    SegDev dev() const {
        SegDev d;
        d.n = n; d.nnz = nnz; d.G = G; d.EPT = EPT;
        d.ecol = d_ecol.p; d.eval = d_eval.p; d.rowlen = d_rowlen.p; d.ell_w = ell_w;
        d.dia = dia ? 1 : 0; d.dpack = d_dpack.p; d.adiag = d_adiag.p;
        for (int k = 0; k < 7; k++) d.doff[k] = doff[k];
        d.x = x.p; d.y1 = y1.p; d.y2 = y2.p; d.z1 = z1.p; d.z2 = z2.p; d.b = b.p; d.rhs = rhs.p; d.r = r.p; d.z = z.p;
        d.tmp = tmp.p; d.dinv = dinv.p; d.td = td.p; d.p0 = p0.p; d.p1 = p1.p; d.live = live.p; d.fixval = fixval.p;
        d.newfix = newfix.p; d.part = part.p; d.xhist = xhist.p; d.ws_cap = ws_cap; d.st = st.p;
        d.c1_init = ref() ? ref_c1(n) : std::pow((double)n, 1.0 / 2);      // pow(n, 1/p), p = 2 (SEGcpp:557,670)
        return d;
    }
};

namespace {

// cv::resize(src, dst, Size(), scale, scale) with INTER_LINEAR on 8-bit data (SEGcpp:705-714), following OpenCV 4.4's
// fixed-point scheme: 11-bit coefficients, horizontal pass in int, vertical pass (((b0*(S0>>4))>>16) + ((b1*(S1>>4))>>16) + 2) >> 2
void resize_linear_u8(const unsigned char *src, int rows, int cols, double scale, std::vector<unsigned char> &dst, int &orows, int &ocols) {
    orows = (int)std::lround(rows * scale); ocols = (int)std::lround(cols * scale);
    dst.assign((size_t)orows * ocols, 0);
    const double inv = 1.0 / scale;
    std::vector<int> xo(ocols), yo(orows);
    std::vector<short> ax(2 * (size_t)ocols), ay(2 * (size_t)orows);
    auto coef = [&](int dpos, int slen, int &ofs, short &c0, short &c1) {
        float f = (float)((dpos + 0.5) * inv - 0.5);
        int sp = (int)std::floor(f); f -= sp;
        if (sp < 0) { f = 0; sp = 0; }
        if (sp >= slen - 1) { f = 0; sp = slen - 1; }
        ofs = sp; c0 = (short)std::lrintf((1.f - f) * 2048); c1 = (short)std::lrintf(f * 2048);
    };
    for (int dx = 0; dx < ocols; dx++) coef(dx, cols, xo[dx], ax[2 * dx], ax[2 * dx + 1]);
    for (int dy = 0; dy < orows; dy++) coef(dy, rows, yo[dy], ay[2 * dy], ay[2 * dy + 1]);
    for (int dy = 0; dy < orows; dy++) {
        const unsigned char *s0 = src + (size_t)yo[dy] * cols, *s1 = src + (size_t)std::min(yo[dy] + 1, rows - 1) * cols;
        for (int dx = 0; dx < ocols; dx++) {
            const int x0 = xo[dx], x1 = std::min(x0 + 1, cols - 1);
            const int r0 = s0[x0] * ax[2 * dx] + s0[x1] * ax[2 * dx + 1], r1 = s1[x0] * ax[2 * dx] + s1[x1] * ax[2 * dx + 1];
            const int v = (((ay[2 * dy] * (r0 >> 4)) >> 16) + ((ay[2 * dy + 1] * (r1 >> 4)) >> 16) + 2) >> 2;
            dst[(size_t)dy * ocols + dx] = (unsigned char)std::clamp(v, 0, 255);
        }
    }
}

// sum in the association of Eigen's vectorised redux (two 2-wide accumulators; Core/Redux.h), used by .mean()/.sum()
double eigen_sum(const std::vector<double> &a) {
    const size_t n = a.size();
    if (n == 0) return 0.0;
    const size_t e2 = (n / 4) * 4, e1 = (n / 2) * 2;
    if (e1 == 0) { double r = a[0]; for (size_t i = 1; i < n; i++) r = r + a[i]; return r; }
    double p0a = a[0], p0b = a[1];
    if (e1 > 2) {
        double p1a = a[2], p1b = a[3];
        for (size_t i = 4; i < e2; i += 4) { p0a += a[i]; p0b += a[i + 1]; p1a += a[i + 2]; p1b += a[i + 3]; }
        p0a = p0a + p1a; p0b = p0b + p1b;
        if (e1 > e2) { p0a = p0a + a[e2]; p0b = p0b + a[e2 + 1]; }
    }
    double r = p0a + p0b;
    for (size_t i = e1; i < n; i++) r = r + a[i];
    return r;
}

// SEGcpp:46-248 (+ :727 scale by 1/263, :747 rounding of the unary costs, :755-756 A_ptr = A/2)
void build_costs(const unsigned char *gray, int rows, int cols, std::vector<int> &rowptr, std::vector<int> &colidx,
                 std::vector<double> &vals, std::vector<double> &b, double &c) {
    const int n = rows * cols;
    std::vector<double> v(n);                                   // vectorize(): column-major flatten (:46-53)
    for (int j = 0; j < cols; j++) for (int i = 0; i < rows; i++) v[(size_t)j * rows + i] = gray[(size_t)i * cols + j] / 263.0;
    const double sigma = 0.1, bb = 0.6, f1 = 0.2, f2 = 0.2;     // :736-739
    const double cc = std::log(2.0 * M_PI) / 2.0 + std::log(sigma);
    std::vector<double> U1(n);
    b.assign(n, 0.0);
    for (int p = 0; p < n; p++) {                               // get_unary_cost :55-81
        const double ab = std::pow(v[p] - bb, 2.0) / (2 * sigma * sigma) + cc;
        const double aa = std::exp(-std::pow(v[p] - f1, 2.0) / (2 * sigma * sigma)) + std::exp(-std::pow(v[p] - f2, 2) / (2 * sigma * sigma));
        const double af = -std::log(aa + 2.220446049250313e-16) + cc + std::log(2.0);
        U1[p] = std::round(ab);
        b[p] = std::round(af) - U1[p];                          // b = U2 - U1 (:232)
    }
    c = eigen_sum(U1);                                          // :245
    const double mean = eigen_sum(v) / n;                       // get_binary_cost :173-224
    std::vector<double> sq(n);
    for (int p = 0; p < n; p++) sq[p] = (v[p] - mean) * (v[p] - mean);
    const double sig = std::sqrt(eigen_sum(sq) / (n - 1));      // sample std, used where a variance is usual (Q3)
    rowptr.assign((size_t)n + 1, 0); colidx.clear(); vals.clear();
    colidx.reserve((size_t)7 * n); vals.reserve((size_t)7 * n);
    for (int i = 0; i < rows; i++) for (int j = 0; j < cols; j++) {
        const int r = i * cols + j;                             // pairs are numbered row-major (:157-158) ...
        rowptr[r] = (int)colidx.size();
        const size_t first = colidx.size();
        for (int a = -1; a <= 1; a++) for (int bq = -1; bq <= 1; bq++) {
            if (a == 0 && bq == 0) { colidx.push_back(r); vals.push_back(0.0); continue; }   // explicit zero diagonal (:213-219)
            if (a == bq || i + a < 0 || i + a >= rows || j + bq < 0 || j + bq >= cols) continue;   // a != b: 6 neighbours (:153-155)
            const int q = (i + a) * cols + (j + bq);
            const double dI = std::pow(v[r] - v[q], 2.0) / sig; // ... but intensities are read column-major (:192-193)
            colidx.push_back(q); vals.push_back(std::round(3 * std::exp(-dI)));
        }
        double We = 0;                                          // get_A_b_from_cost :226-248
        for (size_t e = first; e < colidx.size(); e++) We += (-vals[e]) * 1.0;
        We = -(0.0 + 1.0 * We);
        for (size_t e = first; e < colidx.size(); e++) {
            double a_e = -vals[e];
            if (colidx[e] == r) a_e += We;
            vals[e] = (2 * a_e) / 2;
        }
    }
    rowptr[n] = (int)colidx.size();
}

// Can the matrix be held as diagonals (SegDev::dia)?  At most three distinct column offsets either side of the main diagonal, a stored
// diagonal entry in every row, every off-diagonal value equal to -w for an integer w in 0..255.  True for every problem the image cost
// builder makes (SEGcpp:144-248: offsets {+-1, +-(ncols-1), +-ncols}, w = round(3 exp(.))); anything else keeps the ELL form.
bool as_diagonals(const SegSolver *s, int (&doff)[7], std::vector<unsigned long long> &dpack, std::vector<double> &adiag) {
    const int n = s->n;
    std::vector<int> neg, pos;
    auto note = [](std::vector<int> &v, int off) {
        for (int o : v) if (o == off) return true;
        if (v.size() == 3) return false;
        v.push_back(off);
        return true;
    };
    for (int i = 0; i < n; i++) {
        bool have_diag = false;
        for (int k = s->rowptr[i]; k < s->rowptr[i + 1]; k++) {
            const int off = s->colidx[k] - i;
            if (off == 0) { have_diag = true; continue; }
            const double v = s->vals[k];
            if (!(v <= 0.0 && v >= -255.0 && v == std::floor(v))) return false;
            if (!note(off < 0 ? neg : pos, off)) return false;
        }
        if (!have_diag) return false;
    }
    std::sort(neg.begin(), neg.end()); std::sort(pos.begin(), pos.end());
    // slots 0..2: negative offsets ascending (missing ones in front), 3: the diagonal, 4..6: positive ascending (missing ones behind);
    // a missing slot points at a harmless neighbour and carries w = 0 in every row
    for (int k = 0; k < 3; k++) doff[k] = -1, doff[4 + k] = 1;
    doff[3] = 0;
    std::vector<std::pair<int, int>> slot_of;                     // (offset, byte of dpack)
    for (size_t k = 0; k < neg.size(); k++) { const int q = 3 - (int)neg.size() + (int)k; doff[q] = neg[k]; slot_of.push_back({neg[k], q}); }
    for (size_t k = 0; k < pos.size(); k++) { const int q = 4 + (int)k; doff[q] = pos[k]; slot_of.push_back({pos[k], q - 1}); }
    dpack.assign((size_t)n, 0ull); adiag.assign((size_t)n, 0.0);
    for (int i = 0; i < n; i++)
        for (int k = s->rowptr[i]; k < s->rowptr[i + 1]; k++) {
            const int off = s->colidx[k] - i;
            if (off == 0) { adiag[i] = s->vals[k]; continue; }
            for (auto &so : slot_of)
                if (so.first == off) dpack[i] |= (unsigned long long)(unsigned)(-s->vals[k]) << (8 * so.second);
        }
    return true;
}

int upload(SegSolver *s) {
    int rc = use_device(s->device);
    if (rc) return rc;
    const int n = s->n;
    s->EPT = 2;
    if (const char *e = getenv("LPBOX_SEG_EPT")) { int v = atoi(e); if (v == 1 || v == 2 || v == 4 || v == 8) s->EPT = v; }   // tuning only
    while ((n + SEG_T * s->EPT - 1) / (SEG_T * s->EPT) > 2 * SEG_T && s->EPT < 64) s->EPT *= 2;   // keep G <= 512 partials
    s->G = (n + SEG_T * s->EPT - 1) / (SEG_T * s->EPT);
    if (s->G > 2 * SEG_T) return lpbox_fail(LPBOX_E_UNSUPPORTED, "n = %d is beyond the two-level reduction of the segmentation kernels", n);
    if (!s->stream) HIPCHK(hipStreamCreate(&s->stream));
    HIPCHK(s->timer.create());
    int w = 0;
    for (int i = 0; i < n; i++) w = std::max(w, s->rowptr[i + 1] - s->rowptr[i]);
    if (w > 255) return lpbox_fail(LPBOX_E_UNSUPPORTED, "a row of A stores %d entries; the ELL layout of the segmentation kernels holds at most 255", w);
    s->ell_w = w;
    std::vector<unsigned long long> dpack; std::vector<double> adiag;
    s->dia = n >= 2 && w <= 7 && !getenv("LPBOX_SEG_NODIA") && as_diagonals(s, s->doff, dpack, adiag);      // LPBOX_SEG_NODIA: keep ELL (A/B, tests)
    if (s->dia) {
        s->d_ecol.release(); s->d_eval.release();
        HIPCHK(s->d_dpack.alloc(n)); HIPCHK(s->d_adiag.alloc(n));
        HIPCHK(hipMemcpy(s->d_dpack.p, dpack.data(), sizeof(unsigned long long) * (size_t)n, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(s->d_adiag.p, adiag.data(), sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
    } else {
        s->d_dpack.release(); s->d_adiag.release();
        HIPCHK(s->d_ecol.alloc((size_t)w * n)); HIPCHK(s->d_eval.alloc((size_t)w * n));
    }
    HIPCHK(s->d_rowlen.alloc(n)); HIPCHK(s->d_left.alloc(n));
    for (DevBuf<double> *bp : {&s->x, &s->y1, &s->y2, &s->z1, &s->z2, &s->b, &s->rhs, &s->r, &s->z, &s->tmp, &s->dinv, &s->td, &s->p0, &s->p1})
        HIPCHK(bp->alloc(n));
    HIPCHK(s->live.alloc(n)); HIPCHK(s->fixval.alloc(n)); HIPCHK(s->newfix.alloc(n));
    HIPCHK(s->part.alloc((size_t)5 * SEG_NPART * s->G)); HIPCHK(s->st.alloc(2));
    if (!s->dia) {
        std::vector<int> ecol((size_t)w * n); std::vector<double> eval((size_t)w * n, 0.0); std::vector<uint8_t> rl(n);
        for (int i = 0; i < n; i++) {
            const int len = s->rowptr[i + 1] - s->rowptr[i];
            rl[i] = (uint8_t)len;
            for (int k = 0; k < w; k++) {
                ecol[(size_t)k * n + i] = k < len ? s->colidx[s->rowptr[i] + k] : i;
                if (k < len) eval[(size_t)k * n + i] = s->vals[s->rowptr[i] + k];
            }
        }
        HIPCHK(hipMemcpy(s->d_ecol.p, ecol.data(), sizeof(int) * ecol.size(), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(s->d_eval.p, eval.data(), sizeof(double) * eval.size(), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(s->d_rowlen.p, rl.data(), rl.size(), hipMemcpyHostToDevice));
    }
    HIPCHK(hipMemset(s->part.p, 0, sizeof(double) * (size_t)5 * SEG_NPART * s->G));
    HIPCHK(hipMemset(s->newfix.p, 0, n));
    if (s->ref()) {
        HIPCHK(s->d_rank.alloc(n)); HIPCHK(s->d_cnt.alloc(1)); HIPCHK(s->d_stage.alloc((size_t)SEG_REF_ROWS * n)); HIPCHK(s->d_red.alloc(SEG_REF_ROWS));
        HIPCHK(hipMemset(s->d_red.p, 0, sizeof(double) * SEG_REF_ROWS));
        HIPCHK(hipMemset(s->d_cnt.p, 0, sizeof(int)));
    }
    s->uploaded = true;
    return LPBOX_OK;
}

int read_state(SegSolver *s) {
    HIPCHK(hipMemcpyAsync(&s->hst, s->st.p + s->parity, sizeof(SegState), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return LPBOX_OK;
}

// run iterations up to iter_end (the window must already be set); returns when stopped / window done / all fixed.
// Each batch enqueues kmax (matvec, update) pairs per outer iteration; kernels fall through once the PCG has converged, so
// kmax only has to cover the iteration counts seen recently; a batch that runs out of pairs halts itself (SEG_HALT_PCG_MORE)
// and is resumed (chain_run).  One hipGraph = 4 outer iterations of 3 + 2 kmax launches: an even number of launches, so the
// state ping-pong parity is preserved across replays.  The enqueue helpers of the kernels file do not count: launches by formula.
struct SegChainOps {
    SegSolver *s;
    int read_state(ChainView &v) { CHK(::read_state(s)); v = chain_view(s->hst); return LPBOX_OK; }
    int resume_pcg() {
        if (s->ref()) {
            HIPCHK(segr_enqueue_pcg_more(s->dev(), s->rf(), CHAIN_PAIRS_PER_RESUME, &s->parity, s->stream));
            s->launches += 3 + 4 * CHAIN_PAIRS_PER_RESUME;
            return LPBOX_OK;
        }
        HIPCHK(seg_enqueue_pcg_more(s->dev(), CHAIN_PAIRS_PER_RESUME, &s->parity, s->stream));
        s->launches += 2 + 2 * CHAIN_PAIRS_PER_RESUME;
        return LPBOX_OK;
    }
    int batch_head() {
        HIPCHK(seg_launch_copy(s->dev(), 1, &s->parity, s->stream));       // pcg_max = 0 for the coming batch
        if (s->ref()) {
            HIPCHK(segr_enqueue_prep(s->dev(), s->rf(), &s->parity, s->stream));
            s->launches += 3;
            return LPBOX_OK;
        }
        HIPCHK(seg_enqueue_prep(s->dev(), &s->parity, s->stream));         // head of the batch (inside it post + yrhs do prep's work)
        s->launches += 2;
        return LPBOX_OK;
    }
    int enqueue(int n) {
        if (s->ref()) {
            HIPCHK(segr_enqueue_iterations(s->dev(), s->rf(), n, s->chain.kmax, &s->parity, s->stream));
            s->launches += (long long)n * (5 + 4 * s->chain.kmax);
            return LPBOX_OK;
        }
        HIPCHK(seg_enqueue_iterations(s->dev(), n, s->chain.kmax, &s->parity, s->stream));
        s->launches += (long long)n * (3 + 2 * s->chain.kmax);
        return LPBOX_OK;
    }
    int finalize() {
        if (s->ref()) HIPCHK(segr_enqueue_finalize(s->dev(), s->rf(), &s->parity, s->stream));
        else HIPCHK(seg_enqueue_finalize(s->dev(), &s->parity, s->stream));
        s->launches += 1;
        return LPBOX_OK;
    }
};

int run_window(SegSolver *s, int iter_end) {
    HIPCHK(s->timer.start(s->stream));
    CHK(chain_run(s->chain, s->graphs, ChainIo{s->stream, s->parity, s->launches, s->collectives, s->use_graph, true}, iter_end, SegChainOps{s}));
    double ms = 0.0;
    HIPCHK(s->timer.stop_sync(s->stream, &ms));
    s->kernel_ms += ms;
    return LPBOX_OK;
}

// the host copy of the live list after device-side fixes (batched windows compact d_left on the device)
int refresh_left(SegSolver *s) {
    if (!s->left_stale) return LPBOX_OK;
    s->left_idx.resize((size_t)s->hst.n_live);
    if (!s->left_idx.empty())
        HIPCHK(hipMemcpy(s->left_idx.data(), s->d_left.p, sizeof(int) * s->left_idx.size(), hipMemcpyDeviceToHost));
    s->left_stale = false;
    return LPBOX_OK;
}

// the host side of segc_init for a member of a batch: upload, b, identity live list (the init KERNEL runs batched)
int batch_reset_handle(SegSolver *s) {
    int rc = s->uploaded ? use_device(s->device) : upload(s);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(s->b.p, s->orgb.data(), sizeof(double) * (size_t)s->n, hipMemcpyHostToDevice, s->stream));
    s->left_idx.resize(s->n);
    for (int k = 0; k < s->n; k++) s->left_idx[k] = k;
    s->left_stale = false; s->dleft_valid = false; s->win_serial++;
    s->chain.pcg_resumes = 0;
    return LPBOX_OK;
}

// The launches of the lockstep chain of a batch (chain_run_lockstep; devs = device array of A descriptors, the window already set): each
// problem on its own control state -- one that has stopped, is all fixed or whose PCG has converged falls through, a SEG_HALT_PCG_MORE on
// any problem resumes the chain.  hs[A] receives the final states.  The launches are eager and counted by formula.
struct SegBatchOps {
    const SegDev *devs; SegState *dstates; int A, Gmax; SegState *hs; int &parity; long long &launches; hipStream_t st;
    const SegRef *refs = nullptr;                // the members' staging descriptors: a batch in the reference's summation order
    int collect(ChainView *v) {
        HIPCHK(segb_collect_states(devs, A, parity, dstates, st));
        HIPCHK(hipMemcpyAsync(hs, dstates, sizeof(SegState) * (size_t)A, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (int i = 0; i < A; i++) v[i] = chain_view(hs[i]);
        return LPBOX_OK;
    }
    int resume_pcg() {
        if (refs) { HIPCHK(segrb_enqueue_pcg_more(devs, refs, A, Gmax, CHAIN_PAIRS_PER_RESUME, &parity, st)); launches += 3 + 4 * CHAIN_PAIRS_PER_RESUME; return LPBOX_OK; }
        HIPCHK(segb_enqueue_pcg_more(devs, A, Gmax, CHAIN_PAIRS_PER_RESUME, &parity, st)); launches += 2 + 2 * CHAIN_PAIRS_PER_RESUME; return LPBOX_OK;
    }
    // (counts the whole batch: copy, iterations, finalize; reference order: copy, prep, walk, iterations, finalize)
    int batch_head(int iters, int kmax) {
        HIPCHK(segb_launch_copy(devs, A, 1, &parity, st));
        if (refs) { HIPCHK(segrb_enqueue_prep(devs, refs, A, Gmax, &parity, st)); launches += 4 + (long long)iters * (5 + 4 * kmax); return LPBOX_OK; }
        launches += 2 + (long long)iters * (4 + 2 * kmax); return LPBOX_OK;
    }
    int enqueue(int n, int kmax) {
        if (refs) HIPCHK(segrb_enqueue_iterations(devs, refs, A, Gmax, n, kmax, &parity, st));
        else HIPCHK(segb_enqueue_iterations(devs, A, Gmax, n, kmax, &parity, st));
        return LPBOX_OK;
    }
    int finalize() {
        if (refs) HIPCHK(segrb_enqueue_finalize(devs, refs, A, Gmax, &parity, st));
        else HIPCHK(segb_enqueue_finalize(devs, A, Gmax, &parity, st));
        return LPBOX_OK;
    }
};

// all members of a batch run in ONE summation order, member 0's; a member in the other order is refused by name
int batch_order_ok(SegSolver *const *ss, int B) {
    for (int i = 1; i < B; i++) {
        if (ss[i]->ref() && !ss[0]->ref()) return lpbox_fail(LPBOX_E_UNSUPPORTED, "problem %d of the batch runs in the reference summation order; the batch runs the default order (problem 0's)", i);
        if (!ss[i]->ref() && ss[0]->ref()) return lpbox_fail(LPBOX_E_UNSUPPORTED, "problem %d of the batch runs in the default order; the batch runs the reference summation order (problem 0's)", i);
    }
    return LPBOX_OK;
}

// iterations up to iter_end for the A problems behind `ops`, from *kmax on (written back after a chain that completed); act: see chain_run_lockstep
int segb_run_chain(const ChainRules &rules, int *kmax, bool adaptive, const int *act, int iter_end, long long *resumes, SegBatchOps ops) {
    ChainLockstep ctl(rules, *kmax, adaptive);
    GraphCache none; long long collectives = 0; bool use_graph = false;          // the batch launches eagerly
    CHK(chain_run_lockstep(ctl, ops.A, act, none, ChainIo{ops.st, ops.parity, ops.launches, collectives, use_graph, false}, iter_end, resumes, ops));
    *kmax = ctl.kmax;
    return LPBOX_OK;
}

// `(int)energy` of SEGcpp:1379 as a defined conversion: truncation toward zero while the result fits an int, INT_MIN otherwise (NaN
// included) -- the value the reference's cast yields on x86-64 (cvttsd2si), where the C++ cast itself is undefined.  oracle/seg_oracle.c
// and oracle/bqp_numpy.py convert the same way.
int energy_int(double e) {
    return e > -2147483649.0 && e < 2147483648.0 ? (int)e : INT_MIN;
}

}  // namespace

SegSolver *segc_create(int print_info, int device) {
    SegSolver *s = new SegSolver();
    s->print_info = print_info; s->device = device;
    memset(&s->hst, 0, sizeof(s->hst));
    if (const char *e = getenv("LPBOX_SEG_KMAX")) { int v = atoi(e); if (v >= 1 && v <= SEG_KMAX_LIMIT) s->chain.force_kmax(v); }
    return s;
}

void segc_destroy(SegSolver *s) {
    if (!s) return;
    if (s->uploaded) (void)hipSetDevice(s->device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    s->graphs.clear();
    s->timer.destroy();
    if (s->stream) (void)hipStreamDestroy(s->stream);
    delete s;
}

int segc_set_problem(SegSolver *s, int n, int nnz, const int *rowptr, const int *colidx, const double *vals, const double *b,
                     double c, int rows, int cols, bool from_image) {
    if (s->uploaded) return lpbox_fail(LPBOX_E_STATE, "problem already uploaded; create a new handle to change it");
    if (n <= 0 || nnz <= 0 || !rowptr || !colidx || !vals || !b) return lpbox_fail(LPBOX_E_BADARG, "bad problem arguments");
    if (rowptr[0] != 0 || rowptr[n] != nnz) return lpbox_fail(LPBOX_E_BADARG, "rowptr does not span nnz");
    for (int i = 0; i < n; i++) {
        bool diag = false;
        if (rowptr[i + 1] < rowptr[i]) return lpbox_fail(LPBOX_E_BADARG, "rowptr not monotone");
        for (int k = rowptr[i]; k < rowptr[i + 1]; k++) {
            if (colidx[k] < 0 || colidx[k] >= n) return lpbox_fail(LPBOX_E_BADARG, "column index out of range");
            if (k > rowptr[i] && colidx[k] <= colidx[k - 1]) return lpbox_fail(LPBOX_E_BADARG, "column indices must ascend inside a row");
            if (!from_image && !std::isfinite(vals[k])) return lpbox_fail(LPBOX_E_BADARG, "vals has a non-finite stored value (row %d, column %d)", i, colidx[k]);
            diag |= colidx[k] == i;
        }
        if (!diag) return lpbox_fail(LPBOX_E_BADARG, "row %d stores no diagonal entry (the reference always stores one, SEGcpp:213-219)", i);
    }
    // a NaN in b makes every PCG exit test false: up to 1e4 x 1e3 PCG iterations of halt-and-resume chains before the call returns (the
    // reference accepts it and computes garbage; the same deliberate deviation as the LP path's, DESIGN.md sections 24 and 26).  What
    // the library's own cost builder made of an image is taken as it is: a constant image divides by a zero variance, every weight is
    // NaN, and the reference's result there -- NaN iterates -- is reproduced bit for bit (tests/test_seg_fuzz_gpu.py).
    for (int i = 0; i < n && !from_image; i++)
        if (!std::isfinite(b[i])) return lpbox_fail(LPBOX_E_BADARG, "b has a non-finite entry (index %d)", i);
    if (!from_image && !std::isfinite(c)) return lpbox_fail(LPBOX_E_BADARG, "c is not finite");
    s->n = n; s->nnz = nnz; s->rows = rows; s->cols = cols; s->c = c;
    s->rowptr.assign(rowptr, rowptr + n + 1); s->colidx.assign(colidx, colidx + nnz); s->vals.assign(vals, vals + nnz);
    s->orgb.assign(b, b + n);
    s->has_problem = true;
    return LPBOX_OK;
}

// Opt-in: the reference's summation order.  Before the problem: the staging buffers are allocated with it.
int segc_set_order(SegSolver *s, int mode) {
    if (mode != LPBOX_ORDER_DEFAULT && mode != LPBOX_ORDER_REFERENCE) return lpbox_fail(LPBOX_E_BADARG, "unknown summation order %d", mode);
    if (s->has_problem || s->uploaded || s->inited) return lpbox_fail(LPBOX_E_STATE, "set the summation order before lpbox_seg_set_image / lpbox_set_problem_bqp");
    s->order = mode;
    return LPBOX_OK;
}

int segc_set_image(SegSolver *s, const unsigned char *gray, int rows, int cols, int num_nodes) {
    if (!gray || rows <= 0 || cols <= 0 || num_nodes <= 0) return lpbox_fail(LPBOX_E_BADARG, "bad image arguments");
    const double scale = std::sqrt(num_nodes / (double)((long)rows * cols));     // SEGcpp:707
    std::vector<unsigned char> scaled;
    int sr = rows, sc = cols;
    const unsigned char *src = gray;
    if (scale != 1.0) { resize_linear_u8(gray, rows, cols, scale, scaled, sr, sc); src = scaled.data(); }
    if (sr < 2 || sc < 2) return lpbox_fail(LPBOX_E_BADARG, "scaled image %dx%d too small", sr, sc);
    std::vector<int> rowptr, colidx; std::vector<double> vals, b; double c = 0;
    build_costs(src, sr, sc, rowptr, colidx, vals, b, c);
    return segc_set_problem(s, sr * sc, (int)colidx.size(), rowptr.data(), colidx.data(), vals.data(), b.data(), c, sr, sc, true);
}

int segc_init(SegSolver *s) {
    if (!s->has_problem) return lpbox_fail(LPBOX_E_STATE, "no problem set");
    int rc = s->uploaded ? use_device(s->device) : upload(s);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(s->b.p, s->orgb.data(), sizeof(double) * (size_t)s->n, hipMemcpyHostToDevice, s->stream));
    s->left_idx.resize(s->n);
    for (int i = 0; i < s->n; i++) s->left_idx[i] = i;
    s->left_stale = false; s->dleft_valid = false; s->win_serial++;
    s->xi_valid = false; s->parity = 0; s->chain.pcg_resumes = 0;
    HIPCHK(seg_launch_init(s->dev(), s->ref() ? ref_c1(s->n) : std::pow((double)s->n, 1.0 / 2), s->stream));    // pow(n, 1/p), p = 2 (SEGcpp:557,670)
    if (s->ref()) { HIPCHK(segr_launch_rank(s->dev(), s->rf(), s->stream)); s->launches++; }      // the identity: every variable is live
    rc = read_state(s);
    if (rc) return rc;
    s->inited = true;
    return 1;
}

int segc_legacy(SegSolver *s, int *energy) {                                  // ADMM_bqp_unconstrained_legacy SEGcpp:1200-1380
    if (!s->inited) return lpbox_fail(LPBOX_E_STATE, "solve_init has not been called");
    int rc = use_device(s->device);
    if (rc) return rc;
    if (s->record > 0 && (!s->xhist.p || s->ws_cap < s->record)) {
        HIPCHK(hipStreamSynchronize(s->stream));
        HIPCHK(s->xhist.alloc((size_t)s->record * s->n)); s->ws_cap = s->record; s->graphs.clear();
        HIPCHK(hipMemsetAsync(s->xhist.p, 0, sizeof(double) * (size_t)s->ws_cap * s->n, s->stream));
    }
    HIPCHK(seg_launch_set_window(s->dev(), 0, SEG_MAX_ITERS, s->record > 0 ? 2 : 0, &s->parity, s->stream));
    rc = run_window(s, SEG_MAX_ITERS);
    if (rc) return rc;
    s->rec_cols = s->record > 0 ? std::min(s->hst.cc, s->ws_cap) : 0;
    s->xi_valid = false; s->win_serial++;
    if (energy) *energy = energy_int(s->hst.cur_obj + s->c);                   // :1379
    return LPBOX_OK;
}

// ADMM_bqp_unconstrained_init + _legacy (SEGcpp:658-810, 1200-1380) for B problems advanced in LOCKSTEP by one launch chain
// (image_segmentation.cpp:24-29 solves images 0..99 at 10^4 nodes one after the other: there a solve is launch-bound and the GPU
// mostly idle).  Every problem keeps its own control state, so the arithmetic of each is exactly that of a solve on its own.
int segc_legacy_batch(SegSolver **ss, int B, int *energies) {
    if (!ss || B <= 0) return lpbox_fail(LPBOX_E_BADARG, "empty batch");
    SegSolver *s0 = ss[0];
    for (int i = 0; i < B; i++) {
        if (!ss[i] || !ss[i]->has_problem) return lpbox_fail(LPBOX_E_STATE, "problem %d of the batch has no image / problem", i);
        if (ss[i]->device != s0->device) return lpbox_fail(LPBOX_E_BADARG, "all problems of a batch must live on one device");
        if (ss[i]->record > 0) return lpbox_fail(LPBOX_E_UNSUPPORTED, "recording is per-solver (lpbox_seg_legacy)");
        for (int k = 0; k < i; k++)                                 // one handle twice = every launch advancing the same buffers twice
            if (ss[k] == ss[i]) return lpbox_fail(LPBOX_E_BADARG, "problem %d and problem %d of the batch are the same handle", k, i);
    }
    if (int orc = batch_order_ok(ss, B)) return orc;
    // a solver counts as initialised only once the whole chain has completed: an early error return leaves every member of the
    // batch in the "solve_init has not been called" state instead of flagged ready with half-written device state
    for (int i = 0; i < B; i++) { ss[i]->inited = false; ss[i]->xi_valid = false; }
    int rc = LPBOX_OK;
    int Gmax = 0;
    for (int i = 0; i < B; i++) {                                   // upload + host-side reset of segc_init (the init KERNEL runs batched)
        if ((rc = batch_reset_handle(ss[i]))) return rc;
        Gmax = std::max(Gmax, ss[i]->G);
    }
    for (int i = 0; i < B; i++) HIPCHK(hipStreamSynchronize(ss[i]->stream));
    hipStream_t st = s0->stream;
    std::vector<SegDev> hd(B);
    for (int i = 0; i < B; i++) hd[i] = ss[i]->dev();
    DevBuf<SegDev> devs; DevBuf<SegState> dstates; DevBuf<SegRef> refs;
    HIPCHK(devs.alloc(B)); HIPCHK(dstates.alloc(B));
    HIPCHK(hipMemcpyAsync(devs.p, hd.data(), sizeof(SegDev) * (size_t)B, hipMemcpyHostToDevice, st));
    std::vector<SegRef> hr;
    if (s0->ref()) {
        hr.resize(B);
        for (int i = 0; i < B; i++) hr[i] = ss[i]->rf();
        HIPCHK(refs.alloc(B));
        HIPCHK(hipMemcpyAsync(refs.p, hr.data(), sizeof(SegRef) * (size_t)B, hipMemcpyHostToDevice, st));
    }
    std::vector<SegState> hs(B);
    int parity = 0, kmax = s0->chain.kmax;
    long long launches = 0;
    std::vector<long long> resumes(B, 0);
    HIPCHK(s0->timer.start(st));
    HIPCHK(segb_launch_init(devs.p, B, Gmax, st));
    if (refs.p) { HIPCHK(segrb_launch_rank(devs.p, refs.p, B, st)); launches++; }
    HIPCHK(segb_launch_set_window(devs.p, B, 0, SEG_MAX_ITERS, 0, &parity, st));
    launches += 2;
    if ((rc = segb_run_chain(s0->chain.rules, &kmax, s0->chain.adaptive, nullptr, SEG_MAX_ITERS, resumes.data(),
                             SegBatchOps{devs.p, dstates.p, B, Gmax, hs.data(), parity, launches, st, refs.p}))) return rc;
    double ms = 0.0;
    HIPCHK(s0->timer.stop_sync(st, &ms));
    for (int i = 0; i < B; i++) {
        SegSolver *s = ss[i];
        s->hst = hs[i]; s->parity = parity; s->rec_cols = 0; s->xi_valid = false; s->inited = true;
        s->chain.pcg_resumes += resumes[i];
        if (energies) energies[i] = energy_int(s->hst.cur_obj + s->c); // :1379
    }
    s0->kernel_ms += ms; s0->launches += launches;
    return LPBOX_OK;
}

int segc_l2f(SegSolver *s, int iter_start, int iter_end, const double *vec, int num, int *ret) {   // SEGcpp:917-1195
    if (!s->inited) return lpbox_fail(LPBOX_E_STATE, "solve_init has not been called");
    const int ws = iter_end - iter_start;
    if (ws > SEG_XITERS_COLS) return lpbox_fail(LPBOX_E_BADARG, "window of %d iterations exceeds the %d columns of x_iters (SEGcpp:924)", ws, SEG_XITERS_COLS);
    int rc = use_device(s->device);
    if (rc) return rc;
    if ((rc = refresh_left(s))) return rc;
    const int n_live = (int)s->left_idx.size();
    if (num < 0 || num > n_live) return lpbox_fail(LPBOX_E_BADARG, "fix count %d outside [0,%d]", num, n_live);
    if (num != 0) {
        if (!vec) return lpbox_fail(LPBOX_E_BADARG, "fix vector missing");
        int cnt = 0;
        for (int q = 0; q < n_live; q++) if (vec[q] == 1 || vec[q] == 0) cnt++;
        if (cnt != num) return lpbox_fail(LPBOX_E_BADARG, "vec fixes %d variables but num = %d", cnt, num);
    }
    HIPCHK(seg_launch_set_window(s->dev(), iter_start, iter_end, 3, &s->parity, s->stream));
    if (num != 0) {
        std::vector<uint8_t> nf(s->n, 0);
        std::vector<int> keep; keep.reserve(n_live - num);
        for (int q = 0; q < n_live; q++) {
            const int org = s->left_idx[q];
            if (vec[q] == 1) nf[org] = 2; else if (vec[q] == 0) nf[org] = 1; else keep.push_back(org);
        }
        s->left_idx.swap(keep);
        HIPCHK(hipMemcpy(s->newfix.p, nf.data(), nf.size(), hipMemcpyHostToDevice));
        HIPCHK(seg_launch_fix(s->dev(), n_live - num, s->ref() ? ref_c1(n_live - num) : std::pow((double)(n_live - num), 1.0 / 2), &s->parity, s->stream));
        if (s->ref()) { HIPCHK(segr_launch_rank(s->dev(), s->rf(), s->stream)); s->launches++; }   // the live set has changed
        HIPCHK(hipMemsetAsync(s->newfix.p, 0, s->n, s->stream));
    }
    s->xi_rows = n_live - num; s->xi_left_idx = s->left_idx;
    if (ws > 0 && (!s->xhist.p || s->ws_cap < ws)) {
        HIPCHK(hipStreamSynchronize(s->stream));
        HIPCHK(s->xhist.alloc((size_t)SEG_XITERS_COLS * s->n)); s->ws_cap = SEG_XITERS_COLS; s->graphs.clear();
    }
    if (s->ws_cap > 0 && s->xhist.p) HIPCHK(hipMemsetAsync(s->xhist.p, 0, sizeof(double) * (size_t)s->ws_cap * s->n, s->stream));   // x_iters = Zero (SEGcpp:924): ALL staged columns, also those of an earlier, longer window
    s->rec_cols = 0;
    if (!s->left_idx.empty()) HIPCHK(hipMemcpyAsync(s->d_left.p, s->left_idx.data(), sizeof(int) * s->left_idx.size(), hipMemcpyHostToDevice, s->stream));
    s->dleft_valid = true;
    rc = run_window(s, iter_end);
    if (rc) return rc;
    s->last_ws = ws; s->xi_valid = true; s->win_serial++;
    if (ret) *ret = s->hst.ret;
    return LPBOX_OK;
}

int segc_get_n(SegSolver *s) { return s->inited ? s->hst.n_live : s->n; }
int segc_get_org_n(SegSolver *s) { return s->n; }
int segc_get_iter(SegSolver *s) { return s->inited ? s->hst.iter : 0; }
int segc_get_shape(SegSolver *s, int *rows, int *cols) { if (rows) *rows = s->rows; if (cols) *cols = s->cols; return LPBOX_OK; }

int segc_set_record(SegSolver *s, int on) {
    s->record = on <= 0 ? 0 : (on == 1 ? SEG_REC_COLS : on);
    return LPBOX_OK;
}

int segc_get_x_history(SegSolver *s, int first, int count, double *out) {     // rows of ../xiter/<problem>.csv (SEGcpp:1270-1277)
    if (!out) return s->rec_cols;
    if (first < 0 || count < 0 || first + count > s->rec_cols)
        return lpbox_fail(LPBOX_E_BADARG, "iterations [%d,%d) outside the %d recorded", first, first + count, s->rec_cols);
    int rc = use_device(s->device);
    if (rc) return rc;
    if (count) HIPCHK(hipMemcpy(out, s->xhist.p + (size_t)first * s->n, sizeof(double) * (size_t)count * s->n, hipMemcpyDeviceToHost));
    return count;
}

int segc_get_x_iters(SegSolver *s, int ws, double *out) {                     // get_x_iters_d SEGcpp:839-851
    if (!s->xi_valid) return lpbox_fail(LPBOX_E_STATE, "solve_iter_l2f has not been called");
    if (ws < 0 || ws > SEG_XITERS_COLS) return lpbox_fail(LPBOX_E_BADARG, "ws = %d outside [0,%d]", ws, SEG_XITERS_COLS);
    const int rows = s->xi_rows;
    if (!out || rows == 0 || ws == 0) return rows;
    int rc = use_device(s->device);
    if (rc) return rc;
    if (s->xi_out.count < (size_t)rows * ws) HIPCHK(s->xi_out.alloc((size_t)s->n * SEG_XITERS_COLS));
    HIPCHK(seg_launch_pack_xiters(s->dev(), s->d_left.p, rows, ws, s->xi_out.p, s->stream));
    HIPCHK(hipMemcpyAsync(out, s->xi_out.p, sizeof(double) * (size_t)rows * ws, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return rows;
}

// the same (rows x ws) row-major window left on the device (stride = rows * ws doubles: one problem per handle)
int segc_get_x_iters_device(SegSolver *s, int ws, void **dev_ptr, long *stride) {
    if (!s->xi_valid) return lpbox_fail(LPBOX_E_STATE, "solve_iter_l2f has not been called");
    if (ws <= 0 || ws > SEG_XITERS_COLS) return lpbox_fail(LPBOX_E_BADARG, "ws = %d outside (0,%d]", ws, SEG_XITERS_COLS);
    int rc = use_device(s->device);
    if (rc) return rc;
    const int rows = s->xi_rows;
    if (s->xi_out.count < (size_t)std::max(rows, 1) * ws) HIPCHK(s->xi_out.alloc((size_t)s->n * SEG_XITERS_COLS));
    HIPCHK(seg_launch_pack_xiters(s->dev(), s->d_left.p, rows, ws, s->xi_out.p, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    if (dev_ptr) *dev_ptr = s->xi_out.p;
    if (stride) *stride = (long)rows * ws;
    return LPBOX_OK;
}

static int fetch_solution(SegSolver *s, std::vector<double> &sol) {            // get_x_sol SEGcpp:895-914
    std::vector<double> x(s->n); std::vector<uint8_t> live(s->n), fv(s->n);
    HIPCHK(hipMemcpy(x.data(), s->x.p, sizeof(double) * (size_t)s->n, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(live.data(), s->live.p, s->n, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(fv.data(), s->fixval.p, s->n, hipMemcpyDeviceToHost));
    sol.resize(s->n);
    for (int i = 0; i < s->n; i++) sol[i] = live[i] ? (x[i] >= 0.5 ? 1.0 : 0.0) : (double)fv[i];
    return LPBOX_OK;
}

int segc_get_x_sol(SegSolver *s, double *out) {
    if (!s->inited || !out) return lpbox_fail(LPBOX_E_STATE, "not initialised");
    int rc = use_device(s->device);
    if (rc) return rc;
    std::vector<double> sol;
    if ((rc = fetch_solution(s, sol))) return rc;
    memcpy(out, sol.data(), sizeof(double) * (size_t)s->n);
    return s->n;
}

int segc_get_obj(SegSolver *s, double *out) {                                 // get_final_obj SEGcpp:868-893
    if (!s->inited || !out) return lpbox_fail(LPBOX_E_STATE, "not initialised");
    int rc = use_device(s->device);
    if (rc) return rc;
    std::vector<double> xx;
    if ((rc = fetch_solution(s, xx))) return rc;
    if (s->ref()) {
        // reference order: x.dot(A x) and b.dot(x) over the full-length vectors in Eigen's redux association (SEGcpp:868-893); the
        // problem need not be an image's, so the terms need not be integers
        std::vector<double> t1((size_t)s->n), t2((size_t)s->n);
        for (int i = 0; i < s->n; i++) {
            double t = 0;
            for (int k = s->rowptr[i]; k < s->rowptr[i + 1]; k++) t += s->vals[k] * xx[s->colidx[k]];
            double r = 0.0;
            r += 1.0 * t;
            t1[i] = xx[i] * r; t2[i] = s->orgb[i] * xx[i];
        }
        *out = (eigen_sum(t1) + eigen_sum(t2)) + s->c;
        return LPBOX_OK;
    }
    // compute_cost(xx, org_A, org_b) = xx.(A xx) + b.xx; every term is an integer, so the summation order is immaterial
    double val = 0.0, val2 = 0.0;
    for (int i = 0; i < s->n; i++) {
        double t = 0;
        for (int k = s->rowptr[i]; k < s->rowptr[i + 1]; k++) t += s->vals[k] * xx[s->colidx[k]];
        val += xx[i] * (0.0 + 1.0 * t);
        val2 += s->orgb[i] * xx[i];
    }
    *out = (val + val2) + s->c;
    return LPBOX_OK;
}

int segc_get_config(SegSolver *s, int *threads, int *ept, int *groups) {
    if (!s->uploaded) { int rc = upload(s); if (rc) return rc; }
    if (threads) *threads = SEG_T;
    if (ept) *ept = s->EPT;
    if (groups) *groups = s->G;
    return LPBOX_OK;
}

int segc_get_counters(SegSolver *s, long long *outer, long long *pcg) {
    if (outer) *outer = s->hst.outer_total;
    if (pcg) *pcg = s->hst.pcg_total;
    return LPBOX_OK;
}

int segc_get_stop(SegSolver *s, int *reason, int *legacy_iter_p1) {
    if (reason) *reason = s->hst.stop;
    if (legacy_iter_p1) *legacy_iter_p1 = s->hst.legacy_iter_p1;
    return LPBOX_OK;
}

int segc_kernel_time(SegSolver *s, double *ms, long long *launches, int reset) {
    if (ms) *ms = s->kernel_ms;
    if (launches) *launches = s->launches;
    if (reset) { s->kernel_ms = 0.0; s->launches = 0; }
    return LPBOX_OK;
}

int segc_debug_vec(SegSolver *s, const char *name, double *out, int cap) {
    if (!s->inited) return lpbox_fail(LPBOX_E_STATE, "not initialised");
    int rc = use_device(s->device);
    if (rc) return rc;
    const double *src = nullptr;
    if (!strcmp(name, "x")) src = s->x.p; else if (!strcmp(name, "z1")) src = s->z1.p; else if (!strcmp(name, "z2")) src = s->z2.p;
    else if (!strcmp(name, "b")) src = s->b.p; else if (!strcmp(name, "y1")) src = s->y1.p; else if (!strcmp(name, "y2")) src = s->y2.p;
    else if (!strcmp(name, "td")) src = s->td.p;
    else return lpbox_fail(LPBOX_E_BADARG, "unknown vector '%s'", name);
    if (cap < s->n) return lpbox_fail(LPBOX_E_BADARG, "buffer too small");
    HIPCHK(hipMemcpy(out, src, sizeof(double) * (size_t)s->n, hipMemcpyDeviceToHost));
    return s->n;
}

int segc_debug_scalar(SegSolver *s, const char *name, double *out) {
    const SegState &h = s->hst;
    struct { const char *n; double v; } tab[] = {
        {"rho1", h.rho1}, {"gamma", h.gamma_val}, {"cur_obj", h.cur_obj}, {"std_obj", h.std_obj}, {"cvg1", h.cvg1}, {"cvg2", h.cvg2},
        {"obj_val", h.obj_val}, {"best_bin_obj", h.best_bin_obj}, {"c", s->c}, {"last_pcg", (double)h.last_pcg}, {"iter", (double)h.iter},
        {"matrix_as_diagonals", s->dia ? 1.0 : 0.0}, {"ell_width", (double)s->ell_w},
        {"pcg_resumes", (double)s->chain.pcg_resumes}, {"kmax", (double)s->chain.kmax}, {"order", (double)s->order},
    };
    for (auto &e : tab) if (!strcmp(e.n, name)) { *out = e.v; return LPBOX_OK; }
    return lpbox_fail(LPBOX_E_BADARG, "unknown scalar '%s'", name);
}

int segc_get_problem(SegSolver *s, int *n, int *nnz, int *rowptr, int *colidx, double *vals, double *b, double *c) {
    if (!s->has_problem) return lpbox_fail(LPBOX_E_STATE, "no problem set");
    if (n) *n = s->n;
    if (nnz) *nnz = s->nnz;
    if (rowptr) memcpy(rowptr, s->rowptr.data(), sizeof(int) * ((size_t)s->n + 1));
    if (colidx) memcpy(colidx, s->colidx.data(), sizeof(int) * (size_t)s->nnz);
    if (vals) memcpy(vals, s->vals.data(), sizeof(double) * (size_t)s->nnz);
    if (b) memcpy(b, s->orgb.data(), sizeof(double) * (size_t)s->n);
    if (c) *c = s->c;
    return LPBOX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Early-fixing windows (SEGcpp:917-1195; the loop of SEG/trainer.py:699-745) for a BATCH of handles: every active problem runs
// iterations [iter_start, iter_end) through one lockstep launch chain (the chain of segc_legacy_batch, cut at iter_end), the
// fix of all problems is one launch, the live lists are compacted on the device and the windows are packed into one buffer.
// Per problem the arithmetic is that of segc_l2f on its own; the handles stay ordinary handles.
struct lpbox_seg_batch {
    std::vector<SegSolver *> ss;
    std::vector<uint8_t> active;
    int B = 0, kmax = 10;
    ChainRules rules = seg_rules();
    hipStream_t stream = nullptr;
    StreamTimer timer;
    DevBuf<SegDev> devs; DevBuf<SegBatchAux> aux; DevBuf<SegFixPar> par; DevBuf<SegState> dstates; DevBuf<int> counts; DevBuf<double> pack;
    bool ref = false;                            // every member runs in the reference's summation order (checked at create)
    DevBuf<SegRef> refs; std::vector<SegRef> h_refs;   // ... then the staging descriptors of the handles behind devs, in that order
    uint8_t *h_newfix = nullptr;                 // pinned staging of the host-vector form, problem i at nf_off[i]
    std::vector<size_t> nf_off;
    std::vector<SegDev> h_devs; std::vector<SegBatchAux> h_aux;   // host side of devs / aux (alive until the stream has taken them)
    // the most recent pack: rows of handle i = [row_off[i], row_off[i+1]), taken after window pack_serial[i] of that handle (-1: not packed)
    std::vector<int> row_off; std::vector<long> pack_serial;
    bool pack_valid = false;
};

namespace {

int segb_ensure(lpbox_seg_batch *b) {
    if (b->stream) return LPBOX_OK;
    const int B = b->B;
    HIPCHK(hipStreamCreate(&b->stream));
    HIPCHK(b->timer.create());
    HIPCHK(b->devs.alloc(B)); HIPCHK(b->aux.alloc(B)); HIPCHK(b->par.alloc(B)); HIPCHK(b->dstates.alloc(B)); HIPCHK(b->counts.alloc(2 * (size_t)B));
    if (b->ref) HIPCHK(b->refs.alloc(B));
    size_t tot = 0;
    b->nf_off.assign(B, 0);
    for (int i = 0; i < B; i++) { b->nf_off[i] = tot; tot += (size_t)b->ss[i]->n; }
    HIPCHK(hipHostMalloc((void **)&b->h_newfix, tot));
    return LPBOX_OK;
}

// descriptors of the handles `act` (device arrays devs / aux in that order); rows[k] / row0[k]: live count and first packed row
int segb_describe(lpbox_seg_batch *b, const std::vector<int> &act, const std::vector<int> &rows, const std::vector<int> &row0) {
    std::vector<SegDev> &hd = b->h_devs; std::vector<SegBatchAux> &ha = b->h_aux;
    hd.resize(act.size()); ha.resize(act.size());
    for (size_t k = 0; k < act.size(); k++) {
        SegSolver *s = b->ss[act[k]];
        hd[k] = s->dev();
        ha[k].left = s->d_left.p; ha[k].row0 = row0[k]; ha[k].rows = rows[k];
    }
    HIPCHK(hipMemcpyAsync(b->devs.p, hd.data(), sizeof(SegDev) * hd.size(), hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipMemcpyAsync(b->aux.p, ha.data(), sizeof(SegBatchAux) * ha.size(), hipMemcpyHostToDevice, b->stream));
    if (b->ref) {
        b->h_refs.resize(act.size());
        for (size_t k = 0; k < act.size(); k++) b->h_refs[k] = b->ss[act[k]]->rf();
        HIPCHK(hipMemcpyAsync(b->refs.p, b->h_refs.data(), sizeof(SegRef) * act.size(), hipMemcpyHostToDevice, b->stream));
    }
    return LPBOX_OK;
}

// one window.  Host-vector form: vecs / nums (deter_fix_2 done by the caller); score form: scores (device, float32, one per packed row of
// the last pack) or NULL, the rule runs on the device.  `score_form` selects which.
int segb_window(lpbox_seg_batch *b, int iter_start, int iter_end, bool score_form, const double *vecs, long vec_stride, const int *nums,
                const float *scores, double hi, double lo, int min_fix, int *rets, int *fixed) {
    const int ws = iter_end - iter_start;
    if (ws > SEG_XITERS_COLS) return lpbox_fail(LPBOX_E_BADARG, "window of %d iterations exceeds the %d columns of x_iters (SEGcpp:924)", ws, SEG_XITERS_COLS);
    const std::vector<int> act = active_members(b->active);
    const int A = (int)act.size();
    std::vector<int> live(A), num(A, 0);
    for (int k = 0; k < A; k++) { SegSolver *s = b->ss[act[k]]; live[k] = s->inited ? s->hst.n_live : s->n; }
    if (!score_form) {
        for (int k = 0; k < A; k++) {
            const int i = act[k];
            num[k] = nums ? nums[i] : 0;
            if (num[k] < 0 || num[k] > live[k]) return lpbox_fail(LPBOX_E_BADARG, "problem %d of the batch: fix count %d outside [0,%d]", i, num[k], live[k]);
            if (num[k] == 0) continue;
            if (!vecs) return lpbox_fail(LPBOX_E_BADARG, "problem %d of the batch: fix vector missing", i);
            if (vec_stride < live[k]) return lpbox_fail(LPBOX_E_BADARG, "problem %d of the batch: fix vector holds %ld entries, %d live variables", i, vec_stride, live[k]);
            const double *vec = vecs + (size_t)i * vec_stride;
            int cnt = 0;
            for (int q = 0; q < live[k]; q++) if (vec[q] == 1 || vec[q] == 0) cnt++;
            if (cnt != num[k]) return lpbox_fail(LPBOX_E_BADARG, "problem %d of the batch: vec fixes %d variables but num = %d", i, cnt, num[k]);
        }
    } else if (scores) {
        if (!b->pack_valid) return lpbox_fail(LPBOX_E_STATE, "scores given, but lpbox_seg_batch_get_x_iters_device has not been called since the last window");
        for (int k = 0; k < A; k++)
            if (b->pack_serial[act[k]] != b->ss[act[k]]->win_serial || b->pack_serial[act[k]] < 0 ||
                b->row_off[act[k] + 1] - b->row_off[act[k]] != live[k])
                return lpbox_fail(LPBOX_E_STATE, "problem %d of the batch is active but its window is not in the packed buffer the scores refer to", act[k]);
    }
    for (int k = 0; k < A; k++)
        if (!b->ss[act[k]]->inited) return lpbox_fail(LPBOX_E_STATE, "problem %d of the batch: solve_init has not been called", act[k]);
    int rc = use_device(b->ss[0]->device);
    if (rc) return rc;
    if (A == 0) return LPBOX_OK;
    if ((rc = segb_ensure(b))) return rc;
    hipStream_t st = b->stream;
    int Gmax = 0;
    for (int k = 0; k < A; k++) {
        SegSolver *s = b->ss[act[k]];
        Gmax = std::max(Gmax, s->G);
        if (ws > 0 && (!s->xhist.p || s->ws_cap < ws)) {
            HIPCHK(hipStreamSynchronize(s->stream));
            HIPCHK(s->xhist.alloc((size_t)SEG_XITERS_COLS * s->n)); s->ws_cap = SEG_XITERS_COLS; s->graphs.clear();
        }
        if (!s->dleft_valid) {                       // first early-fixing window after an init: the identity list
            if (!s->left_idx.empty()) HIPCHK(hipMemcpyAsync(s->d_left.p, s->left_idx.data(), sizeof(int) * s->left_idx.size(), hipMemcpyHostToDevice, st));
            s->dleft_valid = true;
        }
    }
    // one ping-pong parity for the chain: a handle that ran windows of its own in between may sit on the other one
    int parity = b->ss[act[0]]->parity;
    long long launches = 0;
    for (int k = 1; k < A; k++) {
        SegSolver *s = b->ss[act[k]];
        if (s->parity != parity) { HIPCHK(seg_launch_copy(s->dev(), 0, &s->parity, st)); launches++; }
    }
    std::vector<int> row0(A, 0);
    if (score_form && scores) for (int k = 0; k < A; k++) row0[k] = b->row_off[act[k]];
    if ((rc = segb_describe(b, act, live, row0))) return rc;
    HIPCHK(b->timer.start(st));

    std::vector<SegFixPar> hp(A);
    std::vector<int> applied(A, 0);
    std::vector<std::vector<int>> kept(A);        // host-vector form: the new live lists, taken over once the window has completed
    bool any = false;
    if (score_form && scores) {
        std::vector<int> hc(2 * (size_t)A);
        HIPCHK(hipMemsetAsync(b->counts.p, 0, sizeof(int) * hc.size(), st));
        HIPCHK(segb_launch_decide(b->devs.p, b->aux.p, A, *std::max_element(live.begin(), live.end()), scores, hi, lo, b->counts.p, st));
        HIPCHK(hipMemcpyAsync(hc.data(), b->counts.p, sizeof(int) * hc.size(), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        launches++;
        for (int k = 0; k < A; k++) { const int kf = hc[2 * k] + hc[2 * k + 1]; if (kf > min_fix) applied[k] = kf; }     // SEG/trainer.py:735-736
    } else if (!score_form) {
        for (int k = 0; k < A; k++) {
            if (num[k] == 0) continue;
            SegSolver *s = b->ss[act[k]];
            if ((rc = refresh_left(s))) return rc;
            const double *vec = vecs + (size_t)act[k] * vec_stride;
            uint8_t *nf = b->h_newfix + b->nf_off[act[k]];
            memset(nf, 0, (size_t)s->n);
            std::vector<int> &keep = kept[k]; keep.reserve(live[k] - num[k]);
            for (int q = 0; q < live[k]; q++) {
                const int org = s->left_idx[q];
                if (vec[q] == 1) nf[org] = 2; else if (vec[q] == 0) nf[org] = 1; else keep.push_back(org);
            }
            HIPCHK(hipMemcpyAsync(s->newfix.p, nf, (size_t)s->n, hipMemcpyHostToDevice, st));
            applied[k] = num[k];
        }
    }
    for (int k = 0; k < A; k++) {
        const int nl = live[k] - applied[k];
        hp[k].apply = applied[k] > 0 ? 1 : 0; hp[k].n_live_new = nl;
        hp[k].c1_new = b->ref ? ref_c1(nl) : std::pow((double)nl, 1.0 / 2);             // on the host, as segc_l2f: pow and a device sqrt differ by an ulp now and then
        any |= applied[k] > 0;
    }
    HIPCHK(hipMemcpyAsync(b->par.p, hp.data(), sizeof(SegFixPar) * (size_t)A, hipMemcpyHostToDevice, st));
    HIPCHK(segb_launch_set_window(b->devs.p, A, iter_start, iter_end, 3, &parity, st));
    HIPCHK(segb_launch_fix(b->devs.p, b->par.p, A, Gmax, &parity, st));          // also x_iters = Zero, all staged columns
    launches += 2;
    if (any) { HIPCHK(segb_launch_compact(b->devs.p, b->aux.p, b->par.p, A, st)); launches++; }
    if (any && b->ref) { HIPCHK(segrb_launch_rank(b->devs.p, b->refs.p, A, st)); launches++; }      // the live sets have changed

    std::vector<SegState> hs(A);
    std::vector<long long> resumes(A, 0);
    if ((rc = segb_run_chain(b->rules, &b->kmax, b->ss[0]->chain.adaptive, act.data(), iter_end, resumes.data(),
                             SegBatchOps{b->devs.p, b->dstates.p, A, Gmax, hs.data(), parity, launches, st, b->ref ? b->refs.p : nullptr}))) return rc;
    double ms = 0.0;
    HIPCHK(b->timer.stop_sync(st, &ms));
    for (int k = 0; k < A; k++) {
        SegSolver *s = b->ss[act[k]];
        s->hst = hs[k]; s->parity = parity; s->rec_cols = 0;
        s->xi_rows = live[k] - applied[k]; s->last_ws = ws; s->xi_valid = true; s->win_serial++;
        s->chain.pcg_resumes += resumes[k];
        if (score_form && applied[k]) s->left_stale = true;          // fixed on the device: the host list follows on demand
        else if (applied[k]) s->left_idx.swap(kept[k]);
        s->xi_left_idx.clear();
        if (rets) rets[act[k]] = s->hst.ret;
        if (fixed) fixed[act[k]] = applied[k];
    }
    b->ss[act[0]]->kernel_ms += ms; b->ss[act[0]]->launches += launches;
    b->pack_valid = false;
    return LPBOX_OK;
}

}  // namespace

lpbox_seg_batch *segbc_create(SegSolver **ss, int B) {
    auto refuse = [](int) -> lpbox_seg_batch * { return nullptr; };        // lpbox_fail has recorded status and text
    if (!ss || B <= 0) return refuse(lpbox_fail(LPBOX_E_BADARG, "empty batch"));
    for (int i = 0; i < B; i++) {                                   // the checks of segc_legacy_batch; no device call
        if (!ss[i] || !ss[i]->has_problem) return refuse(lpbox_fail(LPBOX_E_STATE, "problem %d of the batch has no image / problem", i));
        if (ss[i]->device != ss[0]->device) return refuse(lpbox_fail(LPBOX_E_BADARG, "problem %d of the batch lives on another device than problem 0", i));
        if (ss[i]->record > 0) return refuse(lpbox_fail(LPBOX_E_UNSUPPORTED, "problem %d of the batch is recording; recording is per-solver (lpbox_seg_legacy)", i));
        for (int k = 0; k < i; k++)
            if (ss[k] == ss[i]) return refuse(lpbox_fail(LPBOX_E_BADARG, "problem %d and problem %d of the batch are the same handle", k, i));
    }
    if (int orc = batch_order_ok(ss, B)) return refuse(orc);
    lpbox_seg_batch *b = new lpbox_seg_batch();
    b->ref = ss[0]->ref();
    b->ss.assign(ss, ss + B); b->B = B; b->active.assign(B, 1); b->kmax = ss[0]->chain.kmax;
    b->row_off.assign((size_t)B + 1, 0); b->pack_serial.assign(B, -1);
    return b;
}

void segbc_destroy(lpbox_seg_batch *b) {
    if (!b) return;
    if (b->stream) {
        (void)hipSetDevice(b->ss[0]->device);
        (void)hipStreamSynchronize(b->stream);
        if (b->h_newfix) (void)hipHostFree(b->h_newfix);
        b->timer.destroy();
        (void)hipStreamDestroy(b->stream);
    }
    delete b;
}

int segbc_set_active(lpbox_seg_batch *b, const unsigned char *active) {
    for (int i = 0; i < b->B; i++) b->active[i] = active ? (active[i] ? 1 : 0) : 1;
    return LPBOX_OK;
}

// lpbox_init on every handle: upload, host-side reset, ONE batched init launch (the head of segc_legacy_batch)
int segbc_init(lpbox_seg_batch *b) {
    const int B = b->B;
    for (int i = 0; i < B; i++) { b->ss[i]->inited = false; b->ss[i]->xi_valid = false; }
    b->pack_valid = false;
    int rc = LPBOX_OK, Gmax = 0;
    for (int i = 0; i < B; i++) {
        if ((rc = batch_reset_handle(b->ss[i]))) return rc;
        Gmax = std::max(Gmax, b->ss[i]->G);
    }
    for (int i = 0; i < B; i++) HIPCHK(hipStreamSynchronize(b->ss[i]->stream));
    if ((rc = segb_ensure(b))) return rc;
    std::vector<int> all(B), zero(B, 0);
    for (int i = 0; i < B; i++) all[i] = i;
    if ((rc = segb_describe(b, all, zero, zero))) return rc;
    HIPCHK(segb_launch_init(b->devs.p, B, Gmax, b->stream));
    if (b->ref) { HIPCHK(segrb_launch_rank(b->devs.p, b->refs.p, B, b->stream)); b->ss[0]->launches += 1; }
    std::vector<SegState> hs(B);
    HIPCHK(segb_collect_states(b->devs.p, B, 0, b->dstates.p, b->stream));
    HIPCHK(hipMemcpyAsync(hs.data(), b->dstates.p, sizeof(SegState) * (size_t)B, hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    for (int i = 0; i < B; i++) { SegSolver *s = b->ss[i]; s->hst = hs[i]; s->parity = 0; s->rec_cols = 0; s->inited = true; }
    b->ss[0]->launches += 1;
    return 1;
}

int segbc_l2f(lpbox_seg_batch *b, int iter_start, int iter_end, const double *vecs, long vec_stride, const int *nums, int *rets) {
    return segb_window(b, iter_start, iter_end, false, vecs, vec_stride, nums, nullptr, 0.0, 0.0, 0, rets, nullptr);
}

int segbc_l2f_scores(lpbox_seg_batch *b, int iter_start, int iter_end, const float *scores_dev, double hi, double lo, int min_fix,
                     int *rets, int *fixed) {
    return segb_window(b, iter_start, iter_end, true, nullptr, 0, nullptr, scores_dev, hi, lo, min_fix, rets, fixed);
}

// the (n_live x ws) windows of all active handles, one after the other, in ONE buffer of the batch (one launch)
int segbc_get_x_iters_device(lpbox_seg_batch *b, int ws, void **dev_ptr, long *row_off) {
    if (ws <= 0 || ws > SEG_XITERS_COLS) return lpbox_fail(LPBOX_E_BADARG, "ws = %d outside (0,%d]", ws, SEG_XITERS_COLS);
    const std::vector<int> act = active_members(b->active);
    const int A = (int)act.size();
    for (int k = 0; k < A; k++)
        if (!b->ss[act[k]]->xi_valid) return lpbox_fail(LPBOX_E_STATE, "problem %d of the batch: solve_iter_l2f has not been called", act[k]);
    int rc = use_device(b->ss[0]->device);
    if (rc) return rc;
    if ((rc = segb_ensure(b))) return rc;
    std::vector<int> rows(A), row0(A);
    std::fill(b->pack_serial.begin(), b->pack_serial.end(), -1L);
    int tot = 0, k = 0, max_rows = 0;
    for (int i = 0; i < b->B; i++) {
        b->row_off[i] = tot;
        if (k < A && act[k] == i) {
            rows[k] = b->ss[i]->xi_rows; row0[k] = tot; tot += rows[k]; max_rows = std::max(max_rows, rows[k]);
            b->pack_serial[i] = b->ss[i]->win_serial; k++;
        }
    }
    b->row_off[b->B] = tot;
    if (!b->pack.p) {
        size_t cap = 0;
        for (int i = 0; i < b->B; i++) cap += (size_t)b->ss[i]->n;
        HIPCHK(b->pack.alloc(cap * SEG_XITERS_COLS));
    }
    if (A > 0 && tot > 0) {
        if ((rc = segb_describe(b, act, rows, row0))) return rc;
        HIPCHK(segb_launch_pack_xiters(b->devs.p, b->aux.p, A, max_rows, ws, b->pack.p, b->stream));
        HIPCHK(hipStreamSynchronize(b->stream));
        b->ss[act[0]]->launches += 1;
    }
    b->pack_valid = true;
    if (dev_ptr) *dev_ptr = b->pack.p;
    if (row_off) for (int i = 0; i <= b->B; i++) row_off[i] = b->row_off[i];
    return LPBOX_OK;
}
