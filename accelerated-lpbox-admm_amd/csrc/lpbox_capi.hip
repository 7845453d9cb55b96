// lpbox_capi.hip -- the C-ABI of liblpbox_hip.so (include/lpbox_hip.h): handle management, host-side index
// bookkeeping of early fixing, instance readers and result getters.  All solver arithmetic runs in the HIP kernels of
// lpbox_lp_kernels.hip; there is no CPU fallback.  The error-check macros, use_device, the device buffer and the stream timer are those of
// lpbox_host.h, shared with the other host files.
//
// Reference citations: LPcpp = LinerProgramming/LinearProgramming/cython_solver/LPboxADMMsolver.cpp,
//                      LPh   = .../cython_solver/LPboxADMMsolver.h, pxd = .../cython_solver/LPboxADMMsolver.pxd
#include "../../include/lpbox_hip.h"
#include "lpbox_lp.h"
#include "lpbox_lp_layout.h"
#include "lpbox_capi_internal.h"
#include "lpbox_host.h"
#include "lpbox_policy.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace {

thread_local std::string g_err;
thread_local int g_device = 0;
thread_local int g_status = 0;        // the code that came with g_err

}  // namespace

int lpbox_fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf; g_status = code;
    return code;
}

namespace {

struct LpInstance {
    int n = 0, l = 0, nnz = 0;
    std::vector<int> colptr, rowidx;   // CSC of E, as read (LPcpp:2416-2444)
    std::vector<int> rowptr, colidx;   // CSR of the same matrix
    std::vector<double> vals, vals_csr; // stored values in CSC / CSR entry order; empty = every entry is 1.0 (a unit instance)
    LpInstanceLayout lay;              // storage layout and the index tables of the kernels (plan)
    std::vector<int> dir_g;            // direct x-update: dense index of row r among the G rows, -1 = D row (lpbox_set_x_update)
    int nG = 0;
    std::vector<double> b, f_org;
    // early-fix bookkeeping (LPcpp:1192-1206): original index of each live variable, in compact order
    std::vector<int> left_idx;
    std::vector<int> xi_left_idx;      // live map at the time of the last l2f call (rows of x_iters)
    int xi_rows = 0;
    bool set = false;
};

}  // namespace

struct lpbox_solver {
    int flavour = LPBOX_FLAVOUR_LP, B = 0, print_info = 0, device = 0;
    SegSolver *seg = nullptr;         // flavour SEG: everything lives in the segmentation host object
    std::vector<LpInstance> inst;
    bool planned = false, finalized = false, inited = false;   // layout planned on the host (plan) / batch on the device (upload) / lpbox_init done
    LpLayoutOptions opt;              // the LPBOX_LP_* knobs, read when the layout is planned
    LpGeometry geo;
    bool identity_rows = true;   // row storage index == row id (bank-aware placement off)
    bool direct = false;          // opt-in direct x-update (lpbox_set_x_update)
    int order = LPBOX_ORDER_DEFAULT;   // opt-in reference summation order (lpbox_set_order): own kernels, identity layout
    bool valued = false, vals_in_lds = false;   // reference order only: some instance stores a value other than 1.0
    DevBuf<double> vr, vc, r4v;        // ... then the values in CSR / CSC entry order and the entries of rho4_E_transpose, ZS per instance
    int HL = 0, HLD = 0;
    size_t lds = 0, lds_direct = 0;
    bool log_on = false; int log_rows = 0; DevBuf<double> logbuf; int log_cap = 0;   // lpbox_set_log: records of the last plain call
    hipStream_t stream = nullptr;
    StreamTimer timer;
    double kernel_ms = 0.0;
    long long launches = 0;
    DevBuf<int> rs_ptr, cs_ptr, hs_ptr, isc, ctl, left_idx, xi_rows;
    DevBuf<uint16_t> rs_col, cs_row, rid, rmeta, rgl, cmeta;
    DevBuf<int16_t> rdir;
    DevBuf<int> dng;
    DevBuf<double> x, z1, z2, b, pd, z4, f, f_org, dsc, hist, dctl, c1_init, xhist, xi_out, Hinv;
    DevBuf<uint8_t> live, newfix, live_init;
    DevBuf<unsigned long long> stamps;
    int ws_cap = 0;        // columns of the current xhist staging buffer
    int last_ws = 0;       // window length of the last l2f call
    bool xi_valid = false;
    bool record = false;   // plain loop keeps x of every iteration (lpbox_set_record; print_fix_info 2/3)
    long xi_out_stride = 0;
    int xi_out_ws = 0;
    // row table of the last l2f window for a policy on the device (lpbox_get_x_iters_rows_device) and what the device decided from its scores
    DevBuf<long long> row_off;
    DevBuf<int> first_row, fix_counts;
    DevBuf<uint8_t> fix_codes;
    std::vector<int> h_first_row;     // B + 1: stacked rows of instance i are h_first_row[i] .. h_first_row[i + 1] - 1
    bool rows_valid = false;          // built since the last window
    bool rows_mask_changed = false;   // lpbox_set_active changed the mask after it was built
    int rows_ws = 0;
    std::vector<int> h_isc;   // host mirror, refreshed after every solver call
    std::vector<double> h_dsc;

    LpBatchDev dev() const {
        LpBatchDev d;
        d.B = B; d.NS = geo.NS; d.LS = geo.LS; d.ZS = geo.ZS;
        d.rs_ptr = rs_ptr.p; d.rs_col = rs_col.p; d.cs_ptr = cs_ptr.p; d.cs_row = cs_row.p; d.hs_ptr = hs_ptr.p; d.cmeta = cmeta.p; d.rid = rid.p; d.rmeta = rmeta.p; d.rgl = rgl.p;
        d.x = x.p; d.z1 = z1.p; d.z2 = z2.p; d.b = b.p; d.pd = pd.p; d.live = live.p; d.newfix = newfix.p;
        d.z4 = z4.p; d.f = f.p; d.dsc = dsc.p; d.isc = isc.p; d.hist = hist.p;
        d.ctl = ctl.p; d.dctl = dctl.p; d.xhist = xhist.p; d.ws_cap = ws_cap; d.logbuf = nullptr; d.log_cap = 0; d.stamps = stamps.p; d.stamp_wave = getenv("LPBOX_STAMP_WAVE") ? atoi(getenv("LPBOX_STAMP_WAVE")) : 0;
        d.pcg_generic = opt.pcg_generic ? 1 : 0;
        d.H = direct ? Hinv.p : nullptr; d.HL = direct ? HL : 0; d.HLD = direct ? HLD : 0; d.rdir = rdir.p; d.dng = dng.p;
        return d;
    }
    LpRefVals ref_vals() const {
        LpRefVals v;
        v.vr = valued ? vr.p : nullptr; v.vc = valued ? vc.p : nullptr; v.r4v = valued ? r4v.p : nullptr; v.in_lds = vals_in_lds ? 1 : 0;
        return v;
    }
};

namespace {

bool valid_handle(lpbox_t *h) { return h != nullptr && h->B > 0; }

int check_idx(lpbox_t *h, int idx) {
    if (!valid_handle(h)) return lpbox_fail(LPBOX_E_BADHANDLE, "bad handle");
    if (idx < 0 || idx >= h->B) return lpbox_fail(LPBOX_E_BADARG, "instance index %d out of range [0,%d)", idx, h->B);
    return LPBOX_OK;
}

int refresh_scalars(lpbox_t *h) {
    h->h_isc.resize((size_t)h->B * NI_COUNT);
    h->h_dsc.resize((size_t)h->B * ND_COUNT);
    HIPCHK(hipMemcpyAsync(h->h_isc.data(), h->isc.p, h->h_isc.size() * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(h->h_dsc.data(), h->dsc.p, h->h_dsc.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return LPBOX_OK;
}

LpProblemView view_of(const LpInstance &I) {
    LpProblemView P;
    P.n = I.n; P.l = I.l; P.nnz = I.nnz;
    P.colptr = I.colptr.data(); P.rowidx = I.rowidx.data(); P.rowptr = I.rowptr.data(); P.colidx = I.colidx.data();
    return P;
}

// LDS footprint of the chosen geometry (the kernel files know it) and, for a valued batch, where the stored values live.
int size_lds(lpbox_t *h, int big) {
    const LpGeometry &g = h->geo;
    const bool ref = h->order == LPBOX_ORDER_REFERENCE;
    h->lds = ref ? lp_ref_lds_bytes(g.NS, g.LS, g.ZS) : lp_window_lds_bytes(g.T, g.NS, g.LS, g.ZS);
    if (ref && !lp_ref_supported(g.T, g.EPT))
        return lpbox_fail(LPBOX_E_TOOLARGE, "reference order: instance with max(n,l)=%d exceeds the on-chip kernel (%d threads x %d slots)", big, g.T, g.EPT);
    h->vals_in_lds = false;
    if (h->valued) {
        // the values (CSR order, CSC order) and rho4_E_transpose sit in LDS where they fit next to the index sets, else in global memory;
        // LPBOX_LP_REF_VALS=global / =lds overrides (tuning and tests only; lds fails below when it does not fit)
        const size_t with_vals = lp_ref_lds_bytes(g.NS, g.LS, g.ZS, true);
        h->vals_in_lds = h->opt.ref_vals >= 0 ? h->opt.ref_vals == 1 : with_vals <= 160 * 1024;
        if (h->vals_in_lds) h->lds = with_vals;
    }
    if (h->lds > 160 * 1024) return lpbox_fail(LPBOX_E_TOOLARGE, "instance needs %zu B of LDS (> 160 KiB per CU)", h->lds);
    return LPBOX_OK;
}

// Everything a launch is shaped by, decided on the host alone: the options, the workgroup geometry, the LDS size and the layout of
// every instance (lpbox_lp_layout.h).  No HIP call: the layout getters answer on a machine without a device.
int plan(lpbox_t *h) {
    if (h->planned) return LPBOX_OK;
    for (int i = 0; i < h->B; i++)
        if (!h->inst[i].set) return lpbox_fail(LPBOX_E_STATE, "instance %d has no problem (call read_File / set_problem first)", i);
    int nmax = 0, lmax = 0, zmax = 0;
    for (auto &I : h->inst) { nmax = std::max(nmax, I.n); lmax = std::max(lmax, I.l); zmax = std::max(zmax, I.nnz); }
    const bool ref = h->order == LPBOX_ORDER_REFERENCE;
    h->opt = lp_layout_options_from_env();
    std::string why;
    int rc = lp_choose_geometry(nmax, lmax, zmax, ref, h->opt, &h->geo, &why);
    if (rc) return lpbox_fail(rc, "%s", why.c_str());
    h->valued = false;
    for (auto &I : h->inst) h->valued = h->valued || !I.vals.empty();
    if (h->valued && !ref) return lpbox_fail(LPBOX_E_UNSUPPORTED, "E has stored values != 1; only the reference order carries them (lpbox_set_order)");
    rc = size_lds(h, std::max(nmax, lmax));
    if (rc) return rc;
    int caps[3];
    lp_pcg_list_caps(&caps[0], &caps[1], &caps[2]);
    h->identity_rows = true;
    for (auto &I : h->inst) {
        if (ref) lp_plan_identity_layout(view_of(I), h->geo, &I.lay);
        else lp_plan_layout(view_of(I), h->geo, h->opt, caps, &I.lay);
        h->identity_rows = h->identity_rows && I.lay.identity_rows;
    }
    h->planned = true;
    return LPBOX_OK;
}

// One table of every instance's layout -> one pool of the batch at a common stride (`fill` where an instance's table is shorter).
template <typename Tp>
std::vector<Tp> pooled(const lpbox_t *h, std::vector<Tp> LpInstanceLayout::*table, size_t stride, Tp fill) {
    std::vector<Tp> pool((size_t)h->B * stride, fill);
    for (int i = 0; i < h->B; i++) {
        const std::vector<Tp> &v = h->inst[i].lay.*table;
        std::copy(v.begin(), v.end(), pool.begin() + (size_t)i * stride);
    }
    return pool;
}

// Create the stream, allocate the batch and copy the planned layout and the problem data to the device.
int upload(lpbox_t *h) {
    if (h->finalized) return LPBOX_OK;
    int rc = use_device(h->device);
    if (rc) return rc;
    if (!h->stream) HIPCHK(hipStreamCreate(&h->stream));
    HIPCHK(h->timer.create());
    const size_t B = h->B, NS = h->geo.NS, LS = h->geo.LS, ZS = h->geo.ZS;
    HIPCHK(h->x.alloc(B * NS)); HIPCHK(h->z1.alloc(B * NS)); HIPCHK(h->z2.alloc(B * NS)); HIPCHK(h->pd.alloc(B * NS));
    HIPCHK(h->live.alloc(B * NS)); HIPCHK(h->newfix.alloc(B * NS));
    HIPCHK(h->z4.alloc(B * LS)); HIPCHK(h->f.alloc(B * LS));
    HIPCHK(h->dsc.alloc(B * ND_COUNT)); HIPCHK(h->hist.alloc(B * LP_HIST));
    HIPCHK(h->ctl.alloc(B * 4)); HIPCHK(h->dctl.alloc(B));
    HIPCHK(h->left_idx.alloc(B * NS)); HIPCHK(h->xi_rows.alloc(B));
#ifdef LPBOX_STAMPS
    HIPCHK(h->stamps.alloc(B * 16)); HIPCHK(hipMemset(h->stamps.p, 0, B * 16 * sizeof(unsigned long long)));
#endif
    HIPCHK(h->rs_ptr.upload(pooled(h, &LpInstanceLayout::rs_ptr, NS + 1, 0)));
    HIPCHK(h->cs_ptr.upload(pooled(h, &LpInstanceLayout::cs_ptr, NS + 1, 0)));
    HIPCHK(h->hs_ptr.upload(pooled(h, &LpInstanceLayout::hs_ptr, NS + 1, 0)));
    HIPCHK(h->rs_col.upload(pooled(h, &LpInstanceLayout::rs_col, ZS, (uint16_t)0)));
    HIPCHK(h->cs_row.upload(pooled(h, &LpInstanceLayout::cs_row, ZS, (uint16_t)0)));
    HIPCHK(h->rid.upload(pooled(h, &LpInstanceLayout::rid, NS, (uint16_t)0xFFFF)));
    HIPCHK(h->rgl.upload(pooled(h, &LpInstanceLayout::rgl, NS, (uint16_t)0)));
    HIPCHK(h->rmeta.upload(pooled(h, &LpInstanceLayout::rmeta, NS, (uint16_t)0x10)));
    HIPCHK(h->cmeta.upload(pooled(h, &LpInstanceLayout::cmeta, NS, (uint16_t)0)));
    // the problem data: b and the live mask by storage position, f by row id
    std::vector<int> h_isc(B * NI_COUNT, 0);
    std::vector<uint8_t> h_live(B * NS, 0);
    std::vector<double> h_b(B * NS, 0.0), h_f(B * LS, 0.0), h_c1(B, 0.0), h_vr, h_vc;
    if (h->valued) { h_vr.assign(B * ZS, 0.0); h_vc.assign(B * ZS, 0.0); }
    for (size_t i = 0; i < B; i++) {
        const LpInstance &I = h->inst[i];
        for (int j = 0; j < I.n; j++) { h_b[i * NS + I.lay.cpos[j]] = I.b[j]; h_live[i * NS + I.lay.cpos[j]] = 1; }
        for (int r = 0; r < I.l; r++) h_f[i * LS + r] = I.f_org[r];
        for (int k = 0; k < I.nnz && h->valued; k++) {
            h_vr[i * ZS + k] = I.vals.empty() ? 1.0 : I.vals_csr[k];
            h_vc[i * ZS + k] = I.vals.empty() ? 1.0 : I.vals[k];
        }
        h_isc[i * NI_COUNT + NI_N] = I.n; h_isc[i * NI_COUNT + NI_L] = I.l; h_isc[i * NI_COUNT + NI_NNZ] = I.nnz;
        h_isc[i * NI_COUNT + NI_ACTIVE] = 1;
        h_c1[i] = std::pow((double)I.n, 1.0 / 2);     // std::pow(n, 1.0/p), p = projection_lp = 2 (LPcpp:427,503)
    }
    HIPCHK(h->b.upload(h_b)); HIPCHK(h->live_init.upload(h_live)); HIPCHK(h->f_org.upload(h_f));
    HIPCHK(h->isc.upload(h_isc)); HIPCHK(h->c1_init.upload(h_c1));
    if (h->valued) {
        HIPCHK(h->vr.upload(h_vr)); HIPCHK(h->vc.upload(h_vc));
        HIPCHK(h->r4v.alloc(B * ZS)); HIPCHK(hipMemset(h->r4v.p, 0, B * ZS * sizeof(double)));
    }
    HIPCHK(hipMemset(h->ctl.p, 0, B * 4 * sizeof(int)));
    HIPCHK(hipMemset(h->dctl.p, 0, B * sizeof(double)));
    HIPCHK(hipMemset(h->newfix.p, 0, B * NS));
    h->finalized = true;
    return LPBOX_OK;
}

int plan_and_upload(lpbox_t *h) {
    int rc = plan(h);
    return rc ? rc : upload(h);
}

int run_window(lpbox_t *h, int iter_start, int iter_end, int l2f, bool log = false) {
    HIPCHK(h->timer.start(h->stream));
    LpBatchDev bd = h->dev();
    if (log) { bd.logbuf = h->logbuf.p; bd.log_cap = h->log_cap; }
    if (h->order == LPBOX_ORDER_REFERENCE) HIPCHK(lp_ref_launch_window(bd, h->ref_vals(), h->geo.EPT, h->lds, iter_start, iter_end, l2f, h->stream));
    else HIPCHK(lp_launch_window(bd, h->geo.T, h->geo.EPT, h->direct ? h->lds_direct : h->lds, iter_start, iter_end, l2f, h->stream, h->direct, log));
    HIPCHK(h->timer.stop(h->stream));
    int rc = refresh_scalars(h);     // synchronises the stream
    if (rc) return rc;
    double ms = 0.0;
    HIPCHK(h->timer.read(&ms));
    h->kernel_ms += ms;
    h->launches++;
    return LPBOX_OK;
}

int set_instance(lpbox_t *h, int idx, int n, int l, int nnz, const int *colptr, const int *rowidx, const double *vals,
                 const double *b, const double *f) {
    if (h->planned) return lpbox_fail(LPBOX_E_STATE, "layout already planned (lpbox_init or a layout getter was called); create a new handle to change the problem");
    if (n <= 0 || l <= 0 || nnz < 0 || !colptr || (!rowidx && nnz) || !b) return lpbox_fail(LPBOX_E_BADARG, "bad problem arguments");
    if (n == l) return lpbox_fail(LPBOX_E_UNSUPPORTED, "n == l: the reference's aliased sparse product is ill-defined here (LPcpp:103-107,150)");
    if (colptr[0] != 0 || colptr[n] != nnz) return lpbox_fail(LPBOX_E_BADARG, "colptr does not span nnz");
    // validate everything BEFORE touching the instance (a rejected call leaves it as it was) and before reading rowidx / vals through colptr
    bool valued = false;
    for (int j = 0; j < n; j++) {
        if (colptr[j] < 0 || colptr[j + 1] < colptr[j] || colptr[j + 1] > nnz) return lpbox_fail(LPBOX_E_BADARG, "colptr not monotone inside [0, nnz]");
        for (int k = colptr[j]; k < colptr[j + 1]; k++) {
            if (rowidx[k] < 0 || rowidx[k] >= l) return lpbox_fail(LPBOX_E_BADARG, "row index out of range");
            if (k > colptr[j] && rowidx[k] <= rowidx[k - 1]) return lpbox_fail(LPBOX_E_BADARG, "row indices must ascend inside a column");
            if (vals && !std::isfinite(vals[k])) return lpbox_fail(LPBOX_E_BADARG, "E has a non-finite stored value (column %d, row %d)", j, rowidx[k]);
            if (vals && vals[k] != 1.0) {
                if (h->order != LPBOX_ORDER_REFERENCE)
                    return lpbox_fail(LPBOX_E_UNSUPPORTED, "E has a stored value %g != 1; the default-order LP kernels hold E implicitly as a 0/1 pattern "
                                "(call lpbox_set_order(LPBOX_ORDER_REFERENCE) first: the reference-order kernels carry stored values)", vals[k]);
                valued = true;
            }
        }
    }
    // the objective vector: a NaN in b would run every x-update to the PCG cap for up to 2e4 outer iterations (the reference accepts it
    // and computes garbage; a deliberate deviation).  Subnormals, zeros and either sign are ordinary values.
    for (int j = 0; j < n; j++)
        if (!std::isfinite(b[j])) return lpbox_fail(LPBOX_E_BADARG, "b has a non-finite entry (index %d)", j);
    LpInstance &I = h->inst[idx];
    I.n = n; I.l = l; I.nnz = nnz;
    I.dir_g.clear();                  // lpbox_get_direct_rows may have answered for the problem that was here
    if (valued) I.vals.assign(vals, vals + nnz); else I.vals.clear();     // all ones = a unit instance
    I.vals_csr.assign(valued ? nnz : 0, 0.0);
    I.colptr.assign(colptr, colptr + n + 1);
    I.rowidx.assign(rowidx, rowidx + nnz);
    // CSR of E: rows in ascending column order (the order Eigen's column-major product accumulates a row in)
    I.rowptr.assign(l + 1, 0);
    for (int k = 0; k < nnz; k++) I.rowptr[rowidx[k] + 1]++;
    for (int r = 0; r < l; r++) I.rowptr[r + 1] += I.rowptr[r];
    I.colidx.assign(nnz, 0);
    std::vector<int> cur(I.rowptr.begin(), I.rowptr.end() - 1);
    for (int j = 0; j < n; j++)
        for (int k = colptr[j]; k < colptr[j + 1]; k++) {
            const int at = cur[rowidx[k]]++;
            I.colidx[at] = j;
            if (valued) I.vals_csr[at] = vals[k];
        }
    I.b.assign(b, b + n);
    if (f) I.f_org.assign(f, f + l); else I.f_org.assign(l, 1.0);
    I.left_idx.resize(n);
    for (int j = 0; j < n; j++) I.left_idx[j] = j;
    I.set = true;
    return LPBOX_OK;
}

// n-vectors come back in ORIGINAL variable order (by_var = true undoes the storage permutation); l-vectors are stored by row id
int fetch_vec(lpbox_t *h, const double *pool, size_t stride, int idx, int len, std::vector<double> &out, bool by_var = true) {
    out.resize(len);
    if (len == 0) return LPBOX_OK;
    const size_t cnt = by_var ? (size_t)h->geo.NS : (size_t)len;      // n-vectors are stored by position (NS slots incl. holes)
    std::vector<double> tmp(cnt);
    HIPCHK(hipMemcpy(tmp.data(), pool + (size_t)idx * stride, sizeof(double) * cnt, hipMemcpyDeviceToHost));
    const LpInstance &I = h->inst[idx];
    if (by_var) for (int j = 0; j < len; j++) out[j] = tmp[I.lay.cpos[j]];
    else out.swap(tmp);
    return LPBOX_OK;
}

int fetch_live(lpbox_t *h, int idx, std::vector<uint8_t> &out) {
    const LpInstance &I = h->inst[idx];
    std::vector<uint8_t> tmp(h->geo.NS);
    out.resize(I.n);
    HIPCHK(hipMemcpy(tmp.data(), h->live.p + (size_t)idx * h->geo.NS, tmp.size(), hipMemcpyDeviceToHost));
    for (int j = 0; j < I.n; j++) out[j] = tmp[I.lay.cpos[j]];
    return LPBOX_OK;
}

}  // namespace

// =================================================================================================
extern "C" {

const char *lpbox_version(void) { return "lpbox_hip 0.1 (gfx950)"; }
const char *lpbox_last_error(void) { return g_err.c_str(); }
int lpbox_last_status(void) { return g_status; }

int lpbox_device_count(void) {
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess) return 0;
    return cnt;
}

int lpbox_set_device(int device) {
    int cnt = lpbox_device_count();
    if (device < 0 || device >= cnt) return lpbox_fail(LPBOX_E_NODEVICE, "device %d not available (%d visible)", device, cnt);
    g_device = device;
    return LPBOX_OK;
}

lpbox_t *lpbox_create(int flavour, int batch, int print_info) {
    if (batch <= 0 || (flavour != LPBOX_FLAVOUR_LP && flavour != LPBOX_FLAVOUR_SEG) || (flavour == LPBOX_FLAVOUR_SEG && batch != 1)) {
        lpbox_fail(LPBOX_E_BADARG, "lpbox_create: unsupported flavour %d or batch %d", flavour, batch);
        return nullptr;
    }
    lpbox_t *h = new lpbox_solver();
    h->flavour = flavour; h->B = batch; h->print_info = print_info; h->device = g_device;
    if (flavour == LPBOX_FLAVOUR_SEG) h->seg = segc_create(print_info, g_device);
    else h->inst.resize(batch);
    return h;
}

void lpbox_destroy(lpbox_t *h) {
    if (!h) return;
    if (h->seg) { segc_destroy(h->seg); delete h; return; }
    if (h->finalized) (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    h->timer.destroy();
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

int lpbox_set_problem_lp(lpbox_t *h, int idx, int n, int l, int nnz, const int *colptr, const int *rowidx,
                         const double *vals, const double *b, const double *f) {
    if (valid_handle(h) && h->seg) return lpbox_fail(LPBOX_E_STATE, "this entry point belongs to the LP flavour");
    int rc = check_idx(h, idx);
    if (rc) return rc;
    return set_instance(h, idx, n, l, nnz, colptr, rowidx, vals, b, f);
}

// readSparseMat LPcpp:2416-2444, readDenseVec :2407-2414, readFile :2446-2545
int lpbox_read_files_lp(lpbox_t *h, int idx, const char *path_C, const char *path_b, int k) {
    if (valid_handle(h) && h->seg) return lpbox_fail(LPBOX_E_STATE, "this entry point belongs to the LP flavour");
    int rc = check_idx(h, idx);
    if (rc) return rc;
    if (!path_C || !path_b) return lpbox_fail(LPBOX_E_BADARG, "null path");
    FILE *fc = fopen(path_C, "r");
    if (!fc) return lpbox_fail(LPBOX_E_IO, "cannot open %s", path_C);
    struct Trip { int r, c; double v; };
    std::vector<Trip> t;
    int row, col, max_row = 0, max_col = 0;
    double val;
    while (fscanf(fc, "%d,%d,%lf\n", &row, &col, &val) == 3) {
        if (row < 1 || col < 1) { fclose(fc); return lpbox_fail(LPBOX_E_IO, "%s: indices are 1-based", path_C); }
        max_row = std::max(max_row, row); max_col = std::max(max_col, col);
        t.push_back({row - 1, col - 1, k == 2 ? -1.0 * val : val});      // :2436-2439
    }
    fclose(fc);
    if (t.empty()) return lpbox_fail(LPBOX_E_IO, "%s: no 'row,col,val' triplets", path_C);
    // setFromTriplets (:2441-2443): column-major, sorted rows, duplicates summed
    std::vector<int> colptr(max_col + 1, 0);
    for (auto &e : t) colptr[e.c + 1]++;
    for (int j = 0; j < max_col; j++) colptr[j + 1] += colptr[j];
    std::vector<Trip> s(t.size());
    {
        std::vector<int> pos(colptr.begin(), colptr.end() - 1);
        for (auto &e : t) s[pos[e.c]++] = e;
    }
    std::vector<int> rowidx; std::vector<double> vals; std::vector<int> cp(max_col + 1, 0);
    for (int j = 0; j < max_col; j++) {
        std::stable_sort(s.begin() + colptr[j], s.begin() + colptr[j + 1], [](const Trip &a, const Trip &b2) { return a.r < b2.r; });
        for (int q = colptr[j]; q < colptr[j + 1]; q++) {
            if (q > colptr[j] && s[q].r == s[q - 1].r) vals.back() += s[q].v;
            else { rowidx.push_back(s[q].r); vals.push_back(s[q].v); }
        }
        cp[j + 1] = (int)rowidx.size();
    }
    FILE *fb = fopen(path_b, "r");
    if (!fb) return lpbox_fail(LPBOX_E_IO, "cannot open %s", path_b);
    std::vector<double> b(max_col);
    for (int i = 0; i < max_col; i++) {
        if (fscanf(fb, "%lf\n", &b[i]) != 1) { fclose(fb); return lpbox_fail(LPBOX_E_IO, "error when reading dense vector %s (entry %d)", path_b, i); }
        b[i] = -1.0 * b[i];                                                // :2520
    }
    fclose(fb);
    std::vector<double> f(max_row, 1.0);                                   // :2522
    return set_instance(h, idx, max_col, max_row, (int)rowidx.size(), cp.data(), rowidx.data(), vals.data(), b.data(), f.data());
}

int lpbox_read_file(lpbox_t *h, int idx, const char *root, int i, int k, int j) {
    std::string r = root ? root : "../cython_solver/data";                 // :2451
    char pc[1024], pb[1024];
    snprintf(pc, sizeof(pc), "%s/instance/%d_%d/instance_%d_C.txt", r.c_str(), k, j, i);   // :2492
    snprintf(pb, sizeof(pb), "%s/instance/%d_%d/instance_%d_b.txt", r.c_str(), k, j, i);   // :2494
    return lpbox_read_files_lp(h, idx, pc, pb, k);
}

int lpbox_init(lpbox_t *h) {
    if (valid_handle(h) && h->seg) return segc_init(h->seg);
    if (!valid_handle(h)) return lpbox_fail(LPBOX_E_BADHANDLE, "bad handle");
    int rc = plan_and_upload(h);
    if (rc) return rc;
    rc = use_device(h->device);
    if (rc) return rc;
    for (auto &I : h->inst) {
        I.left_idx.resize(I.n);
        for (int j = 0; j < I.n; j++) I.left_idx[j] = j;
        I.xi_rows = 0; I.xi_left_idx.clear();
    }
    h->xi_valid = false;
    h->rows_valid = false;
    HIPCHK(hipMemsetAsync(h->ctl.p, 0, (size_t)h->B * 4 * sizeof(int), h->stream));
    if (h->order == LPBOX_ORDER_REFERENCE) HIPCHK(lp_ref_launch_init(h->dev(), h->ref_vals(), h->lds, h->f_org.p, h->c1_init.p, h->live_init.p, h->stream));
    else HIPCHK(lp_launch_init(h->dev(), h->geo.T, h->geo.EPT, h->f_org.p, h->c1_init.p, h->live_init.p, h->stream));
    rc = refresh_scalars(h);
    if (rc) return rc;
    h->inited = true;
    return 1;                                                              // LPcpp:762
}

// Upload the per-window control words and clear the x_iters staging buffer (ws columns of NS doubles per instance).
static int stage_xiters(lpbox_t *h, int ws, const std::vector<int> &h_ctl, const std::vector<double> &h_dctl,
                        const std::vector<uint8_t> *h_newfix, const std::vector<int> &h_left, const std::vector<int> &h_rows) {
    const size_t B = h->B, NS = h->geo.NS;
    if ((double)B * ws * NS * sizeof(double) > 64e9)
        return lpbox_fail(LPBOX_E_BADARG, "x history of %d iterations x %zu instances would need %.1f GB", ws, B, (double)B * ws * NS * 8 / 1e9);
    if (ws > 0 && (h->ws_cap < ws || !h->xhist.p)) {
        HIPCHK(hipStreamSynchronize(h->stream));
        HIPCHK(h->xhist.alloc(B * (size_t)ws * NS));
        h->ws_cap = ws;
    }
    HIPCHK(hipMemcpyAsync(h->ctl.p, h_ctl.data(), h_ctl.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->dctl.p, h_dctl.data(), h_dctl.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (h_newfix) HIPCHK(hipMemcpyAsync(h->newfix.p, h_newfix->data(), h_newfix->size(), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->left_idx.p, h_left.data(), h_left.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->xi_rows.p, h_rows.data(), h_rows.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    if (ws > 0) HIPCHK(hipMemsetAsync(h->xhist.p, 0, B * (size_t)h->ws_cap * NS * sizeof(double), h->stream));   // x_iters starts as zeros
    return LPBOX_OK;
}

}  // extern "C"

namespace {

// The part of an l2f window the two entry points share (LPcpp:1124-1206 index bookkeeping, then the launch): instance i fixes num[i] of
// its live variables, code_of(i, q) is the code of the q-th one (2 = fix to 1, 1 = fix to 0, 0 = stays live).  host_newfix: the codes go
// to the device from here (the vec form); false = the decide kernel has already written them (the scores form).
template <typename CodeOf>
int l2f_window(lpbox_t *h, int iter_start, int iter_end, const std::vector<int> &num, bool host_newfix, CodeOf code_of, int *rets) {
    const int ws = iter_end - iter_start;
    const size_t B = h->B, NS = h->geo.NS;
    std::vector<int> h_ctl(B * 4, 0);
    std::vector<double> h_dctl(B, 0.0);
    std::vector<uint8_t> h_newfix;
    if (host_newfix) h_newfix.assign(B * NS, 0);
    std::vector<int> h_rows(B, 0);
    std::vector<int> h_left(B * NS, 0);
    for (size_t i = 0; i < B; i++) {
        LpInstance &I = h->inst[i];
        const int n_live = (int)I.left_idx.size();
        if (num[i] != 0) {                                                  // LPcpp:1124-1206 index bookkeeping
            std::vector<int> keep;
            keep.reserve(n_live - num[i]);
            for (int q = 0; q < n_live; q++) {
                const int org = I.left_idx[q];
                const int code = code_of(i, q);
                if (code == 0) keep.push_back(org);
                else if (host_newfix) h_newfix[i * NS + I.lay.cpos[org]] = (uint8_t)code;
            }
            I.left_idx.swap(keep);
            h_ctl[i * 4 + 0] = 1; h_ctl[i * 4 + 1] = num[i]; h_ctl[i * 4 + 2] = n_live - num[i];
            h_dctl[i] = std::pow((double)(n_live - num[i]), 1.0 / 2);      // LPcpp:427 with the shrunken n
        }
        I.xi_rows = n_live - num[i];                                        // x_iters = Zero(n - fix_num, 500), :1113
        I.xi_left_idx = I.left_idx;
        h_rows[i] = I.xi_rows;
        for (int q = 0; q < I.xi_rows; q++) h_left[i * NS + q] = I.lay.cpos[I.left_idx[q]];   // storage position of the q-th live variable
    }
    h->rows_valid = false;
    int rc = stage_xiters(h, ws, h_ctl, h_dctl, host_newfix ? &h_newfix : nullptr, h_left, h_rows);
    if (rc) return rc;
    rc = run_window(h, iter_start, iter_end, 3);    // synchronises: the host staging vectors above stay alive until here
    if (rc) return rc;
    h->last_ws = ws;
    h->xi_valid = true;
    h->xi_out_ws = 0;
    for (size_t i = 0; i < B; i++) {
        if (rets) rets[i] = h->h_isc[i * NI_COUNT + NI_RET];
    }
    return h->h_isc[NI_RET];
}

// Pack the iterate windows of the whole batch at `ws` columns unless the last pack already did (once per (call, ws)).
int pack_xiters(lpbox_t *h, int ws) {
    if (h->xi_out_ws == ws) return LPBOX_OK;
    const long stride = (long)h->geo.NS * ws;
    if (h->xi_out.count < (size_t)h->B * stride) HIPCHK(h->xi_out.alloc((size_t)h->B * stride));
    HIPCHK(lp_launch_pack_xiters(h->dev(), h->left_idx.p, h->xi_rows.p, ws, h->xi_out.p, stride, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->xi_out_ws = ws; h->xi_out_stride = stride;
    return LPBOX_OK;
}

}  // namespace

extern "C" {

int lpbox_iterate(lpbox_t *h, int iter_start, int iter_end, int *rets) {
    if (valid_handle(h) && h->seg) return lpbox_fail(LPBOX_E_STATE, "this entry point belongs to the LP flavour");
    if (!valid_handle(h)) return lpbox_fail(LPBOX_E_BADHANDLE, "bad handle");
    if (!h->inited) return lpbox_fail(LPBOX_E_STATE, "solve_init has not been called");
    int rc = use_device(h->device);
    if (rc) return rc;
    const bool rec = h->record && iter_end > iter_start;
    h->rows_valid = false;
    if (rec) {                         // print_fix_info 2/3 (LPcpp:776-779,903-909): keep x of every iteration of this call
        const size_t B = h->B, NS = h->geo.NS;
        std::vector<int> h_ctl(B * 4, 0), h_rows(B, 0), h_left(B * NS, 0);
        std::vector<double> h_dctl(B, 0.0);
        for (size_t i = 0; i < B; i++) {
            LpInstance &I = h->inst[i];
            I.xi_rows = (int)I.left_idx.size();
            I.xi_left_idx = I.left_idx;
            h_rows[i] = I.xi_rows;
            for (int q = 0; q < I.xi_rows; q++) h_left[i * NS + q] = I.lay.cpos[I.left_idx[q]];
        }
        rc = stage_xiters(h, iter_end - iter_start, h_ctl, h_dctl, nullptr, h_left, h_rows);
        if (rc) return rc;
    } else {
        HIPCHK(hipMemsetAsync(h->ctl.p, 0, (size_t)h->B * 4 * sizeof(int), h->stream));
    }
    const bool log = h->log_on && iter_end > iter_start;
    if (log) {                         // does_log (LPcpp:1013-1067): the values of the reference's per-iteration text log, one record per iteration
        if (h->direct || !lp_log_supported(h->geo.T, h->geo.EPT)) return lpbox_fail(LPBOX_E_UNSUPPORTED, "the iteration log is built for the default PCG kernels (512 threads per instance)");
        const size_t need = (size_t)h->B * (size_t)(iter_end - iter_start) * LP_LOG_VALS;
        if (need * sizeof(double) > (size_t)1 << 30) return lpbox_fail(LPBOX_E_UNSUPPORTED, "the iteration log of this call would exceed 1 GiB");
        if (h->logbuf.count < need) HIPCHK(h->logbuf.alloc(need));
        h->log_cap = iter_end - iter_start;
        HIPCHK(hipMemsetAsync(h->logbuf.p, 0xFF, need * sizeof(double), h->stream));      // NaN = iteration not logged (it broke off, or was never reached)
    }
    rc = run_window(h, iter_start, iter_end, rec ? 2 : 0, log);
    if (rc) return rc;
    h->log_rows = log ? iter_end - iter_start : 0;
    if (rec) { h->last_ws = iter_end - iter_start; h->xi_valid = true; h->xi_out_ws = 0; }
    for (int i = 0; i < h->B; i++)
        if (rets) rets[i] = h->h_isc[(size_t)i * NI_COUNT + NI_RET];
    return h->h_isc[NI_RET];
}

int lpbox_iterate_l2f(lpbox_t *h, int iter_start, int iter_end, const double *vec, long vec_stride, const int *nums,
                      int *rets) {
    if (valid_handle(h) && h->seg) {
        int ret = 0;
        if (nums && nums[0] != 0 && vec_stride < segc_get_n(h->seg))
            return lpbox_fail(LPBOX_E_BADARG, "fix vector holds %ld entries, %d live variables", vec_stride, segc_get_n(h->seg));
        int rc = segc_l2f(h->seg, iter_start, iter_end, vec, nums ? nums[0] : 0, &ret);
        if (rc < 0) return rc;
        if (rets) rets[0] = ret;
        return ret;
    }
    if (!valid_handle(h)) return lpbox_fail(LPBOX_E_BADHANDLE, "bad handle");
    if (!h->inited) return lpbox_fail(LPBOX_E_STATE, "solve_init has not been called");
    const int ws = iter_end - iter_start;
    if (ws > LP_XITERS_COLS) return lpbox_fail(LPBOX_E_BADARG, "window of %d iterations exceeds the %d columns of x_iters (LPcpp:1113)", ws, LP_XITERS_COLS);
    int rc = use_device(h->device);
    if (rc) return rc;
    const size_t B = h->B;
    bool any_fix = false;
    // validate everything before touching any state
    for (size_t i = 0; i < B; i++) {
        const LpInstance &I = h->inst[i];
        const int n_live = (int)I.left_idx.size();
        const int num = nums ? nums[i] : 0;
        if (num != 0 && !h->h_isc[i * NI_COUNT + NI_ACTIVE]) return lpbox_fail(LPBOX_E_BADARG, "instance %zu is parked (lpbox_set_active) but has a fix request", i);
        if (num < 0 || num > n_live) return lpbox_fail(LPBOX_E_BADARG, "instance %zu: fix count %d outside [0,%d]", i, num, n_live);
        if (num != 0) {
            if (!vec) return lpbox_fail(LPBOX_E_BADARG, "fix vector missing");
            if (vec_stride < n_live) return lpbox_fail(LPBOX_E_BADARG, "instance %zu: fix vector holds %ld entries, %d live variables", i, vec_stride, n_live);
            const double *v = vec + (size_t)i * vec_stride;
            int cnt = 0;
            for (int q = 0; q < n_live; q++) if (v[q] == 1 || v[q] == 0) cnt++;
            if (cnt != num)                                                 // the reference would run out of bounds (LPcpp:1135-1149)
                return lpbox_fail(LPBOX_E_BADARG, "instance %zu: vec fixes %d variables but num = %d", i, cnt, num);
            any_fix = true;
        }
    }
    std::vector<int> k(B, 0);
    for (size_t i = 0; i < B; i++) k[i] = nums ? nums[i] : 0;
    // the code of the q-th live variable: 2 = fix to 1, 1 = fix to 0, 0 = stays live
    return l2f_window(h, iter_start, iter_end, k, any_fix, [&](size_t i, int q) {
        const double v = vec[i * (size_t)vec_stride + q];
        return v == 1 ? 2 : (v == 0 ? 1 : 0);
    }, rets);
}

int lpbox_set_x_update(lpbox_t *h, int mode) {
    if (valid_handle(h) && h->seg) return lpbox_fail(LPBOX_E_STATE, "this entry point belongs to the LP flavour");
    if (!valid_handle(h)) return lpbox_fail(LPBOX_E_BADHANDLE, "bad handle");
    if (mode != LPBOX_XUPDATE_PCG && mode != LPBOX_XUPDATE_DIRECT) return lpbox_fail(LPBOX_E_BADARG, "x-update mode %d", mode);
    if (mode == LPBOX_XUPDATE_PCG) { h->direct = false; return LPBOX_OK; }
    if (h->order == LPBOX_ORDER_REFERENCE) return lpbox_fail(LPBOX_E_UNSUPPORTED, "the direct x-update has no reference-order variant (lpbox_set_order)");
    int rc = plan_and_upload(h);       // the geometry decides whether the dense inverse fits
    if (rc) return rc;
    rc = use_device(h->device);
    if (rc) return rc;
    if (!lp_direct_supported(h->geo.T, h->geo.EPT))
        return lpbox_fail(LPBOX_E_UNSUPPORTED, "direct x-update needs n <= 512 (this batch: %d threads x %d slots)", h->geo.T, h->geo.EPT);
    if (!h->identity_rows) return lpbox_fail(LPBOX_E_UNSUPPORTED, "direct x-update needs the plain row placement (unset LPBOX_LP_BANKAWARE)");
    if (!h->Hinv.p) {
        // Rows with pairwise disjoint columns (D) are inverted in closed form, the rest (G) through a dense |G| x |G| inverse in LDS.
        const size_t B = h->B, NS = h->geo.NS;
        int gmax = 0;
        for (auto &I : h->inst) {
            I.nG = lp_plan_direct_rows(view_of(I), &I.dir_g);
            gmax = std::max(gmax, I.nG);
        }
        if (gmax > 128) return lpbox_fail(LPBOX_E_UNSUPPORTED, "direct x-update: %d rows of E share columns (at most 128 fit the on-chip inverse)", gmax);
        // pitch = 4 (mod 32) doubles: the quads of a half-wave (8 rows x 4 consecutive columns) fall on 64 distinct LDS banks
        h->HL = std::max(gmax, 1); h->HLD = ((h->HL + 27) / 32) * 32 + 4;
        h->lds_direct = lp_window_lds_bytes(h->geo.T, h->geo.NS, h->geo.LS, h->geo.ZS, h->HL, h->HLD);
        if (h->lds_direct > 160 * 1024)
            return lpbox_fail(LPBOX_E_UNSUPPORTED, "direct x-update needs %zu B of LDS (> 160 KiB per CU)", h->lds_direct);
        std::vector<int16_t> h_rdir(B * NS, -1);
        std::vector<int> h_ng(B, 0);
        for (size_t i = 0; i < B; i++) {
            const LpInstance &I = h->inst[i];
            h_ng[i] = I.nG;
            for (size_t p = 0; p < NS; p++) { const int r = I.lay.rid[p]; if (r != 0xFFFF && r < I.l) h_rdir[i * NS + p] = (int16_t)I.dir_g[r]; }
        }
        HIPCHK(h->rdir.alloc(B * NS)); HIPCHK(h->dng.alloc(B));
        HIPCHK(hipMemcpy(h->rdir.p, h_rdir.data(), h_rdir.size() * sizeof(int16_t), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(h->dng.p, h_ng.data(), h_ng.size() * sizeof(int), hipMemcpyHostToDevice));
        HIPCHK(h->Hinv.alloc(B * ((size_t)h->HL * h->HLD + h->geo.LS)));
    }
    // the saved inverses belong to whatever ran before: every instance rebuilds its own at its next x-update
    HIPCHK(hipMemset2DAsync(h->isc.p + NI_H_VALID, NI_COUNT * sizeof(int), 0, sizeof(int), (size_t)h->B, h->stream));
    h->direct = true;
    return LPBOX_OK;
}

int lpbox_set_record(lpbox_t *h, int on) {
    if (!valid_handle(h)) return lpbox_fail(LPBOX_E_BADHANDLE, "bad handle");
    if (h->seg) return segc_set_record(h->seg, on);
    h->record = on != 0;
    return LPBOX_OK;
}

// The values of the reference's per-iteration text log (does_log, LPh:148, LPcpp:1013-1067), opt-in: while on, every lpbox_iterate call
// leaves one record of LPBOX_LOG_VALS doubles per iteration it completed.
int lpbox_set_log(lpbox_t *h, int on) {
    if (!valid_handle(h)) return lpbox_fail(LPBOX_E_BADHANDLE, "bad handle");
    if (h->seg) return lpbox_fail(LPBOX_E_UNSUPPORTED, "the segmentation solver of the reference writes no iteration log (SEGh:225)");
    if (on && h->order == LPBOX_ORDER_REFERENCE) return lpbox_fail(LPBOX_E_UNSUPPORTED, "the iteration log has no reference-order variant (lpbox_set_order)");
    h->log_on = on != 0;
    if (!h->log_on) h->log_rows = 0;
    return LPBOX_OK;
}

// Summation order of the on-chip kernels.  The layout is built when the problem is uploaded, so the order is
// chosen before that.
int lpbox_set_order(lpbox_t *h, int mode) {
    if (valid_handle(h) && h->seg) return lpbox_fail(LPBOX_E_STATE, "this entry point belongs to the LP flavour");
    if (!valid_handle(h)) return lpbox_fail(LPBOX_E_BADHANDLE, "bad handle");
    if (mode != LPBOX_ORDER_DEFAULT && mode != LPBOX_ORDER_REFERENCE) return lpbox_fail(LPBOX_E_BADARG, "summation order %d", mode);
    if (mode == LPBOX_ORDER_DEFAULT)
        for (size_t i = 0; i < h->inst.size(); i++)
            if (!h->inst[i].vals.empty())
                return lpbox_fail(LPBOX_E_UNSUPPORTED, "instance %zu stores values != 1; only the reference order carries them", i);
    if (mode == LPBOX_ORDER_REFERENCE && h->direct) return lpbox_fail(LPBOX_E_UNSUPPORTED, "the direct x-update has no reference-order variant");
    if (mode == LPBOX_ORDER_REFERENCE && h->log_on) return lpbox_fail(LPBOX_E_UNSUPPORTED, "the iteration log has no reference-order variant");
    if (h->planned) return lpbox_fail(LPBOX_E_STATE, "layout already planned; choose the summation order before lpbox_init and the layout getters");
    h->order = mode;
    return LPBOX_OK;
}

// out[r * LPBOX_LOG_VALS + k], r = 0 .. returned rows - 1: the records of instance idx from the last lpbox_iterate call, in iteration order
// (iterations that stopped the loop are not logged, as in the reference).  Value 10 is converted to seconds since the call started.
int lpbox_get_log(lpbox_t *h, int idx, double *out, int cap_rows) {
    int rc = check_idx(h, idx);
    if (rc) return rc;
    if (h->seg) return lpbox_fail(LPBOX_E_STATE, "this entry point belongs to the LP flavour");
    if (!out || cap_rows < 0) return lpbox_fail(LPBOX_E_BADARG, "null output");
    if (h->log_rows <= 0) return 0;
    rc = use_device(h->device);
    if (rc) return rc;
    std::vector<double> t((size_t)h->log_rows * LP_LOG_VALS);
    HIPCHK(hipMemcpy(t.data(), h->logbuf.p + (size_t)idx * h->log_cap * LP_LOG_VALS, t.size() * sizeof(double), hipMemcpyDeviceToHost));
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, h->device) != hipSuccess || khz <= 0) khz = 100000;
    int rows = 0;
    for (int r = 0; r < h->log_rows && rows < cap_rows; r++) {
        const double *src = &t[(size_t)r * LP_LOG_VALS];
        if (src[11] != src[11]) continue;                            // NaN: not logged
        double *dst = out + (size_t)rows * LP_LOG_VALS;
        for (int k = 0; k < LP_LOG_VALS; k++) dst[k] = src[k];
        dst[10] = src[10] / (1e3 * khz);
        rows++;
    }
    return rows;
}

int lpbox_seg_get_x_history(lpbox_t *h, int first, int count, double *out) {
    if (!valid_handle(h) || !h->seg) return lpbox_fail(LPBOX_E_BADHANDLE, "bad handle (segmentation flavour only)");
    return segc_get_x_history(h->seg, first, count, out);
}

int lpbox_policy_layout(int tokens, long *weight_halves, long *const_floats) {
    if (tokens != 20 && tokens != 5) return lpbox_fail(LPBOX_E_BADARG, "tokens must be 20 (LP) or 5 (segmentation)");
    if (weight_halves) *weight_halves = 2L * POLICY_FRAGS_PER_LAYER * 512;
    if (const_floats) *const_floats = POLICY_OFF_LAYER(tokens) + 2L * POLICY_LAYER_CONSTS;
    return LPBOX_OK;
}

int lpbox_policy_encode_f16(const double *x_dev, const long long *row_off_dev, long rows, int tokens, int tok_stride,
                            const void *weights_dev, const float *consts_dev, void *out_dev, void *hip_stream) {
    if (tokens != 20 && tokens != 5) return lpbox_fail(LPBOX_E_BADARG, "tokens must be 20 (LP) or 5 (segmentation)");
    if (rows < 0 || tok_stride < 1) return lpbox_fail(LPBOX_E_BADARG, "bad rows / token stride");
    if (rows == 0) return LPBOX_OK;
    if (!x_dev || !row_off_dev || !weights_dev || !consts_dev || !out_dev) return lpbox_fail(LPBOX_E_BADARG, "null device pointer");
    PolicyArgs pa;
    pa.x = x_dev; pa.row_off = row_off_dev; pa.rows = rows; pa.tok_stride = tok_stride;
    pa.weights = weights_dev; pa.consts = consts_dev; pa.out = out_dev;
    HIPCHK(policy_launch_body(pa, tokens, (hipStream_t)hip_stream));
    return LPBOX_OK;
}

int lpbox_policy_f32frag_layout(int tokens, long *weight_floats, long *const_floats) {
    if (tokens != 20 && tokens != 5) return lpbox_fail(LPBOX_E_BADARG, "tokens must be 20 (LP) or 5 (segmentation)");
    if (weight_floats) *weight_floats = policy_f32frag_floats();
    if (const_floats) *const_floats = POLICY_OFF_LAYER(tokens) + 2L * POLICY_LAYER_CONSTS;
    return LPBOX_OK;
}

int lpbox_policy_encode_f32(const double *x_dev, const long long *row_off_dev, long rows, int tokens, int tok_stride,
                            const float *weights_dev, const float *consts_dev, float *out_dev, void *hip_stream) {
    if (tokens != 20 && tokens != 5) return lpbox_fail(LPBOX_E_BADARG, "tokens must be 20 (LP) or 5 (segmentation)");
    if (rows < 0 || tok_stride < 1) return lpbox_fail(LPBOX_E_BADARG, "bad rows / token stride");
    if (rows == 0) return LPBOX_OK;
    if (!x_dev || !row_off_dev || !weights_dev || !consts_dev || !out_dev) return lpbox_fail(LPBOX_E_BADARG, "null device pointer");
    PolicyArgs pa;
    pa.x = x_dev; pa.row_off = row_off_dev; pa.rows = rows; pa.tok_stride = tok_stride;
    pa.weights = weights_dev; pa.consts = consts_dev; pa.out = out_dev;
    HIPCHK(policy_launch_body_f32(pa, tokens, (hipStream_t)hip_stream));
    return LPBOX_OK;
}

int lpbox_policy_f32_layout(int tokens, long *weight_floats) {
    if (tokens != 20 && tokens != 5) return lpbox_fail(LPBOX_E_BADARG, "tokens must be 20 (LP) or 5 (segmentation)");
    if (weight_floats) *weight_floats = policy_f32_weight_floats(tokens);
    return LPBOX_OK;
}

int lpbox_policy_score_f32(const double *x_dev, const long long *row_off_dev, long rows, int tokens, int tok_stride,
                           const float *weights_dev, float *sigmoid_dev, float *logit_dev, void *hip_stream) {
    if (tokens != 20 && tokens != 5) return lpbox_fail(LPBOX_E_BADARG, "tokens must be 20 (LP) or 5 (segmentation)");
    if (rows < 0 || tok_stride < 1) return lpbox_fail(LPBOX_E_BADARG, "bad rows / token stride");
    if (rows == 0) return LPBOX_OK;
    if (!x_dev || !row_off_dev || !weights_dev || !sigmoid_dev) return lpbox_fail(LPBOX_E_BADARG, "null device pointer");
    HIPCHK(policy_launch_f32(x_dev, row_off_dev, rows, tokens, tok_stride, weights_dev, sigmoid_dev, logit_dev, 0.f, 0.f, 0.f, nullptr, (hipStream_t)hip_stream));
    return LPBOX_OK;
}

int lpbox_policy_rescore_f32(const double *x_dev, const long long *row_off_dev, long rows, int tokens, int tok_stride,
                             const float *weights_dev, float *sigmoid_dev, float band, float thr_hi, float thr_lo,
                             unsigned long long *count_dev, void *hip_stream) {
    if (tokens != 20 && tokens != 5) return lpbox_fail(LPBOX_E_BADARG, "tokens must be 20 (LP) or 5 (segmentation)");
    if (rows < 0 || tok_stride < 1 || !(band > 0.f)) return lpbox_fail(LPBOX_E_BADARG, "bad rows / token stride / band");
    if (rows == 0) return LPBOX_OK;
    if (!x_dev || !row_off_dev || !weights_dev || !sigmoid_dev) return lpbox_fail(LPBOX_E_BADARG, "null device pointer");
    HIPCHK(policy_launch_f32(x_dev, row_off_dev, rows, tokens, tok_stride, weights_dev, sigmoid_dev, nullptr, band, thr_hi, thr_lo, count_dev, (hipStream_t)hip_stream));
    return LPBOX_OK;
}

int lpbox_set_active(lpbox_t *h, const int *active) {
    if (!valid_handle(h) || h->seg) return lpbox_fail(LPBOX_E_BADHANDLE, "bad handle (LP flavour only)");
    if (!h->inited) return lpbox_fail(LPBOX_E_STATE, "solve_init has not been called");
    int rc = use_device(h->device);
    if (rc) return rc;
    std::vector<int> a(h->B, 1);
    for (int i = 0; i < h->B && active; i++) a[i] = active[i] != 0;
    HIPCHK(hipMemcpy2D(h->isc.p + NI_ACTIVE, NI_COUNT * sizeof(int), a.data(), sizeof(int), sizeof(int), h->B, hipMemcpyHostToDevice));
    for (int i = 0; i < h->B; i++) {
        if (h->h_isc[(size_t)i * NI_COUNT + NI_ACTIVE] != a[i]) h->rows_mask_changed = true;      // a row table built before this call is stale
        h->h_isc[(size_t)i * NI_COUNT + NI_ACTIVE] = a[i];
    }
    return LPBOX_OK;
}

int lpbox_get_n(lpbox_t *h, int idx) {
    if (valid_handle(h) && h->seg) return segc_get_n(h->seg);
    int rc = check_idx(h, idx);
    if (rc) return rc;
    if (!h->inited) return h->inst[idx].n;
    return h->h_isc[(size_t)idx * NI_COUNT + NI_NLIVE];
}

int lpbox_get_org_n(lpbox_t *h, int idx) {
    if (valid_handle(h) && h->seg) return segc_get_org_n(h->seg);
    int rc = check_idx(h, idx);
    if (rc) return rc;
    return h->inst[idx].n;
}

int lpbox_get_l(lpbox_t *h, int idx) {
    int rc = check_idx(h, idx);
    if (rc) return rc;
    return h->inst[idx].l;
}

int lpbox_get_iter(lpbox_t *h, int idx) {
    if (valid_handle(h) && h->seg) return segc_get_iter(h->seg);
    int rc = check_idx(h, idx);
    if (rc) return rc;
    if (!h->inited) return 0;
    return h->h_isc[(size_t)idx * NI_COUNT + NI_ITER];
}

int lpbox_get_x_iters(lpbox_t *h, int idx, int ws, double *out) {
    if (valid_handle(h) && h->seg) return segc_get_x_iters(h->seg, ws, out);
    int rc = check_idx(h, idx);
    if (rc) return rc;
    if (!h->xi_valid) return lpbox_fail(LPBOX_E_STATE, "solve_iter_l2f has not been called");
    const int ws_max = std::max(LP_XITERS_COLS, h->ws_cap);      // x_iters has 500 columns (LPcpp:1113); a recorded plain window may be longer
    if (ws < 0 || ws > ws_max) return lpbox_fail(LPBOX_E_BADARG, "ws = %d outside [0,%d]", ws, ws_max);
    const int rows = h->inst[idx].xi_rows;
    if (!out || rows == 0 || ws == 0) return rows;
    rc = use_device(h->device);
    if (rc) return rc;
    const int wsd = std::min(ws, h->ws_cap);          // columns beyond the staged window stay zero, like the reference's matrix
    rc = pack_xiters(h, wsd);                          // the whole batch, once per (call, ws)
    if (rc) return rc;
    if (wsd == ws) {
        HIPCHK(hipMemcpy(out, h->xi_out.p + (size_t)idx * h->xi_out_stride, sizeof(double) * (size_t)rows * ws, hipMemcpyDeviceToHost));
    } else {
        std::vector<double> tmp((size_t)rows * wsd);
        HIPCHK(hipMemcpy(tmp.data(), h->xi_out.p + (size_t)idx * h->xi_out_stride, sizeof(double) * tmp.size(), hipMemcpyDeviceToHost));
        for (int r = 0; r < rows; r++)
            for (int c = 0; c < ws; c++) out[(size_t)r * ws + c] = c < wsd ? tmp[(size_t)r * wsd + c] : 0.0;
    }
    return rows;
}

int lpbox_get_x_iters_device(lpbox_t *h, int ws, void **dev_ptr, long *stride_doubles) {
    if (valid_handle(h) && h->seg) return segc_get_x_iters_device(h->seg, ws, dev_ptr, stride_doubles);
    if (!valid_handle(h)) return lpbox_fail(LPBOX_E_BADHANDLE, "bad handle");
    if (!h->xi_valid) return lpbox_fail(LPBOX_E_STATE, "solve_iter_l2f has not been called");
    if (ws <= 0 || ws > h->ws_cap) return lpbox_fail(LPBOX_E_BADARG, "ws = %d outside (0,%d] (the last window)", ws, h->ws_cap);
    int rc = use_device(h->device);
    if (rc) return rc;
    rc = pack_xiters(h, ws);
    if (rc) return rc;
    if (dev_ptr) *dev_ptr = h->xi_out.p;
    if (stride_doubles) *stride_doubles = h->xi_out_stride;
    return LPBOX_OK;
}

long lpbox_get_x_iters_rows_device(lpbox_t *h, int ws, void **row_off_dev, int *first_row) {
    if (valid_handle(h) && h->seg) return lpbox_fail(LPBOX_E_STATE, "this entry point belongs to the LP flavour");
    if (!valid_handle(h)) return lpbox_fail(LPBOX_E_BADHANDLE, "bad handle");
    if (!h->xi_valid) return lpbox_fail(LPBOX_E_STATE, "solve_iter_l2f has not been called");
    if (ws <= 0 || ws > h->ws_cap) return lpbox_fail(LPBOX_E_BADARG, "ws = %d outside (0,%d] (the last window)", ws, h->ws_cap);
    int rc = use_device(h->device);
    if (rc) return rc;
    rc = pack_xiters(h, ws);
    if (rc) return rc;
    const int B = h->B;
    if (!h->rows_valid || h->rows_mask_changed || h->rows_ws != ws) {
        h->rows_valid = false;
        h->h_first_row.assign((size_t)B + 1, 0);
        for (int i = 0; i < B; i++)
            h->h_first_row[i + 1] = h->h_first_row[i] + (h->h_isc[(size_t)i * NI_COUNT + NI_ACTIVE] ? h->inst[i].xi_rows : 0);
        const size_t rows = (size_t)h->h_first_row[B];
        if (!h->first_row.p) { HIPCHK(h->first_row.alloc((size_t)B + 1)); HIPCHK(h->fix_counts.alloc(2 * (size_t)B)); }
        if (h->row_off.count < rows) { HIPCHK(h->row_off.alloc(rows)); HIPCHK(h->fix_codes.alloc(rows)); }
        HIPCHK(hipMemcpyAsync(h->first_row.p, h->h_first_row.data(), ((size_t)B + 1) * sizeof(int), hipMemcpyHostToDevice, h->stream));
        if (rows) HIPCHK(lp_launch_row_offsets(B, h->geo.NS, h->xi_rows.p, h->isc.p, h->first_row.p, ws, h->xi_out_stride, h->row_off.p, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));       // the caller reads the table on a stream of its own; h_first_row stays alive until here
        h->rows_valid = true; h->rows_mask_changed = false; h->rows_ws = ws;
    }
    if (row_off_dev) *row_off_dev = h->row_off.p;
    if (first_row) std::copy(h->h_first_row.begin(), h->h_first_row.end(), first_row);
    return (long)h->h_first_row[B];
}

int lpbox_iterate_l2f_scores(lpbox_t *h, int iter_start, int iter_end, const float *scores_dev, double hi, double lo, int min_fix,
                             int *rets, int *fixed) {
    if (valid_handle(h) && h->seg) return lpbox_fail(LPBOX_E_STATE, "this entry point belongs to the LP flavour (segmentation: lpbox_seg_batch_iterate_l2f_scores)");
    if (!valid_handle(h)) return lpbox_fail(LPBOX_E_BADHANDLE, "bad handle");
    const int ws = iter_end - iter_start;
    if (ws > LP_XITERS_COLS) return lpbox_fail(LPBOX_E_BADARG, "window of %d iterations exceeds the %d columns of x_iters (LPcpp:1113)", ws, LP_XITERS_COLS);
    if (min_fix < 0) return lpbox_fail(LPBOX_E_BADARG, "min_fix = %d is negative", min_fix);
    if (!std::isfinite(hi) || !std::isfinite(lo) || hi < lo) return lpbox_fail(LPBOX_E_BADARG, "thresholds hi = %g, lo = %g: both must be finite and hi >= lo", hi, lo);
    if (scores_dev && !h->rows_valid)
        return lpbox_fail(LPBOX_E_STATE, "scores given but lpbox_get_x_iters_rows_device has not been called since the last window");
    if (scores_dev && h->rows_mask_changed)
        return lpbox_fail(LPBOX_E_STATE, "scores given but lpbox_set_active changed the active instances after the row table was built");
    if (!h->inited) return lpbox_fail(LPBOX_E_STATE, "solve_init has not been called");
    int rc = use_device(h->device);
    if (rc) return rc;
    const size_t B = h->B;
    std::vector<int> k(B, 0);
    std::vector<uint8_t> codes;
    const std::vector<int> first = h->h_first_row;      // (l2f_window invalidates the table)
    if (scores_dev && first[B] > 0) {
        std::vector<int> counts(2 * B, 0);
        codes.resize((size_t)first[B]);
        // codes of earlier windows sit at positions that have been fixed since: the decide kernel writes live positions only
        HIPCHK(hipMemsetAsync(h->newfix.p, 0, B * (size_t)h->geo.NS, h->stream));
        HIPCHK(lp_launch_decide_fix((int)B, h->geo.NS, scores_dev, h->xi_rows.p, h->isc.p, h->first_row.p, h->left_idx.p, hi, lo, h->newfix.p,
                                    h->fix_codes.p, h->fix_counts.p, h->stream));
        HIPCHK(hipMemcpyAsync(counts.data(), h->fix_counts.p, counts.size() * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(codes.data(), h->fix_codes.p, codes.size(), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        for (size_t i = 0; i < B; i++) {
            if (first[i + 1] == first[i]) continue;                         // parked
            const int n = counts[2 * i] + counts[2 * i + 1];
            if (n > min_fix) k[i] = n;                                      // LP/trainer.py:533-535: k <= min_fix fixes nothing
        }
    }
    if (fixed) std::copy(k.begin(), k.end(), fixed);
    return l2f_window(h, iter_start, iter_end, k, false, [&](size_t i, int q) { return (int)codes[(size_t)first[i] + q]; }, rets);
}

int lpbox_get_x_sol(lpbox_t *h, int idx, double *out) {
    if (valid_handle(h) && h->seg) return segc_get_x_sol(h->seg, out);
    int rc = check_idx(h, idx);
    if (rc) return rc;
    if (!h->inited || !out) return lpbox_fail(LPBOX_E_STATE, "not initialised");
    rc = use_device(h->device);
    if (rc) return rc;
    std::vector<double> x; std::vector<uint8_t> live;
    if ((rc = fetch_vec(h, h->x.p, h->geo.NS, idx, h->inst[idx].n, x))) return rc;
    if ((rc = fetch_live(h, idx, live))) return rc;
    for (int j = 0; j < h->inst[idx].n; j++) out[j] = live[j] ? (x[j] >= 0.5 ? 1.0 : 0.0) : x[j];   // LPcpp:1648-1665
    return h->inst[idx].n;
}

int lpbox_get_final_x_sol(lpbox_t *h, int idx, double *out) {
    int rc = check_idx(h, idx);
    if (rc) return rc;
    if (!h->inited || !out) return lpbox_fail(LPBOX_E_STATE, "not initialised");
    rc = use_device(h->device);
    if (rc) return rc;
    std::vector<double> x;
    if ((rc = fetch_vec(h, h->x.p, h->geo.NS, idx, h->inst[idx].n, x))) return rc;
    const auto &li = h->inst[idx].left_idx;
    for (size_t q = 0; q < li.size(); q++) out[q] = x[li[q]];              // LPcpp:1668-1685: the live (compacted) x_sol
    return (int)li.size();
}

int lpbox_cal_obj(lpbox_t *h, int idx, double *out) {
    int rc = check_idx(h, idx);
    if (rc) return rc;
    if (!h->inited || !out) return lpbox_fail(LPBOX_E_STATE, "not initialised");
    const double *d = &h->h_dsc[(size_t)idx * ND_COUNT];
    const int n_live = h->h_isc[(size_t)idx * NI_COUNT + NI_NLIVE];
    *out = n_live != 0 ? d[ND_SUM_FIX_OBJ] + d[ND_CUR_OBJ] : d[ND_SUM_FIX_OBJ];   // LPcpp:1630-1642
    return LPBOX_OK;
}

int lpbox_cur_bin_obj(lpbox_t *h, int idx, double *out) {
    int rc = check_idx(h, idx);
    if (rc) return rc;
    if (!h->inited || !out) return lpbox_fail(LPBOX_E_STATE, "not initialised");
    *out = h->h_dsc[(size_t)idx * ND_COUNT + ND_CUR_OBJ];
    return LPBOX_OK;
}

int lpbox_get_problem_lp(lpbox_t *h, int idx, int *n, int *l, int *nnz, int *colptr, int *rowidx, double *b, double *f) {
    int rc = check_idx(h, idx);
    if (rc) return rc;
    const LpInstance &I = h->inst[idx];
    if (!I.set) return lpbox_fail(LPBOX_E_STATE, "instance %d has no problem (call read_File / set_problem first)", idx);
    if (n) *n = I.n;
    if (l) *l = I.l;
    if (nnz) *nnz = I.nnz;
    if (colptr) std::copy(I.colptr.begin(), I.colptr.end(), colptr);
    if (rowidx) std::copy(I.rowidx.begin(), I.rowidx.end(), rowidx);
    if (b) std::copy(I.b.begin(), I.b.end(), b);
    if (f) std::copy(I.f_org.begin(), I.f_org.end(), f);
    return LPBOX_OK;
}

int lpbox_get_problem_lp_vals(lpbox_t *h, int idx, double *vals) {
    if (valid_handle(h) && h->seg) return lpbox_fail(LPBOX_E_STATE, "this entry point belongs to the LP flavour");
    int rc = check_idx(h, idx);
    if (rc) return rc;
    const LpInstance &I = h->inst[idx];
    if (!I.set) return lpbox_fail(LPBOX_E_STATE, "instance %d has no problem (call read_File / set_problem first)", idx);
    if (vals) {
        if (I.vals.empty()) std::fill(vals, vals + I.nnz, 1.0);
        else std::copy(I.vals.begin(), I.vals.end(), vals);
    }
    return I.nnz;
}

int lpbox_check_infeasible_lpbox(lpbox_t *h, int idx) {                     // LPcpp:1577-1591: rows of the CURRENT E with (E x)_i > 1
    int rc = check_idx(h, idx);
    if (rc) return rc;
    if (!h->inited) return lpbox_fail(LPBOX_E_STATE, "not initialised");
    rc = use_device(h->device);
    if (rc) return rc;
    const LpInstance &I = h->inst[idx];
    if (I.left_idx.empty()) return 0;
    std::vector<double> x; std::vector<uint8_t> live;
    if ((rc = fetch_vec(h, h->x.p, h->geo.NS, idx, I.n, x))) return rc;
    if ((rc = fetch_live(h, idx, live))) return rc;
    int inf = 0;
    for (int r = 0; r < I.l; r++) {
        double s = 0.0;
        // mat_mul_vec on the compacted E: res_i += val * (1.0 * x_j) over the live columns, ascending, from 0
        for (int k = I.rowptr[r]; k < I.rowptr[r + 1]; k++) if (live[I.colidx[k]]) s += (I.vals.empty() ? 1.0 : I.vals_csr[k]) * (1.0 * x[I.colidx[k]]);
        if (!(s <= 1.0)) inf++;
    }
    return inf;
}

int lpbox_check_infeasible_l2f(lpbox_t *h, int idx) {                       // LPcpp:1593-1612: ORIGINAL E times the rounded full-length x
    int rc = check_idx(h, idx);
    if (rc) return rc;
    if (!h->inited) return lpbox_fail(LPBOX_E_STATE, "not initialised");
    const LpInstance &I = h->inst[idx];
    std::vector<double> sol(I.n);
    rc = lpbox_get_x_sol(h, idx, sol.data());
    if (rc < 0) return rc;
    int inf = 0;
    for (int r = 0; r < I.l; r++) {
        double s = 0.0;
        for (int k = I.rowptr[r]; k < I.rowptr[r + 1]; k++) s += (I.vals.empty() ? 1.0 : I.vals_csr[k]) * (1.0 * sol[I.colidx[k]]);
        if (!(s <= 1.0)) inf++;
    }
    return inf;
}

int lpbox_get_config(lpbox_t *h, int *threads, int *elems_per_thread, int *lds_bytes) {
    if (valid_handle(h) && h->seg) return segc_get_config(h->seg, threads, elems_per_thread, lds_bytes);
    if (!valid_handle(h)) return lpbox_fail(LPBOX_E_BADHANDLE, "bad handle");
    int rc = plan(h);
    if (rc) return rc;
    if (threads) *threads = h->geo.T;
    if (elems_per_thread) *elems_per_thread = h->geo.EPT;
    if (lds_bytes) *lds_bytes = (int)h->lds;
    return LPBOX_OK;
}

int lpbox_get_pcg_loop(lpbox_t *h, int *specialised) {
    if (!valid_handle(h) || h->seg) return lpbox_fail(LPBOX_E_BADHANDLE, "bad handle");
    int rc = plan(h);
    if (rc) return rc;
    if (!specialised) return lpbox_fail(LPBOX_E_BADARG, "null output");
    *specialised = (h->order != LPBOX_ORDER_REFERENCE && !h->direct && !h->log_on && lp_pcg_specialised(h->geo.T, h->geo.EPT) && !h->opt.pcg_generic) ? 1 : 0;
    return LPBOX_OK;
}

int lpbox_wave_class_rule(int lanes, const int *row_len, const int *col_len, const int *help_len, int *class4) {
    if (lanes < 0 || !class4 || (lanes > 0 && (!row_len || !col_len || !help_len))) return lpbox_fail(LPBOX_E_BADARG, "null or negative argument");
    int caps[3];
    lp_pcg_list_caps(&caps[0], &caps[1], &caps[2]);
    lp_wave_class_rule(lanes, row_len, col_len, help_len, caps, class4);
    return LPBOX_OK;
}

int lpbox_get_wave_classes(lpbox_t *h, int idx, int *classes4) {
    int rc = check_idx(h, idx);
    if (rc) return rc;
    if (h->seg) return lpbox_fail(LPBOX_E_BADHANDLE, "bad handle");
    rc = plan(h);
    if (rc) return rc;
    if (!classes4) return lpbox_fail(LPBOX_E_BADARG, "null output");
    const LpInstance &I = h->inst[idx];
    if (I.lay.wave_class.empty()) return lpbox_fail(LPBOX_E_UNSUPPORTED, "wave classes are defined for the 512 x 1 kernel of the default order");
    for (size_t k = 0; k < I.lay.wave_class.size(); k++) classes4[k] = I.lay.wave_class[k];
    return (int)(I.lay.wave_class.size() / 4);
}

int lpbox_get_layout(lpbox_t *h, int idx, int *pos_of_var) {
    int rc = check_idx(h, idx);
    if (rc) return rc;
    rc = plan(h);
    if (rc) return rc;
    if (!pos_of_var) return lpbox_fail(LPBOX_E_BADARG, "null output");
    const LpInstance &I = h->inst[idx];
    for (int j = 0; j < I.n; j++) pos_of_var[j] = I.lay.cpos[j];
    return I.n;
}

int lpbox_get_row_split(lpbox_t *h, int idx, int *lanes_of_row) {
    int rc = check_idx(h, idx);
    if (rc) return rc;
    rc = plan(h);
    if (rc) return rc;
    if (!lanes_of_row) return lpbox_fail(LPBOX_E_BADARG, "null output");
    const LpInstance &I = h->inst[idx];
    for (int r = 0; r < I.l; r++) lanes_of_row[r] = I.lay.rowG[r];
    return I.l;
}

int lpbox_get_col_split(lpbox_t *h, int idx, int *own, int *help4) {
    int rc = check_idx(h, idx);
    if (rc) return rc;
    rc = plan(h);
    if (rc) return rc;
    if (!own || !help4) return lpbox_fail(LPBOX_E_BADARG, "null output");
    const LpInstance &I = h->inst[idx];
    for (int j = 0; j < I.n; j++) own[j] = I.lay.col_own[j];
    for (int k = 0; k < 4 * I.n; k++) help4[k] = I.lay.col_help[k];
    return I.n;
}

int lpbox_get_direct_rows(lpbox_t *h, int idx, int *gidx_of_row) {
    int rc = check_idx(h, idx);
    if (rc) return rc;
    if (h->seg) return lpbox_fail(LPBOX_E_STATE, "this entry point belongs to the LP flavour");
    LpInstance &I = h->inst[idx];
    if (!I.set) return lpbox_fail(LPBOX_E_STATE, "instance %d has no problem (call read_File / set_problem first)", idx);
    if (!gidx_of_row) return lpbox_fail(LPBOX_E_BADARG, "null output");
    if ((int)I.dir_g.size() != I.l) I.nG = lp_plan_direct_rows(view_of(I), &I.dir_g);     // a function of the instance alone: no device, no mode
    for (int r = 0; r < I.l; r++) gidx_of_row[r] = I.dir_g[r];
    return I.nG;
}

int lpbox_get_counters(lpbox_t *h, int idx, long long *outer_iters, long long *pcg_iters) {
    if (valid_handle(h) && h->seg) return segc_get_counters(h->seg, outer_iters, pcg_iters);
    int rc = check_idx(h, idx);
    if (rc) return rc;
    if (!h->inited) return lpbox_fail(LPBOX_E_STATE, "not initialised");
    if (outer_iters) *outer_iters = h->h_isc[(size_t)idx * NI_COUNT + NI_OUTER_TOTAL];
    if (pcg_iters) *pcg_iters = h->h_isc[(size_t)idx * NI_COUNT + NI_PCG_TOTAL];
    return LPBOX_OK;
}

int lpbox_get_stop(lpbox_t *h, int idx, int *reason, int *plain_iter_plus1) {
    if (valid_handle(h) && h->seg) return segc_get_stop(h->seg, reason, plain_iter_plus1);
    int rc = check_idx(h, idx);
    if (rc) return rc;
    if (!h->inited) return lpbox_fail(LPBOX_E_STATE, "not initialised");
    if (reason) *reason = h->h_isc[(size_t)idx * NI_COUNT + NI_STOP];
    if (plain_iter_plus1) *plain_iter_plus1 = h->h_isc[(size_t)idx * NI_COUNT + NI_PLAIN_ITER_P1];
    return LPBOX_OK;
}

int lpbox_kernel_time(lpbox_t *h, double *ms_total, long long *launches, int reset) {
    if (valid_handle(h) && h->seg) return segc_kernel_time(h->seg, ms_total, launches, reset);
    if (!valid_handle(h)) return lpbox_fail(LPBOX_E_BADHANDLE, "bad handle");
    if (ms_total) *ms_total = h->kernel_ms;
    if (launches) *launches = h->launches;
    if (reset) { h->kernel_ms = 0.0; h->launches = 0; }
    return LPBOX_OK;
}

// Host only: a table of the planned layout of instance idx as the device sees it, i.e. at the stride of the batch.
int lpbox_debug_get_lp_table(lpbox_t *h, int idx, const char *name, int *out, int cap) {
    int rc = check_idx(h, idx);
    if (rc) return rc;
    if (h->seg) return lpbox_fail(LPBOX_E_STATE, "this entry point belongs to the LP flavour");
    if (!name || !out) return lpbox_fail(LPBOX_E_BADARG, "null argument");
    rc = plan(h);
    if (rc) return rc;
    const LpInstanceLayout &L = h->inst[idx].lay;
    const size_t NS = h->geo.NS, ZS = h->geo.ZS;
    auto give = [&](const auto &table, size_t stride, int fill) {
        if ((size_t)cap < stride) return lpbox_fail(LPBOX_E_BADARG, "buffer too small");
        for (size_t q = 0; q < stride; q++) out[q] = q < table.size() ? (int)table[q] : fill;
        return (int)stride;
    };
    if (!strcmp(name, "rs_ptr")) return give(L.rs_ptr, NS + 1, 0);
    if (!strcmp(name, "cs_ptr")) return give(L.cs_ptr, NS + 1, 0);
    if (!strcmp(name, "hs_ptr")) return give(L.hs_ptr, NS + 1, 0);
    if (!strcmp(name, "rs_col")) return give(L.rs_col, ZS, 0);
    if (!strcmp(name, "cs_row")) return give(L.cs_row, ZS, 0);
    if (!strcmp(name, "rid")) return give(L.rid, NS, 0xFFFF);
    if (!strcmp(name, "rgl")) return give(L.rgl, NS, 0);
    if (!strcmp(name, "rmeta")) return give(L.rmeta, NS, 0x10);
    if (!strcmp(name, "cmeta")) return give(L.cmeta, NS, 0);
    return lpbox_fail(LPBOX_E_BADARG, "unknown table '%s'", name);
}

int lpbox_debug_get_vec(lpbox_t *h, int idx, const char *name, double *out, int cap) {
    if (valid_handle(h) && h->seg) return segc_debug_vec(h->seg, name, out, cap);
    int rc = check_idx(h, idx);
    if (rc) return rc;
    if (!h->inited || !name || !out) return lpbox_fail(LPBOX_E_STATE, "not initialised");
    rc = use_device(h->device);
    if (rc) return rc;
    const LpInstance &I = h->inst[idx];
    const double *pool = nullptr; size_t stride = h->geo.NS; int len = I.n; bool by_var = true;
    if (!strcmp(name, "x")) pool = h->x.p;
    else if (!strcmp(name, "z1")) pool = h->z1.p;
    else if (!strcmp(name, "z2")) pool = h->z2.p;
    else if (!strcmp(name, "b")) pool = h->b.p;
    else if (!strcmp(name, "pd")) pool = h->pd.p;
    else if (!strcmp(name, "z4")) { pool = h->z4.p; stride = h->geo.LS; len = I.l; by_var = false; }
    else if (!strcmp(name, "f")) { pool = h->f.p; stride = h->geo.LS; len = I.l; by_var = false; }
    else if (!strcmp(name, "r4v")) {     // valued reference-order batches: the entries of rho4_E_transpose, CSC entry order
        if (!h->valued) return lpbox_fail(LPBOX_E_BADARG, "no stored values in this batch");
        if (I.nnz > cap) return lpbox_fail(LPBOX_E_BADARG, "buffer too small");
        HIPCHK(hipMemcpy(out, h->r4v.p + (size_t)idx * h->geo.ZS, sizeof(double) * (size_t)I.nnz, hipMemcpyDeviceToHost));
        return I.nnz;
    }
    else if (!strcmp(name, "live")) {
        std::vector<uint8_t> live;
        if ((rc = fetch_live(h, idx, live))) return rc;
        if (I.n > cap) return lpbox_fail(LPBOX_E_BADARG, "buffer too small");
        for (int j = 0; j < I.n; j++) out[j] = live[j];
        return I.n;
    } else return lpbox_fail(LPBOX_E_BADARG, "unknown vector '%s'", name);
    if (len > cap) return lpbox_fail(LPBOX_E_BADARG, "buffer too small");
    std::vector<double> v;
    if ((rc = fetch_vec(h, pool, stride, idx, len, v, by_var))) return rc;
    memcpy(out, v.data(), sizeof(double) * (size_t)len);
    return len;
}

// diagnostic build only: the 16 phase counters (shader cycles of wave 0) of instance idx from the last launch
int lpbox_debug_get_stamps(lpbox_t *h, int idx, unsigned long long *out16) {
    int rc = check_idx(h, idx);
    if (rc) return rc;
    if (!h->stamps.p) return lpbox_fail(LPBOX_E_UNSUPPORTED, "library built without LPBOX_STAMPS");
    HIPCHK(hipMemcpy(out16, h->stamps.p + (size_t)idx * 16, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return LPBOX_OK;
}

int lpbox_debug_get_scalar(lpbox_t *h, int idx, const char *name, double *out) {
    if (valid_handle(h) && h->seg) return segc_debug_scalar(h->seg, name, out);
    int rc = check_idx(h, idx);
    if (rc) return rc;
    if (!h->inited || !name || !out) return lpbox_fail(LPBOX_E_STATE, "not initialised");
    const double *d = &h->h_dsc[(size_t)idx * ND_COUNT];
    const int *q = &h->h_isc[(size_t)idx * NI_COUNT];
    struct { const char *n; double v; } tab[] = {
        {"rho1", d[ND_RHO1]}, {"rho2", d[ND_RHO2]}, {"rho4", d[ND_RHO4]}, {"prev_rho1", d[ND_PREV_RHO1]},
        {"prev_rho4", d[ND_PREV_RHO4]}, {"gamma", d[ND_GAMMA]}, {"dI", d[ND_DI]}, {"rho4Et", d[ND_R4ET]},
        {"std_obj", d[ND_STD_OBJ]}, {"cur_obj", d[ND_CUR_OBJ]}, {"sum_fix_obj", d[ND_SUM_FIX_OBJ]},
        {"best_bin_obj", d[ND_BEST_BIN_OBJ]}, {"cvg1", d[ND_CVG1]}, {"cvg2", d[ND_CVG2]}, {"obj_val", d[ND_OBJ_VAL]},
        {"rhoUpdated", (double)q[NI_RHO_UPDATED]}, {"last_pcg", (double)q[NI_LAST_PCG]},
    };
    for (auto &e : tab) if (!strcmp(e.n, name)) { *out = e.v; return LPBOX_OK; }
    return lpbox_fail(LPBOX_E_BADARG, "unknown scalar '%s'", name);
}

int lpbox_debug_block_sum(int threads, int nv, int stage, int groups, int rounds, const double *in, double *out) {
    if (!in || !out || groups <= 0 || groups > 1024 || rounds <= 0 || rounds > 1024) return lpbox_fail(LPBOX_E_BADARG, "lpbox_debug_block_sum: bad argument");
    if (threads <= 0 || threads > 1024 || nv <= 0 || nv > 6 || stage < 0 || stage > 5 || (stage != 0 && threads != 512))    // stages 1..5 are built for 512 threads
        return lpbox_fail(LPBOX_E_BADARG, "lpbox_debug_block_sum: no kernel for %d threads, %d values, stage %d", threads, nv, stage);
    if (lpbox_device_count() < 1) return lpbox_fail(LPBOX_E_NODEVICE, "no HIP device");
    HIPCHK(hipSetDevice(g_device));
    const size_t per = (size_t)rounds * threads * nv;
    DevBuf<double> din, dout;                                                    // freed on every return path
    HIPCHK(din.alloc(per));
    HIPCHK(dout.alloc(per * groups));
    HIPCHK(hipMemcpy(din.p, in, per * sizeof(double), hipMemcpyHostToDevice));
    hipError_t e = lp_launch_debug_block_sum(threads, nv, stage, groups, rounds, din.p, dout.p, nullptr);
    if (e == hipErrorInvalidConfiguration) return lpbox_fail(LPBOX_E_BADARG, "lpbox_debug_block_sum: no kernel for %d threads, %d values, stage %d", threads, nv, stage);
    HIPCHK(e);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, dout.p, per * groups * sizeof(double), hipMemcpyDeviceToHost));
    return LPBOX_OK;
}

int lpbox_debug_handover(int form, int nv, int l_lo, int l_hi, int groups, int rounds, const int *pos, const double *v0, double *last, double *totals) {
    if (!pos || !v0 || !last || !totals || groups <= 0 || groups > 1024 || rounds <= 0 || rounds > 100000)
        return lpbox_fail(LPBOX_E_BADARG, "lpbox_debug_handover: bad argument");
    if (lpbox_device_count() < 1) return lpbox_fail(LPBOX_E_NODEVICE, "no HIP device");
    HIPCHK(hipSetDevice(g_device));
    const size_t T = 512, ntot = (size_t)groups * rounds * (nv == 2 ? 2 : 1);
    DevBuf<int> dpos;                                                            // freed on every return path
    DevBuf<double> dv0, dlast, dtot;
    HIPCHK(dpos.alloc(12 * T));
    HIPCHK(dv0.alloc(T));
    HIPCHK(dlast.alloc(groups * T));
    HIPCHK(dtot.alloc(ntot));
    HIPCHK(hipMemcpy(dpos.p, pos, 12 * T * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dv0.p, v0, T * sizeof(double), hipMemcpyHostToDevice));
    hipError_t e = lp_launch_debug_handover(form, nv, l_lo, l_hi, groups, rounds, dpos.p, dv0.p, dlast.p, dtot.p, nullptr);
    if (e == hipErrorInvalidConfiguration)
        return lpbox_fail(LPBOX_E_BADARG, "lpbox_debug_handover: no kernel for form %d, %d values, list lengths %d / %d", form, nv, l_lo, l_hi);
    HIPCHK(e);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(last, dlast.p, groups * T * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(totals, dtot.p, ntot * sizeof(double), hipMemcpyDeviceToHost));
    return LPBOX_OK;
}

// ---- segmentation flavour (SEG pxd = Segmentation/Segmentation/cython/src/LPboxADMMsolver.pxd) ----
static int seg_handle(lpbox_t *h) {
    if (!valid_handle(h)) return lpbox_fail(LPBOX_E_BADHANDLE, "bad handle");
    if (!h->seg) return lpbox_fail(LPBOX_E_STATE, "this entry point belongs to the segmentation flavour");
    return LPBOX_OK;
}

int lpbox_set_problem_bqp(lpbox_t *h, int n, int nnz, const int *rowptr, const int *colidx, const double *vals,
                          const double *b, double c, int rows, int cols) {
    int rc = seg_handle(h);
    if (rc) return rc;
    return segc_set_problem(h->seg, n, nnz, rowptr, colidx, vals, b, c, rows, cols);
}

int lpbox_seg_set_image(lpbox_t *h, const unsigned char *gray, int rows, int cols, int num_nodes) {
    int rc = seg_handle(h);
    if (rc) return rc;
    return segc_set_image(h->seg, gray, rows, cols, num_nodes);
}

int lpbox_seg_set_order(lpbox_t *h, int mode) {
    int rc = seg_handle(h);
    if (rc) return rc;
    return segc_set_order(h->seg, mode);
}

int lpbox_seg_legacy(lpbox_t *h, int *energy) {
    int rc = seg_handle(h);
    if (rc) return rc;
    return segc_legacy(h->seg, energy);
}

int lpbox_seg_legacy_batch(lpbox_t **hs, int count, int *energies) {
    if (!hs || count <= 0) return lpbox_fail(LPBOX_E_BADARG, "empty batch");
    std::vector<SegSolver *> ss(count);
    for (int i = 0; i < count; i++) {
        int rc = seg_handle(hs[i]);
        if (rc) return rc;
        ss[i] = hs[i]->seg;
    }
    return segc_legacy_batch(ss.data(), count, energies);
}

// ---- early-fixing windows for a batch of segmentation handles (lpbox_seg_capi.hip) ----
lpbox_seg_batch_t *lpbox_seg_batch_create(lpbox_t **hs, int count) {
    if (!hs || count <= 0) { lpbox_fail(LPBOX_E_BADARG, "empty batch"); return nullptr; }
    std::vector<SegSolver *> ss(count);
    for (int i = 0; i < count; i++) {
        if (!valid_handle(hs[i])) { lpbox_fail(LPBOX_E_BADHANDLE, "problem %d of the batch is not a handle", i); return nullptr; }
        if (!hs[i]->seg) { lpbox_fail(LPBOX_E_STATE, "problem %d of the batch is an LP-flavour handle", i); return nullptr; }
        ss[i] = hs[i]->seg;
    }
    return segbc_create(ss.data(), count);                         // NULL: refused, lpbox_last_status() / lpbox_last_error() say why
}

void lpbox_seg_batch_destroy(lpbox_seg_batch_t *b) { segbc_destroy(b); }

#define SEG_BATCH_OR_FAIL(b) do { if (!(b)) return lpbox_fail(LPBOX_E_BADHANDLE, "bad batch handle"); } while (0)
int lpbox_seg_batch_init(lpbox_seg_batch_t *b) { SEG_BATCH_OR_FAIL(b); return segbc_init(b); }
int lpbox_seg_batch_set_active(lpbox_seg_batch_t *b, const unsigned char *active) { SEG_BATCH_OR_FAIL(b); return segbc_set_active(b, active); }
int lpbox_seg_batch_iterate_l2f(lpbox_seg_batch_t *b, int iter_start, int iter_end, const double *vecs, long vec_stride, const int *nums,
                                int *rets) {
    SEG_BATCH_OR_FAIL(b);
    return segbc_l2f(b, iter_start, iter_end, vecs, vec_stride, nums, rets);
}
int lpbox_seg_batch_get_x_iters_device(lpbox_seg_batch_t *b, int ws, void **dev_ptr, long *row_off) {
    SEG_BATCH_OR_FAIL(b);
    return segbc_get_x_iters_device(b, ws, dev_ptr, row_off);
}
int lpbox_seg_batch_iterate_l2f_scores(lpbox_seg_batch_t *b, int iter_start, int iter_end, const float *scores_dev, double hi, double lo,
                                       int min_fix, int *rets, int *fixed) {
    SEG_BATCH_OR_FAIL(b);
    return segbc_l2f_scores(b, iter_start, iter_end, scores_dev, hi, lo, min_fix, rets, fixed);
}

int lpbox_seg_get_obj(lpbox_t *h, double *out) {
    int rc = seg_handle(h);
    if (rc) return rc;
    return segc_get_obj(h->seg, out);
}

int lpbox_seg_get_shape(lpbox_t *h, int *rows, int *cols) {
    int rc = seg_handle(h);
    if (rc) return rc;
    return segc_get_shape(h->seg, rows, cols);
}

int lpbox_seg_get_problem(lpbox_t *h, int *n, int *nnz, int *rowptr, int *colidx, double *vals, double *b, double *c) {
    int rc = seg_handle(h);
    if (rc) return rc;
    return segc_get_problem(h->seg, n, nnz, rowptr, colidx, vals, b, c);
}

}  // extern "C"
