// lpbox_genb_capi.hip -- host side + C-ABI (lpbox_bqp_batch_* in include/lpbox_hip.h) of the BATCH of small generic constrained
// binary QPs: the reference's ADMM_bqp (SEGcpp:1384-1832) for many independent problems with max(n, m, l) <= 2048 at once, one
// persistent workgroup each (lpbox_genb_kernels.hip).  Validation, presets and messages are those of the one-problem handle
// (lpbox_gen_host.h); a problem gives the same bits here and through lpbox_bqp_*.  Device buffers, timer and error-check macros: lpbox_host.h.
#include "lpbox_gen_host.h"
#include "lpbox_genb.h"
#include "lpbox_host.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {
constexpr int GENB_DEFAULT_WINDOW = 64;      // outer iterations per launch
struct BatchProblem : GenHostProblem { GenParams prm; bool set = false; };
}  // namespace

struct lpbox_bqp_batch {
    int device = 0, count = 0;
    std::vector<BatchProblem> prob;
    bool uploaded = false, solved = false;
    bool ref = false;                        // LPBOX_ORDER_REFERENCE: the REF kernels, c1 through libm's pow
    int nmax = 0, mmax = 0, lmax = 0, slots = 2, window = GENB_DEFAULT_WINDOW;
    hipStream_t stream = nullptr;
    StreamTimer timer;
    DevBuf<int> ipool; DevBuf<double> dpool; DevBuf<GenbProb> dprob; DevBuf<GenState> dst;
    std::vector<GenbProb> hprob;             // the descriptors as uploaded (device pointers): the getters read through them
    std::vector<GenState> hst;
    double kernel_ms = 0.0; long long launches = 0;
};

namespace {
int check_index(lpbox_bqp_batch *h, int idx, bool all_ok) {
    if (!h) return lpbox_fail(LPBOX_E_BADHANDLE, "bad handle");
    if ((idx == -1 && all_ok) || (idx >= 0 && idx < h->count)) return LPBOX_OK;
    return lpbox_fail(LPBOX_E_BADARG, "problem index %d out of range [0,%d)", idx, h->count);
}

// Placement: every matrix and every vector of ADMM state goes into two pooled device arrays (ints, doubles), a slice per problem;
// the kernel keeps only the gathered vectors (n + m + l doubles of the largest problem) in LDS, so there is no nnz limit.
int upload(lpbox_bqp_batch *h) {
    h->uploaded = false;
    std::vector<int> ip; std::vector<double> dp;
    struct Off { size_t aptr, aidx, adiag, crp, cri, ccp, cci, erp, eri, ecp, eci, aval, tmval, crv, ccv, ccsv, erv, ecv, ecsv, x0, b, d, f, nvec, z3, lvec; };
    std::vector<Off> off(h->count);
    auto put_i = [&](const std::vector<int> &v) { const size_t o = ip.size(); ip.insert(ip.end(), v.begin(), v.end()); return o; };
    auto put_d = [&](const std::vector<double> &v) { const size_t o = dp.size(); dp.insert(dp.end(), v.begin(), v.end()); return o; };
    auto room_d = [&](size_t c) { const size_t o = dp.size(); dp.resize(o + c, 0.0); return o; };
    h->nmax = h->mmax = h->lmax = 0;
    for (int i = 0; i < h->count; i++) {
        const BatchProblem &p = h->prob[i];
        Off &o = off[i];
        h->nmax = std::max(h->nmax, p.n); h->mmax = std::max(h->mmax, p.m); h->lmax = std::max(h->lmax, p.l);
        o.aptr = put_i(p.A.ptr); o.aidx = put_i(p.A.idx); o.adiag = put_i(p.adiag);
        o.crp = put_i(p.C.ptr); o.cri = put_i(p.C.idx); o.ccp = put_i(p.Ct.ptr); o.cci = put_i(p.Ct.idx);
        o.erp = put_i(p.E.ptr); o.eri = put_i(p.E.idx); o.ecp = put_i(p.Et.ptr); o.eci = put_i(p.Et.idx);
        o.aval = put_d(p.A.val); o.tmval = room_d(p.A.val.size());
        o.crv = put_d(p.C.val); o.ccv = put_d(p.Ct.val); o.ccsv = room_d(p.Ct.val.size());
        o.erv = put_d(p.E.val); o.ecv = put_d(p.Et.val); o.ecsv = room_d(p.Et.val.size());
        o.x0 = put_d(p.x0); o.b = put_d(p.b); o.d = put_d(p.d); o.f = put_d(p.f);
        o.nvec = room_d((size_t)10 * p.n); o.z3 = room_d(p.m); o.lvec = room_d((size_t)4 * p.l);
    }
    h->slots = h->nmax <= 512 ? 2 : h->nmax <= 1024 ? 4 : 8;
    HIPCHK(h->ipool.upload(ip, 1)); HIPCHK(h->dpool.upload(dp, 1));     // (at least one element, as lpbox_gen_capi.hip)
    HIPCHK(h->dprob.alloc((size_t)h->count)); HIPCHK(h->dst.alloc((size_t)h->count));
    h->hprob.assign(h->count, GenbProb());
    for (int i = 0; i < h->count; i++) {
        const BatchProblem &p = h->prob[i];
        const Off &o = off[i];
        GenbProb &g = h->hprob[i];
        const int *I = h->ipool.p; double *D = h->dpool.p;
        g.n = p.n; g.m = p.m; g.l = p.l; g.eq = p.m > 0; g.ineq = p.l > 0; g.prm = p.prm;
        g.c1 = h->ref ? gen_ref_c1(p.n) : std::pow((double)p.n, 1.0 / 2);                 // std::pow(n, 1.0 / p), p = 2 (SEGcpp:556)
        g.aptr = I + o.aptr; g.aidx = I + o.aidx; g.adiag = I + o.adiag; g.aval = D + o.aval; g.tmval = D + o.tmval;
        g.Cr = GenCsr{I + o.crp, I + o.cri, D + o.crv}; g.Cc = GenCsr{I + o.ccp, I + o.cci, D + o.ccv}; g.Cc_sv = D + o.ccsv;
        g.Er = GenCsr{I + o.erp, I + o.eri, D + o.erv}; g.Ec = GenCsr{I + o.ecp, I + o.eci, D + o.ecv}; g.Ec_sv = D + o.ecsv;
        g.Cnnz = (int)p.C.idx.size(); g.Ennz = (int)p.E.idx.size();
        g.x0 = D + o.x0; g.b = D + o.b; g.d = D + o.d; g.f = D + o.f;
        double *nv = D + o.nvec; const size_t n = (size_t)p.n;
        g.x = nv; g.y1 = nv + n; g.y2 = nv + 2 * n; g.z1 = nv + 3 * n; g.z2 = nv + 4 * n; g.pdiag = nv + 5 * n; g.dinv = nv + 6 * n;
        g.Csq = nv + 7 * n; g.Esq = nv + 8 * n; g.best = nv + 9 * n;
        g.z3 = D + o.z3;
        double *lv = D + o.lvec; const size_t l = (size_t)p.l;
        g.z4 = lv; g.y3 = lv + l; g.fy = lv + 2 * l; g.Ex = lv + 3 * l;
    }
    HIPCHK(hipMemcpy(h->dprob.p, h->hprob.data(), sizeof(GenbProb) * (size_t)h->count, hipMemcpyHostToDevice));
    h->uploaded = true;
    return LPBOX_OK;
}
}  // namespace

extern "C" {

lpbox_bqp_batch_t *lpbox_bqp_batch_create(int count, int device) {
    if (count <= 0) { lpbox_fail(LPBOX_E_BADARG, "count must be positive"); return nullptr; }
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0) { lpbox_fail(LPBOX_E_NODEVICE, "no HIP device available"); return nullptr; }
    lpbox_bqp_batch *h = new lpbox_bqp_batch();
    h->device = device; h->count = count;
    h->prob.resize(count);
    for (auto &p : h->prob) gen_preset(p.prm, 0);
    if (const char *w = getenv("LPBOX_BQP_BATCH_WINDOW")) { const int v = atoi(w); if (v >= 1) h->window = v; }
    return h;
}

void lpbox_bqp_batch_destroy(lpbox_bqp_batch_t *h) {
    if (!h) return;
    if (h->uploaded || h->stream) (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    h->timer.destroy();
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

int lpbox_bqp_batch_preset(lpbox_bqp_batch_t *h, int idx, int type) {
    CHK(check_index(h, idx, true));
    GenParams tmp;
    CHK(gen_preset(tmp, type));
    for (int i = 0; i < h->count; i++) if (idx == -1 || idx == i) h->prob[i].prm = tmp;
    h->uploaded = false;
    return LPBOX_OK;
}

int lpbox_bqp_batch_set_params(lpbox_bqp_batch_t *h, int idx, const double *p11) {
    if (!h || !p11) return lpbox_fail(LPBOX_E_BADHANDLE, "bad handle");
    CHK(check_index(h, idx, true));
    GenParams tmp;
    CHK(gen_set_params(tmp, p11));
    for (int i = 0; i < h->count; i++) if (idx == -1 || idx == i) h->prob[i].prm = tmp;
    h->uploaded = false;
    return LPBOX_OK;
}

int lpbox_bqp_batch_set_problem(lpbox_bqp_batch_t *h, int idx, int n, const int *Ap, const int *Ai, const double *Av, const double *b,
                                const double *x0, int m, const int *Cp, const int *Ci, const double *Cv, const double *d,
                                int l, const int *Ep, const int *Ei, const double *Ev, const double *f) {
    CHK(check_index(h, idx, false));
    if (n > GENB_MAXDIM || m > GENB_MAXDIM || l > GENB_MAXDIM)
        return lpbox_fail(LPBOX_E_TOOLARGE, "problem %d: n = %d, m = %d, l = %d; a batch holds problems with max(n, m, l) <= %d -- use lpbox_bqp_* "
                          "(one problem per handle) for this one", idx, n, m, l, GENB_MAXDIM);
    GenHostProblem tmp;                       // a rejected call leaves the problem that was set before untouched
    CHK(gen_load_problem(tmp, n, Ap, Ai, Av, b, x0, m, Cp, Ci, Cv, d, l, Ep, Ei, Ev, f));
    static_cast<GenHostProblem &>(h->prob[idx]) = std::move(tmp);
    h->prob[idx].set = true;
    h->uploaded = false; h->solved = false;
    return LPBOX_OK;
}

int lpbox_bqp_batch_set_order(lpbox_bqp_batch_t *h, int mode) {
    if (!h) return lpbox_fail(LPBOX_E_BADHANDLE, "bad handle");
    if (mode != LPBOX_ORDER_DEFAULT && mode != LPBOX_ORDER_REFERENCE)
        return lpbox_fail(LPBOX_E_BADARG, "unknown order %d (LPBOX_ORDER_DEFAULT or LPBOX_ORDER_REFERENCE)", mode);
    h->ref = mode == LPBOX_ORDER_REFERENCE;
    h->uploaded = false; h->solved = false;                  // c1 of the descriptors follows the order
    return LPBOX_OK;
}

int lpbox_bqp_batch_solve(lpbox_bqp_batch_t *h, int *iterations) {                 // ADMM_bqp SEGcpp:1384-1832, every problem of the batch
    if (!h) return lpbox_fail(LPBOX_E_BADHANDLE, "bad handle");
    for (int i = 0; i < h->count; i++) if (!h->prob[i].set) return lpbox_fail(LPBOX_E_STATE, "no problem set at index %d", i);
    CHK(use_device(h->device));
    if (!h->stream) {
        HIPCHK(hipStreamCreate(&h->stream));
        HIPCHK(h->timer.create());
    }
    if (!h->uploaded) CHK(upload(h));
    if (h->ref) {                                            // the staging rows of the reference order must fit beside the gathered vectors
        const size_t lds = genb_lds_bytes(h->nmax, h->mmax, h->lmax, true);
        if (lds + GENB_STATIC_LDS > GENB_LDS_LIMIT)
            return lpbox_fail(LPBOX_E_UNSUPPORTED, "reference order: the batch needs %zu B of LDS per workgroup (n <= %d, m <= %d, l <= %d), more than "
                              "%d B", lds + GENB_STATIC_LDS, h->nmax, h->mmax, h->lmax, GENB_LDS_LIMIT);
    }
    h->kernel_ms = 0; h->launches = 0; h->solved = false;
    h->hst.assign(h->count, GenState());
    HIPCHK(h->timer.start(h->stream));
    HIPCHK(genb_launch_init(h->dprob.p, h->dst.p, h->count, h->slots, h->nmax, h->ref, h->stream)); h->launches++;
    for (;;) {
        HIPCHK(genb_launch_window(h->dprob.p, h->dst.p, h->count, h->slots, h->window, h->nmax, h->mmax, h->lmax, h->ref, h->stream)); h->launches++;
        HIPCHK(hipMemcpyAsync(h->hst.data(), h->dst.p, sizeof(GenState) * (size_t)h->count, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        bool all = true;
        for (const GenState &s : h->hst) if (s.halt == GEN_HALT_NONE) { all = false; break; }
        if (all) break;
    }
    HIPCHK(h->timer.stop_sync(h->stream, &h->kernel_ms));
    h->solved = true;
    if (iterations) for (int i = 0; i < h->count; i++) iterations[i] = h->hst[i].iter;
    return LPBOX_OK;
}

int lpbox_bqp_batch_get_vec(lpbox_bqp_batch_t *h, int idx, const char *name, double *out, long cap) {
    if (!h || !h->solved || !h->uploaded || !out || !name) return lpbox_fail(LPBOX_E_STATE, "not solved");
    CHK(check_index(h, idx, false));
    CHK(use_device(h->device));
    const GenbProb &g = h->hprob[idx];
    const double *src = nullptr; long len = g.n;
    if (!strcmp(name, "x")) src = g.x; else if (!strcmp(name, "y1")) src = g.y1; else if (!strcmp(name, "y2")) src = g.y2;
    else if (!strcmp(name, "z1")) src = g.z1; else if (!strcmp(name, "z2")) src = g.z2; else if (!strcmp(name, "best_sol")) src = g.best;
    else if (!strcmp(name, "z3")) { src = g.z3; len = g.m; } else if (!strcmp(name, "z4")) { src = g.z4; len = g.l; }
    else if (!strcmp(name, "y3")) { src = g.y3; len = g.l; }
    else return lpbox_fail(LPBOX_E_BADARG, "unknown vector '%s'", name);
    if (cap < len) return lpbox_fail(LPBOX_E_BADARG, "buffer too small");
    if (len) HIPCHK(hipMemcpy(out, src, sizeof(double) * (size_t)len, hipMemcpyDeviceToHost));
    return (int)len;
}

int lpbox_bqp_batch_get_scalar(lpbox_bqp_batch_t *h, int idx, const char *name, double *out) {
    if (!h || !h->solved || !out || !name) return lpbox_fail(LPBOX_E_STATE, "not solved");
    struct { const char *n; double v; } wide[] = {
        {"kernel_ms", h->kernel_ms}, {"launches", (double)h->launches}, {"threads", (double)GEN_T}, {"chunk", (double)(GEN_T * 2)},
        {"window", (double)h->window}, {"slots", (double)h->slots}, {"order", (double)(h->ref ? LPBOX_ORDER_REFERENCE : LPBOX_ORDER_DEFAULT)},
    };
    for (auto &e : wide) if (!strcmp(e.n, name)) { *out = e.v; return LPBOX_OK; }
    CHK(check_index(h, idx, false));
    const GenState &s = h->hst[idx];
    struct { const char *n; double v; } tab[] = {
        {"rho1", s.rho1}, {"rho3", s.rho3}, {"rho4", s.rho4}, {"gamma", s.gamma_val}, {"std_obj", s.std_obj}, {"cvg1", s.cvg1}, {"cvg2", s.cvg2},
        {"cur_obj", s.cur_obj}, {"best_bin_obj", s.best_bin_obj}, {"obj_val", s.obj_val}, {"iters", (double)s.iter}, {"stop", (double)s.stop},
        {"total_pcg", (double)s.pcg_total}, {"outer_total", (double)s.outer_total}, {"last_pcg", (double)s.last_pcg},
    };
    for (auto &e : tab) if (!strcmp(e.n, name)) { *out = e.v; return LPBOX_OK; }
    return lpbox_fail(LPBOX_E_BADARG, "unknown scalar '%s'", name);
}

}  // extern "C"
