// lpbox_gen_capi.hip -- host side + C-ABI (lpbox_bqp_* in include/lpbox_hip.h) of the GENERIC constrained binary-QP path:
// the reference's ADMM_bqp (SEGcpp:1384-1832) behind its four wrappers ADMM_bqp_unconstrained / _linear_eq / _linear_ineq /
// _linear_eq_and_uneq (SEGcpp:1834-2109).  The kernels are in lpbox_gen_kernels.hip (and, for the opt-in reference summation order of
// lpbox_bqp_set_order, lpbox_gen_ref_kernels.hip); the host loop of the launch chain is chain_run of
// lpbox_host.h with the rules of lpbox_chain.h (CHAIN_RULES_GEN), which also holds the graph cache, the device buffer and the macros.
#include "lpbox_gen_host.h"
#include "lpbox_host.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace {
static_assert(GEN_HALT_NONE == CHAIN_HALT_NONE && GEN_HALT_PCG_MORE == CHAIN_HALT_PCG_MORE, "lpbox_chain.h reads GenState::halt");
constexpr size_t FLOOR = 1;          // this path alone allocates at least one element: its kernels are handed a pointer for empty vectors
struct DevCsr { DevBuf<int> ptr, idx; DevBuf<double> val; GenCsr view() const { return GenCsr{ptr.p, idx.p, val.p}; } };

hipError_t upload(DevCsr &D, const GenHostCsr &H) {
    hipError_t e = D.ptr.upload(H.ptr, FLOOR); if (e != hipSuccess) return e;
    e = D.idx.upload(H.idx, FLOOR); if (e != hipSuccess) return e;
    return D.val.upload(H.val, FLOOR);
}
}  // namespace

struct lpbox_bqp : GenHostProblem {
    int device = 0;
    GenParams prm;
    bool has_problem = false, uploaded = false, solved = false;
    hipStream_t stream = nullptr;
    StreamTimer timer;
    int G = 0, Gm = 0, Gl = 0, EPT = 2, EPTm = 2, EPTl = 2, parity = 0;
    ChainController chain{CHAIN_RULES_GEN};      // kmax, and pcg_resumes of the last lpbox_bqp_solve
    double kernel_ms = 0.0; long long launches = 0, collectives = 0;   // (no collectives on this path)
    GraphCache graphs;                           // of the order in use: lpbox_bqp_set_order clears it
    bool use_graph = true;
    bool ref = false;                            // LPBOX_ORDER_REFERENCE: the staging producers and the walker, c1 through libm's pow
    DevBuf<double> stage;                        // GEN_REF_NSTAGE rows of n, allocated by the first solve in that order
    GenRef rf() const { return GenRef{stage.p}; }
    DevCsr dA, dCr, dCc, dEr, dEc;
    DevBuf<int> d_adiag;
    DevBuf<double> tmval, Cc_sv, Ec_sv, x, xt, y1, y2, z1, z2, db, rhs, r, z, tmp, p0, p1, gsrc, pdiag, dinv, Csq, Esq, best, dx0,
        z3, qC, dd, y3, z4, fy, qE, Ex, df, part, red;
    DevBuf<double2> zp;
    DevBuf<GenState> st;
    GenState hst;

    GenDev dev() const {
        GenDev g;
        g.n = n; g.m = m; g.l = l; g.G = G; g.Gm = Gm; g.Gl = Gl; g.EPT = EPT; g.EPTm = EPTm; g.EPTl = EPTl;
        g.eq = m > 0; g.ineq = l > 0; g.prm = prm;
        g.aptr = dA.ptr.p; g.aidx = dA.idx.p; g.aval = dA.val.p; g.tmval = tmval.p; g.adiag = d_adiag.p;
        g.Cr = dCr.view(); g.Cc = dCc.view(); g.Er = dEr.view(); g.Ec = dEc.view(); g.Cc_sv = Cc_sv.p; g.Ec_sv = Ec_sv.p;
        g.Cnnz = (int)C.idx.size(); g.Ennz = (int)E.idx.size();
        g.x = x.p; g.xt = xt.p; g.y1 = y1.p; g.y2 = y2.p; g.z1 = z1.p; g.z2 = z2.p; g.rhs = rhs.p; g.r = r.p; g.z = z.p; g.tmp = tmp.p;
        g.p0 = p0.p; g.p1 = p1.p; g.gsrc = gsrc.p; g.pdiag = pdiag.p; g.dinv = dinv.p; g.Csq = Csq.p; g.Esq = Esq.p; g.best = best.p;
        g.b = db.p; g.zp = zp.p; g.z3 = z3.p; g.qC = qC.p; g.d = dd.p; g.y3 = y3.p; g.z4 = z4.p; g.fy = fy.p; g.qE = qE.p; g.Ex = Ex.p;
        g.f = df.p; g.part = part.p; g.red = red.p; g.st = st.p;
        return g;
    }
};

namespace {
// the six kernels that feed a reduction have reference-order counterparts (KL); the launch behind each of them is the reduction over
// the workgroup partials or, in reference order, the walk over the staged terms of the state the producer has just written
// (h->parity after its flip).  One launch either way: the `launches` of a solve do not depend on the order.
#define KL(name, ...) (h->ref ? genref_launch_##name(d, h->rf(), ##__VA_ARGS__) : gen_launch_##name(d, ##__VA_ARGS__))
#define FIN(nv, pcg) do { HIPCHK(h->ref ? genref_launch_walk(d, h->rf(), nv, 0, h->parity, pcg, h->stream) : gen_launch_fin(d, nv, h->stream)); \
                          h->launches++; } while (0)
#define ROWS(mode) do { HIPCHK(gen_launch_rows(d, mode, &h->parity, h->stream)); h->launches++; } while (0)

int enqueue_pcg(lpbox_bqp *h, const GenDev &d, int pairs) {
    for (int k = 0; k < pairs; k++) {
        ROWS(1);
        HIPCHK(KL(pcg_cols, &h->parity, h->stream)); h->launches++;
        FIN(1, 1);
        HIPCHK(KL(pcg_upd, &h->parity, h->stream)); h->launches++;
        FIN(2, 1);
    }
    return LPBOX_OK;
}
int enqueue_tail(lpbox_bqp *h, const GenDev &d) {
    HIPCHK(KL(post, &h->parity, h->stream)); h->launches++;
    FIN(7, 0);
    ROWS(0);
    HIPCHK(gen_launch_dual(d, 0, &h->parity, h->stream)); h->launches++;
    return LPBOX_OK;
}
int enqueue_iteration(lpbox_bqp *h, const GenDev &d) {
    HIPCHK(KL(prep, 1, &h->parity, h->stream)); h->launches++;
    FIN(1, 0);
    HIPCHK(gen_launch_y(d, &h->parity, h->stream)); h->launches++;
    HIPCHK(gen_launch_rhs_cols(d, &h->parity, h->stream)); h->launches++;
    ROWS(0);
    HIPCHK(KL(resid, &h->parity, h->stream)); h->launches++;
    FIN(3, 0);
    CHK(enqueue_pcg(h, d, h->chain.kmax));
    return enqueue_tail(h, d);
}
int read_state(lpbox_bqp *h) {
    HIPCHK(hipMemcpyAsync(&h->hst, h->st.p + h->parity, sizeof(GenState), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return LPBOX_OK;
}
// The iteration chain is a static launch sequence (device-side control state, fall-through launches), so chain_run replays it from
// a hipGraph like the large-LP chain: an outer iteration flips the state ping-pong 8 + 3 kmax times, two iterations return to the start
// parity.  Short kernels (n ~ 1e5) are launch-bound without it.
struct GenChainOps {
    lpbox_bqp *h; const GenDev &d;
    int read_state(ChainView &v) { CHK(::read_state(h)); v = chain_view(h->hst); return LPBOX_OK; }
    int resume_pcg() {
        HIPCHK(gen_launch_resume(d, 0, &h->parity, h->stream));
        CHK(enqueue_pcg(h, d, CHAIN_PAIRS_PER_RESUME));
        return enqueue_tail(h, d);
    }
    int batch_head() { HIPCHK(gen_launch_resume(d, 1, &h->parity, h->stream)); return LPBOX_OK; }
    int enqueue(int n) { for (int it = 0; it < n; it++) CHK(enqueue_iteration(h, d)); return LPBOX_OK; }
    int finalize() { HIPCHK(KL(prep, 0, &h->parity, h->stream)); h->launches++; return LPBOX_OK; }
};
}  // namespace

extern "C" {

lpbox_bqp_t *lpbox_bqp_create(int device) {
    lpbox_bqp *h = new lpbox_bqp();
    h->device = device;
    memset(&h->hst, 0, sizeof(h->hst));
    lpbox_bqp_preset(h, 0);
    if (getenv("LPBOX_BQP_NOGRAPH")) h->use_graph = false;
    if (const char *e = getenv("LPBOX_BQP_KMAX")) { int v = atoi(e); if (v >= 1 && v <= 1000) h->chain.force_kmax(v); }
    return h;
}

void lpbox_bqp_destroy(lpbox_bqp_t *h) {
    if (!h) return;
    if (h->uploaded) (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    h->graphs.clear();
    h->timer.destroy();
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

int lpbox_bqp_preset(lpbox_bqp_t *h, int type) {
    if (!h) return lpbox_fail(LPBOX_E_BADHANDLE, "bad handle");
    return gen_preset(h->prm, type);
}

int lpbox_bqp_set_params(lpbox_bqp_t *h, const double *p11) {
    if (!h || !p11) return lpbox_fail(LPBOX_E_BADHANDLE, "bad handle");
    GenParams tmp;                            // a rejected call leaves the parameters as they were
    CHK(gen_set_params(tmp, p11));
    h->prm = tmp;
    return LPBOX_OK;
}

int lpbox_bqp_set_order(lpbox_bqp_t *h, int mode) {
    if (!h) return lpbox_fail(LPBOX_E_BADHANDLE, "bad handle");
    if (mode != LPBOX_ORDER_DEFAULT && mode != LPBOX_ORDER_REFERENCE)
        return lpbox_fail(LPBOX_E_BADARG, "summation order %d: LPBOX_ORDER_DEFAULT or LPBOX_ORDER_REFERENCE", mode);
    const bool ref = mode == LPBOX_ORDER_REFERENCE;
    if (ref == h->ref) return LPBOX_OK;
    if (h->uploaded) {                           // the captured graphs hold the launches of the other order
        CHK(use_device(h->device));
        HIPCHK(hipStreamSynchronize(h->stream));
        h->graphs.clear();
    }
    h->ref = ref;
    h->solved = false;                           // what the getters hold was computed in the other order
    return LPBOX_OK;
}

int lpbox_bqp_set_problem(lpbox_bqp_t *h, int n, const int *Ap, const int *Ai, const double *Av, const double *b, const double *x0,
                          int m, const int *Cp, const int *Ci, const double *Cv, const double *d,
                          int l, const int *Ep, const int *Ei, const double *Ev, const double *f) {
    if (!h) return lpbox_fail(LPBOX_E_BADHANDLE, "bad handle");
    if (h->uploaded) return lpbox_fail(LPBOX_E_STATE, "problem already uploaded; create a new handle");
    GenHostProblem tmp;                       // a rejected call leaves the problem that was set before untouched
    CHK(gen_load_problem(tmp, n, Ap, Ai, Av, b, x0, m, Cp, Ci, Cv, d, l, Ep, Ei, Ev, f));
    static_cast<GenHostProblem &>(*h) = std::move(tmp);
    h->has_problem = true;
    return LPBOX_OK;
}

int lpbox_bqp_solve(lpbox_bqp_t *h, int *iterations) {                              // ADMM_bqp SEGcpp:1384-1832
    if (!h) return lpbox_fail(LPBOX_E_BADHANDLE, "bad handle");
    if (!h->has_problem) return lpbox_fail(LPBOX_E_STATE, "no problem set");
    CHK(use_device(h->device));
    const int n = h->n, m = h->m, l = h->l;
    if (!h->uploaded) {
        auto groups = [](int len, int &ept) { ept = 2; while ((len + GEN_T * ept - 1) / (GEN_T * ept) > 4096 && ept < 64) ept *= 2; return len > 0 ? (len + GEN_T * ept - 1) / (GEN_T * ept) : 0; };
        h->G = groups(n, h->EPT); h->Gm = groups(m, h->EPTm); h->Gl = groups(l, h->EPTl);
        HIPCHK(hipStreamCreate(&h->stream));
        HIPCHK(h->timer.create());
        HIPCHK(upload(h->dA, h->A)); HIPCHK(h->d_adiag.upload(h->adiag, FLOOR)); HIPCHK(h->tmval.alloc(h->A.val.size(), FLOOR));
        HIPCHK(upload(h->dCr, h->C)); HIPCHK(upload(h->dCc, h->Ct)); HIPCHK(h->Cc_sv.alloc(h->Ct.val.size(), FLOOR));
        HIPCHK(upload(h->dEr, h->E)); HIPCHK(upload(h->dEc, h->Et)); HIPCHK(h->Ec_sv.alloc(h->Et.val.size(), FLOOR));
        for (DevBuf<double> *bp : {&h->x, &h->xt, &h->y1, &h->y2, &h->z1, &h->z2, &h->rhs, &h->r, &h->z, &h->tmp, &h->p0, &h->p1, &h->gsrc, &h->pdiag, &h->dinv,
                                &h->Csq, &h->Esq, &h->best})
            HIPCHK(bp->alloc(n, FLOOR));
        HIPCHK(h->zp.alloc(n, FLOOR));
        HIPCHK(h->db.upload(h->b, FLOOR)); HIPCHK(h->dx0.upload(h->x0, FLOOR)); HIPCHK(h->dd.upload(h->d, FLOOR)); HIPCHK(h->df.upload(h->f, FLOOR));
        for (DevBuf<double> *bp : {&h->z3, &h->qC}) HIPCHK(bp->alloc(m, FLOOR));
        for (DevBuf<double> *bp : {&h->y3, &h->z4, &h->fy, &h->qE, &h->Ex}) HIPCHK(bp->alloc(l, FLOOR));
        HIPCHK(h->part.alloc((size_t)GEN_NPART * h->G, FLOOR)); HIPCHK(h->red.alloc(GEN_NPART)); HIPCHK(h->st.alloc(2));
        HIPCHK(hipMemset(h->part.p, 0, sizeof(double) * (size_t)GEN_NPART * h->G));
        HIPCHK(hipMemset(h->red.p, 0, sizeof(double) * GEN_NPART));
        h->uploaded = true;
    }
    if (h->ref && !h->stage.p) HIPCHK(h->stage.alloc((size_t)GEN_REF_NSTAGE * n));
    const GenDev d = h->dev();
    h->parity = 0; h->kernel_ms = 0; h->launches = 0; h->chain.pcg_resumes = 0;
    h->chain.rules.pcg_cap = h->prm.pcg_maxiters;
    HIPCHK(h->timer.start(h->stream));
    // c1 = std::pow(n, 1.0 / p), p = 2 (SEGcpp:556); in the reference's order through libm's pow with an exponent no compiler folds
    HIPCHK(KL(init, h->ref ? gen_ref_c1(n) : std::pow((double)n, 1.0 / 2), h->dx0.p, h->stream));
    HIPCHK(gen_launch_init2(d, h->stream));
    ROWS(0);                                                                        // E x0 for the first y3
    HIPCHK(gen_launch_dual(d, 1, &h->parity, h->stream));
    CHK(chain_run(h->chain, h->graphs, ChainIo{h->stream, h->parity, h->launches, h->collectives, h->use_graph, true}, h->prm.max_iters,
                  GenChainOps{h, d}));
    // best_sol = x_sol of the last improving iteration (:1792) is copied by the NEXT iteration's y kernel; if the loop ended right after an
    // improvement, do it here (x is not touched after the halt)
    if (h->hst.copy_best) HIPCHK(hipMemcpyAsync(h->best.p, h->x.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h->timer.stop_sync(h->stream, &h->kernel_ms));
    h->solved = true;
    if (iterations) *iterations = h->hst.iter;
    return LPBOX_OK;
}

int lpbox_bqp_get_vec(lpbox_bqp_t *h, const char *name, double *out, long cap) {
    if (!h || !h->solved || !out || !name) return lpbox_fail(LPBOX_E_STATE, "not solved");
    CHK(use_device(h->device));
    const double *src = nullptr; long len = h->n;
    if (!strcmp(name, "x")) src = h->x.p; else if (!strcmp(name, "y1")) src = h->y1.p; else if (!strcmp(name, "y2")) src = h->y2.p;
    else if (!strcmp(name, "z1")) src = h->z1.p; else if (!strcmp(name, "z2")) src = h->z2.p; else if (!strcmp(name, "best_sol")) src = h->best.p;
    else if (!strcmp(name, "z3")) { src = h->z3.p; len = h->m; } else if (!strcmp(name, "z4")) { src = h->z4.p; len = h->l; }
    else if (!strcmp(name, "y3")) { src = h->y3.p; len = h->l; }
    else return lpbox_fail(LPBOX_E_BADARG, "unknown vector '%s'", name);
    if (cap < len) return lpbox_fail(LPBOX_E_BADARG, "buffer too small");
    if (len) HIPCHK(hipMemcpy(out, src, sizeof(double) * (size_t)len, hipMemcpyDeviceToHost));
    return (int)len;
}

int lpbox_bqp_get_scalar(lpbox_bqp_t *h, const char *name, double *out) {
    // the order is a setting, not a result: readable at any time, before the first solve and straight after lpbox_bqp_set_order too
    if (h && out && name && !strcmp(name, "order")) { *out = h->ref ? (double)LPBOX_ORDER_REFERENCE : (double)LPBOX_ORDER_DEFAULT; return LPBOX_OK; }
    if (!h || !h->solved || !out || !name) return lpbox_fail(LPBOX_E_STATE, "not solved");
    const GenState &s = h->hst;
    struct { const char *n; double v; } tab[] = {
        {"rho1", s.rho1}, {"rho3", s.rho3}, {"rho4", s.rho4}, {"gamma", s.gamma_val}, {"std_obj", s.std_obj}, {"cvg1", s.cvg1}, {"cvg2", s.cvg2},
        {"cur_obj", s.cur_obj}, {"best_bin_obj", s.best_bin_obj}, {"obj_val", s.obj_val}, {"iters", (double)s.iter}, {"stop", (double)s.stop},
        {"total_pcg", (double)s.pcg_total}, {"outer_total", (double)s.outer_total}, {"last_pcg", (double)s.last_pcg},
        {"kernel_ms", h->kernel_ms}, {"launches", (double)h->launches}, {"threads", (double)GEN_T}, {"chunk", (double)(GEN_T * h->EPT)},
        {"pcg_resumes", (double)h->chain.pcg_resumes}, {"kmax", (double)h->chain.kmax}, {"kmax_kept", (double)h->chain.kept},
        {"graph_revisits", (double)h->graphs.revisits}, {"order", h->ref ? (double)LPBOX_ORDER_REFERENCE : (double)LPBOX_ORDER_DEFAULT},
    };
    for (auto &e : tab) if (!strcmp(e.n, name)) { *out = e.v; return LPBOX_OK; }
    return lpbox_fail(LPBOX_E_BADARG, "unknown scalar '%s'", name);
}

}  // extern "C"
