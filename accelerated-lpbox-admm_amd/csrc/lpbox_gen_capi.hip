// lpbox_gen_capi.hip -- host side + C-ABI (lpbox_bqp_* in include/lpbox_hip.h) of the GENERIC constrained binary-QP path:
// the reference's ADMM_bqp (SEGcpp:1384-1832) behind its four wrappers ADMM_bqp_unconstrained / _linear_eq / _linear_ineq /
// _linear_eq_and_uneq (SEGcpp:1834-2109).  The kernels are in lpbox_gen_kernels.hip (and, for the opt-in reference summation order of
// lpbox_bqp_set_order, lpbox_gen_ref_kernels.hip); the host loop of the launch chain is chain_run of
// lpbox_host.h with the rules of lpbox_chain.h (CHAIN_RULES_GEN), which also holds the graph cache, the device buffer and the macros.
// At the end of the file: a batch of handles through one chain in lockstep (lpbox_bqp_lockstep_*, chain_run_lockstep).
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

// What precedes the chain of a solve, on the handle's own stream (the device is the current one): the upload at the first solve, the
// counters and the timer started, the init launches.  lpbox_bqp_solve goes on with chain_run, a lockstep batch with the chain it shares.
static int gen_begin_solve(lpbox_bqp *h) {
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
    return LPBOX_OK;
}

int lpbox_bqp_solve(lpbox_bqp_t *h, int *iterations) {                              // ADMM_bqp SEGcpp:1384-1832
    if (!h) return lpbox_fail(LPBOX_E_BADHANDLE, "bad handle");
    if (!h->has_problem) return lpbox_fail(LPBOX_E_STATE, "no problem set");
    CHK(use_device(h->device));
    CHK(gen_begin_solve(h));
    const GenDev d = h->dev();
    const int n = h->n;
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

// ---------------------------------------------------------------------------------------------------------------------
// A BATCH of handles through ONE launch chain in lockstep: ADMM_bqp of every member at once, grid (X, B) per
// launch, each member on its own control state -- one that has stopped, reached its own max_iters or whose PCG has converged falls
// through; a GEN_HALT_PCG_MORE on any member resumes the chain for all.  The handles are borrowed and stay ordinary handles: per member
// the arithmetic is that of lpbox_bqp_solve on its own, bit for bit.  Default summation order only.
struct lpbox_bqp_lockstep {
    std::vector<lpbox_bqp *> hs;
    int B = 0, device = 0;
    ChainLockstep chain{CHAIN_RULES_GEN, CHAIN_RULES_GEN.kmax_start};
    int kmax_forced = 0;                            // LPBOX_BQP_KMAX at create (0: adaptive, every solve starts at the rules' kmax)
    bool use_graph = false;                         // LPBOX_BQP_LOCKSTEP_GRAPH
    hipStream_t stream = nullptr;
    StreamTimer timer;
    GraphCache graphs;                              // two iterations per (kmax, start parity), for the member count and extents of `grid`
    GenBatchGrid grid{0, 0, 0, 0};
    DevBuf<GenDev> devs; DevBuf<GenState> dstates;
    std::vector<GenDev> h_devs; std::vector<GenState> h_states;
    std::vector<long long> resumes;                 // per member, of the last solve
    double kernel_ms = 0.0; long long launches = 0, collectives = 0;
    bool solved = false;
};

namespace {

// what a member must be for the lockstep chain; `i` names it in the message.  Checked at create and at every solve: a handle can be
// changed between the calls (lpbox_bqp_set_order).
int genl_member_ok(const lpbox_bqp *h, int i) {
    if (!h || !h->has_problem) return lpbox_fail(LPBOX_E_STATE, "problem %d of the batch has no problem", i);
    if (h->ref) return lpbox_fail(LPBOX_E_UNSUPPORTED, "problem %d of the batch runs in the reference summation order; the batch runs the default order (lpbox_bqp_solve per handle)", i);
    return LPBOX_OK;
}

// The launches of the lockstep chain (chain_run_lockstep) over the members whose descriptors stand in devs: the solo chain's launches,
// launch for launch, so the counts are those of enqueue_iteration / enqueue_pcg / enqueue_tail.  b->h_states[k]: the final states.
struct GenLockstepOps {
    lpbox_bqp_lockstep *b; const GenDev *devs; hipStream_t st; GenBatchGrid g; int &parity;
    int collect(ChainView *v) {
        HIPCHK(genb_collect_states(devs, g, parity, b->dstates.p, st));
        HIPCHK(hipMemcpyAsync(b->h_states.data(), b->dstates.p, sizeof(GenState) * (size_t)g.B, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (int i = 0; i < g.B; i++) v[i] = chain_view(b->h_states[i]);
        return LPBOX_OK;
    }
    int resume_pcg() {
        HIPCHK(genb_launch_resume(devs, g, 0, &parity, st));
        HIPCHK(genb_enqueue_pcg(devs, g, CHAIN_PAIRS_PER_RESUME, &parity, st));
        HIPCHK(genb_enqueue_tail(devs, g, &parity, st));
        b->launches += 5 + 5 * CHAIN_PAIRS_PER_RESUME;
        return LPBOX_OK;
    }
    int batch_head(int, int) { HIPCHK(genb_launch_resume(devs, g, 1, &parity, st)); b->launches += 1; return LPBOX_OK; }
    int enqueue(int n, int kmax) {
        HIPCHK(genb_enqueue_iterations(devs, g, n, kmax, &parity, st));
        b->launches += (long long)n * (16 + 5 * kmax);
        return LPBOX_OK;
    }
    int finalize() { HIPCHK(genb_launch_prep(devs, g, 0, &parity, st)); b->launches += 1; return LPBOX_OK; }
};

}  // namespace

extern "C" {

lpbox_bqp_lockstep_t *lpbox_bqp_lockstep_create(lpbox_bqp_t **handles, int count) {
    auto refuse = [](int) -> lpbox_bqp_lockstep * { return nullptr; };     // lpbox_fail has recorded status and text
    if (!handles || count <= 0) return refuse(lpbox_fail(LPBOX_E_BADARG, "empty batch"));
    if (count > GEN_BATCH_MAX) return refuse(lpbox_fail(LPBOX_E_BADARG, "%d problems: a lockstep batch takes at most %d", count, GEN_BATCH_MAX));
    for (int i = 0; i < count; i++) {                               // no device call
        if (genl_member_ok(handles[i], i) < 0) return nullptr;
        if (handles[i]->device != handles[0]->device) return refuse(lpbox_fail(LPBOX_E_BADARG, "problem %d of the batch lives on another device than problem 0", i));
        for (int k = 0; k < i; k++)
            if (handles[k] == handles[i]) return refuse(lpbox_fail(LPBOX_E_BADARG, "problem %d and problem %d of the batch are the same handle", k, i));
    }
    lpbox_bqp_lockstep *b = new lpbox_bqp_lockstep();
    b->hs.assign(handles, handles + count); b->B = count; b->device = handles[0]->device;
    b->resumes.assign(count, 0);
    if (const char *e = getenv("LPBOX_BQP_KMAX")) { int v = atoi(e); if (v >= 1 && v <= 1000) b->kmax_forced = v; }
    if (const char *e = getenv("LPBOX_BQP_LOCKSTEP_GRAPH")) b->use_graph = atoi(e) != 0;   // replay captured iterations instead of eager launches
    return b;
}

void lpbox_bqp_lockstep_destroy(lpbox_bqp_lockstep_t *b) {
    if (!b) return;
    if (b->stream) {
        (void)hipSetDevice(b->device);
        (void)hipStreamSynchronize(b->stream);
        b->graphs.clear();
        b->timer.destroy();
        (void)hipStreamDestroy(b->stream);
    }
    delete b;
}

// ADMM_bqp (SEGcpp:1384-1832) of every member, each to its own stop; iterations[i] = member i's iteration count
int lpbox_bqp_lockstep_solve(lpbox_bqp_lockstep_t *b, int *iterations) {
    if (!b) return lpbox_fail(LPBOX_E_BADHANDLE, "bad handle");
    for (int i = 0; i < b->B; i++) CHK(genl_member_ok(b->hs[i], i));
    CHK(use_device(b->device));
    b->solved = false;
    // per member, on its own stream: the upload at its first solve and the init launches of lpbox_bqp_solve (a handful, once per solve)
    for (int i = 0; i < b->B; i++) { b->hs[i]->solved = false; CHK(gen_begin_solve(b->hs[i])); }
    for (int i = 0; i < b->B; i++) HIPCHK(hipStreamSynchronize(b->hs[i]->stream));
    if (!b->stream) {
        HIPCHK(hipStreamCreate(&b->stream));
        HIPCHK(b->timer.create());
        HIPCHK(b->devs.alloc(b->B)); HIPCHK(b->dstates.alloc(b->B));
        b->h_devs.resize(b->B); b->h_states.resize(b->B);
    }
    GenBatchGrid g{b->B, 0, 1, 1};
    int iter_end = 0, pcg_cap = 1;
    for (int i = 0; i < b->B; i++) {
        const lpbox_bqp *h = b->hs[i];
        g.cols = std::max(g.cols, h->G); g.y = std::max(g.y, std::max(h->G, h->Gl)); g.rows = std::max(g.rows, std::max(h->Gm, h->Gl));
        iter_end = std::max(iter_end, h->prm.max_iters); pcg_cap = std::max(pcg_cap, h->prm.pcg_maxiters);
        b->h_devs[i] = h->dev();
    }
    if (g.cols != b->grid.cols || g.y != b->grid.y || g.rows != b->grid.rows || g.B != b->grid.B) b->graphs.clear();   // the captured launches carry the grid
    b->grid = g;
    hipStream_t st = b->stream;
    HIPCHK(hipMemcpyAsync(b->devs.p, b->h_devs.data(), sizeof(GenDev) * (size_t)b->B, hipMemcpyHostToDevice, st));
    b->chain.rules = CHAIN_RULES_GEN; b->chain.rules.pcg_cap = pcg_cap;
    b->chain.kmax = b->kmax_forced ? b->kmax_forced : CHAIN_RULES_GEN.kmax_start;       // every solve starts where a fresh handle starts
    b->chain.adaptive = !b->kmax_forced;
    b->launches = 0; b->kernel_ms = 0.0;
    std::fill(b->resumes.begin(), b->resumes.end(), 0);
    int parity = 0;                                 // where gen_begin_solve leaves every member (two flips after the init)
    for (int i = 0; i < b->B; i++)
        if (b->hs[i]->parity != parity) return lpbox_fail(LPBOX_E_STATE, "problem %d of the batch: unexpected state parity after its init", i);
    HIPCHK(b->timer.start(st));
    const int rc = chain_run_lockstep(b->chain, b->B, nullptr, b->graphs, ChainIo{st, parity, b->launches, b->collectives, b->use_graph, true}, iter_end,
                                      b->resumes.data(), GenLockstepOps{b, b->devs.p, st, g, parity});
    if (rc >= 0)
        // best_sol of a member whose loop ended right after an improvement: as lpbox_bqp_solve does behind its loop
        for (int i = 0; i < b->B; i++) {
            const lpbox_bqp *h = b->hs[i];
            if (b->h_states[i].copy_best) HIPCHK(hipMemcpyAsync(h->best.p, h->x.p, sizeof(double) * (size_t)h->n, hipMemcpyDeviceToDevice, st));
        }
    double ms = 0.0;
    const hipError_t e = b->timer.stop_sync(st, &ms);
    if (rc < 0) return rc;
    HIPCHK(e);
    b->kernel_ms = ms;
    for (int i = 0; i < b->B; i++) {
        lpbox_bqp *h = b->hs[i];
        double own = 0.0;
        HIPCHK(h->timer.stop_sync(h->stream, &own));                // (started by gen_begin_solve; the chain's time and launches are the batch's)
        h->hst = b->h_states[i]; h->parity = parity; h->solved = true;
        h->chain.pcg_resumes = b->resumes[i]; h->kernel_ms = 0.0; h->launches = 0;
        if (iterations) iterations[i] = h->hst.iter;
    }
    b->solved = true;
    return LPBOX_OK;
}

int lpbox_bqp_lockstep_get_scalar(lpbox_bqp_lockstep_t *b, const char *name, double *out) {
    if (!b || !name || !out) return lpbox_fail(LPBOX_E_BADHANDLE, "bad handle");
    struct { const char *n; double v; } tab[] = {
        {"count", (double)b->B}, {"launches", (double)b->launches}, {"kernel_ms", b->kernel_ms},
        {"kmax", (double)(b->solved || b->kmax_forced ? b->chain.kmax : CHAIN_RULES_GEN.kmax_start)}, {"graph", b->use_graph ? 1.0 : 0.0},
        {"graph_entries", (double)b->graphs.entries.size()},
        {"grid_cols", (double)b->grid.cols}, {"grid_y", (double)b->grid.y}, {"grid_rows", (double)b->grid.rows},
    };
    for (auto &e : tab) if (!strcmp(e.n, name)) { *out = e.v; return LPBOX_OK; }
    if (!strncmp(name, "pcg_resumes_", 12)) {
        char *end = nullptr;
        const long i = strtol(name + 12, &end, 10);
        if (end != name + 12 && !*end && i >= 0 && i < b->B) { *out = (double)b->resumes[(size_t)i]; return LPBOX_OK; }
    }
    return lpbox_fail(LPBOX_E_BADARG, "unknown scalar '%s'", name);
}

}  // extern "C"
