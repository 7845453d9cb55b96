// lpbox_big_capi.hip -- host side + C-ABI of the LARGE-instance LP path (lpbox_big_* in include/lpbox_hip.h):
// one LP, variable-sharded over ranks (one process per GPU).  The library launches the kernels; where the algorithm needs a
// sum over all variables it calls the caller-supplied all-reduce (RCCL through torch.distributed in lpbox_hip/big.py) on
// the same HIP stream.  With one rank no collective is issued.  The host loops of the launch chains are chain_run (one handle) and
// chain_run_lockstep (a batch) of lpbox_host.h with the rules of lpbox_chain.h (CHAIN_RULES_BIG); the graph cache, the device buffer, the timer and the error-check macros are there too.
#include "../../include/lpbox_hip.h"
#include "lpbox_big.h"
#include "lpbox_capi_internal.h"
#include "lpbox_host.h"

#include <rccl/rccl.h>     // types only: the library is dlopen'ed (no link dependency; a process that has torch loaded shares torch's copy)
#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace {
static_assert(BIG_HALT_NONE == CHAIN_HALT_NONE && BIG_HALT_PCG_MORE == CHAIN_HALT_PCG_MORE, "lpbox_chain.h reads BigState::halt");
static_assert(CHAIN_RULES_BIG.pcg_cap == LP_PCG_MAXITERS, "the resume limit follows the PCG cap of the kernels");
// RCCL entry points, resolved at run time
struct RcclApi {
    void *lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
};
RcclApi g_rccl;

int rccl_load() {
    if (g_rccl.lib) return LPBOX_OK;
    const char *names[] = {getenv("LPBOX_RCCL_LIB"), "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so"};
    void *lib = nullptr;
    for (const char *nm : names) if (nm && *nm && (lib = dlopen(nm, RTLD_NOW | RTLD_GLOBAL))) break;
    if (!lib) return lpbox_fail(LPBOX_E_STATE, "cannot load librccl.so: %s", dlerror());
#define RSYM(field, name) do { *(void **)&g_rccl.field = dlsym(lib, name); if (!g_rccl.field) return lpbox_fail(LPBOX_E_STATE, "librccl.so lacks %s", name); } while (0)
    RSYM(GetUniqueId, "ncclGetUniqueId"); RSYM(CommInitRank, "ncclCommInitRank"); RSYM(CommDestroy, "ncclCommDestroy");
    RSYM(AllGather, "ncclAllGather"); RSYM(Send, "ncclSend"); RSYM(Recv, "ncclRecv");
    RSYM(GroupStart, "ncclGroupStart"); RSYM(GroupEnd, "ncclGroupEnd"); RSYM(GetErrorString, "ncclGetErrorString");
#undef RSYM
    g_rccl.lib = lib;
    return LPBOX_OK;
}
#define NCCLCHK(expr)                                                                                                      \
    do {                                                                                                                   \
        ncclResult_t r_ = (expr);                                                                                          \
        if (r_ != ncclSuccess) return lpbox_fail(LPBOX_E_HIP, "%s failed: %s", #expr, g_rccl.GetErrorString(r_));          \
    } while (0)
}  // namespace

struct lpbox_big {
    int rank = 0, world = 1, device = 0;
    long n_glob = 0; int c0 = 0, n_loc = 0, l = 0, nnz = 0;
    std::vector<int> cptr, crow, rptr, rcol;
    std::vector<double> b, f;
    bool has_problem = false, uploaded = false, inited = false, own_stream = false;
    hipStream_t stream = nullptr;
    StreamTimer timer;
    lpbox_allgather_fn ag = nullptr; void *ag_user = nullptr;   // exchange through the caller (tests: gloo) ...
    ncclComm_t comm = nullptr;                                  // ... or through RCCL, driven from here (no Python in the loop)
    long q_cap = 0;                                             // doubles allocated behind q (l rounded up to a multiple of world)
    // launch-bound inner loop: two outer iterations captured once per (PCG launch count, start parity) and replayed
    GraphCache graphs;
    bool use_graph = true;
    ChainController chain{CHAIN_RULES_BIG};                     // kmax; margin: LPBOX_BIG_KMARGIN
    int G = 0, Gl = 0, EPT = 2, EPTl = 2, P = 1, Glr = 0, parity = 0;
    bool fold = false; int Gs = 0, Gr[BIG_MAXW] = {0};        // folded reductions (BigDev::fold): partial stride, workgroups of every rank
    DevBuf<double> gpart;                                          // W > 1, folded: the gathered partials [phase][rank][nv][Gs]
    bool lean = false;                                          // lpbox_big_set_pcg_mode(LPBOX_PCG_COMM_LEAN), before lpbox_big_init
    int Gq = 0, Gqs = 0, Gqr[BIG_MAXW] = {0};                   // q.q partials: of this rank, stride, of every rank (BigDev::Gq)
    DevBuf<double> lsmall, gsmall;
    double kernel_ms = 0.0; long long launches = 0, collectives = 0;
    DevBuf<int> d_rptr, d_rcol, d_cptr, d_crow;
    DevBuf<double> x, y1, y2, z1, z2, db, pd, dinv, rhs, r, z, tmp, p0, p1, gsrc, y3, z4, df, Ex, q, part, red, xt, xhist, xi_out, gath, flag;
    DevBuf<uint8_t> live, newfix;
    DevBuf<double2> zp, fz;
    DevBuf<int> d_live_idx;
    std::vector<int> left_idx, xi_left;   // local indices of the live variables (now / as of the last l2f window)
    long n_live_glob = 0;                 // live variables over all ranks
    int ws_cap = 0, xi_rows = 0;
    bool xi_valid = false;
    // a batch's device-decided fix (lpbox_big_batch_iterate_l2f_scores) compacts d_live_idx on the device: left_idx then follows on demand
    // (refresh_left).  dlive_valid: d_live_idx holds the current live list.  win_serial counts the windows (a batch's pack refers to one).
    bool left_stale = false, dlive_valid = false;
    long win_serial = 0;
    bool record = false, xi_plain = false;   // lpbox_big_set_record: the plain loop stages every iterate; the last staged window came from it
    DevBuf<BigState> st;
    BigState hst;
    // reference-order mode (lpbox_big_set_order): one rank, one column slice, no folded reductions; see BigRef in lpbox_big.h
    bool ref = false, valued = false;
    std::vector<double> vals, vcsr_h;     // stored values of E in the order of crow / rcol (empty: a unit instance)
    DevBuf<double> d_vcsc, d_vcsr, r4v, stage;
    DevBuf<int> d_rank, d_frank, d_cnt;

    BigRef rfd;
    const BigRef *rf() {                  // what the big_launch_* helpers take: nullptr in the default order
        if (!ref) return nullptr;
        BigRef &r = rfd;
        r.valued = valued ? 1 : 0; r.vcsr = d_vcsr.p; r.vcsc = d_vcsc.p; r.r4v = r4v.p; r.stage = stage.p;
        r.rank = d_rank.p; r.frank = d_frank.p; r.cnt = d_cnt.p;
        return &r;
    }

    BigDev dev() const {
        BigDev d;
        d.n_loc = n_loc; d.l = l; d.G = G; d.Gl = Gl; d.EPT = EPT; d.EPTl = EPTl; d.P = P; d.Glr = Glr; d.n_glob = n_glob;
        d.rptr = d_rptr.p; d.rcol = d_rcol.p; d.cptr = d_cptr.p; d.crow = d_crow.p;
        d.x = x.p; d.y1 = y1.p; d.y2 = y2.p; d.z1 = z1.p; d.z2 = z2.p; d.b = db.p; d.pd = pd.p; d.dinv = dinv.p; d.rhs = rhs.p;
        d.r = r.p; d.z = z.p; d.tmp = tmp.p; d.p0 = p0.p; d.p1 = p1.p; d.gsrc = gsrc.p;
        d.zp = zp.p; d.xt = xt.p; d.live = live.p; d.newfix = newfix.p; d.xhist = xhist.p; d.ws_cap = ws_cap;
        d.y3 = y3.p; d.z4 = z4.p; d.f = df.p; d.fz = fz.p; d.Ex = Ex.p; d.q = q.p; d.part = part.p; d.red = red.p; d.st = st.p;
        d.fold = fold ? 1 : 0; d.W = world; d.Gs = Gs; d.gpart = gpart.p; d.gathered = gpart.p != nullptr;
        for (int r = 0; r < BIG_MAXW; r++) { d.Gr[r] = Gr[r]; d.Gqr[r] = Gqr[r]; }
        d.lean = lean ? 1 : 0; d.Gq = Gq; d.Gqs = Gqs; d.lsmall = lsmall.p; d.gsmall = gsmall.p;
        return d;
    }
};

namespace {

// In-place sum of `count` doubles at ptr over all ranks with a FIXED association: element i = ((c0[i] + c1[i]) + c2[i]) + ...
// in rank order, whatever the transport -- so a W-rank run is reproducible and comparable bit for bit with the oracle's model of
// the rank partition (oracle/lpbox_oracle.c lpo_set_ranks).  Transport: RCCL driven from here (vectors: exchange of row blocks
// = reduce-scatter with our own adds, then an all-gather of the reduced blocks; scalars: one all-gather), or the caller's
// all-gather callback (tests: gloo).  One rank without a transport: nothing to do.
int allreduce(lpbox_big *h, double *ptr, long count) {
    if (!h->comm && !h->ag) {
        if (h->world > 1) return lpbox_fail(LPBOX_E_STATE, "world = %d but neither an RCCL communicator nor an all-gather callback was set", h->world);
        return LPBOX_OK;
    }
    const int W = h->world;
    if (h->comm && count > 64) {
        const long lb = (count + W - 1) / W;                        // row block per rank (ptr has room for W * lb doubles)
        if ((long)W * lb > h->q_cap || ptr != h->q.p) return lpbox_fail(LPBOX_E_STATE, "vector exchange outside the padded buffer");
        NCCLCHK(g_rccl.GroupStart());
        for (int pr = 0; pr < W; pr++) {
            NCCLCHK(g_rccl.Send(ptr + (long)pr * lb, (size_t)lb, ncclDouble, pr, h->comm, h->stream));
            NCCLCHK(g_rccl.Recv(h->gath.p + (long)pr * lb, (size_t)lb, ncclDouble, pr, h->comm, h->stream));
        }
        NCCLCHK(g_rccl.GroupEnd());
        HIPCHK(big_launch_rank_sum(h->gath.p, W, lb, lb, ptr + (long)h->rank * lb, h->stream));
        NCCLCHK(g_rccl.AllGather(ptr + (long)h->rank * lb, ptr, (size_t)lb, ncclDouble, h->comm, h->stream));
        h->collectives += 2;
        return LPBOX_OK;
    }
    if (h->comm) NCCLCHK(g_rccl.AllGather(ptr, h->gath.p, (size_t)count, ncclDouble, h->comm, h->stream));
    else {
        const int rc = h->ag(ptr, count, h->gath.p, h->ag_user);
        if (rc != 0) return lpbox_fail(LPBOX_E_HIP, "all-gather callback failed (%d)", rc);
    }
    HIPCHK(big_launch_rank_sum(h->gath.p, W, count, count, ptr, h->stream));
    h->collectives++;
    return LPBOX_OK;
}

// the host's live list after a fix that was decided on the device: one copy of the device's list, where the host list is read
int refresh_left(lpbox_big *h) {
    if (!h->left_stale) return LPBOX_OK;
    CHK(use_device(h->device));
    h->left_idx.resize((size_t)h->n_live_glob);
    if (h->n_live_glob) HIPCHK(hipMemcpy(h->left_idx.data(), h->d_live_idx.p, sizeof(int) * (size_t)h->n_live_glob, hipMemcpyDeviceToHost));
    h->left_stale = false;
    return LPBOX_OK;
}

// every rank learns whether ANY rank wants to bail out, before a state-changing collective is entered (a rank that returned early
// on its own would leave the others waiting inside the next exchange)
int agree_ok(lpbox_big *h, bool ok_here) {
    if (!h->comm && !h->ag) return ok_here ? LPBOX_OK : -1;
    const double v = ok_here ? 0.0 : 1.0;
    HIPCHK(hipMemcpyAsync(h->flag.p, &v, sizeof(double), hipMemcpyHostToDevice, h->stream));
    int rc = allreduce(h, h->flag.p, 1);
    if (rc < 0) return rc;
    double tot = 0.0;
    HIPCHK(hipMemcpyAsync(&tot, h->flag.p, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return tot == 0.0 ? LPBOX_OK : -1;
}

// c1 = pow(n, 1/p), p = 2 (LPcpp:427,503) through libm's pow, as the reference and the oracle call it: with the literal exponent the
// compiler turns the call into sqrt, and glibc's pow is not correctly rounded (n = 2921: one ulp apart).  Reference order only; the
// default order keeps the expression it has always had.
static double ref_c1(long n) {
    volatile double e = 1.0 / 2;
    return std::pow((double)n, e);
}
// the totals of a phase's workgroup partials for its consumers.  Folded route: the consumers add them up themselves; only W > 1 ranks
// have something to do here -- ONE all-gather of the partials (nv * Gs doubles per rank), no reduction launch, no rank-sum launch.
// Other route: the reduction launch leaves them in red[], all-reduced over the ranks in rank order.
int gather_partials(lpbox_big *h, const BigDev &d, int phase, int nv) {
    const size_t PS = (size_t)BIG_NPART * h->Gs;
    double *src = h->part.p + (size_t)phase * PS, *dst = h->gpart.p + (size_t)phase * h->world * PS;
    const long count = (long)nv * h->Gs;
    if (h->comm) NCCLCHK(g_rccl.AllGather(src, dst, (size_t)count, ncclDouble, h->comm, h->stream));
    else if (h->ag) {
        const int rc = h->ag(src, count, dst, h->ag_user);
        if (rc != 0) return lpbox_fail(LPBOX_E_HIP, "all-gather callback failed (%d)", rc);
    } else return lpbox_fail(LPBOX_E_STATE, "world = %d but neither an RCCL communicator nor an all-gather callback was set", h->world);
    h->collectives++;
    return LPBOX_OK;
}
// reference order: the walker in the place of the reduction launch (no folding, one rank); every other launch of the chain is the same
// big_launch_* call in both orders, with h->rf()
#define WALK(nv, phase, which, sidx) do { HIPCHK(bigref_launch_walk(d, *h->rf(), nv, phase, which, sidx, h->stream)); h->launches++; } while (0)
#define FIN(nv, phase) do { if (h->ref) WALK(nv, phase, 0, h->parity); else if (h->fold) { if (h->gpart.p) CHK(gather_partials(h, d, phase, nv)); } \
                            else { HIPCHK(big_launch_fin(d, nv, phase, h->stream)); h->launches++; CHK(allreduce(h, d.red + (phase) * BIG_NPART, nv)); } } while (0)
#define FINX(nv) do { HIPCHK(big_launch_fin(d, nv, BIG_PH_X, h->stream)); h->launches++; CHK(allreduce(h, d.red + BIG_PH_X * BIG_NPART, nv)); } while (0)
#define ROWS(mode) do { HIPCHK(big_launch_rows(d, h->rf(), mode, &h->parity, h->stream)); h->launches++; CHK(allreduce(h, d.q, h->l)); } while (0)

// comm-lean PCG, W > 1: the q exchange of allreduce() with the scalars riding along -- the row blocks go to their owners (one grouped
// send/recv), the owner adds its block in rank order and squares it (big_k_rank_sum_qq: q.q partials behind the p.p partials the row
// kernel left in lsmall), then ONE grouped all-gather brings back the reduced blocks and everybody's partials.
int exchange_q_lean(lpbox_big *h, const BigDev &d) {
    const int W = h->world;
    const long lb = ((long)h->l + W - 1) / W;
    const long lo = std::min<long>((long)h->rank * lb, h->l), mine = std::min<long>(lb, h->l - lo);
    const size_t small = (size_t)h->Gs + h->Gqs;
    if (h->comm) {
        NCCLCHK(g_rccl.GroupStart());
        for (int pr = 0; pr < W; pr++) {
            NCCLCHK(g_rccl.Send(h->q.p + (long)pr * lb, (size_t)lb, ncclDouble, pr, h->comm, h->stream));
            NCCLCHK(g_rccl.Recv(h->gath.p + (long)pr * lb, (size_t)lb, ncclDouble, pr, h->comm, h->stream));
        }
        NCCLCHK(g_rccl.GroupEnd());
        HIPCHK(big_launch_rank_sum_qq(h->gath.p, W, mine, lb, h->q.p + (long)h->rank * lb, h->lsmall.p + h->Gs, h->stream));
        NCCLCHK(g_rccl.GroupStart());
        NCCLCHK(g_rccl.AllGather(h->q.p + (long)h->rank * lb, h->q.p, (size_t)lb, ncclDouble, h->comm, h->stream));
        NCCLCHK(g_rccl.AllGather(h->lsmall.p, h->gsmall.p, small, ncclDouble, h->comm, h->stream));
        NCCLCHK(g_rccl.GroupEnd());
        h->collectives += 2;
        return LPBOX_OK;
    }
    if (!h->ag) return lpbox_fail(LPBOX_E_STATE, "world = %d but neither an RCCL communicator nor an all-gather callback was set", W);
    // callback transport (tests): whole contributions are gathered, every rank adds all rows in rank order; only its own block's squares count
    int rc = h->ag(h->q.p, h->l, h->gath.p, h->ag_user);
    if (rc != 0) return lpbox_fail(LPBOX_E_HIP, "all-gather callback failed (%d)", rc);
    HIPCHK(big_launch_rank_sum(h->gath.p, W, h->l, h->l, h->q.p, h->stream));
    HIPCHK(big_launch_rank_sum_qq(h->gath.p + lo, W, mine, h->l, h->q.p + lo, h->lsmall.p + h->Gs, h->stream));
    rc = h->ag(h->lsmall.p, (long)small, h->gsmall.p, h->ag_user);
    if (rc != 0) return lpbox_fail(LPBOX_E_HIP, "all-gather callback failed (%d)", rc);
    h->collectives += 2;
    return LPBOX_OK;
}

int enqueue_pcg(lpbox_big *h, const BigDev &d, int pairs) {
    if (h->lean) {
        for (int k = 0; k < pairs; k++) {
            HIPCHK(big_launch_rows(d, h->rf(), 1, &h->parity, h->stream)); h->launches++;
            if (h->world > 1 || h->comm) CHK(exchange_q_lean(h, d));
            HIPCHK(big_launch_pcg_lean(d, &h->parity, h->stream)); h->launches++;
            FIN(2, BIG_PH_D);
        }
        return LPBOX_OK;
    }
    for (int k = 0; k < pairs; k++) {
        ROWS(1);
        HIPCHK(big_launch_pcg_cols(d, h->rf(), &h->parity, h->stream)); h->launches++;
        FIN(1, BIG_PH_C);
        HIPCHK(big_launch_pcg_upd(d, h->rf(), &h->parity, h->stream)); h->launches++;
        FIN(2, BIG_PH_D);
    }
    return LPBOX_OK;
}

int enqueue_tail(lpbox_big *h, const BigDev &d) {
    HIPCHK(big_launch_post(d, h->rf(), &h->parity, h->stream)); h->launches++;
    FIN(5, BIG_PH_E);
    ROWS(0);
    HIPCHK(big_launch_z4(d, 0, &h->parity, h->stream)); h->launches++;
    return LPBOX_OK;
}

int enqueue_iteration(lpbox_big *h, const BigDev &d) {
    HIPCHK(big_launch_prep(d, h->rf(), 1, &h->parity, h->stream)); h->launches++;
    FIN(1, BIG_PH_A);
    HIPCHK(big_launch_y(d, h->rf(), &h->parity, h->stream)); h->launches++;
    HIPCHK(big_launch_rhs_cols(d, h->rf(), &h->parity, h->stream)); h->launches++;
    ROWS(0);
    HIPCHK(big_launch_resid(d, h->rf(), &h->parity, h->stream)); h->launches++;
    FIN(3, BIG_PH_B);
    CHK(enqueue_pcg(h, d, h->chain.kmax));
    return enqueue_tail(h, d);
}

int read_state(lpbox_big *h) {
    HIPCHK(hipMemcpyAsync(&h->hst, h->st.p + h->parity, sizeof(BigState), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return LPBOX_OK;
}

// An outer iteration is 8 + 3*kmax launches that flip the state ping-pong, so two iterations return to the parity they started
// from: chain_run captures one hipGraph of two iterations per (kmax, start parity).  The caller's all-gather callback cannot be
// captured (it runs host code at enqueue time); RCCL operations and the single-rank chain can.
struct BigChainOps {
    lpbox_big *h; const BigDev &d;
    int read_state(ChainView &v) { CHK(::read_state(h)); v = chain_view(h->hst); return LPBOX_OK; }
    int resume_pcg() {
        HIPCHK(big_launch_resume(d, 0, &h->parity, h->stream));
        CHK(enqueue_pcg(h, d, CHAIN_PAIRS_PER_RESUME));
        return enqueue_tail(h, d);
    }
    int batch_head() { HIPCHK(big_launch_resume(d, 1, &h->parity, h->stream)); return LPBOX_OK; }
    int enqueue(int n) { for (int it = 0; it < n; it++) CHK(enqueue_iteration(h, d)); return LPBOX_OK; }
    int finalize() { HIPCHK(big_launch_prep(d, h->rf(), 0, &h->parity, h->stream)); h->launches++; return LPBOX_OK; }
};

}  // namespace

extern "C" {

lpbox_big_t *lpbox_big_create(int rank, int world, int device) {
    if (world < 1 || rank < 0 || rank >= world) { lpbox_fail(LPBOX_E_BADARG, "bad rank/world %d/%d", rank, world); return nullptr; }
    lpbox_big *h = new lpbox_big();
    h->rank = rank; h->world = world; h->device = device;
    memset(&h->hst, 0, sizeof(h->hst));
    if (getenv("LPBOX_BIG_NOGRAPH")) h->use_graph = false;                        // eager launches (profilers that dislike graphs)
    if (const char *e = getenv("LPBOX_BIG_KMAX")) { int v = atoi(e); if (v >= 1 && v <= 1000) h->chain.force_kmax(v); }
    return h;
}

void lpbox_big_destroy(lpbox_big_t *h) {
    if (!h) return;
    if (h->uploaded) (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    h->graphs.clear();
    if (h->comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(h->comm);
    h->timer.destroy();
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

int lpbox_big_set_stream(lpbox_big_t *h, void *hip_stream) {
    if (!h) return lpbox_fail(LPBOX_E_BADHANDLE, "bad handle");
    if (h->own_stream && h->stream) { (void)hipStreamDestroy(h->stream); h->own_stream = false; }
    h->stream = (hipStream_t)hip_stream;
    return LPBOX_OK;
}

// The plain loop's per-iteration dump (print_fix_info 2, LPcpp:777-780, :903-909) behind the size hand-over: the next lpbox_big_iterate
// calls keep x after every iteration in the staging buffer the l2f window uses ([iterations][n_loc] on the device); read it back with
// lpbox_big_get_x_iters(ws = iterations of the call).  Refused per call when the buffer would exceed 4 GiB.
int lpbox_big_set_record(lpbox_big_t *h, int on) {
    if (!h) return lpbox_fail(LPBOX_E_BADHANDLE, "bad handle");
    h->record = on != 0;
    return LPBOX_OK;
}

// Opt-in, NOT the reference's arithmetic: the PCG's step length from p.Mp = dI (p.p) + r4Et (q.q) with q = E p, which
// lets the p.p partials ride with the q exchange and fuses the column product with the vector updates -- 3 instead of 4 RCCL operations and
// 2 instead of 3 kernels per PCG iteration.  Before lpbox_big_init; needs the folded reductions (<= 1024 workgroups, <= 16 ranks).
int lpbox_big_set_pcg_mode(lpbox_big_t *h, int mode) {
    if (!h) return lpbox_fail(LPBOX_E_BADHANDLE, "bad handle");
    if (h->inited) return lpbox_fail(LPBOX_E_STATE, "set the PCG mode before lpbox_big_init");
    if (mode != LPBOX_PCG_REFERENCE && mode != LPBOX_PCG_COMM_LEAN) return lpbox_fail(LPBOX_E_BADARG, "unknown PCG mode %d", mode);
    if (h->ref && mode == LPBOX_PCG_COMM_LEAN) return lpbox_fail(LPBOX_E_UNSUPPORTED, "the comm-lean PCG is not the reference's arithmetic: not available in the reference summation order");
    h->lean = mode == LPBOX_PCG_COMM_LEAN;
    return LPBOX_OK;
}

int lpbox_big_set_allgather(lpbox_big_t *h, lpbox_allgather_fn fn, void *user) {
    if (!h) return lpbox_fail(LPBOX_E_BADHANDLE, "bad handle");
    // the exchange buffers are sized by lpbox_big_init from the transport that is set then (as for lpbox_big_rccl_init)
    if (h->inited) return lpbox_fail(LPBOX_E_STATE, "set the all-gather callback before lpbox_big_init");
    if (h->ref && fn) return lpbox_fail(LPBOX_E_UNSUPPORTED, "the reference summation order runs on one rank without a transport");
    h->ag = fn; h->ag_user = user;
    return LPBOX_OK;
}

int lpbox_big_rccl_unique_id(void *out128) {
    if (!out128) return lpbox_fail(LPBOX_E_BADARG, "null output");
    int rc = rccl_load();
    if (rc < 0) return rc;
    ncclUniqueId id;
    NCCLCHK(g_rccl.GetUniqueId(&id));
    memcpy(out128, &id, sizeof(id));
    return (int)sizeof(id);
}

int lpbox_big_rccl_init(lpbox_big_t *h, const void *unique_id128) {
    if (!h || !unique_id128) return lpbox_fail(LPBOX_E_BADHANDLE, "bad handle / id");
    if (h->comm) return lpbox_fail(LPBOX_E_STATE, "communicator already created");
    if (h->ref) return lpbox_fail(LPBOX_E_UNSUPPORTED, "the reference summation order runs on one rank without a transport");
    if (h->inited) return lpbox_fail(LPBOX_E_STATE, "the communicator must be created before solve_init");
    int rc = rccl_load();
    if (rc < 0) return rc;
    rc = use_device(h->device);
    if (rc < 0) return rc;
    ncclUniqueId id;
    memcpy(&id, unique_id128, sizeof(id));
    NCCLCHK(g_rccl.CommInitRank(&h->comm, h->world, id, h->rank));
    return LPBOX_OK;
}

// Opt-in: the reference's summation order on this path, one rank.  Before lpbox_big_set_problem.
int lpbox_big_set_order(lpbox_big_t *h, int mode) {
    if (!h) return lpbox_fail(LPBOX_E_BADHANDLE, "bad handle");
    if (mode != LPBOX_ORDER_DEFAULT && mode != LPBOX_ORDER_REFERENCE) return lpbox_fail(LPBOX_E_BADARG, "unknown summation order %d", mode);
    if (h->has_problem || h->uploaded || h->inited) return lpbox_fail(LPBOX_E_STATE, "set the summation order before lpbox_big_set_problem");
    if (mode == LPBOX_ORDER_REFERENCE) {
        if (h->world != 1) return lpbox_fail(LPBOX_E_UNSUPPORTED, "the reference summation order runs on one rank (world = %d)", h->world);
        if (h->comm || h->ag) return lpbox_fail(LPBOX_E_UNSUPPORTED, "the reference summation order runs on one rank without a transport");
        if (h->lean) return lpbox_fail(LPBOX_E_UNSUPPORTED, "the comm-lean PCG is not the reference's arithmetic: not available in the reference summation order");
    }
    h->ref = mode == LPBOX_ORDER_REFERENCE;
    return LPBOX_OK;
}

static int big_set_problem(lpbox_big_t *h, long n_glob, int c0, int n_loc, int l, const int *colptr, const int *rowidx,
                           const double *b, const double *f, const double *vals);

int lpbox_big_set_problem(lpbox_big_t *h, long n_glob, int c0, int n_loc, int l, const int *colptr, const int *rowidx,
                          const double *b, const double *f) {
    return big_set_problem(h, n_glob, c0, n_loc, l, colptr, rowidx, b, f, nullptr);
}

// lpbox_big_set_problem plus the stored values of E in the order of rowidx (NULL: ones).  Any finite value; an explicit zero stays a
// stored entry; values that are all exactly 1.0 make a unit instance.  A default-order handle takes unit values only.
int lpbox_big_set_problem_vals(lpbox_big_t *h, long n_glob, int c0, int n_loc, int l, const int *colptr, const int *rowidx,
                               const double *b, const double *f, const double *vals) {
    return big_set_problem(h, n_glob, c0, n_loc, l, colptr, rowidx, b, f, vals);
}

static int big_set_problem(lpbox_big_t *h, long n_glob, int c0, int n_loc, int l, const int *colptr, const int *rowidx,
                           const double *b, const double *f, const double *vals) {
    if (!h) return lpbox_fail(LPBOX_E_BADHANDLE, "bad handle");
    if (h->uploaded) return lpbox_fail(LPBOX_E_STATE, "problem already uploaded");
    if (n_glob <= 0 || n_loc <= 0 || l <= 0 || c0 < 0 || (long)c0 + n_loc > n_glob || !colptr || !b || colptr[0] != 0)
        return lpbox_fail(LPBOX_E_BADARG, "bad problem arguments");
    const int nnz = colptr[n_loc];
    if (nnz < 0 || (nnz > 0 && !rowidx)) return lpbox_fail(LPBOX_E_BADARG, "row indices missing");
    for (int j = 0; j < n_loc; j++) {
        if (colptr[j] < 0 || colptr[j + 1] < colptr[j] || colptr[j + 1] > nnz) return lpbox_fail(LPBOX_E_BADARG, "colptr not monotone inside [0, nnz]");
        for (int k = colptr[j]; k < colptr[j + 1]; k++) {
            if (rowidx[k] < 0 || rowidx[k] >= l) return lpbox_fail(LPBOX_E_BADARG, "row index out of range");
            if (k > colptr[j] && rowidx[k] <= rowidx[k - 1]) return lpbox_fail(LPBOX_E_BADARG, "row indices must ascend inside a column");
        }
    }
    bool valued = false;
    if (vals) {
        for (int k = 0; k < nnz; k++) {
            if (!std::isfinite(vals[k])) return lpbox_fail(LPBOX_E_BADARG, "stored value %d of E is not finite", k);
            if (vals[k] != 1.0) valued = true;
        }
        if (valued && !h->ref)
            return lpbox_fail(LPBOX_E_UNSUPPORTED, "stored values of E other than 1 need the reference summation order: call lpbox_big_set_order(h, LPBOX_ORDER_REFERENCE) first");
    }
    for (int j = 0; j < n_loc; j++)              // as lpbox_set_problem_lp: a non-finite objective entry never reaches the device
        if (!std::isfinite(b[j])) return lpbox_fail(LPBOX_E_BADARG, "b has a non-finite entry (local index %d, global %ld)", j, (long)c0 + j);
    h->valued = valued;
    h->n_glob = n_glob; h->c0 = c0; h->n_loc = n_loc; h->l = l; h->nnz = nnz;
    h->cptr.assign(colptr, colptr + n_loc + 1); h->crow.assign(rowidx, rowidx + nnz);
    // Row-side storage, slice-major (lpbox_big_kernels.hip row_sum_sliced): the columns are cut into P slices of SW columns so that
    // one slice of the gathered (z, p) table (16 B per variable) stays resident in an XCD's L2; run (slice ph, row i) starts at
    // rptr[ph * l + i] and the runs follow each other.  P = 1 (a shard that fits anyway, or LPBOX_BIG_SLICE_KB=0) is plain CSR.
    long slice_kb = 2048;
    if (const char *e = getenv("LPBOX_BIG_SLICE_KB")) slice_kb = atol(e);
    long SW = slice_kb > 0 ? std::max<long>(1024, slice_kb * 1024 / 16) : (long)n_loc;
    int P = (int)std::min<long>(((long)n_loc + SW - 1) / SW, 64);
    if (P <= 1) { P = 1; SW = n_loc; } else SW = ((long)n_loc + P - 1) / P;
    if ((size_t)P * (size_t)l + 1 > (size_t)INT32_MAX) { P = 1; SW = n_loc; }
    if (h->ref) { P = 1; SW = n_loc; }          // reference order: one lane sums the whole row; LPBOX_BIG_SLICE_KB is ignored
    h->P = P;
    h->rptr.assign((size_t)P * l + 1, 0);
    for (int j = 0; j < n_loc; j++) {
        const size_t base = (size_t)(j / SW) * l + 1;
        for (int k = colptr[j]; k < colptr[j + 1]; k++) h->rptr[base + rowidx[k]]++;
    }
    for (size_t i = 0; i < (size_t)P * l; i++) h->rptr[i + 1] += h->rptr[i];
    h->rcol.assign(nnz, 0);
    h->vals.clear(); h->vcsr_h.clear();
    if (valued) { h->vals.assign(vals, vals + nnz); h->vcsr_h.assign(nnz, 1.0); }
    std::vector<int> cur(h->rptr.begin(), h->rptr.end() - 1);
    for (int j = 0; j < n_loc; j++) {
        const size_t base = (size_t)(j / SW) * l;
        for (int k = colptr[j]; k < colptr[j + 1]; k++) {
            const int pos = cur[base + rowidx[k]]++;
            h->rcol[pos] = j;
            if (valued) h->vcsr_h[pos] = vals[k];
        }
    }
    h->b.assign(b, b + n_loc);
    if (f) h->f.assign(f, f + l); else h->f.assign(l, 1.0);
    h->has_problem = true;
    return LPBOX_OK;
}

int lpbox_big_init(lpbox_big_t *h) {
    if (!h) return lpbox_fail(LPBOX_E_BADHANDLE, "bad handle");
    if (!h->has_problem) return lpbox_fail(LPBOX_E_STATE, "no problem set");
    if (h->ref && (h->world != 1 || h->comm || h->ag || h->lean))
        return lpbox_fail(LPBOX_E_UNSUPPORTED, "the reference summation order runs on one rank, without a transport and with the reference's PCG");
    CHK(use_device(h->device));
    if (!h->uploaded) {
        const int n = h->n_loc, l = h->l;
        if (!h->stream) { HIPCHK(hipStreamCreate(&h->stream)); h->own_stream = true; }
        HIPCHK(h->flag.alloc(64));
        h->q_cap = (long)h->world * (((long)l + h->world - 1) / h->world);           // whole row blocks for the exchange
        if (h->comm) HIPCHK(h->gath.alloc((size_t)std::max<long>(h->q_cap, 64L * h->world)));          // W row blocks, or W scalar groups
        else if (h->ag) HIPCHK(h->gath.alloc((size_t)h->world * (size_t)std::max(l, 64)));              // W whole contributions
        // every rank learns the shard sizes of all ranks: the slots per thread (hence the partial stride) must be the same everywhere
        std::vector<double> nloc_all((size_t)std::max(h->world, 1), 0.0);
        nloc_all[h->rank] = (double)n;
        if (h->world > 1 && h->world <= 64) {
            HIPCHK(hipMemcpyAsync(h->flag.p, nloc_all.data(), sizeof(double) * (size_t)h->world, hipMemcpyHostToDevice, h->stream));
            CHK(allreduce(h, h->flag.p, h->world));
            HIPCHK(hipMemcpyAsync(nloc_all.data(), h->flag.p, sizeof(double) * (size_t)h->world, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(hipStreamSynchronize(h->stream));
        }
        long nmax = n;
        for (double v : nloc_all) nmax = std::max(nmax, (long)v);
        // slots per thread: as few as keep the workgroup partials within reach of the folded reductions (G <= BIG_FOLD_U * BIG_T: the
        // consumers add them up themselves, no reduction launch; 10^6 variables on one rank: 4 slots, 977 workgroups), beyond that the
        // reduction launch with at most 4096 partials
        const int fold_cap = BIG_FOLD_U * BIG_T;
        auto groups = [](long nn, int ept) { return (int)((nn + (long)BIG_T * ept - 1) / ((long)BIG_T * ept)); };
        h->EPT = 2; while (groups(nmax, h->EPT) > fold_cap && h->EPT < 8) h->EPT *= 2;
        if (groups(nmax, h->EPT) > fold_cap) { h->EPT = 2; while (groups(nmax, h->EPT) > 2 * BIG_T * 8 && h->EPT < 64) h->EPT *= 2; }
        // tuning: MORE slots per thread than the rule above picks, never fewer (the rule's EPT is at least 2, so 1 and 2 would change nothing)
        if (const char *e = getenv("LPBOX_BIG_EPT")) { const int v = atoi(e); if (v == 4 || v == 8 || v == 16) h->EPT = std::max(v, h->EPT); }
        h->G = groups(n, h->EPT);
        h->Gs = std::max(groups(nmax, h->EPT), 1);
        h->fold = !h->ref && h->Gs <= fold_cap && h->world <= BIG_MAXW && getenv("LPBOX_BIG_NOFOLD") == nullptr;   // LPBOX_BIG_NOFOLD: keep the reduction launches (A/B)
        for (int r = 0; r < BIG_MAXW; r++) h->Gr[r] = r < h->world ? groups((long)nloc_all[r], h->EPT) : 0;
        h->EPTl = 2; h->Gl = (l + BIG_T * h->EPTl - 1) / (BIG_T * h->EPTl);
        h->Glr = (l + BIG_T - 1) / BIG_T;
        if (const char *e = getenv("LPBOX_BIG_KMARGIN")) h->chain.rules.margin = std::max(0, atoi(e));
        HIPCHK(h->timer.create());
        HIPCHK(h->d_rptr.alloc((size_t)h->P * l + 1)); HIPCHK(h->d_rcol.alloc(h->nnz)); HIPCHK(h->d_cptr.alloc((size_t)n + 1)); HIPCHK(h->d_crow.alloc(h->nnz));
        for (DevBuf<double> *bp : {&h->x, &h->y1, &h->y2, &h->z1, &h->z2, &h->db, &h->pd, &h->dinv, &h->rhs, &h->r, &h->z, &h->tmp, &h->p0, &h->p1, &h->gsrc, &h->xt})
            HIPCHK(bp->alloc(n));
        HIPCHK(h->live.alloc(n)); HIPCHK(h->newfix.alloc(n)); HIPCHK(h->d_live_idx.alloc(n)); HIPCHK(h->zp.alloc(n));
        HIPCHK(hipMemset(h->newfix.p, 0, (size_t)n));
        for (DevBuf<double> *bp : {&h->y3, &h->z4, &h->df, &h->Ex}) HIPCHK(bp->alloc(l));
        HIPCHK(h->fz.alloc(l));
        HIPCHK(h->q.alloc((size_t)h->q_cap)); HIPCHK(hipMemset(h->q.p, 0, sizeof(double) * (size_t)h->q_cap));
        HIPCHK(h->part.alloc((size_t)BIG_PH_COUNT * BIG_NPART * h->Gs)); HIPCHK(h->red.alloc(BIG_PH_COUNT * BIG_NPART)); HIPCHK(h->st.alloc(2));
        if (h->lean) {
            if (!h->fold) return lpbox_fail(LPBOX_E_UNSUPPORTED, "the comm-lean PCG needs the folded reductions (at most 1024 workgroups per rank, 16 ranks)");
            const int W = h->world;
            const long lb = ((long)l + W - 1) / W;
            const bool xch = W > 1 || h->comm;              // the q exchange runs (also against a one-rank communicator: tests)
            if (xch) {
                for (int r = 0; r < W; r++) { const long lo = std::min<long>((long)r * lb, l), cnt = std::min<long>(lb, l - lo); h->Gqr[r] = (int)((cnt + BIG_T - 1) / BIG_T); }
                h->Gq = h->Gqr[h->rank]; h->Gqs = (int)((lb + BIG_T - 1) / BIG_T);
            } else { h->Gq = h->P > 1 ? h->Glr : h->Gl; h->Gqs = h->Gq; h->Gqr[0] = h->Gq; }
            if (h->Gq > 8 * BIG_T) return lpbox_fail(LPBOX_E_UNSUPPORTED, "the comm-lean PCG sums at most %d row-workgroup partials per rank", 8 * BIG_T);
            HIPCHK(h->lsmall.alloc((size_t)h->Gs + h->Gqs)); HIPCHK(hipMemset(h->lsmall.p, 0, sizeof(double) * ((size_t)h->Gs + h->Gqs)));
            if (xch) { HIPCHK(h->gsmall.alloc((size_t)W * ((size_t)h->Gs + h->Gqs))); HIPCHK(hipMemset(h->gsmall.p, 0, sizeof(double) * (size_t)W * ((size_t)h->Gs + h->Gqs))); }
        }
        if (h->fold && (h->world > 1 || h->comm)) {         // (a one-rank RCCL communicator runs the exchange against itself: tests)
            HIPCHK(h->gpart.alloc((size_t)BIG_PH_COUNT * h->world * BIG_NPART * h->Gs));
            HIPCHK(hipMemset(h->gpart.p, 0, sizeof(double) * (size_t)BIG_PH_COUNT * h->world * BIG_NPART * h->Gs));
        }
        if (h->ref) {
            HIPCHK(h->stage.alloc((size_t)BIG_REF_NSTAGE * n)); HIPCHK(hipMemset(h->stage.p, 0, sizeof(double) * (size_t)BIG_REF_NSTAGE * n));
            HIPCHK(h->d_rank.alloc(n)); HIPCHK(h->d_frank.alloc(n)); HIPCHK(h->d_cnt.alloc(2));
            HIPCHK(hipMemset(h->d_rank.p, 0xff, sizeof(int) * (size_t)n)); HIPCHK(hipMemset(h->d_frank.p, 0xff, sizeof(int) * (size_t)n));
            HIPCHK(hipMemset(h->d_cnt.p, 0, sizeof(int) * 2));
            if (h->valued) {
                const size_t z = (size_t)std::max(h->nnz, 1);
                HIPCHK(h->d_vcsc.alloc(z)); HIPCHK(h->d_vcsr.alloc(z)); HIPCHK(h->r4v.alloc(z));
                HIPCHK(hipMemset(h->r4v.p, 0, sizeof(double) * z));
                HIPCHK(hipMemcpy(h->d_vcsc.p, h->vals.data(), sizeof(double) * (size_t)h->nnz, hipMemcpyHostToDevice));
                HIPCHK(hipMemcpy(h->d_vcsr.p, h->vcsr_h.data(), sizeof(double) * (size_t)h->nnz, hipMemcpyHostToDevice));
            }
        }
        HIPCHK(hipMemcpy(h->d_rptr.p, h->rptr.data(), sizeof(int) * ((size_t)h->P * l + 1), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(h->d_rcol.p, h->rcol.data(), sizeof(int) * (size_t)h->nnz, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(h->d_cptr.p, h->cptr.data(), sizeof(int) * ((size_t)n + 1), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(h->d_crow.p, h->crow.data(), sizeof(int) * (size_t)h->nnz, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(h->db.p, h->b.data(), sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
        HIPCHK(hipMemset(h->part.p, 0, sizeof(double) * (size_t)BIG_PH_COUNT * BIG_NPART * h->Gs));
        HIPCHK(hipMemset(h->red.p, 0, sizeof(double) * BIG_PH_COUNT * BIG_NPART));
        h->uploaded = true;
    }
    HIPCHK(hipMemcpyAsync(h->df.p, h->f.data(), sizeof(double) * (size_t)h->l, hipMemcpyHostToDevice, h->stream));
    h->left_idx.resize(h->n_loc);
    for (int j = 0; j < h->n_loc; j++) h->left_idx[j] = j;
    h->n_live_glob = h->n_glob; h->xi_valid = false;
    h->left_stale = false; h->dlive_valid = false; h->win_serial++;
    const BigDev d = h->dev();
    h->parity = 0;
    HIPCHK(big_launch_init(d, h->rf(), h->ref ? ref_c1(h->n_glob) : std::pow((double)h->n_glob, 1.0 / 2), h->stream));   // pow(n, 1/p), p = 2 (LPcpp:427,503), n = ALL variables
    if (h->ref) {
        HIPCHK(bigref_launch_rank(d, *h->rf(), 0, h->stream));                      // every variable is live: rank = index
        HIPCHK(bigref_launch_walk(d, *h->rf(), 1, BIG_PH_X, 0, -1, h->stream));     // b.x0 (:727)
    } else CHK(allreduce(h, d.red + BIG_PH_X * BIG_NPART, 1));
    HIPCHK(big_launch_init2(d, h->stream));
    ROWS(0);                                                                        // E * x0 for the first y3 (:720)
    HIPCHK(big_launch_z4(d, 1, &h->parity, h->stream));
    CHK(read_state(h));
    h->inited = true;
    return 1;
}

static int run_window(lpbox_big *h, const BigDev &d, int iter_end) {
    HIPCHK(h->timer.start(h->stream));
    CHK(chain_run(h->chain, h->graphs, ChainIo{h->stream, h->parity, h->launches, h->collectives, h->use_graph, !h->ag}, iter_end, BigChainOps{h, d}));
    double ms = 0.0;
    HIPCHK(h->timer.stop_sync(h->stream, &ms));
    h->kernel_ms += ms;
    return LPBOX_OK;
}

int lpbox_big_iterate(lpbox_big_t *h, int iter_start, int iter_end, int *ret) {     // ADMM_lp_iters LPcpp:766-1095
    if (!h) return lpbox_fail(LPBOX_E_BADHANDLE, "bad handle");
    if (!h->inited) return lpbox_fail(LPBOX_E_STATE, "solve_init has not been called");
    CHK(use_device(h->device));
    const int ws = iter_end - iter_start;
    const bool rec = h->record && ws > 0;
    h->win_serial++;
    if (rec) {
        CHK(refresh_left(h));
        if ((double)ws * h->n_loc * sizeof(double) > 4294967296.0)
            return lpbox_fail(LPBOX_E_UNSUPPORTED, "recording %d iterations of %d variables needs more than 4 GiB", ws, h->n_loc);
        if (h->ws_cap < ws || !h->xhist.p) {
            HIPCHK(hipStreamSynchronize(h->stream));
            HIPCHK(h->xhist.alloc((size_t)ws * h->n_loc));
            h->graphs.clear();                                                      // the captured launches carry the old buffer
            h->ws_cap = ws;
        }
        HIPCHK(hipMemsetAsync(h->xhist.p, 0, sizeof(double) * (size_t)h->ws_cap * h->n_loc, h->stream));
        h->xi_left = h->left_idx; h->xi_rows = (int)h->left_idx.size();
        if (h->xi_rows) HIPCHK(hipMemcpyAsync(h->d_live_idx.p, h->xi_left.data(), sizeof(int) * (size_t)h->xi_rows, hipMemcpyHostToDevice, h->stream));
        h->dlive_valid = true;
    }
    const BigDev d = h->dev();
    HIPCHK(big_launch_set_window(d, iter_start, iter_end, rec ? 2 : 0, &h->parity, h->stream));
    CHK(run_window(h, d, iter_end));
    if (rec) { h->xi_valid = true; h->xi_plain = true; }
    if (ret) *ret = h->hst.ret;
    return LPBOX_OK;
}

// ADMM_lp_iters_l2f (LPcpp:1098-1574).  vec_local: this rank's slice of the fix vector, one entry per LOCAL live variable in
// ascending order (1 / 0 = fix, anything else = leave); num_global: fixes over all ranks (the caller sums the local counts).
int lpbox_big_iterate_l2f(lpbox_big_t *h, int iter_start, int iter_end, const double *vec_local, long num_global, int *ret) {
    if (!h) return lpbox_fail(LPBOX_E_BADHANDLE, "bad handle");
    if (!h->inited) return lpbox_fail(LPBOX_E_STATE, "solve_init has not been called");
    const int ws = iter_end - iter_start;
    if (ws > LP_XITERS_COLS) return lpbox_fail(LPBOX_E_BADARG, "window of %d iterations exceeds the %d columns of x_iters (LPcpp:1113)", ws, LP_XITERS_COLS);
    if (num_global < 0 || num_global > h->n_live_glob) return lpbox_fail(LPBOX_E_BADARG, "fix count %ld outside [0,%ld]", num_global, h->n_live_glob);
    CHK(use_device(h->device));
    CHK(refresh_left(h));
    const int n_live_loc = (int)h->left_idx.size();
    std::vector<uint8_t> nf;
    std::vector<int> keep;
    bool ok = true;
    if (num_global != 0) {
        if (!vec_local && n_live_loc) { lpbox_fail(LPBOX_E_BADARG, "fix vector missing"); ok = false; }
        else {
            nf.assign(h->n_loc, 0);
            keep.reserve(n_live_loc);
            long cnt = 0;
            for (int q = 0; q < n_live_loc; q++) {
                const int j = h->left_idx[q];
                if (vec_local[q] == 1) { nf[j] = 2; cnt++; } else if (vec_local[q] == 0) { nf[j] = 1; cnt++; } else keep.push_back(j);
            }
            if (h->world == 1 && cnt != num_global) { lpbox_fail(LPBOX_E_BADARG, "vec fixes %ld variables but num = %ld", cnt, num_global); ok = false; }
            else if (cnt > num_global) { lpbox_fail(LPBOX_E_BADARG, "this rank fixes %ld variables, more than the global count %ld", cnt, num_global); ok = false; }
        }
    }
    // all ranks fail together: nobody enters the state-changing collectives below unless everybody passed validation
    if (agree_ok(h, ok) != LPBOX_OK) return ok ? lpbox_fail(LPBOX_E_BADARG, "another rank rejected its arguments of this call") : LPBOX_E_BADARG;
    if (num_global != 0) h->left_idx.swap(keep);
    if (ws > 0 && (h->ws_cap < ws || !h->xhist.p)) {
        HIPCHK(hipStreamSynchronize(h->stream));
        HIPCHK(h->xhist.alloc((size_t)ws * h->n_loc));
        h->graphs.clear();                                                      // the captured launches carry the old window buffer
        h->ws_cap = ws;
    }
    const BigDev d = h->dev();
    HIPCHK(big_launch_set_window(d, iter_start, iter_end, 1, &h->parity, h->stream));
    if (num_global != 0) {
        const long n_live_new = h->n_live_glob - num_global;
        HIPCHK(hipMemcpyAsync(h->newfix.p, nf.data(), nf.size(), hipMemcpyHostToDevice, h->stream));
        if (h->ref) { HIPCHK(bigref_launch_rank(d, *h->rf(), 1, h->stream)); h->launches++; }    // rank among the newly fixed
        HIPCHK(big_launch_fix1(d, h->rf(), h->stream)); h->launches++;
        if (h->ref) WALK(1, BIG_PH_X, 1, -1); else FINX(1);                         // fix_obj = b2.x2 (reference order: redux over the newly fixed)
        ROWS(0);                                                                    // q = E2 * x2
        if (h->ref) { HIPCHK(bigref_launch_rank(d, *h->rf(), 2, h->stream)); h->launches++; }    // the live ranks after this fix
        HIPCHK(big_launch_fix2(d, h->rf(), &h->parity, h->stream)); h->launches++;
        if (h->ref) WALK(1, BIG_PH_X, 0, -1); else FINX(1);                         // |x_live|^2
        HIPCHK(big_launch_fix3(d, h->rf(), n_live_new, h->ref ? ref_c1(n_live_new) : std::pow((double)n_live_new, 1.0 / 2), &h->parity, h->stream)); h->launches++;
        if (n_live_new != 0) {
            ROWS(0);                                                                // E * x (live columns) for the first y3
            HIPCHK(big_launch_z4(d, 1, &h->parity, h->stream)); h->launches++;
        }
        HIPCHK(hipMemsetAsync(h->newfix.p, 0, (size_t)h->n_loc, h->stream));
        h->n_live_glob = n_live_new;
    }
    h->xi_left = h->left_idx; h->xi_rows = (int)h->left_idx.size();
    if (h->ws_cap > 0) HIPCHK(hipMemsetAsync(h->xhist.p, 0, sizeof(double) * (size_t)h->ws_cap * h->n_loc, h->stream));   // x_iters = Zero (:1113): ALL staged columns, also those of an earlier, longer window
    if (h->xi_rows) HIPCHK(hipMemcpyAsync(h->d_live_idx.p, h->xi_left.data(), sizeof(int) * (size_t)h->xi_rows, hipMemcpyHostToDevice, h->stream));
    CHK(run_window(h, d, iter_end));        // synchronises: nf / xi_left stay alive until here
    h->xi_valid = true; h->xi_plain = false; h->dlive_valid = true; h->win_serial++;
    if (ret) *ret = h->hst.ret;
    return LPBOX_OK;
}

int lpbox_big_get_n(lpbox_big_t *h) {                                               // live variables of this rank
    if (!h || !h->inited) return lpbox_fail(LPBOX_E_STATE, "not initialised");
    CHK(refresh_left(h));
    return (int)h->left_idx.size();
}

// (rows x ws) row-major x_iters of this rank's live variables, left on the device; rows = live variables when the window started
int lpbox_big_get_x_iters_device(lpbox_big_t *h, int ws, void **dev_ptr, int *rows) {
    if (!h || !h->inited) return lpbox_fail(LPBOX_E_STATE, "not initialised");
    if (!h->xi_valid) return lpbox_fail(LPBOX_E_STATE, "solve_iter_l2f has not been called");
    const int ws_max = h->xi_plain ? h->ws_cap : LP_XITERS_COLS;                 // a recorded plain call may be longer than an l2f window
    if (ws <= 0 || ws > ws_max) return lpbox_fail(LPBOX_E_BADARG, "ws = %d outside (0,%d]", ws, ws_max);
    CHK(use_device(h->device));
    const size_t need = (size_t)std::max(h->xi_rows, 1) * ws;
    if (h->xi_out.count < need) { HIPCHK(hipStreamSynchronize(h->stream)); HIPCHK(h->xi_out.alloc(need)); }
    HIPCHK(big_launch_pack_xiters(h->dev(), h->d_live_idx.p, h->xi_rows, ws, h->xi_out.p, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (dev_ptr) *dev_ptr = h->xi_out.p;
    if (rows) *rows = h->xi_rows;
    return LPBOX_OK;
}

int lpbox_big_get_x_iters(lpbox_big_t *h, int ws, double *out) {
    void *p = nullptr; int rows = 0;
    if (!out) { if (!h || !h->xi_valid) return lpbox_fail(LPBOX_E_STATE, "solve_iter_l2f has not been called"); return h->xi_rows; }
    CHK(lpbox_big_get_x_iters_device(h, ws, &p, &rows));
    if (rows) HIPCHK(hipMemcpy(out, p, sizeof(double) * (size_t)rows * ws, hipMemcpyDeviceToHost));
    return rows;
}

// binary solution of this rank's variables: fixed ones at their value, live ones rounded (get_x_sol, LPcpp:1648-1666)
int lpbox_big_get_x_sol(lpbox_big_t *h, double *out_local) {
    if (!h || !h->inited || !out_local) return lpbox_fail(LPBOX_E_STATE, "not initialised");
    CHK(use_device(h->device));
    std::vector<uint8_t> lv(h->n_loc);
    HIPCHK(hipMemcpy(out_local, h->x.p, sizeof(double) * (size_t)h->n_loc, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(lv.data(), h->live.p, (size_t)h->n_loc, hipMemcpyDeviceToHost));
    for (int j = 0; j < h->n_loc; j++) if (lv[j]) out_local[j] = out_local[j] >= 0.5 ? 1.0 : 0.0;
    return h->n_loc;
}

int lpbox_big_cal_obj(lpbox_big_t *h, double *out) {                                // cal_Obj, LPcpp:1630-1642
    if (!h || !h->inited || !out) return lpbox_fail(LPBOX_E_STATE, "not initialised");
    *out = h->n_live_glob != 0 ? h->hst.sum_fix_obj + h->hst.cur_obj : h->hst.sum_fix_obj;
    return LPBOX_OK;
}

int lpbox_big_get_x(lpbox_big_t *h, double *out_local) {
    if (!h || !h->inited || !out_local) return lpbox_fail(LPBOX_E_STATE, "not initialised");
    CHK(use_device(h->device));
    HIPCHK(hipMemcpy(out_local, h->x.p, sizeof(double) * (size_t)h->n_loc, hipMemcpyDeviceToHost));
    return h->n_loc;
}

int lpbox_big_get_vec(lpbox_big_t *h, const char *name, double *out, long cap) {
    if (!h || !h->inited || !out || !name) return lpbox_fail(LPBOX_E_STATE, "not initialised");
    CHK(use_device(h->device));
    const double *src = nullptr; long len = h->n_loc;
    if (!strcmp(name, "x")) src = h->x.p; else if (!strcmp(name, "z1")) src = h->z1.p; else if (!strcmp(name, "z2")) src = h->z2.p;
    else if (!strcmp(name, "pd")) src = h->pd.p; else if (!strcmp(name, "b")) src = h->db.p;
    else if (!strcmp(name, "f")) { src = h->df.p; len = h->l; }
    else if (!strcmp(name, "z4")) { src = h->z4.p; len = h->l; } else if (!strcmp(name, "Ex")) { src = h->Ex.p; len = h->l; }
    else if (h->ref && (!strcmp(name, "r4v") || !strcmp(name, "vals"))) {     // per stored entry, in the order of rowidx
        len = h->nnz;
        if (cap < len) return lpbox_fail(LPBOX_E_BADARG, "buffer too small");
        if (!h->valued) {                                                          // a unit instance carries the scalar / ones
            for (long k = 0; k < len; k++) out[k] = name[0] == 'r' ? h->hst.r4Et : 1.0;
            return (int)len;
        }
        if (len) HIPCHK(hipMemcpy(out, name[0] == 'r' ? h->r4v.p : h->d_vcsc.p, sizeof(double) * (size_t)len, hipMemcpyDeviceToHost));
        return (int)len;
    }
    else if (!strcmp(name, "live")) {
        if (cap < len) return lpbox_fail(LPBOX_E_BADARG, "buffer too small");
        std::vector<uint8_t> lv((size_t)len);
        HIPCHK(hipMemcpy(lv.data(), h->live.p, (size_t)len, hipMemcpyDeviceToHost));
        for (long j = 0; j < len; j++) out[j] = lv[j] ? 1.0 : 0.0;
        return (int)len;
    }
    else return lpbox_fail(LPBOX_E_BADARG, "unknown vector '%s'", name);
    if (cap < len) return lpbox_fail(LPBOX_E_BADARG, "buffer too small");
    HIPCHK(hipMemcpy(out, src, sizeof(double) * (size_t)len, hipMemcpyDeviceToHost));
    return (int)len;
}

int lpbox_big_check_infeasible(lpbox_big_t *h, int which) {
    if (!h || !h->inited) return lpbox_fail(LPBOX_E_STATE, "not initialised");
    if (h->world != 1) return lpbox_fail(LPBOX_E_UNSUPPORTED, "the infeasibility counts need every column: one rank only");
    CHK(use_device(h->device));
    const int n = h->n_loc, l = h->l;
    std::vector<double> v(n);
    std::vector<uint8_t> live(n, 1);
    if (which == 0) {                                            // LPcpp:1577-1591: current E (live columns), raw iterate
        if (h->n_live_glob == 0) return 0;
        HIPCHK(hipMemcpy(v.data(), h->x.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(live.data(), h->live.p, (size_t)n, hipMemcpyDeviceToHost));
    } else {                                                     // LPcpp:1593-1612: original E, binary full-length solution
        int rc = lpbox_big_get_x_sol(h, v.data());
        if (rc < 0) return rc;
    }
    // rows in ascending column order (the slices of the row storage follow each other in column order)
    std::vector<double> s(l, 0.0);
    for (int ph = 0; ph < h->P; ph++)
        for (int i = 0; i < l; i++)
            for (int k = h->rptr[(size_t)ph * l + i]; k < h->rptr[(size_t)ph * l + i + 1]; k++)
                if (live[h->rcol[k]]) s[i] += (h->valued ? h->vcsr_h[k] : 1.0) * (1.0 * v[h->rcol[k]]);
    int inf = 0;
    for (int i = 0; i < l; i++) if (!(s[i] <= 1.0)) inf++;          // the reference compares with 1.0, not with f
    return inf;
}

int lpbox_big_get_scalar(lpbox_big_t *h, const char *name, double *out) {
    if (h && out && name && !strcmp(name, "order")) { *out = h->ref ? (double)LPBOX_ORDER_REFERENCE : (double)LPBOX_ORDER_DEFAULT; return LPBOX_OK; }
    if (h && out && name && !strcmp(name, "valued")) { *out = h->valued ? 1.0 : 0.0; return LPBOX_OK; }
    if (!h || !h->inited || !out || !name) return lpbox_fail(LPBOX_E_STATE, "not initialised");
    const BigState &s = h->hst;
    struct { const char *n; double v; } tab[] = {
        {"rho1", s.rho1}, {"rho4", s.rho4}, {"gamma", s.gamma_val}, {"dI", s.dI}, {"rho4Et", s.r4Et}, {"std_obj", s.std_obj},
        {"cur_obj", s.cur_obj}, {"best_bin_obj", s.best_bin_obj}, {"cvg1", s.cvg1}, {"cvg2", s.cvg2}, {"obj_val", s.obj_val},
        {"iter", (double)s.iter}, {"outer_total", (double)s.outer_total}, {"pcg_total", (double)s.pcg_total}, {"last_pcg", (double)s.last_pcg},
        {"sum_fix_obj", s.sum_fix_obj}, {"fix_obj", s.fix_obj}, {"c1", s.c1}, {"ret", (double)s.ret}, {"n_live", (double)h->n_live_glob},
        {"stop", (double)s.stop}, {"plain_iter_p1", (double)s.plain_iter_p1}, {"kmax", (double)h->chain.kmax}, {"pcg_resumes", (double)h->chain.pcg_resumes}, {"kmax_kept", (double)h->chain.kept},
        {"graph_revisits", (double)h->graphs.revisits},
        {"launches", (double)h->launches}, {"collectives", (double)h->collectives}, {"kernel_ms", h->kernel_ms},
        {"threads", (double)BIG_T}, {"chunk", (double)(BIG_T * h->EPT)}, {"groups", (double)h->G}, {"row_slices", (double)h->P}, {"folded_reductions", h->fold ? 1.0 : 0.0}, {"pcg_comm_lean", h->lean ? 1.0 : 0.0},
        {"row_chunk", (double)((h->world > 1 || h->comm) ? BIG_T : (h->P > 1 ? BIG_T : BIG_T * h->EPTl))},
    };
    for (auto &e : tab) if (!strcmp(e.n, name)) { *out = e.v; return LPBOX_OK; }
    return lpbox_fail(LPBOX_E_BADARG, "unknown scalar '%s'", name);
}


}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------
// A BATCH of large-route handles through ONE launch chain in lockstep: plain windows (ADMM_lp_iters) of every
// member at once, grid (X, B) per launch, each member on its own control state -- one that has stopped, reached the end of the
// window or whose PCG has converged falls through; a BIG_HALT_PCG_MORE on any member resumes the chain for all.  The handles are
// borrowed and stay ordinary handles: per member the arithmetic is that of lpbox_big_iterate on its own, bit for bit.
struct lpbox_big_batch {
    std::vector<lpbox_big *> hs;
    int B = 0, device = 0;
    bool inited = false;
    ChainLockstep chain{CHAIN_RULES_BIG, CHAIN_RULES_BIG.kmax_start};   // rules, kmax (carried over the windows), adaptive
    bool use_graph = false;
    hipStream_t stream = nullptr;
    StreamTimer timer;
    GraphCache graphs;                              // two iterations per (kmax, start parity); the grid extents never change
    BigBatchGrid grid{0, 0, 0, 0, 0};
    DevBuf<BigDev> devs; DevBuf<BigState> dstates;
    std::vector<BigDev> h_devs;                     // host side of devs (alive until the stream has taken it)
    // the batch's summation order is member 0's at create; reference order: the members' BigRef descriptors in a
    // device array parallel to devs, uploaded with it, and the walker launches counted
    bool ref = false;
    DevBuf<BigRef> refs; std::vector<BigRef> h_refs;
    long long walks = 0;
    int kinds = 0;                                  // BIGREF_KIND_*: the kinds of member of the window being run
    std::vector<BigState> h_states;
    double kernel_ms = 0.0; long long launches = 0, collectives = 0, parity_copies = 0;
    // early-fixing windows
    std::vector<uint8_t> active;                    // lpbox_big_batch_set_active; governs the l2f calls and the pack only
    int graph_B = 0;                                // members in the captured launches' grid
    DevBuf<BigFixPar> par; std::vector<BigFixPar> h_par;
    DevBuf<int> counts; DevBuf<uint8_t> codes; DevBuf<double> pack;
    uint8_t *h_codes = nullptr; size_t h_codes_cap = 0;     // pinned staging of the host-vector form: one code per live row of every fixing member
    // the most recent pack: rows of member i = [row_off[i], row_off[i+1]), taken after window pack_serial[i] of that member (-1: not packed)
    std::vector<long> row_off, pack_serial;
    bool pack_valid = false;
    long long fix_launches = 0, packs = 0;
};

namespace {

// what a member must be for the lockstep chain; `i` names it in the message.  Checked at create, init and iterate: a handle can be
// changed between the calls (recording switched on, an early-fixing window of its own).
int bigb_member_ok(const lpbox_big *h, int i, bool ref_batch, bool allow_fixed = false) {      // ref_batch: the batch's order; allow_fixed: the early-fixing calls
    if (!h || !h->has_problem) return lpbox_fail(LPBOX_E_STATE, "problem %d of the batch has no problem", i);
    if (h->ref && !ref_batch) return lpbox_fail(LPBOX_E_UNSUPPORTED, "problem %d of the batch runs in the reference summation order; the batch runs the default order", i);
    if (!h->ref && ref_batch) return lpbox_fail(LPBOX_E_UNSUPPORTED, "problem %d of the batch runs in the default order; the batch runs the reference summation order (problem 0's)", i);
    if (h->world != 1) return lpbox_fail(LPBOX_E_UNSUPPORTED, "problem %d of the batch is sharded over %d ranks; the batch runs one rank per problem", i, h->world);
    if (h->comm || h->ag) return lpbox_fail(LPBOX_E_UNSUPPORTED, "problem %d of the batch has a transport; the batch issues no collectives", i);
    if (h->lean) return lpbox_fail(LPBOX_E_UNSUPPORTED, "problem %d of the batch uses the comm-lean PCG", i);
    if (h->record) return lpbox_fail(LPBOX_E_UNSUPPORTED, "problem %d of the batch is recording; recording is per handle (lpbox_big_iterate)", i);
    if (!ref_batch && h->uploaded && !h->fold)             // (the reference order runs with the fold off: its walker writes the totals)
        return lpbox_fail(LPBOX_E_UNSUPPORTED, "problem %d of the batch runs without folded reductions (LPBOX_BIG_NOFOLD, or more than %d workgroups)", i, BIG_FOLD_U * BIG_T);
    if (!allow_fixed && h->inited && h->n_live_glob != h->n_glob)
        return lpbox_fail(LPBOX_E_UNSUPPORTED, "problem %d of the batch has fixed variables; early-fixing windows are per handle (lpbox_big_iterate_l2f)", i);
    return LPBOX_OK;
}

// The launches of the lockstep chain (chain_run_lockstep) over the g.B members whose descriptors stand in devs; the grid extents stay the
// maxima over all members.  Reference order: the solo chain's launches with a BigRef, launch for launch.  b->h_states[k]: the final states.
struct BigBatchOps {
    lpbox_big_batch *b; const BigDev *devs; const BigRef *refs; hipStream_t st; BigBatchGrid g; int &parity;
    int collect(ChainView *v) {
        HIPCHK(bigb_collect_states(devs, g, parity, b->dstates.p, st));
        HIPCHK(hipMemcpyAsync(b->h_states.data(), b->dstates.p, sizeof(BigState) * (size_t)g.B, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (int i = 0; i < g.B; i++) v[i] = chain_view(b->h_states[i]);
        return LPBOX_OK;
    }
    int resume_pcg() {
        HIPCHK(bigb_launch_resume(devs, g, 0, &parity, st));
        if (b->ref) { HIPCHK(bigrefb_enqueue_pcg(devs, refs, g, CHAIN_PAIRS_PER_RESUME, &parity, st)); HIPCHK(bigrefb_enqueue_tail(devs, refs, g, &parity, st)); }
        else { HIPCHK(bigb_enqueue_pcg(devs, g, CHAIN_PAIRS_PER_RESUME, &parity, st)); HIPCHK(bigb_enqueue_tail(devs, g, &parity, st)); }
        b->launches += b->ref ? 5 + 5 * CHAIN_PAIRS_PER_RESUME : 4 + 3 * CHAIN_PAIRS_PER_RESUME;
        b->walks += b->ref ? 1 + 2 * CHAIN_PAIRS_PER_RESUME : 0;
        return LPBOX_OK;
    }
    int batch_head(int iters, int kmax) {                           // the walks of the batch here: replayed or eager, every iteration has them
        HIPCHK(bigb_launch_resume(devs, g, 1, &parity, st));
        b->launches += 1; b->walks += b->ref ? (long long)iters * (3 + 2 * kmax) : 0;
        return LPBOX_OK;
    }
    int enqueue(int n, int kmax) {
        if (b->ref) HIPCHK(bigrefb_enqueue_iterations(devs, refs, g, b->kinds, n, kmax, &parity, st)); else HIPCHK(bigb_enqueue_iterations(devs, g, n, kmax, &parity, st));
        b->launches += (long long)n * (b->ref ? 11 + 5 * kmax + (b->kinds == (BIGREF_KIND_UNIT | BIGREF_KIND_VALUED) ? 1 : 0) : 8 + 3 * kmax);
        return LPBOX_OK;
    }
    int finalize() {
        if (b->ref) HIPCHK(bigrefb_launch_prep(devs, refs, g, 0, &parity, st)); else HIPCHK(bigb_launch_prep(devs, g, 0, &parity, st));
        b->launches += 1;
        return LPBOX_OK;
    }
};

// the chain up to iter_end (the window already set) over the A members behind b->devs (act[k]: the member behind descriptor k; nullptr: all)
int bigb_chain(lpbox_big_batch *b, int A, const int *act, int iter_end, int *parity, long long *resumes) {
    BigBatchGrid g = b->grid; g.B = A;
    if (b->graph_B != A) { b->graphs.clear(); b->graph_B = A; }     // the captured launches carry the member count
    return chain_run_lockstep(b->chain, A, act, b->graphs, ChainIo{b->stream, *parity, b->launches, b->collectives, b->use_graph, true}, iter_end,
                              resumes, BigBatchOps{b, b->devs.p, b->refs.p, b->stream, g, *parity});
}

// the early-fixing calls on a batch in the reference order: they would need batched rank passes (bigref_k_rank per fix); nothing changes
int bigb_no_fixing() {
    return lpbox_fail(LPBOX_E_UNSUPPORTED, "the early-fixing windows of a batch need the default order; this batch runs the reference summation order (lpbox_big_iterate_l2f per handle)");
}

// descriptors (b->h_devs) and records (b->h_par) of the first A slots -> device, one copy each
int bigb_upload_devs(lpbox_big_batch *b, int A) {
    HIPCHK(hipMemcpyAsync(b->devs.p, b->h_devs.data(), sizeof(BigDev) * (size_t)A, hipMemcpyHostToDevice, b->stream));
    return LPBOX_OK;
}
int bigb_upload_par(lpbox_big_batch *b, int A) {
    HIPCHK(hipMemcpyAsync(b->par.p, b->h_par.data(), sizeof(BigFixPar) * (size_t)A, hipMemcpyHostToDevice, b->stream));
    return LPBOX_OK;
}

// One early-fixing window (ADMM_lp_iters_l2f, LPcpp:1098-1574) of all active members.  Host-vector form: vecs /
// nums, the caller has decided; score form: scores (device, float32, one per packed row of the last pack) or NULL, the rule runs on the
// device.  Everything is validated before anything changes.
int bigb_window(lpbox_big_batch *b, int iter_start, int iter_end, bool score_form, const double *vecs, long vec_stride, const long *nums,
                const float *scores, double hi, double lo, int min_fix, int *rets, int *fixed) {
    const int ws = iter_end - iter_start;
    if (ws > LP_XITERS_COLS) return lpbox_fail(LPBOX_E_BADARG, "window of %d iterations exceeds the %d columns of x_iters (LPcpp:1113)", ws, LP_XITERS_COLS);
    const std::vector<int> act = active_members(b->active);
    const int A = (int)act.size();
    std::vector<long> live(A), num(A, 0);
    for (int k = 0; k < A; k++) { const lpbox_big *h = b->hs[act[k]]; live[k] = h && h->inited ? h->n_live_glob : (h ? h->n_glob : 0); }
    if (!score_form)
        for (int k = 0; k < A; k++) {
            const int i = act[k];
            num[k] = nums ? nums[i] : 0;
            if (num[k] < 0 || num[k] > live[k]) return lpbox_fail(LPBOX_E_BADARG, "problem %d of the batch: fix count %ld outside [0,%ld]", i, num[k], live[k]);
            if (num[k] == 0) continue;
            if (!vecs) return lpbox_fail(LPBOX_E_BADARG, "problem %d of the batch: fix vector missing", i);
            if (vec_stride < live[k]) return lpbox_fail(LPBOX_E_BADARG, "problem %d of the batch: fix vector holds %ld entries, %ld live variables", i, vec_stride, live[k]);
            const double *vec = vecs + (size_t)i * vec_stride;
            long cnt = 0;
            for (long q = 0; q < live[k]; q++) if (vec[q] == 1 || vec[q] == 0) cnt++;
            if (cnt != num[k]) return lpbox_fail(LPBOX_E_BADARG, "problem %d of the batch: vec fixes %ld variables but num = %ld", i, cnt, num[k]);
        }
    if (!b->inited) return lpbox_fail(LPBOX_E_STATE, "lpbox_big_batch_init has not been called");
    for (int k = 0; k < A; k++) {
        CHK(bigb_member_ok(b->hs[act[k]], act[k], false, true));
        if (!b->hs[act[k]]->inited) return lpbox_fail(LPBOX_E_STATE, "problem %d of the batch: solve_init has not been called", act[k]);
    }
    if (score_form && scores) {
        if (!b->pack_valid) return lpbox_fail(LPBOX_E_STATE, "scores given, but lpbox_big_batch_get_x_iters_device has not been called since the last window");
        for (int k = 0; k < A; k++) {
            const int i = act[k];
            if (b->pack_serial[i] < 0 || b->pack_serial[i] != b->hs[i]->win_serial || b->row_off[i + 1] - b->row_off[i] != live[k])
                return lpbox_fail(LPBOX_E_STATE, "problem %d of the batch is active but its window is not in the packed buffer the scores refer to", i);
        }
    }
    CHK(use_device(b->device));
    if (A == 0) return LPBOX_OK;
    hipStream_t st = b->stream;
    for (int k = 0; k < A; k++) HIPCHK(hipStreamSynchronize(b->hs[act[k]]->stream));     // windows of its own in between have completed

    // host-vector form: one code per live row of every fixing member in pinned memory, and the new host lists
    std::vector<std::vector<int>> kept(A);
    std::vector<long> row0(A, 0);
    long code_rows = 0;
    if (!score_form) {
        for (int k = 0; k < A; k++) if (num[k]) { row0[k] = code_rows; code_rows += live[k]; }
        if ((size_t)code_rows > b->h_codes_cap) {
            if (b->h_codes) HIPCHK(hipHostFree(b->h_codes));
            b->h_codes = nullptr; b->h_codes_cap = 0;
            size_t cap = 0;
            for (int i = 0; i < b->B; i++) cap += (size_t)b->hs[i]->n_loc;
            HIPCHK(hipHostMalloc((void **)&b->h_codes, cap));
            HIPCHK(b->codes.alloc(cap));
            b->h_codes_cap = cap;
        }
        for (int k = 0; k < A; k++) {
            if (!num[k]) continue;
            lpbox_big *h = b->hs[act[k]];
            CHK(refresh_left(h));
            const double *vec = vecs + (size_t)act[k] * vec_stride;
            uint8_t *code = b->h_codes + row0[k];
            kept[k].reserve((size_t)(live[k] - num[k]));
            for (long q = 0; q < live[k]; q++) {
                code[q] = vec[q] == 1 ? 2 : (vec[q] == 0 ? 1 : 0);
                if (!code[q]) kept[k].push_back(h->left_idx[q]);
            }
        }
    }
    // the staged window of a member grows on the host, only when this window is longer than any before it; the member's live list
    // goes up once, when its device copy is not current
    for (int k = 0; k < A; k++) {
        lpbox_big *h = b->hs[act[k]];
        if (ws > 0 && (h->ws_cap < ws || !h->xhist.p)) {
            HIPCHK(h->xhist.alloc((size_t)ws * h->n_loc));
            h->graphs.clear();                                                      // the captured launches carry the old window buffer
            h->ws_cap = ws;
        }
        if (!h->dlive_valid) {
            if (!h->left_idx.empty()) HIPCHK(hipMemcpyAsync(h->d_live_idx.p, h->left_idx.data(), sizeof(int) * h->left_idx.size(), hipMemcpyHostToDevice, st));
            h->dlive_valid = true;
        }
    }
    // one ping-pong parity for the chain (section 28)
    int parity = b->hs[act[0]]->parity;
    long long copies = 0;
    for (int k = 1; k < A; k++) {
        lpbox_big *h = b->hs[act[k]];
        if (h->parity != parity) { HIPCHK(big_launch_resume(h->dev(), 0, &h->parity, st)); copies++; }
    }
    BigBatchGrid g = b->grid;
    g.B = A;
    long max_rows = 0, max_stage = 0;
    for (int k = 0; k < A; k++) {
        const lpbox_big *h = b->hs[act[k]];
        b->h_devs[k] = h->dev();
        BigFixPar &p = b->h_par[k];
        p.apply = !score_form && num[k] ? 1 : 0; p.clear = 0;
        p.rows = score_form || num[k] ? (int)live[k] : 0;
        p.row0 = score_form ? (scores ? (int)b->row_off[act[k]] : 0) : (int)row0[k];
        p.n_live_new = live[k] - num[k];
        p.c1_new = std::pow((double)p.n_live_new, 1.0 / 2);         // on the host, as lpbox_big_iterate_l2f
        p.live_idx = h->d_live_idx.p;
        max_rows = std::max<long>(max_rows, p.rows);
        max_stage = std::max<long>(max_stage, h->xhist.p ? (long)h->ws_cap * h->n_loc : 0);
    }
    CHK(bigb_upload_devs(b, A));
    CHK(bigb_upload_par(b, A));
    HIPCHK(b->timer.start(st));
    const long long l0 = b->launches;
    b->launches += copies; b->parity_copies += copies;
    HIPCHK(bigb_launch_set_window_l2f(b->devs.p, g, iter_start, iter_end, &parity, st));
    b->launches++;

    std::vector<long> applied(num);
    bool any = false, any_clear = false;
    if (score_form && scores) {
        std::vector<int> hc(2 * (size_t)A, 0);
        HIPCHK(hipMemsetAsync(b->counts.p, 0, sizeof(int) * hc.size(), st));
        HIPCHK(bigb_launch_decide(b->devs.p, b->par.p, g, (int)max_rows, scores, nullptr, hi, lo, b->counts.p, st));
        HIPCHK(hipMemcpyAsync(hc.data(), b->counts.p, sizeof(int) * hc.size(), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        b->launches++;
        for (int k = 0; k < A; k++) {
            const long kf = (long)hc[2 * k] + hc[2 * k + 1];
            BigFixPar &p = b->h_par[k];
            if (kf > min_fix) {                                                     // LP/trainer.py:533-535
                applied[k] = kf; p.apply = 1; p.n_live_new = live[k] - kf;
                p.c1_new = std::pow((double)p.n_live_new, 1.0 / 2);
            } else if (kf > 0) { p.clear = 1; any_clear = true; }
        }
        CHK(bigb_upload_par(b, A));                                                 // the decision: the one extra copy of this form
    } else if (!score_form && code_rows > 0) {
        HIPCHK(hipMemcpyAsync(b->codes.p, b->h_codes, (size_t)code_rows, hipMemcpyHostToDevice, st));
        HIPCHK(bigb_launch_decide(b->devs.p, b->par.p, g, (int)max_rows, nullptr, b->codes.p, 0.0, 0.0, b->counts.p, st));
        b->launches++;
    }
    for (int k = 0; k < A; k++) any |= applied[k] > 0;
    if (any) {                                                                      // no member fixes: no prologue at all
        HIPCHK(bigb_enqueue_fix(b->devs.p, b->par.p, g, &parity, st));
        b->launches += 8; b->fix_launches += 8;
    }
    if (any || any_clear) { HIPCHK(bigb_launch_compact(b->devs.p, b->par.p, g, st)); b->launches++; }
    if (max_stage > 0) { HIPCHK(bigb_launch_clear_xhist(b->devs.p, g, max_stage, st)); b->launches++; }     // x_iters = Zero (:1113)

    std::vector<long long> resumes(A, 0);
    const int rc = bigb_chain(b, A, act.data(), iter_end, &parity, resumes.data());
    double ms = 0.0;
    const hipError_t e = b->timer.stop_sync(st, &ms);
    if (rc < 0) return rc;
    HIPCHK(e);
    b->kernel_ms += ms;
    for (int k = 0; k < A; k++) {
        lpbox_big *h = b->hs[act[k]];
        h->hst = b->h_states[k]; h->parity = parity;
        h->chain.pcg_resumes += resumes[k];
        h->n_live_glob = live[k] - applied[k];
        h->xi_rows = (int)h->n_live_glob; h->xi_valid = true; h->xi_plain = false; h->win_serial++;
        if (applied[k]) {
            if (score_form) h->left_stale = true;                                   // fixed on the device: the host list follows on demand
            else h->left_idx.swap(kept[k]);
        }
        if (rets) rets[act[k]] = h->hst.ret;
        if (fixed) fixed[act[k]] = (int)applied[k];
    }
    b->hs[act[0]]->kernel_ms += ms; b->hs[act[0]]->launches += b->launches - l0;
    b->pack_valid = false;
    return LPBOX_OK;
}

}  // namespace

extern "C" {

lpbox_big_batch_t *lpbox_big_batch_create(lpbox_big_t **handles, int count) {
    auto refuse = [](int) -> lpbox_big_batch * { return nullptr; };        // lpbox_fail has recorded status and text
    if (!handles || count <= 0) return refuse(lpbox_fail(LPBOX_E_BADARG, "empty batch"));
    for (int i = 0; i < count; i++) {                               // no device call
        if (bigb_member_ok(handles[i], i, handles[0] && handles[0]->ref) < 0) return nullptr;
        if (handles[i]->device != handles[0]->device) return refuse(lpbox_fail(LPBOX_E_BADARG, "problem %d of the batch lives on another device than problem 0", i));
        for (int k = 0; k < i; k++)
            if (handles[k] == handles[i]) return refuse(lpbox_fail(LPBOX_E_BADARG, "problem %d and problem %d of the batch are the same handle", k, i));
    }
    lpbox_big_batch *b = new lpbox_big_batch();
    b->hs.assign(handles, handles + count); b->B = count; b->device = handles[0]->device;
    b->ref = handles[0]->ref;
    b->active.assign(count, 1); b->row_off.assign((size_t)count + 1, 0); b->pack_serial.assign(count, -1);
    if (const char *e = getenv("LPBOX_BIG_KMAX")) { int v = atoi(e); if (v >= 1 && v <= 1000) { b->chain.kmax = v; b->chain.adaptive = false; } }
    if (const char *e = getenv("LPBOX_BIG_KMARGIN")) b->chain.rules.margin = std::max(0, atoi(e));
    if (const char *e = getenv("LPBOX_BIG_BATCH_GRAPH")) b->use_graph = atoi(e) != 0;     // replay captured iterations instead of eager launches
    return b;
}

void lpbox_big_batch_destroy(lpbox_big_batch_t *b) {
    if (!b) return;
    if (b->stream) {
        (void)hipSetDevice(b->device);
        (void)hipStreamSynchronize(b->stream);
        b->graphs.clear();
        b->timer.destroy();
        if (b->h_codes) (void)hipHostFree(b->h_codes);
        (void)hipStreamDestroy(b->stream);
    }
    delete b;
}

// lpbox_big_init on every member (a handful of launches once per solve), then the descriptors of all members in one device array
int lpbox_big_batch_init(lpbox_big_batch_t *b) {
    if (!b) return lpbox_fail(LPBOX_E_BADHANDLE, "bad handle");
    for (int i = 0; i < b->B; i++) CHK(bigb_member_ok(b->hs[i], i, b->ref));
    CHK(use_device(b->device));
    b->inited = false;
    for (int i = 0; i < b->B; i++) CHK(lpbox_big_init(b->hs[i]));
    for (int i = 0; i < b->B; i++) CHK(bigb_member_ok(b->hs[i], i, b->ref));   // folded reductions are decided by the upload
    for (int i = 0; i < b->B; i++) HIPCHK(hipStreamSynchronize(b->hs[i]->stream));
    if (!b->stream) {
        HIPCHK(hipStreamCreate(&b->stream));
        HIPCHK(b->timer.create());
        HIPCHK(b->devs.alloc(b->B)); HIPCHK(b->dstates.alloc(b->B)); HIPCHK(b->par.alloc(b->B)); HIPCHK(b->counts.alloc(2 * (size_t)b->B));
        b->h_devs.resize(b->B); b->h_states.resize(b->B); b->h_par.resize(b->B);
        if (b->ref) { HIPCHK(b->refs.alloc(b->B)); b->h_refs.resize(b->B); }
    }
    BigBatchGrid g{b->B, 0, 0, 0, 0};
    for (int i = 0; i < b->B; i++) {
        const lpbox_big *h = b->hs[i];
        g.cols = std::max(g.cols, h->G); g.y = std::max(g.y, std::max(h->G, h->Gl));
        g.rows = std::max(g.rows, h->P > 1 ? h->Glr : h->Gl); g.z4 = std::max(g.z4, h->Gl);
    }
    if (g.cols != b->grid.cols || g.y != b->grid.y || g.rows != b->grid.rows || g.z4 != b->grid.z4) b->graphs.clear();
    b->grid = g;
    b->pack_valid = false;
    b->inited = true;
    return 1;
}

// ADMM_lp_iters (LPcpp:766-1095) of every member over [iter_start, iter_end); rets[i] = member i's return value
int lpbox_big_batch_iterate(lpbox_big_batch_t *b, int iter_start, int iter_end, int *rets) {
    if (!b) return lpbox_fail(LPBOX_E_BADHANDLE, "bad handle");
    if (!b->inited) return lpbox_fail(LPBOX_E_STATE, "lpbox_big_batch_init has not been called");
    for (int i = 0; i < b->B; i++) {
        CHK(bigb_member_ok(b->hs[i], i, b->ref));
        if (!b->hs[i]->inited) return lpbox_fail(LPBOX_E_STATE, "problem %d of the batch: solve_init has not been called", i);
    }
    CHK(use_device(b->device));
    hipStream_t st = b->stream;
    for (int i = 0; i < b->B; i++) HIPCHK(hipStreamSynchronize(b->hs[i]->stream));     // windows of its own in between have completed
    // one ping-pong parity for the chain: a member that ran windows of its own in between may sit on the other one
    int parity = b->hs[0]->parity;
    long long copies = 0;
    for (int i = 1; i < b->B; i++) {
        lpbox_big *h = b->hs[i];
        if (h->parity != parity) { HIPCHK(big_launch_resume(h->dev(), 0, &h->parity, st)); copies++; }   // st[in] -> st[out]; no halt is pending between windows
    }
    for (int i = 0; i < b->B; i++) b->h_devs[i] = b->hs[i]->dev();
    HIPCHK(hipMemcpyAsync(b->devs.p, b->h_devs.data(), sizeof(BigDev) * (size_t)b->B, hipMemcpyHostToDevice, st));
    if (b->ref) {
        int kinds = 0;
        for (int i = 0; i < b->B; i++) { b->h_refs[i] = *b->hs[i]->rf(); kinds |= b->h_refs[i].valued ? BIGREF_KIND_VALUED : BIGREF_KIND_UNIT; }
        if (kinds != b->kinds) b->graphs.clear();                // the captured launches carry the y entries of the kinds they were captured with
        b->kinds = kinds;
        HIPCHK(hipMemcpyAsync(b->refs.p, b->h_refs.data(), sizeof(BigRef) * (size_t)b->B, hipMemcpyHostToDevice, st));
    }
    HIPCHK(b->timer.start(st));
    const long long l0 = b->launches;
    b->launches += copies; b->parity_copies += copies;
    HIPCHK(bigb_launch_set_window(b->devs.p, b->grid, iter_start, iter_end, &parity, st));
    b->launches++;
    std::vector<long long> resumes(b->B, 0);
    const int rc = bigb_chain(b, b->B, nullptr, iter_end, &parity, resumes.data());
    double ms = 0.0;
    const hipError_t e = b->timer.stop_sync(st, &ms);
    if (rc < 0) return rc;
    HIPCHK(e);
    b->kernel_ms += ms;
    for (int i = 0; i < b->B; i++) {
        lpbox_big *h = b->hs[i];
        h->hst = b->h_states[i]; h->parity = parity; h->win_serial++;
        h->chain.pcg_resumes += resumes[i];
        if (rets) rets[i] = h->hst.ret;
    }
    b->hs[0]->kernel_ms += ms; b->hs[0]->launches += b->launches - l0;      // the chain's launches are nobody's in particular: booked on member 0
    return LPBOX_OK;
}

int lpbox_big_batch_set_active(lpbox_big_batch_t *b, const unsigned char *active) {
    if (!b) return lpbox_fail(LPBOX_E_BADHANDLE, "bad handle");
    for (int i = 0; i < b->B; i++) b->active[i] = active ? (active[i] ? 1 : 0) : 1;
    return LPBOX_OK;
}

int lpbox_big_batch_iterate_l2f(lpbox_big_batch_t *b, int iter_start, int iter_end, const double *vecs, long vec_stride, const long *nums, int *rets) {
    if (!b) return lpbox_fail(LPBOX_E_BADHANDLE, "bad handle");
    if (b->ref) return bigb_no_fixing();
    return bigb_window(b, iter_start, iter_end, false, vecs, vec_stride, nums, nullptr, 0.0, 0.0, 0, rets, nullptr);
}

int lpbox_big_batch_iterate_l2f_scores(lpbox_big_batch_t *b, int iter_start, int iter_end, const float *scores_dev, double hi, double lo, int min_fix,
                                       int *rets, int *fixed) {
    if (!b) return lpbox_fail(LPBOX_E_BADHANDLE, "bad handle");
    if (b->ref) return bigb_no_fixing();
    return bigb_window(b, iter_start, iter_end, true, nullptr, 0, nullptr, scores_dev, hi, lo, min_fix, rets, fixed);
}

// the (rows x ws) windows of all active members, one after the other, in ONE buffer of the batch (one launch)
int lpbox_big_batch_get_x_iters_device(lpbox_big_batch_t *b, int ws, void **dev_ptr, long *row_off) {
    if (!b) return lpbox_fail(LPBOX_E_BADHANDLE, "bad handle");
    if (b->ref) return bigb_no_fixing();
    if (ws <= 0 || ws > LP_XITERS_COLS) return lpbox_fail(LPBOX_E_BADARG, "ws = %d outside (0,%d]", ws, LP_XITERS_COLS);
    if (!b->inited) return lpbox_fail(LPBOX_E_STATE, "lpbox_big_batch_init has not been called");
    const std::vector<int> act = active_members(b->active);
    const int A = (int)act.size();
    for (int k = 0; k < A; k++) {
        const lpbox_big *h = b->hs[act[k]];
        if (!h->inited || !h->xi_valid || h->xi_plain || !h->dlive_valid)
            return lpbox_fail(LPBOX_E_STATE, "problem %d of the batch: solve_iter_l2f has not been called", act[k]);
    }
    CHK(use_device(b->device));
    std::fill(b->pack_serial.begin(), b->pack_serial.end(), -1L);
    long tot = 0, max_rows = 0;
    for (int i = 0, k = 0; i < b->B; i++) {
        b->row_off[i] = tot;
        if (k < A && act[k] == i) {
            const lpbox_big *h = b->hs[i];
            HIPCHK(hipStreamSynchronize(h->stream));
            b->h_devs[k] = h->dev();
            BigFixPar &p = b->h_par[k];
            p.apply = 0; p.clear = 0; p.rows = h->xi_rows; p.row0 = (int)tot; p.n_live_new = h->xi_rows; p.c1_new = 0.0; p.live_idx = h->d_live_idx.p;
            tot += h->xi_rows; max_rows = std::max<long>(max_rows, h->xi_rows);
            b->pack_serial[i] = h->win_serial; k++;
        }
    }
    b->row_off[b->B] = tot;
    if ((double)tot * ws > 2147483647.0) return lpbox_fail(LPBOX_E_TOOLARGE, "%ld rows of %d iterates exceed the packed buffer's 2^31 - 1 entries", tot, ws);
    const size_t need = (size_t)std::max<long>(tot, 1) * ws;
    if (b->pack.count < need) { HIPCHK(hipStreamSynchronize(b->stream)); HIPCHK(b->pack.alloc(need)); }       // grows on demand
    if (A > 0 && tot > 0) {
        BigBatchGrid g = b->grid;
        g.B = A;
        CHK(bigb_upload_devs(b, A));
        CHK(bigb_upload_par(b, A));
        HIPCHK(bigb_launch_pack(b->devs.p, b->par.p, g, (int)max_rows, ws, b->pack.p, b->stream));
        HIPCHK(hipStreamSynchronize(b->stream));
        b->launches++; b->hs[act[0]]->launches++;
    }
    b->packs++;
    b->pack_valid = true;
    if (dev_ptr) *dev_ptr = b->pack.p;
    if (row_off) for (int i = 0; i <= b->B; i++) row_off[i] = b->row_off[i];
    return LPBOX_OK;
}

int lpbox_big_batch_get_scalar(lpbox_big_batch_t *b, const char *name, double *out) {
    if (!b || !name || !out) return lpbox_fail(LPBOX_E_BADARG, "bad handle / name / output");
    if (!strncmp(name, "pcg_resumes_", 12)) {
        char *end = nullptr;
        const long i = strtol(name + 12, &end, 10);
        if (end == name + 12 || *end || i < 0 || i >= b->B) return lpbox_fail(LPBOX_E_BADARG, "'%s': no such member", name);
        *out = (double)b->hs[i]->chain.pcg_resumes;
        return LPBOX_OK;
    }
    struct { const char *n; double v; } tab[] = {
        {"count", (double)b->B}, {"launches", (double)b->launches}, {"kernel_ms", b->kernel_ms}, {"kmax", (double)b->chain.kmax},
        {"graph", b->use_graph ? 1.0 : 0.0}, {"parity_copies", (double)b->parity_copies},
        {"grid_cols", (double)b->grid.cols}, {"grid_y", (double)b->grid.y}, {"grid_rows", (double)b->grid.rows}, {"grid_z4", (double)b->grid.z4},
        {"active", (double)std::count(b->active.begin(), b->active.end(), (uint8_t)1)}, {"fix_launches", (double)b->fix_launches},
        {"packs", (double)b->packs}, {"compact_chunk", (double)(BIG_CT * BIG_CE)},
        {"order", b->ref ? (double)LPBOX_ORDER_REFERENCE : (double)LPBOX_ORDER_DEFAULT},
        {"valued_members", (double)std::count_if(b->hs.begin(), b->hs.end(), [](const lpbox_big *h) { return h->valued; })}, {"walks", (double)b->walks},
    };
    for (auto &e : tab) if (!strcmp(e.n, name)) { *out = e.v; return LPBOX_OK; }
    return lpbox_fail(LPBOX_E_BADARG, "unknown scalar '%s'", name);
}

}  // extern "C"
