// lpbox_big.h -- internal layout of the LARGE-instance LP path (BASELINE config 5: one LP with up to ~1e6 variables,
// variable-sharded over the GPUs of a node).  Not part of the C-ABI.
//
// A rank owns the contiguous column block [c0, c1) of E (all rows): its n-vectors x, y1, y2, z1, z2, b, ... are local,
// the l-vectors y3, z4, f, E*x, E*p are REPLICATED (every rank computes all l entries).  One ADMM iteration is a chain of
// kernels cut at the grid-wide dependencies; where the algorithm needs a sum over all variables the chain has a collective:
//   * E*v  = sum over ranks of E[:, shard] * v_shard      -> all-reduce of an l-vector (once per PCG iteration + 2 per outer)
//   * dot products / norms                                 -> all-reduce of <= 5 scalars
// (north_star's "one all-reduce per iteration" under-counts: SURVEY section 8e.)  With one rank the collectives vanish and
// the path is bit-comparable with the oracle (two-level reduction order, rows and columns summed in ascending order).
// Control state lives on the device (BigState, ping-ponged), kernels fall through once the PCG has converged / the solver
// has stopped, so the host enqueues a static sequence.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lpbox_lp.h"   // hyper-parameters LP_* (LPcpp:491-507) and stop reasons

#define BIG_T 256
#define BIG_NPART 8
#define BIG_MAXW 16        // ranks whose workgroup counts fit the descriptor (folded reductions; more ranks use the reduction launch)
#define BIG_FOLD_U 4       // folded reductions: at most this many workgroup partials per thread (G <= BIG_FOLD_U * BIG_T)
// Workgroup partials are kept per PHASE of the chain (a kernel that consumes the partials of one phase while it produces those of the
// next must not overwrite what a slower workgroup still has to read): A prep -> y, B resid -> rows(first), C pcg_cols -> pcg_upd,
// D pcg_upd -> rows / post, E post -> prep; X = the rare passes (init, fix), always reduced by big_k_fin.
enum { BIG_PH_A = 0, BIG_PH_B, BIG_PH_C, BIG_PH_D, BIG_PH_E, BIG_PH_X, BIG_PH_COUNT };

enum { BIG_HALT_NONE = 0, BIG_HALT_STOP = 1, BIG_HALT_WINDOW = 2, BIG_HALT_PCG_MORE = 3 };

struct BigState {
    double rho1, rho2, rho4, prev_rho1, prev_rho2, prev_rho4, gamma_val, dI, r4Et, rcr;
    double std_obj, cur_obj, best_bin_obj, cvg1, cvg2, obj_val, c1;
    double hist[LP_HIST];
    double threshold, absNew, rhsNorm2, beta;
    int rhoUpdated, hist_n, iter, iter_start, iter_end, have_prev, halt, stop, ret;
    int pcg_k, pcg_done, pcg_first, phase;
    int pcg_total, outer_total, last_pcg, plain_iter_p1, pcg_max, expr_ready;
    int l2f, cc, n_live_lo, n_live_hi;      // l2f window semantics (LPcpp:1098-1574); x_iters column; live variables (all ranks), 2 x 31 bits
    double sum_fix_obj, fix_obj, prev_sum, prev_obj;
    int rec;                                // plain loop: keep x of every iteration in xhist too (print_fix_info 2, LPcpp:903-909)
};

struct BigDev {
    int n_loc, l, G, Gl, EPT, EPTl;       // G workgroups over the local variables, Gl over the rows
    int P, Glr;                           // column slices of the row-side storage (1 = plain CSR); workgroups of big_k_rows at one row per thread
    long n_glob;
    // E restricted to the local columns: CSR (rows -> local column index; slice-major when P > 1: rptr has P * l + 1 entries, see
    // row_sum_sliced) and CSC (local column -> rows), values all 1
    const int *rptr, *rcol, *cptr, *crow;
    double *x, *y1, *y2, *z1, *z2, *b, *pd, *dinv, *rhs, *r, *z, *tmp, *p0, *p1, *gsrc;   // local n-vectors
    double *y3, *z4, *f, *Ex, *q;         // replicated l-vectors (q doubles as the all-reduce buffer of E*v)
    double2 *fz;                          // (f - y3, z4) per row: the two l-vectors the rhs assembly gathers, as ONE 16-byte element
    double2 *zp;                          // (z, p) of the last PCG update packed per variable: ONE 16-byte gather per entry of E*p
    double *xt;                           // PCG iterate (committed to x for the live variables after the PCG)
    uint8_t *live;                        // 1 live, 0 fixed (x holds the fixed value)
    const uint8_t *newfix;                // this call's fix request: 0 none, 1 -> 0.0, 2 -> 1.0
    double *xhist; int ws_cap;            // x_iters staging [ws_cap][n_loc]
    double *part;                         // [BIG_PH_COUNT][BIG_NPART][Gs] workgroup partials (Gs = partial stride, the same on every rank)
    double *red;                          // [BIG_PH_COUNT][BIG_NPART] reduced scalars of each phase (all-reduced over the ranks) -- the route
                                          // with a reduction launch.  Per phase: a chain that halts inside the PCG still runs the launches
                                          // enqueued behind it, and the resumed PCG needs the totals it halted on
    // FOLDED reductions (G <= BIG_FOLD_U * BIG_T): no reduction launch -- every consumer workgroup adds up the workgroup partials itself
    // (same two-level tree, same bits); with W > 1 ranks the partials of all ranks are all-gathered into gpart[phase][rank][nv][Gs]
    // and every consumer runs rank r's tree over its Gr[r] partials, then adds the W totals in rank order (what big_k_rank_sum did).
    int fold, W, gathered, Gs, Gr[BIG_MAXW];      // gathered: the consumers read gpart (W > 1, or an RCCL communicator of one rank)
    const double *gpart;
    // opt-in COMM-LEAN PCG (lpbox_big_set_pcg_mode; NOT the reference's arithmetic): the step length comes from
    // p.Mp = dI (p.p) + r4Et (q.q), q = E p.  p.p partials (one per column workgroup) and q.q partials (one per row workgroup: of the
    // row gather on one rank, of the rank's row block otherwise) sit in lsmall[0 .. Gs) and lsmall[Gs .. Gs + Gqs); with W > 1 they ride
    // with the q exchange into gsmall[rank][Gs + Gqs].  pcg_cols and pcg_upd become ONE kernel, the p.Mp exchange disappears.
    int lean, Gq, Gqs, Gqr[BIG_MAXW];
    double *lsmall; const double *gsmall;
    BigState *st;                         // st[0], st[1]
};

// launch helpers (lpbox_big_kernels.hip); every state-carrying launch reads st[*parity], writes st[*parity^1], flips *parity.
// rf: nullptr in the default order; the reference-order descriptor (below) otherwise -- the same launch over the same grid, with the
// phase's terms staged for the walker instead of summed per workgroup, and with the stored values where rf->valued.
struct BigRef;
hipError_t big_launch_init(const BigDev &d, const BigRef *rf, double c1, hipStream_t s);      // state, x = 1, b.x0: partial -> red[0], or staged (the caller ranks and walks)
hipError_t big_launch_init2(const BigDev &d, hipStream_t s);               // best_bin_obj = red[0] (after the all-reduce)
hipError_t big_launch_set_window(const BigDev &d, int iter_start, int iter_end, int l2f, int *parity, hipStream_t s);
hipError_t big_launch_fix1(const BigDev &d, const BigRef *rf, hipStream_t s);                          // gsrc = newly fixed values, terms of b.x2 (:1237)
hipError_t big_launch_fix2(const BigDev &d, const BigRef *rf, int *parity, hipStream_t s);              // f -= E2 x2 (:1278), mask, terms of |x_live|^2
hipError_t big_launch_fix3(const BigDev &d, const BigRef *rf, long n_live_new, double c1_new, int *parity, hipStream_t s);   // state + update_expression (:1329)
hipError_t big_launch_pack_xiters(const BigDev &d, const int *live_idx, int rows, int ws, double *out, hipStream_t s);
hipError_t big_launch_prep(const BigDev &d, const BigRef *rf, int do_prep, int *parity, hipStream_t s);
hipError_t big_launch_fin(const BigDev &d, int nv, int phase, hipStream_t s);         // partials of a phase -> red[0..nv)
hipError_t big_launch_y(const BigDev &d, const BigRef *rf, int *parity, hipStream_t s);                 // y1, y2, refresh, rhs base, y3 (all rows)
hipError_t big_launch_rhs_cols(const BigDev &d, const BigRef *rf, int *parity, hipStream_t s);          // rhs += r4Et E^T(f-y3) - E^T z4
hipError_t big_launch_rows(const BigDev &d, const BigRef *rf, int mode, int *parity, hipStream_t s);    // q = E[:,shard] * v  (mode 0: gsrc, 1: PCG p)
hipError_t big_launch_resid(const BigDev &d, const BigRef *rf, int *parity, hipStream_t s);
hipError_t big_launch_pcg_cols(const BigDev &d, const BigRef *rf, int *parity, hipStream_t s);
hipError_t big_launch_pcg_upd(const BigDev &d, const BigRef *rf, int *parity, hipStream_t s);
hipError_t big_launch_pcg_lean(const BigDev &d, int *parity, hipStream_t s);          // comm-lean mode: tmp = M p, alpha from p.p and q.q, x / r / z updates, partials (r.r, r.z)
hipError_t big_launch_rank_sum_qq(const double *g, int W, long count, long stride, double *out, double *qq_part, hipStream_t s);   // rank-ordered sum of a row block + q.q partials per 256 rows
hipError_t big_launch_post(const BigDev &d, const BigRef *rf, int *parity, hipStream_t s);              // duals z1,z2, terms(5), gsrc = x
hipError_t big_launch_z4(const BigDev &d, int init_only, int *parity, hipStream_t s); // Ex = q [, z4 update]
hipError_t big_launch_resume(const BigDev &d, int reset_pcg_max, int *parity, hipStream_t s);
hipError_t big_launch_rank_sum(const double *g, int W, long count, long stride, double *out, hipStream_t s);   // rank-ordered sum of W gathered contributions

// ---- a BATCH of problems through one launch chain in lockstep (lpbox_big_batch_*; one rank each, folded reductions, plain windows) ----
// devs: device array of B descriptors; every launch has the grid (X, B), X the largest extent of that kernel over the batch -- the
// kernels differ in what they are launched over, so there is one maximum per kind.  Row blockIdx.y of a grid works on problem
// blockIdx.y alone: its own state, partials and vectors, the reduction tree and the row / column order of its own handle.
struct BigBatchGrid {
    int B;
    int cols;      // max G: prep, rhs_cols, resid, pcg_cols, pcg_upd, post
    int y;         // max of max(G, Gl)
    int rows;      // max of (P > 1 ? Glr : Gl)
    int z4;        // max Gl
};
hipError_t bigb_launch_set_window(const BigDev *devs, const BigBatchGrid &g, int iter_start, int iter_end, int *parity, hipStream_t s);
hipError_t bigb_launch_resume(const BigDev *devs, const BigBatchGrid &g, int reset_pcg_max, int *parity, hipStream_t s);
hipError_t bigb_launch_prep(const BigDev *devs, const BigBatchGrid &g, int do_prep, int *parity, hipStream_t s);
hipError_t bigb_enqueue_pcg(const BigDev *devs, const BigBatchGrid &g, int pairs, int *parity, hipStream_t s);      // pairs x (rows(1), pcg_cols, pcg_upd)
hipError_t bigb_enqueue_tail(const BigDev *devs, const BigBatchGrid &g, int *parity, hipStream_t s);                // post, rows(0), z4
hipError_t bigb_enqueue_iterations(const BigDev *devs, const BigBatchGrid &g, int iters, int kmax, int *parity, hipStream_t s);   // 8 + 3 kmax launches each
hipError_t bigb_launch_z4(const BigDev *devs, const BigBatchGrid &g, int *parity, hipStream_t s);                  // the tail's last launch alone
hipError_t bigb_collect_states(const BigDev *devs, const BigBatchGrid &g, int parity, BigState *out, hipStream_t s);   // out[i] = st[parity] of problem i

// ---- early-fixing windows (lpbox_big_iterate_l2f) of a batch: lpbox_big_batch_iterate_l2f / _l2f_scores / _get_x_iters_device ----
// One record per ACTIVE member and window, in the order of devs, uploaded in one copy.  c1_new = pow(n_live_new, 1/2) comes from the
// host's libm as in the one-problem call: a device sqrt is not the same number now and then.
#define BIG_CT 1024        // threads of the live-list compaction ...
#define BIG_CE 4           // ... and entries per thread: chunks of BIG_CT * BIG_CE entries
struct BigFixPar {
    int apply;             // the member fixes in this window (0: it falls through the prologue)
    int clear;             // apply == 0, but fix codes sit in newfix (the guard held the fix back): the compaction launch clears them
    int rows, row0;        // entries of live_idx before this window's fix; first row in the packed buffer / the code staging
    long n_live_new;
    double c1_new;
    int *live_idx;         // the member's live-index list on the device (ascending original indices)
};
hipError_t bigb_launch_set_window_l2f(const BigDev *devs, const BigBatchGrid &g, int iter_start, int iter_end, int *parity, hipStream_t s);
// fix1, fin, rows(gsrc), fix2, fin, fix3, rows(gsrc), z4(init_only): 8 launches, 5 of them move the parity
hipError_t bigb_enqueue_fix(const BigDev *devs, const BigFixPar *par, const BigBatchGrid &g, int *parity, hipStream_t s);
hipError_t bigb_launch_clear_xhist(const BigDev *devs, const BigBatchGrid &g, long max_total, hipStream_t s);      // x_iters = Zero, all ws_cap columns
hipError_t bigb_launch_decide(const BigDev *devs, const BigFixPar *par, const BigBatchGrid &g, int max_rows, const float *scores, const uint8_t *codes,
                              double hi, double lo, int *counts, hipStream_t s);       // newfix codes from scores or host codes; counts[2 * member + {ones, zeros}]
hipError_t bigb_launch_compact(const BigDev *devs, const BigFixPar *par, const BigBatchGrid &g, hipStream_t s);     // live lists in place, codes cleared
hipError_t bigb_launch_pack(const BigDev *devs, const BigFixPar *par, const BigBatchGrid &g, int max_rows, int ws, double *out, hipStream_t s);

// ---- reference-order mode of this path (lpbox_big_set_order(LPBOX_ORDER_REFERENCE), one rank; lpbox_big_ref_kernels.hip) ----
// Every reduction over the live variables follows Eigen's redux (oracle/lpbox_oracle.c redux_sum_eigen): the producers write their
// per-variable terms into `stage` at the variable's LIVE RANK instead of summing them per workgroup, a walker kernel adds them up in
// the four-chain order and leaves the totals in BigDev::red.  The descriptor travels in a kernel argument of its own: BigDev, and with
// it every default-order kernel, is untouched.
#define BIG_REF_MAXV 5     // values of one phase (post)
#define BIG_REF_NSTAGE 13  // staging rows of n_loc doubles: A 1, B 3, C 1, D 2, E 5, X 1 (one set per phase, as BigDev::part)
struct BigRef {
    int valued;                           // any stored value of E differs from 1.0: the VALUED instantiations run
    const double *vcsr, *vcsc;            // the stored values in the order of rcol / crow (valued only)
    double *r4v;                          // rho4_E_transpose, one entry per stored entry in CSC order (valued only; unit: the scalar r4Et)
    double *stage;                        // [BIG_REF_NSTAGE][n_loc]
    int *rank;                            // live rank of every variable (-1: fixed), a device prefix sum at init and in every fix
    int *frank;                           // rank among the variables fixed by the current call (-1: not one of them)
    int *cnt;                             // [0] live variables, [1] variables fixed by the current call
};
__host__ __device__ constexpr int big_ref_stage_off(int phase) {
    return phase == BIG_PH_A ? 0 : phase == BIG_PH_B ? 1 : phase == BIG_PH_C ? 4 : phase == BIG_PH_D ? 5 : phase == BIG_PH_E ? 7 : 12;
}
// mode 0: rank over live -> rank, cnt[0]; 1: over newfix -> frank, cnt[1]; 2: over live && !newfix -> rank, cnt[0] (the live set after the fix)
hipError_t bigref_launch_rank(const BigDev &d, const BigRef &rf, int mode, hipStream_t s);
// red[phase][0..nv) = redux over the first cnt[which] staged terms.  sidx >= 0: skipped when st[sidx] shows that the producer fell through
// (halted chain; for the PCG phases C and D also a finished PCG) -- red[] keeps the totals a resumed PCG needs.
hipError_t bigref_launch_walk(const BigDev &d, const BigRef &rf, int nv, int phase, int which, int sidx, hipStream_t s);
// the staged entries (defined in lpbox_big_ref_kernels.hip, launched by the big_launch_* helpers); _v: the VALUED instantiation
__global__ void bigref_k_init(BigDev d, BigRef rf, double c1);
__global__ void bigref_k_prep(BigDev d, BigRef rf, int in, int out, int do_prep);
__global__ void bigref_k_y_v(BigDev d, BigRef rf, int in, int out);
__global__ void bigref_k_rhs_cols_v(BigDev d, BigRef rf, int in, int out);
__global__ void bigref_k_rows_v(BigDev d, BigRef rf, int in, int out, int mode);
__global__ void bigref_k_resid(BigDev d, BigRef rf, int in, int out);
__global__ void bigref_k_resid_v(BigDev d, BigRef rf, int in, int out);
__global__ void bigref_k_pcg_cols(BigDev d, BigRef rf, int in, int out);
__global__ void bigref_k_pcg_cols_v(BigDev d, BigRef rf, int in, int out);
__global__ void bigref_k_pcg_upd(BigDev d, BigRef rf, int in, int out);
__global__ void bigref_k_post(BigDev d, BigRef rf, int in, int out);
__global__ void bigref_k_fix1(BigDev d, BigRef rf);
__global__ void bigref_k_fix2(BigDev d, BigRef rf, int in, int out);
__global__ void bigref_k_fix3_v(BigDev d, BigRef rf, int in, int out, long n_live_new, double c1_new);

// ---- a batch in lockstep in the reference order (lpbox_big_batch_* whose members all run it) ----
// refs: device array parallel to devs.  The launches are the solo reference chain's, launch for launch, over the grids of BigBatchGrid; a
// walk (bigref_kb_walk, grid (1, B): one walker per member) stands wherever the solo chain has one.  set_window, resume, z4 and collect
// are the bigb_* launches above: no order changes them.
hipError_t bigrefb_launch_prep(const BigDev *devs, const BigRef *refs, const BigBatchGrid &g, int do_prep, int *parity, hipStream_t s);
hipError_t bigrefb_enqueue_pcg(const BigDev *devs, const BigRef *refs, const BigBatchGrid &g, int pairs, int *parity, hipStream_t s);     // pairs x (rows(1), pcg_cols, WALK(1,C), pcg_upd, WALK(2,D))
hipError_t bigrefb_enqueue_tail(const BigDev *devs, const BigRef *refs, const BigBatchGrid &g, int *parity, hipStream_t s);               // post, WALK(5,E), rows(0), z4
// kinds: which kinds of member the batch has.  Unit and valued members share every launch but y, which has an entry per kind.  An
// iteration is 11 + 5 kmax launches, 3 + 2 kmax of them walks; one more (the second y) when the batch has both kinds.
enum { BIGREF_KIND_UNIT = 1, BIGREF_KIND_VALUED = 2 };
hipError_t bigrefb_enqueue_iterations(const BigDev *devs, const BigRef *refs, const BigBatchGrid &g, int kinds, int iters, int kmax, int *parity, hipStream_t s);
