/*
 * lpbox_hip.h -- C-ABI of liblpbox_hip.so, the MI355X (gfx950) Lp-Box ADMM inner solver.
 *
 * This is the drop-in boundary for the reference's Cython solver API.  Each entry point names the
 * reference interface it replaces ("LP pxd" = LinerProgramming/LinearProgramming/cython_solver/LPboxADMMsolver.pxd,
 * "LP pyx" = .../cython_solver/lpbox.pyx, "LPcpp" = .../cython_solver/LPboxADMMsolver.cpp,
 * "SEG pxd/pyx/cpp" = Segmentation/Segmentation/cython/src/{LPboxADMMsolver.pxd,lpbox.pyx,LPboxADMMsolver.cpp}).
 *
 * Conventions
 *  - plain C types only: pointers + sizes, caller-owned buffers, no ownership ever returned
 *    (the reference returns leaked `new double[]`, LPcpp:1620,1657,1677 -- not reproduced);
 *  - every function returns an int status unless documented otherwise: 0 (or a non-negative
 *    payload) = ok, < 0 = LPBOX_E_* error; lpbox_last_error() gives the text.  Nothing calls exit();
 *  - one handle owns one HIP stream; calls on a handle are synchronous and must be serialised by the
 *    caller; different handles may be used from different host threads;
 *  - all arithmetic is fp64 (LPh:16), indices int32 on the API, uint16 inside the kernels;
 *  - there is NO CPU fallback: without a HIP device every compute call fails with LPBOX_E_NODEVICE.  Only the questions about the
 *    planned layout of an LP batch, which no device is involved in, are answered without one: lpbox_get_config, lpbox_get_pcg_loop,
 *    lpbox_get_layout, lpbox_get_row_split, lpbox_get_col_split, lpbox_get_wave_classes, lpbox_get_direct_rows and
 *    lpbox_debug_get_lp_table.  All but lpbox_get_direct_rows plan the layout, which freezes the problem and the
 *    summation order of the handle as lpbox_init does.
 */
#ifndef LPBOX_HIP_H
#define LPBOX_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define LPBOX_OK            0
#define LPBOX_E_BADHANDLE  -1
#define LPBOX_E_BADARG     -2
#define LPBOX_E_STATE      -3   /* call order violated (e.g. iterate before init) */
#define LPBOX_E_IO         -4   /* instance file missing / unparsable (LPcpp:2409-2412 would exit(-1)) */
#define LPBOX_E_HIP        -5   /* HIP runtime error, text in lpbox_last_error() */
#define LPBOX_E_NODEVICE   -6
#define LPBOX_E_UNSUPPORTED -7  /* instance outside what the persistent kernels hold on-chip */
#define LPBOX_E_NOMEM      -8
#define LPBOX_E_TOOLARGE   -9   /* lpbox_init: the instance fits neither the register slots nor the LDS of one CU -- same algorithm,
                                   other entry points: lpbox_big_* (the drop-in classes route there by this code, not by the text) */

#define LPBOX_FLAVOUR_LP   0    /* min b'x  s.t. Ex<=f, x in {0,1}^n      (LPcpp) */
#define LPBOX_FLAVOUR_SEG  1    /* min x'Ax + b'x, x in {0,1}^n           (SEGcpp) */

typedef struct lpbox_solver lpbox_t;      /* one or a batch of independent instances on one GPU */

/* ---- library / device ---------------------------------------------------------------------- */
const char *lpbox_version(void);
const char *lpbox_last_error(void);               /* thread-local text of the last failure */
int lpbox_last_status(void);                       /* the LPBOX_E_* code that came with that text (for calls that return a pointer) */
int  lpbox_device_count(void);                    /* number of HIP devices visible (0 if none) */
int  lpbox_set_device(int device);                /* device used by handles created afterwards on this thread */

/* ---- object life-cycle ---------------------------------------------------------------------- */
/* LP pxd:6-8 / LP pyx:13-14  `LPboxADMMsolver(int print_info)`  (SEG pyx:14-15 for flavour SEG).
 * batch = number of independent instances held by the handle (1 = the reference's single object). */
lpbox_t *lpbox_create(int flavour, int batch, int print_info);
void     lpbox_destroy(lpbox_t *h);

/* ---- problem input (instance index idx in [0,batch)) ------------------------------------------ */
/* What readFile leaves in the object (LPcpp:2446-2545): E (l x n) column-major, row indices ascending in a
 * column, vals = the stored values in the same order (NULL means all ones), b ALREADY NEGATED (LPcpp:2520), f (NULL means all
 * ones, LPcpp:2522).  A handle in the default summation order holds E as a 0/1 pattern: a stored value other than 1.0 ->
 * LPBOX_E_UNSUPPORTED.  After lpbox_set_order(h, LPBOX_ORDER_REFERENCE) any finite value is accepted (negative, zero and tiny ones
 * included: an explicit zero stays a stored entry, as in the reference's readSparseMat, LPcpp:2416-2444); a non-finite value ->
 * LPBOX_E_BADARG.  The same holds for the two file readers below, which negate the values for k == 2 and sum duplicate triplets as
 * the reference does.  Values that are all exactly 1.0 make a unit instance.
 * b may hold any FINITE values: either sign, zeros, subnormals, any scale whose squares do not overflow.  A NaN
 * or an infinity in b -> LPBOX_E_BADARG with the index in lpbox_last_error(), here and in the two file readers, before any device
 * call.  A deliberate deviation: the reference accepts such a vector and computes garbage (a NaN runs every x-update to the PCG cap). */
int lpbox_set_problem_lp(lpbox_t *h, int idx, int n, int l, int nnz, const int *colptr, const int *rowidx,
                         const double *vals, const double *b, const double *f);
/* LP pxd:9 `void readFile(int,int,int)` (LPcpp:2446-2545) with the two paths explicit; k as in the reference. */
int lpbox_read_files_lp(lpbox_t *h, int idx, const char *path_C, const char *path_b, int k);
/* LP pxd:9 verbatim: instance i, k items, j bids under `<root>/instance/<k>_<j>/instance_<i>_{C,b}.txt`;
 * root NULL = the reference's "../cython_solver/data" relative to the CWD (LPcpp:2451). */
int lpbox_read_file(lpbox_t *h, int idx, const char *root, int i, int k, int j);

/* The instance as set_problem / readFile left it in the handle (what LPcpp:2446-2545 leaves in the solver's members n, l, E, b, f): sizes
 * always, arrays where the pointer is not NULL (colptr n+1, rowidx nnz, b n, f l).  Used by the Python class to hand an instance
 * that exceeds the on-chip kernel (max(n, l) > 2048) over to the large-instance path. */
int lpbox_get_problem_lp(lpbox_t *h, int idx, int *n, int *l, int *nnz, int *colptr, int *rowidx, double *b, double *f);
/* The stored values of E of that instance, in the order of rowidx (column-major); ones for a unit instance.  Returns nnz; vals == NULL
 * only queries the count. */
int lpbox_get_problem_lp_vals(lpbox_t *h, int idx, double *vals);

/* ---- solver (whole batch per call) ------------------------------------------------------------ */
/* LP pxd:10 `int ADMM_lp_iters_init()` (LPcpp:489-763).  Returns 1 like the reference. */
int lpbox_init(lpbox_t *h);
/* LP pxd:11 `int ADMM_lp_iters(int,int)` (LPcpp:766-1095).  rets[batch] receives each instance's return value
 * (1 iff stopped by the objective-std test, LPcpp:977-979); may be NULL.  Function returns rets[0]. */
int lpbox_iterate(lpbox_t *h, int iter_start, int iter_end, int *rets);
/* LP pxd:13 `int ADMM_lp_iters_l2f(int,int,double*,int)` (LPcpp:1098-1574).
 * vec: for instance idx the fix vector starts at vec + idx*vec_stride and holds >= n_live entries in {1,0,-1}
 * over the CURRENT live variables; nums[idx] = count of non -1 entries (0 = ignore vec, as LPcpp:1124).
 * rets[batch] as above (1 = converged / all fixed / PCG broke down).  Function returns rets[0]. */
int lpbox_iterate_l2f(lpbox_t *h, int iter_start, int iter_end, const double *vec, long vec_stride,
                      const int *nums, int *rets);

/* ---- results (instance idx) ------------------------------------------------------------------- */
int lpbox_get_n(lpbox_t *h, int idx);                         /* LP pxd:15 get_n(): live variables          */
int lpbox_get_org_n(lpbox_t *h, int idx);                     /* SEG pxd get_org_n(); original n            */
int lpbox_get_l(lpbox_t *h, int idx);
int lpbox_get_iter(lpbox_t *h, int idx);                      /* LP pxd:16 get_iter() (LPh:347-349)         */
/* LP pxd:14 `double* get_x_iters_d(int)` (LPcpp:1616-1627): out[rows*ws] row-major, rows = n_live of the last
 * l2f call; returns rows.  out may be NULL to query rows. */
int lpbox_get_x_iters(lpbox_t *h, int idx, int ws, double *out);
/* Plain loop with print_fix_info 2/3 (LPcpp:776-779, 903-909, 940-946, 986-992): the reference streams x_sol of every iteration to
 * <root>/xiter/<k>_<j>_xiters_<i>.csv.  With record on, lpbox_iterate keeps those iterates on the device (one column per iteration of the
 * call, exactly like the x_iters window of the l2f loop) and lpbox_get_x_iters / _device hand them out; the CSV itself is written by the
 * host wrapper.  Off by default. */
int lpbox_set_record(lpbox_t *h, int on);
/* LP flavour, OPT-IN and without a reference counterpart: how the x-update solves ((rho1+rho2) I + rho4 E^T E) x = rhs (the system of
 * LPcpp:872-894).  LPBOX_XUPDATE_PCG (default) = the reference's Jacobi-PCG to 1e-3 (LPcpp:251-335), bit-exact against the oracle of the
 * reference's algorithm.  LPBOX_XUPDATE_DIRECT = an exact solve through the Woodbury identity with a dense l x l inverse kept in LDS
 * (DESIGN.md section 17): a different (more accurate) x-update, hence different iterates and iteration counts than the reference's;
 * available for n <= 512 with at most 128 rows of E that share columns with other rows (the XOR rows of an auction do not).  May be switched between calls; returns LPBOX_E_UNSUPPORTED when the batch does not fit. */
#define LPBOX_XUPDATE_PCG 0
#define LPBOX_XUPDATE_DIRECT 1
int lpbox_set_x_update(lpbox_t *h, int mode);
/* LP flavour, OPT-IN: the summation order of the on-chip kernels.  LPBOX_ORDER_DEFAULT (default) = the tuned layout, bit-exact against the
 * oracle run in the kernels' own association.  LPBOX_ORDER_REFERENCE = every dot product / norm over the live variables in the order of
 * Eigen 3.3.8's SSE2 redux, every row of E v and column of E^T w summed sequentially in ascending index order:
 * the same iterates, binary solution and iteration counts as the reference's Eigen path, except that the std stop test takes sqrt where
 * the reference calls pow(v, 1/2).  Only before the problem is uploaded (LPBOX_E_STATE after lpbox_init / lpbox_get_config / ...);
 * LPBOX_E_UNSUPPORTED together with the direct x-update or the iteration log (either call order).  An instance beyond the on-chip
 * limit makes lpbox_init fail with LPBOX_E_TOOLARGE.  lpbox_get_layout / _row_split / _col_split then report the identity layout,
 * one lane per row and whole columns.
 * The reference order is also the one that carries STORED VALUES of E other than 1 (lpbox_set_problem_lp): choose
 * it before handing such an instance over.  A batch with a valued instance runs the valued variants of these kernels, bit-exact against
 * the same oracle; going back to LPBOX_ORDER_DEFAULT on a handle that holds a valued instance -> LPBOX_E_UNSUPPORTED. */
#define LPBOX_ORDER_DEFAULT 0
#define LPBOX_ORDER_REFERENCE 1
int lpbox_set_order(lpbox_t *h, int mode);
/* The row split of the direct mode for instance idx (the order of its arithmetic; tests hand it to the oracle's mirror): gidx_of_row[l] =
 * dense index of the row among the rows solved through the on-chip inverse, -1 for a row handled in closed form (its columns meet no
 * other such row).  Returns the number of dense rows.  A function of the instance alone: it answers before lpbox_set_x_update and
 * without a device. */
int lpbox_get_direct_rows(lpbox_t *h, int idx, int *gidx_of_row);
/* Segmentation flavour: with record on (on == 1: up to 2000 iterations, on > 1: that many), lpbox_seg_legacy keeps x_sol of every iteration
 * (print_info 1 -> ../xiter/<problem>.csv, SEGcpp:1209-1213, 1270-1277).  out == NULL: number of iterations recorded; otherwise copies
 * iterations [first, first+count) as count rows of org_n doubles. */
int lpbox_seg_get_x_history(lpbox_t *h, int first, int count, double *out);
/* ---- the early-fixing policy's encoder, fused on the device (the step either side of the solver in LP/trainer.py:523-535) ----
 * GraphAttentionEncoder up to its flatten (LP/mha.py:202-243; SEG/mha.py same with 5 tokens), eval mode, fp16 MFMA with fp32
 * accumulation.  x_dev: fp64 iterates (typically the buffer lpbox_get_x_iters_device returns); variable r's token t is
 * x_dev[row_off_dev[r] + t*tok_stride + 0..4] (LP/trainer.py:526-527 -> tok_stride 5, tokens 20; SEG/trainer.py:721-725 ->
 * tok_stride 1, tokens 5).  weights_dev / consts_dev: packed as csrc/lpbox_policy.h describes (lpbox_hip/policy.py packs a
 * reference state_dict); lpbox_policy_layout gives their sizes.  out_dev: fp16 [rows][tokens*128].  Asynchronous on hip_stream. */
int lpbox_policy_layout(int tokens, long *weight_halves, long *const_floats);
int lpbox_policy_encode_f16(const double *x_dev, const long long *row_off_dev, long rows, int tokens, int tok_stride,
                            const void *weights_dev, const float *consts_dev, void *out_dev, void *hip_stream);
/* The same encoder in FLOAT32 on the matrix cores (v_mfma_f32_16x16x4_f32: f32 in, f32 accumulate -- the reference's arithmetic, LP/mha.py
 * evaluates in float32) at usable speed.  weights_dev: f32 fragments packed by lpbox_hip/policy.py (lpbox_policy_f32frag_layout gives the
 * count; csrc/lpbox_policy_f32_kernels.hip documents the order), consts_dev: the SAME constant block as lpbox_policy_encode_f16.
 * out_dev: float [rows][tokens*128].  Asynchronous on hip_stream. */
int lpbox_policy_f32frag_layout(int tokens, long *weight_floats, long *const_floats);
int lpbox_policy_encode_f32(const double *x_dev, const long long *row_off_dev, long rows, int tokens, int tok_stride,
                            const float *weights_dev, const float *consts_dev, float *out_dev, void *hip_stream);
/* The whole network -- encoder and MLP head -- in fp32 on the device, one workgroup per variable: the reference's arithmetic
 * (LP/mha.py evaluates in float32), for fixing decisions near a threshold and as the fp32 check of the fused kernel; not a fast
 * path.  weights_dev: floats in the order csrc/lpbox_policy_kernels.hip documents (lpbox_policy_f32_layout gives the count);
 * sigmoid_dev[rows] (and logit_dev[rows] if not NULL) receive the scores.  Asynchronous on hip_stream. */
int lpbox_policy_f32_layout(int tokens, long *weight_floats);
int lpbox_policy_score_f32(const double *x_dev, const long long *row_off_dev, long rows, int tokens, int tok_stride,
                           const float *weights_dev, float *sigmoid_dev, float *logit_dev, void *hip_stream);
/* The same kernel as a filter: sigmoid_dev[rows] already holds scores (the fused fp16 path's); every variable whose score lies within
 * `band` of thr_hi or thr_lo is re-evaluated in fp32 and overwritten, the others are left alone; *count_dev (optional, device) is
 * incremented per re-scored variable.  No host round trip: the selection happens on the device. */
int lpbox_policy_rescore_f32(const double *x_dev, const long long *row_off_dev, long rows, int tokens, int tok_stride,
                             const float *weights_dev, float *sigmoid_dev, float band, float thr_hi, float thr_lo,
                             unsigned long long *count_dev, void *hip_stream);
/* Batched use only: park (active[i] == 0) or resume instances.  A parked instance is skipped by lpbox_iterate / _l2f and keeps its
 * state and return code; the reference has no counterpart because its loop simply stops calling a finished solver
 * (LP/trainer.py:511-512).  active == NULL resumes all. */
int lpbox_set_active(lpbox_t *h, const int *active);
/* The same (rows x ws) row-major windows for the WHOLE batch, left on the device: instance idx starts at dev_ptr + idx*stride
 * doubles and holds lpbox_get_x_iters(h, idx, ws, NULL) rows.  Lets a policy network read the iterates without a host
 * round trip (valid until the next solver call). */
int lpbox_get_x_iters_device(lpbox_t *h, int ws, void **dev_ptr, long *stride_doubles);
/* The live rows of the last l2f window of all ACTIVE instances, stacked in instance order, for a policy that reads x_iters on the
 * device.  Packs as lpbox_get_x_iters_device(ws) does if that has not happened.  *row_off_dev: int64[rows], element offset of the
 * row's first iterate in that packed buffer; first_row (may be NULL): B + 1 host ints, rows of instance i are
 * first_row[i] .. first_row[i+1] - 1 (empty for a parked instance).  Returns rows (>= 0). */
long lpbox_get_x_iters_rows_device(lpbox_t *h, int ws, void **row_off_dev, int *first_row);
/* lpbox_iterate_l2f with the fix decided on the device.  scores_dev: float32, one per stacked row of the table above, or NULL = fix
 * nothing.  Per instance deter_fix_2 with the trainer's guard (widened to double: s > hi -> 1, s < lo -> 0, NaN -> nothing; k fixes,
 * k <= min_fix -> nothing fixed).  fixed[B] (may be NULL) = fixes applied.  rets / return value as lpbox_iterate_l2f.  The caller
 * orders its own work on scores_dev before the call.  The table must have been built since the last window, for the active mask that
 * is still in place (LPBOX_E_STATE otherwise; a lpbox_set_active call that repeats the current mask keeps it). */
int lpbox_iterate_l2f_scores(lpbox_t *h, int iter_start, int iter_end, const float *scores_dev, double hi, double lo,
                             int min_fix, int *rets, int *fixed);
int lpbox_get_x_sol(lpbox_t *h, int idx, double *out);        /* LP pxd:17 (LPcpp:1648-1665): out[org_n] in {0,1} */
int lpbox_get_final_x_sol(lpbox_t *h, int idx, double *out);  /* LP pxd:18 (LPcpp:1668-1685): raw live x, returns its length */
int lpbox_cal_obj(lpbox_t *h, int idx, double *out);          /* LP pxd:12 cal_obj() (LPcpp:1630-1642)      */
int lpbox_cur_bin_obj(lpbox_t *h, int idx, double *out);      /* LP pxd:19 get_curBinObj() (LPcpp:1644-1646) */
int lpbox_check_infeasible_lpbox(lpbox_t *h, int idx);        /* LP pxd:20 (LPcpp:1577-1591): count, >= 0   */
int lpbox_check_infeasible_l2f(lpbox_t *h, int idx);          /* LP pxd:21 (LPcpp:1593-1612): count, >= 0   */

/* ---- segmentation flavour (handle created with LPBOX_FLAVOUR_SEG, batch 1) ---------------------
 * The generic entry points above serve it too: lpbox_init = ADMM_bqp_unconstrained_init (SEG pxd:9, SEGcpp:658-810, after the
 * problem has been set), lpbox_iterate_l2f = ADMM_bqp_unconstrained_l2f (SEG pxd:11, SEGcpp:917-1195, windows of <= 10
 * iterations), lpbox_get_x_iters / _get_n / _get_org_n / _get_x_sol (SEG pxd:12-16). */
/* What the reference's init holds after get_A_b_from_cost (SEGcpp:226-248, :755-756): A_ptr = A/2 row-major CSR (columns
 * ascending, every row stores its diagonal), b, the constant c, and the image shape (for save_img). */
int lpbox_set_problem_bqp(lpbox_t *h, int n, int nnz, const int *rowptr, const int *colidx, const double *vals,
                          const double *b, double c, int rows, int cols);
/* The image part of ADMM_bqp_unconstrained_init (SEGcpp:702-756): grayscale pixels (rows x cols, row-major, what
 * cv::imread(path, 0) yields), scaled to ~num_nodes pixels (cv::resize INTER_LINEAR), costs per SEGcpp:46-248. */
int lpbox_seg_set_image(lpbox_t *h, const unsigned char *gray, int rows, int cols, int num_nodes);
/* OPT-IN: the reference's summation order for this flavour, LPBOX_ORDER_DEFAULT / LPBOX_ORDER_REFERENCE as for
 * lpbox_set_order.  REFERENCE = every sum over a problem's live variables (the PCG dot products, the norms of the stop test and of the
 * sphere projection, both compute_cost calls) associated as Eigen 3.3.8's SSE2 redux associates it over the reference's COMPACTED
 * vector, c1 through libm's pow, lpbox_seg_get_obj in the same association: bit for bit oracle/seg_oracle.c in its Eigen order on every
 * vector and scalar, except std_obj (sqrt for pow(v, 1/2): within 2 ulps).  The sparse products and the fix step are the reference's
 * order in both modes.  Call it BEFORE lpbox_seg_set_image / lpbox_set_problem_bqp (the staging rows are allocated with the problem);
 * afterwards -> LPBOX_E_STATE.  Unknown mode -> LPBOX_E_BADARG; an LP-flavour handle -> LPBOX_E_STATE (and lpbox_set_order on a
 * segmentation handle keeps answering LPBOX_E_STATE).  lpbox_debug_get_scalar(h, 0, "order") reports the mode.  Everything else works
 * as in the default order: windows, recording, the launch-chain controls (LPBOX_SEG_KMAX, _KMARGIN, _NOGRAPH, _EPT, _NODIA).
 * lpbox_seg_legacy_batch and lpbox_seg_batch_create take handles that are all in ONE order, problem 0's: a member in the other order
 * -> LPBOX_E_UNSUPPORTED, naming its index.  What it costs: every reduction becomes a walk of n_live / 4 dependent additions by one
 * workgroup per problem; a batch runs its members' walks side by side. */
int lpbox_seg_set_order(lpbox_t *h, int mode);
/* `cv::imread(imagePath, 0)` (SEGcpp:705) without an image library: the luminance plane of a baseline / extended-sequential 8-bit
 * Huffman JPEG, reconstructed with libjpeg's default ISLOW inverse DCT -- bit for bit what libjpeg yields for JCS_GRAYSCALE output,
 * which is what OpenCV's grayscale imread and PIL's draft("L") hand out (csrc/lpbox_jpeg_host.cpp; pinned against PIL in the tests).
 * out == NULL: only *rows / *cols.  Progressive or arithmetic-coded files: LPBOX_E_BADARG with the reason in lpbox_last_error(). */
int lpbox_read_jpeg_gray(const char *path, unsigned char *out, long cap, int *rows, int *cols);
/* SEG pxd:10 `int ADMM_bqp_unconstrained_legacy()` (SEGcpp:1200-1380): *energy = int(cur_obj + c). */
int lpbox_seg_legacy(lpbox_t *h, int *energy);
/* solve_init + solve_iter for `count` segmentation handles (each after lpbox_seg_set_image / lpbox_set_problem_bqp) advanced in lockstep by
 * ONE launch chain -- the workload of image_segmentation.cpp:24-29 (images 0..99 at 1e4 nodes), where a single solve is launch-bound.
 * Per problem the arithmetic is that of lpbox_init + lpbox_seg_legacy on its own (own control state, sums, iteration counts); afterwards
 * every handle answers its getters as usual.  energies[count]. */
int lpbox_seg_legacy_batch(lpbox_t **handles, int count, int *energies);
/* The early-fixing windows of lpbox_iterate_l2f (SEGcpp:917-1195; the loop of SEG/trainer.py:699-745) for a batch of segmentation
 * handles: a batch object that borrows `count` handles (they stay ordinary handles and must outlive it) and owns the descriptor,
 * state and packing buffers.  Per problem the arithmetic is that of the single-handle calls, bit for bit; after any batched window
 * every handle answers every getter and may go on with windows of its own.
 * _create: NULL on refusal, lpbox_last_status() = the code, lpbox_last_error() names the problem's index: LPBOX_E_BADARG empty list, handles on
 *   different devices, one handle twice; LPBOX_E_BADHANDLE not a handle; LPBOX_E_STATE an LP-flavour handle, a handle without image /
 *   problem; LPBOX_E_UNSUPPORTED a recording handle.  No device call.
 * _init: lpbox_init on every handle (upload, reset, one batched init launch); returns 1.
 * _set_active: active[count], NULL = all.  An inactive handle is not touched by the calls below (state, staged window, counters, rets[i]).
 * _iterate_l2f: problem i fixes by vecs + i * vec_stride / nums[i] (validated as lpbox_iterate_l2f does; vecs may be NULL when every
 *   nums[i] is 0), then all active problems run iterations [iter_start, iter_end) through ONE lockstep launch chain.  rets[count].
 *   Arguments are checked first (LPBOX_E_BADARG), then the call order (LPBOX_E_STATE before an init), then the device.
 * _get_x_iters_device: one launch packs the (n_live x ws) row-major windows of all active handles into one buffer of the batch: handle
 *   i's rows are [row_off[i], row_off[i+1]) (row_off[count + 1]; no rows for an inactive handle), row q = its q-th live variable in
 *   ascending original index, the row order of lpbox_get_x_iters.  The buffer stays valid until the next call on the batch.
 * _iterate_l2f_scores: the same window with the fix decided on the device.  scores_dev[r] = float32 score of packed row r of the most
 *   recent _get_x_iters_device (LPBOX_E_STATE: none since the last window, or a handle active now that was not packed then); NULL =
 *   fix nothing.  Per problem deter_fix_2 with the trainer's guard: the score widened to double, s > hi -> 1, s < lo -> 0, NaN -> nothing,
 *   k = number of fixes, k <= min_fix -> nothing fixed.  fixed[count] = fixes applied.  The caller orders its own work on scores_dev
 *   before the call (the batch runs on a stream of its own). */
typedef struct lpbox_seg_batch lpbox_seg_batch_t;
lpbox_seg_batch_t *lpbox_seg_batch_create(lpbox_t **handles, int count);
void lpbox_seg_batch_destroy(lpbox_seg_batch_t *b);
int lpbox_seg_batch_init(lpbox_seg_batch_t *b);
int lpbox_seg_batch_set_active(lpbox_seg_batch_t *b, const unsigned char *active);
int lpbox_seg_batch_iterate_l2f(lpbox_seg_batch_t *b, int iter_start, int iter_end,
                                const double *vecs, long vec_stride, const int *nums, int *rets);
int lpbox_seg_batch_get_x_iters_device(lpbox_seg_batch_t *b, int ws, void **dev_ptr, long *row_off);
int lpbox_seg_batch_iterate_l2f_scores(lpbox_seg_batch_t *b, int iter_start, int iter_end, const float *scores_dev,
                                       double hi, double lo, int min_fix, int *rets, int *fixed);
/* SEG pxd:15 `double get_final_obj()` (SEGcpp:868-893): energy of the assembled rounded solution on the ORIGINAL A, b, plus c. */
int lpbox_seg_get_obj(lpbox_t *h, double *out);
int lpbox_seg_get_shape(lpbox_t *h, int *rows, int *cols);   /* scaled_row, scaled_col (SEGcpp:716-717), for save_img */
/* inspection: the problem the handle holds (pass NULL arrays to query n / nnz first) */
int lpbox_seg_get_problem(lpbox_t *h, int *n, int *nnz, int *rowptr, int *colidx, double *vals, double *b, double *c);

/* ---- extensions beyond the pxd (batching, measurement, inspection) ---------------------------- */
/* Workgroup geometry picked for the batch: threads per instance and slots per thread (threads*slots storage positions;
 * the reduction tree depends on both). */
int lpbox_get_config(lpbox_t *h, int *threads, int *elems_per_thread, int *lds_bytes);
/* PCG loop of the on-chip LP kernel: *specialised = 1 when a wavefront whose gather lists sit in registers runs a copy of the loop
 * compiled for its list lengths (512 threads x 1 slot, default order and x-update, no iteration log), 0 when every wavefront runs the
 * generic loop (every other geometry and mode; LPBOX_LP_PCGLOOP=generic in the environment when the problem is uploaded).  Both give
 * the same bits. */
int lpbox_get_pcg_loop(lpbox_t *h, int *specialised);
/* 512 x 1 kernel: class of every wavefront w of instance idx in the PCG loop, classes4[4*w + {0,1,2,3}] = rn, cn, hn, tail: the
 * chunks of two register entries of the wave's longest row list (capacity 12), own-column list (12) and helper list (8), i.e.
 * ceil(min(longest, capacity) / 2), and tail = 1 when some list of a lane is longer than its capacity (such a wave always runs the
 * generic loop).  Returns the number of wavefronts (8); LPBOX_E_UNSUPPORTED for other geometries and the reference order. */
int lpbox_get_wave_classes(lpbox_t *h, int idx, int *classes4);
/* The class rule itself, on the list lengths of the lanes of one wavefront (host only, no device needed): class4 = rn, cn, hn, tail. */
int lpbox_wave_class_rule(int lanes, const int *row_len, const int *col_len, const int *help_len, int *class4);
/* Storage position of every variable of instance idx (pos_of_var[org_n]): the kernels keep variables sorted by column
 * length, and the reduction tree is defined over positions (element at position p -> thread p % threads). */
int lpbox_get_layout(lpbox_t *h, int idx, int *pos_of_var);
/* Number of lanes (1,2,4,8) that share the sum of each row of E in instance idx (lanes_of_row[l]): lane g adds the entries
 * g, g+G, ... of the row in ascending column order, the G partial sums are combined by a butterfly. */
int lpbox_get_row_split(lpbox_t *h, int idx, int *lanes_of_row);
/* How the kernels add up column j of E (E^T w) in instance idx: own[j] leading entries (ascending row id) by the variable's
 * own lane; for a split column the rest in consecutive chunks of help4[4*j + q] entries by lane q = 0..3 of its quad of lanes
 * (0 for the own lane), the four chunk sums h_q combined as (h0 + h1) + (h2 + h3) and added to the own part.  own[org_n],
 * help4[4*org_n]; an unsplit column has own[j] = its length and help4 = 0. */
int lpbox_get_col_split(lpbox_t *h, int idx, int *own, int *help4);
/* Counters accumulated since init: outer ADMM iterations and PCG iterations of instance idx (LPcpp:894 maxiter). */
/* The reference's per-iteration text log (does_log, LPh:148, written by ADMM_lp_iters, LPcpp:789, :898-901, :1013-1067), opt-in: while on,
 * every lpbox_iterate call keeps LPBOX_LOG_VALS doubles per iteration it completed -- PCG iterations, |x_sol|, |y1|, |y2|, |y3|, |z1|, |z2|,
 * |z4|, b.x ("dou_obj"), b.round(x) ("bin_obj"), seconds since the call started (device clock), iteration -- and lpbox_get_log returns the
 * records of instance idx in iteration order (rows written; an iteration that stopped the loop is not logged, as in the reference).
 * Default PCG kernels only (LPBOX_E_UNSUPPORTED otherwise); the Python wrapper formats the text file. */
#define LPBOX_LOG_VALS 12
int lpbox_set_log(lpbox_t *h, int on);
int lpbox_get_log(lpbox_t *h, int idx, double *out, int cap_rows);
int lpbox_get_counters(lpbox_t *h, int idx, long long *outer_iters, long long *pcg_iters);
/* Which stop fired in the last call: 0 none, 1 y1_y2, 2 obj_std, 3 PCG alpha<0, 4 all fixed; and iter+1 of the last plain call (LPcpp:1081). */
int lpbox_get_stop(lpbox_t *h, int idx, int *reason, int *plain_iter_plus1);
/* Device time (ms, HIP events on the handle's stream) and launch count of the ADMM window kernel since the last reset. */
int lpbox_kernel_time(lpbox_t *h, double *ms_total, long long *launches, int reset);
/* Copy a named device state vector of instance idx ("x","z1","z2","z4","f","pd","b"); returns its length. */
int lpbox_debug_get_vec(lpbox_t *h, int idx, const char *name, double *out, int cap);
int lpbox_debug_get_scalar(lpbox_t *h, int idx, const char *name, double *out);
/* LP flavour, host only (no device needed): one of the index tables the kernels read, for instance idx, as the device sees it -- at the
 * stride of the batch, padding included, widened to int.  name = "rs_ptr", "cs_ptr", "hs_ptr" (threads x slots + 1 entries: the lists of
 * the row task / own column part / helper chunk of every slot), "rs_col", "cs_row" (the index pools they point into), "rid", "rgl",
 * "rmeta", "cmeta" (per slot: row of the task or 0xFFFF, its storage index, lanes << 4 | lane, column length with bit 15 = split).
 * Plans the layout like lpbox_get_layout does; returns the number of entries. */
int lpbox_debug_get_lp_table(lpbox_t *h, int idx, const char *name, int *out, int cap);
/* Test entry for the workgroup reduction of the LP kernels (no solver state, used by no product path): `groups` workgroups of `threads`
 * threads each call the reduction `rounds` times back to back on one scratch area.  in[(r * threads + t) * nv + k] is thread t's
 * partial of value k in round r (the same for every workgroup); out[((g * rounds + r) * threads + t) * nv + k] is what thread t of
 * workgroup g received.  stage: 0 = the default second stage (threads 256 / 512 / 1024), 1 = the one the 512-thread window kernel
 * ran first (threads 512: pair reads), 2 = stage 1 with wide butterfly steps free of register copies; 3 = stage 2 whose rows of 16 lanes
 * are finished for their first lane only, by additions of a row-broadcast operand; 4 = stage 3 with the second stage that reads four
 * partials per lane (what the 512-thread window kernel runs); 5 = stage 2 with that second stage (threads 512 for 1..5); nv = 1, 2, 3
 * or 6.  Anything else: LPBOX_E_BADARG. */
int lpbox_debug_block_sum(int threads, int nv, int stage, int groups, int rounds, const double *in, double *out);
/* Test entry for the LDS hand-over of the 512-thread window kernel (no solver state, used by no product path): `groups` workgroups of 512
 * threads run `rounds` rounds on ONE 512-vector in LDS.  A round: thread t writes v to element t; barrier; s = the sum, in order, of the
 * elements pos[q * 512 + t], q = 0 .. L - 1 (L = l_lo in wavefronts 0-3, l_hi in 4-7; pos: 12 x 512 entries in 0 .. 511); barrier; the
 * workgroup reduction of (s) (nv = 1) or (s, v) (nv = 2) with the window kernel's second stage; v = frac(s * 1.37 + total0 * 0.113
 * [+ total1 * 0.0271] + t / 1024).  v0[t]: the first v.  form: 0 = every barrier is __syncthreads(), 1 = the bare hand-over barrier.
 * last[g * 512 + t]: thread t's v after the last round; totals[(g * rounds + r) * nv + k]: the totals of round r.  Built for
 * (nv, l_lo, l_hi) = (1, 1, 1), (1, 2, 2), (1, 12, 12), (1, 12, 1), (1, 1, 12), (2, 12, 12).  Anything else: LPBOX_E_BADARG. */
int lpbox_debug_handover(int form, int nv, int l_lo, int l_hi, int groups, int rounds, const int *pos, const double *v0, double *last, double *totals);

/* ---- LARGE single LP, variable-sharded over ranks (BASELINE config 5; no reference counterpart: the reference is one
 * process).  Rank r holds the columns [c0, c0+n_loc) of E (all l rows), its slice of b, and the full f; the l-vectors are
 * replicated.  Where the algorithm sums over all variables (E*v: an l-vector once per PCG iteration and twice per outer
 * iteration; <= 5 scalars per reduction) the ranks exchange their contributions and EVERY rank adds them in rank order
 * (c0 + c1) + c2 ..., so a W-rank run is reproducible and has an exact CPU model (oracle lpo_set_ranks).  Transport, chosen
 * before lpbox_big_init:
 *   - RCCL driven by the library itself on the handle's stream (lpbox_big_rccl_unique_id on one rank, the 128 bytes handed to
 *     every rank by the caller's control plane, lpbox_big_rccl_init on every rank): per E*v one grouped send/recv of row blocks
 *     (a reduce-scatter whose adds are ours) + one all-gather; per scalar group one all-gather.  No Python in the loop.
 *   - or a caller-supplied all-gather `fn(send_dev, count, recv_dev, user)`: recv_dev[r*count .. (r+1)*count) := rank r's
 *     send_dev[0..count), stream-ordered after the work already queued on the handle's stream (tests: gloo through torch).
 * world == 1 without a transport issues no collective.  Semantics: ADMM_lp_iters (LPcpp:766-1095). */
typedef struct lpbox_big lpbox_big_t;
typedef int (*lpbox_allgather_fn)(const void *send_dev, long count, void *recv_dev, void *user);
lpbox_big_t *lpbox_big_create(int rank, int world, int device);
void lpbox_big_destroy(lpbox_big_t *h);
int lpbox_big_set_stream(lpbox_big_t *h, void *hip_stream);
int lpbox_big_set_allgather(lpbox_big_t *h, lpbox_allgather_fn fn, void *user);
int lpbox_big_rccl_unique_id(void *out128);                    /* ncclGetUniqueId: 128 bytes, returns 128 */
int lpbox_big_rccl_init(lpbox_big_t *h, const void *unique_id128);   /* ncclCommInitRank(world, id, rank) on the handle's device */
/* b (this rank's n_loc entries, already negated) must be finite, as for lpbox_set_problem_lp: a NaN or an infinity is LPBOX_E_BADARG
 * with the local and global index in lpbox_last_error(), from lpbox_big_set_problem and lpbox_big_set_problem_vals alike. */
int lpbox_big_set_problem(lpbox_big_t *h, long n_glob, int c0, int n_loc, int l, const int *colptr, const int *rowidx,
                          const double *b, const double *f);
/* OPT-IN: the reference's summation order on this path (lpbox_set_order's LPBOX_ORDER_REFERENCE beyond the on-chip limit; DESIGN.md
 * section 21).  Every dot product / norm over the live variables follows Eigen's redux over the live variables in ascending original
 * index, the fix objective the same redux over the variables fixed by the call; rows and columns of E are summed by one lane in
 * ascending order (one column slice: LPBOX_BIG_SLICE_KB is ignored).  Bit-exact against oracle/lpbox_oracle.c in LPO_ORDER_EIGEN; sqrt
 * where the reference calls pow(v, 1/2), as on chip.  Call it before lpbox_big_set_problem (LPBOX_E_STATE later).  One rank only:
 * world != 1, a transport (lpbox_big_set_allgather, lpbox_big_rccl_init) or the comm-lean PCG give LPBOX_E_UNSUPPORTED, whichever of
 * the two calls comes first.  lpbox_big_get_scalar(h, "order") reports the mode and "valued" whether the problem stores a value
 * other than 1.0 (both also before lpbox_big_init). */
int lpbox_big_set_order(lpbox_big_t *h, int mode);
/* lpbox_big_set_problem plus the stored values of E in the order of rowidx (NULL = ones).  Reference order: any finite value (an
 * explicit zero stays a stored entry; a non-finite value is LPBOX_E_BADARG); values that are all exactly 1.0 make a unit instance.
 * Default order: any value other than 1.0 is LPBOX_E_UNSUPPORTED (the message names lpbox_big_set_order).  lpbox_big_get_vec then
 * also serves "vals" and "r4v" (rho4_E_transpose per stored entry), both in the order of rowidx; lpbox_big_check_infeasible
 * multiplies by the stored value. */
int lpbox_big_set_problem_vals(lpbox_big_t *h, long n_glob, int c0, int n_loc, int l, const int *colptr, const int *rowidx,
                               const double *b, const double *f, const double *vals);
/* Opt-in, NOT the reference's arithmetic and outside the parity claim (like lpbox_set_x_update): the PCG's step length from
 * p.Mp = dI (p.p) + r4Et (q.q), q = E p, instead of the dot product p.(M p) of LPcpp:300 -- the p.p partials ride with the q exchange, the column
 * product and the vector updates become one kernel: 3 instead of 4 RCCL operations and 2 instead of 3 launches per PCG iteration.  Call before
 * lpbox_big_init.  Bit-exact against its own oracle mirror (lpo_set_pcg_lean). */
#define LPBOX_PCG_REFERENCE 0
#define LPBOX_PCG_COMM_LEAN 1
int lpbox_big_set_pcg_mode(lpbox_big_t *h, int mode);
int lpbox_big_init(lpbox_big_t *h);                                             /* ADMM_lp_iters_init LPcpp:489-763 */
int lpbox_big_iterate(lpbox_big_t *h, int iter_start, int iter_end, int *ret);  /* ADMM_lp_iters      LPcpp:766-1095 */
/* print_fix_info 2 behind the size hand-over (LPcpp:777-780, :903-909): the following lpbox_big_iterate calls keep x after every
 * iteration on the device; lpbox_big_get_x_iters(ws = iterations of the call) reads the (rows x ws) block back. */
int lpbox_big_set_record(lpbox_big_t *h, int on);
/* ADMM_lp_iters_l2f (LPcpp:1098-1574) on the sharded instance.  vec_local: this rank's slice of the fix vector, one entry per LOCAL
 * live variable in ascending order (1.0 / 0.0 fix, anything else leave); num_global: number of fixes over ALL ranks (callers sum their
 * local counts with one tiny all-reduce; it sets the shrunken n of the sphere projection, LPcpp:427).  x_iters of the window stay on
 * the device per rank: a policy scores its own shard, no gather. */
int lpbox_big_iterate_l2f(lpbox_big_t *h, int iter_start, int iter_end, const double *vec_local, long num_global, int *ret);
int lpbox_big_get_n(lpbox_big_t *h);                                            /* live variables of this rank */
int lpbox_big_get_x_iters(lpbox_big_t *h, int ws, double *out);                 /* (rows x ws) row-major; out == NULL: rows */
int lpbox_big_get_x_iters_device(lpbox_big_t *h, int ws, void **dev_ptr, int *rows);
int lpbox_big_get_x_sol(lpbox_big_t *h, double *out_local);                     /* binary: fixed value / rounded x (LPcpp:1648-1666) */
int lpbox_big_cal_obj(lpbox_big_t *h, double *out);                             /* sum_fix_obj + cur_obj (LPcpp:1630-1642) */
int lpbox_big_get_x(lpbox_big_t *h, double *out_local);                         /* this rank's slice of x_sol */
int lpbox_big_get_vec(lpbox_big_t *h, const char *name, double *out, long cap); /* "x","z1","z2","pd","live" (local), "z4","Ex" (rows) */
/* LP pxd:20 / :21 on the large path, one rank only: which = 0 check_infeasible_lpbox (LPcpp:1577-1591: rows of the CURRENT E, live
 * columns, raw iterate), 1 check_infeasible_l2f (LPcpp:1593-1612: original E times the binary full-length solution); count >= 0. */
int lpbox_big_check_infeasible(lpbox_big_t *h, int which);
int lpbox_big_get_scalar(lpbox_big_t *h, const char *name, double *out);        /* "cur_obj","iter","stop","outer_total","pcg_total",... */

/* A batch of large-route handles through ONE launch chain in lockstep: plain windows (lpbox_big_iterate) of all members at once, every
 * launch on a grid (workgroups, members).  Each member keeps its own control state and falls through once it has stopped; per member
 * the results are those of lpbox_big_iterate on its own, bit for bit.  The handles are borrowed: they stay ordinary handles, their
 * getters and a later lpbox_big_iterate of their own work as if the windows had been their own.  A member must run on one rank without
 * a transport, with the reference's PCG, without recording and without fixed variables (LPBOX_E_UNSUPPORTED otherwise); all members on
 * one device, no handle twice (LPBOX_E_BADARG).
 * Summation order: ALL members run in ONE order, the order of member 0 (lpbox_big_set_order before its problem); a member in the other
 * order is refused at create, init and every iterate (LPBOX_E_UNSUPPORTED, naming the member).  Default order: folded reductions (at
 * most 1024 workgroups) and unit values.  Reference order (LPBOX_ORDER_REFERENCE): per member the bits of lpbox_big_iterate in that
 * order, i.e. the oracle's in ORDER_EIGEN; only there may members carry stored values (lpbox_big_set_problem_vals), unit and valued
 * members mixed freely.  The early-fixing calls below need the default order: on a batch in the reference order they return
 * LPBOX_E_UNSUPPORTED and change nothing.
 * A refused call leaves the batch and its members as they were.  LPBOX_BIG_KMAX / LPBOX_BIG_KMARGIN are read at create;
 * LPBOX_BIG_BATCH_GRAPH=1 replays captured iterations instead of eager launches. */
typedef struct lpbox_big_batch lpbox_big_batch_t;
lpbox_big_batch_t *lpbox_big_batch_create(lpbox_big_t **handles, int count);
void lpbox_big_batch_destroy(lpbox_big_batch_t *b);
int lpbox_big_batch_init(lpbox_big_batch_t *b);                                  /* lpbox_big_init on every member */
int lpbox_big_batch_iterate(lpbox_big_batch_t *b, int iter_start, int iter_end, int *rets);   /* ADMM_lp_iters per member; rets[count] */
/* The early-fixing windows of lpbox_big_iterate_l2f (LPcpp:1098-1574; the loop of LP/trainer.py:504-545) for the batch: the fix
 * prologue, the window, the pack of the iterates and the fix decision of all active members each run in launches over a
 * (workgroups, members) grid.  Per member every result is that of lpbox_big_iterate_l2f on its own with the same fix vectors, bit for
 * bit; fixed variables are allowed here (lpbox_big_batch_create / _init and the plain lpbox_big_batch_iterate keep refusing them), the
 * other member conditions are those above.  After any batched window every member answers every getter and may go on with windows of
 * its own.
 * _set_active: active[count], NULL = all.  It governs the three calls below only (lpbox_big_batch_iterate runs every member).  An
 *   inactive member is not touched by them: state, vectors, staged window, counters, rets[i] / fixed[i].
 * _iterate_l2f: member i fixes by vecs + i * vec_stride over its live variables in ascending order (1 / 0 = fix, anything else =
 *   leave) and nums[i], validated as lpbox_big_iterate_l2f does on one rank (count mismatch, nums[i] outside [0, n_live], missing
 *   vector, window longer than the 500 columns of x_iters); vecs may be NULL when every nums[i] is 0.  All members are validated before
 *   anything changes; a refusal names the member.  Refusals in this order: arguments (LPBOX_E_BADARG), call order (LPBOX_E_STATE before
 *   _init), the member conditions (LPBOX_E_UNSUPPORTED).  rets[count].
 * _get_x_iters_device: one launch packs the (rows x ws) row-major windows of all active members into one buffer of the batch: member
 *   i's rows are [row_off[i], row_off[i+1]) (row_off[count + 1]; no rows for an inactive member), row q = its q-th live variable when
 *   the window started, in ascending original index -- the row order of lpbox_big_get_x_iters.  The buffer grows on demand and stays
 *   valid until the next call on the batch.
 * _iterate_l2f_scores: the same window with the fix decided on the device.  scores_dev[r] = float32 score of packed row r of the most
 *   recent _get_x_iters_device (LPBOX_E_STATE: none since the last window, or a member active now that was not packed then); NULL =
 *   fix nothing.  Per member deter_fix_2 with the trainer's guard: the score widened to double, s > hi -> 1, s < lo -> 0, NaN ->
 *   nothing, k = number of fixes, k <= min_fix -> nothing fixed.  fixed[count] = fixes applied.  The caller orders its own work on
 *   scores_dev before the call (the batch runs on a stream of its own). */
int lpbox_big_batch_set_active(lpbox_big_batch_t *b, const unsigned char *active);
int lpbox_big_batch_iterate_l2f(lpbox_big_batch_t *b, int iter_start, int iter_end,
                                const double *vecs, long vec_stride, const long *nums, int *rets);
int lpbox_big_batch_get_x_iters_device(lpbox_big_batch_t *b, int ws, void **dev_ptr, long *row_off);
int lpbox_big_batch_iterate_l2f_scores(lpbox_big_batch_t *b, int iter_start, int iter_end, const float *scores_dev,
                                       double hi, double lo, int min_fix, int *rets, int *fixed);
/* "count", "launches", "kernel_ms", "kmax", "graph", "parity_copies", "grid_cols" / "grid_y" / "grid_rows" / "grid_z4" (the x-extents
 * of the launches), "pcg_resumes_<i>" (member i); "active" (members), "fix_launches" (launches of the fix prologue), "packs",
 * "compact_chunk" (entries per pass of the live-list compaction); "order" (0 default, 1 reference), "valued_members" (members with
 * stored values other than 1), "walks" (walker launches so far: reference order only; "launches" counts them too) */
int lpbox_big_batch_get_scalar(lpbox_big_batch_t *b, const char *name, double *out);

/* ---- generic constrained binary QP: min x'Ax + b'x  s.t.  Cx = d, Ex <= f, x in {0,1}^n -----------------------------------------
 * The reference's ADMM_bqp (Segmentation/.../LPboxADMMsolver.cpp:1384-1832) behind ADMM_bqp_unconstrained / _linear_eq / _linear_ineq /
 * _linear_eq_and_uneq (:1834-2109; C++ only, not in the pyx).  Matrices are CSR with ascending columns; A must store every diagonal
 * entry (the reference adds rho to A.diagonal() in place, :1483).  m = 0: no equality constraints, l = 0: no inequality constraints. */
typedef struct lpbox_bqp lpbox_bqp_t;
lpbox_bqp_t *lpbox_bqp_create(int device);
void lpbox_bqp_destroy(lpbox_bqp_t *h);
int lpbox_bqp_preset(lpbox_bqp_t *h, int type);      /* hyper-parameters of ADMM_bqp_{unconstrained,linear_eq,linear_ineq,linear_eq_and_uneq}_init (:587-672): 0,1,2,3 */
int lpbox_bqp_set_params(lpbox_bqp_t *h, const double *p11);   /* stop_threshold, std_threshold, gamma_val, gamma_factor, rho_change_step, max_iters, initial_rho, history_size, learning_fact, pcg_tol, pcg_maxiters */
int lpbox_bqp_set_problem(lpbox_bqp_t *h, int n, const int *Ap, const int *Ai, const double *Av, const double *b, const double *x0,
                          int m, const int *Cp, const int *Ci, const double *Cv, const double *d,
                          int l, const int *Ep, const int *Ei, const double *Ev, const double *f);
int lpbox_bqp_solve(lpbox_bqp_t *h, int *iterations);          /* the whole ADMM_bqp loop; *iterations = the `iter` it ended on */
int lpbox_bqp_get_vec(lpbox_bqp_t *h, const char *name, double *out, long cap);   /* Solution (LPh): "x" (x_sol), "y1", "y2", "best_sol"; also "z1","z2","z3","z4","y3" */
int lpbox_bqp_get_scalar(lpbox_bqp_t *h, const char *name, double *out);          /* "iters","stop" (1 xyy, 2 obj_std, 0 max_iters),"cur_obj","best_bin_obj","total_pcg",...,"order" */
/* OPT-IN: the summation order of the one-problem chain, LPBOX_ORDER_DEFAULT / LPBOX_ORDER_REFERENCE as for lpbox_bqp_batch_set_order
 * below -- the only route to the reference's order for a problem with a dimension above 2048.  REFERENCE = every sum over the n
 * elements (the dot products and squared norms of the PCG, of the y2 projection, of the stop tests and of compute_cost) associated as
 * the reference's Eigen 3.3.8 SSE2 redux associates it, and c1 through libm's pow: bit for bit oracle/bqp_oracle.c in its Eigen order on
 * every vector and scalar, except that the std stop test takes sqrt where the reference calls pow(v, 1/2) ("std_obj" within 2 ulps).
 * What it costs: the kernels that fed a reduction write one term per element to seven staging rows of n doubles (allocated by the
 * first solve in this order) and one workgroup walks them, n / 4 dependent additions per reduction; DESIGN.md section 14.3 holds the
 * measurements.  Allowed at any time, also between two lpbox_bqp_solve calls on one handle (a solve re-initialises); a call that
 * changes the order marks the handle as not solved: the results of the other order are refused until the next solve, while
 * lpbox_bqp_get_scalar(h, "order") answers at any time, before the first solve too.  "threads", "chunk" and "launches" keep their values.  Bad handle ->
 * LPBOX_E_BADHANDLE; unknown mode -> LPBOX_E_BADARG, and the handle stays as it was. */
int lpbox_bqp_set_order(lpbox_bqp_t *h, int mode);

/* ---- a batch of SMALL generic constrained binary QPs (max(n, m, l) <= 2048 each), one persistent workgroup per problem -------------
 * The same ADMM_bqp loop (SEGcpp:1384-1832: the y updates :1598-1613, the rho refresh :1619-1650, the PCG on the matrix expression
 * :361-469, the duals :1733-1739, the stop tests and the rho / gamma schedule :1742-1794) solved for `count` independent problems in
 * one launch per window of outer iterations.  The problems of a batch may differ in size, type and hyper-parameters.  Everything
 * the getters return for a problem is bit for bit what lpbox_bqp_solve returns for it alone.  Validation and messages are those of
 * lpbox_bqp_*; a problem with max(n, m, l) > 2048 is refused with LPBOX_E_TOOLARGE (use lpbox_bqp_* for it) and leaves the rest of
 * the batch untouched.  No device: lpbox_bqp_batch_create returns NULL with LPBOX_E_NODEVICE in lpbox_last_error. */
typedef struct lpbox_bqp_batch lpbox_bqp_batch_t;
lpbox_bqp_batch_t *lpbox_bqp_batch_create(int count, int device);
void lpbox_bqp_batch_destroy(lpbox_bqp_batch_t *h);
int lpbox_bqp_batch_preset(lpbox_bqp_batch_t *h, int idx, int type);               /* the *_init presets (:587-672) of lpbox_bqp_preset; idx -1 = every problem */
int lpbox_bqp_batch_set_params(lpbox_bqp_batch_t *h, int idx, const double *p11);  /* the 11 values of lpbox_bqp_set_params; idx -1 = every problem */
int lpbox_bqp_batch_set_problem(lpbox_bqp_batch_t *h, int idx, int n, const int *Ap, const int *Ai, const double *Av, const double *b,
                                const double *x0, int m, const int *Cp, const int *Ci, const double *Cv, const double *d,
                                int l, const int *Ep, const int *Ei, const double *Ev, const double *f);
int lpbox_bqp_batch_solve(lpbox_bqp_batch_t *h, int *iterations);                  /* ADMM_bqp (:1384-1832) for every problem, each to its own stop; iterations[count] may be NULL; LPBOX_E_STATE while an index is unset */
int lpbox_bqp_batch_get_vec(lpbox_bqp_batch_t *h, int idx, const char *name, double *out, long cap);   /* the names of lpbox_bqp_get_vec */
int lpbox_bqp_batch_get_scalar(lpbox_bqp_batch_t *h, int idx, const char *name, double *out);          /* the names of lpbox_bqp_get_scalar per problem; batch-wide (idx ignored): "kernel_ms","launches","threads","chunk","window","slots","order" */
/* OPT-IN: the summation order of the batch kernels, LPBOX_ORDER_DEFAULT / LPBOX_ORDER_REFERENCE as for lpbox_set_order.  DEFAULT (the
 * default) = the kernels' own reduction tree, bit for bit lpbox_bqp_solve and the oracle run in that association.  REFERENCE = every sum
 * over the n elements of a problem (the dot products and squared norms of the PCG, of the y2 projection, of the stop tests and of
 * compute_cost) associated as the reference's Eigen 3.3.8 SSE2 redux associates it: four accumulators over the index order, then the
 * left-over pair, then the odd last element -- bit for bit oracle/bqp_oracle.c in its Eigen order on every vector and scalar, except
 * that the std stop test takes sqrt where the reference calls pow(v, 1/2) ("std_obj" within 2 ulps).  Rows and columns are summed in
 * the reference's order in both modes.  What it costs: each reduction becomes a strictly sequential walk of n / 4 dependent additions
 * by four lanes (two walks per PCG step) instead of a tree, and four staging rows of LDS per workgroup (about 32 n bytes for the batch's
 * largest n; DESIGN.md section 14.2 holds the plan and the measurements: 1.4 to 1.5 times the default order's kernel time); a batch whose LDS need exceeds one workgroup's 160 KB -> LPBOX_E_UNSUPPORTED
 * from lpbox_bqp_batch_solve.  Allowed at any time before a solve; marks the batch as not solved.  "threads" and "chunk" keep their values
 * (they describe the default order).  Unknown mode -> LPBOX_E_BADARG.  lpbox_bqp_* (one problem per handle): lpbox_bqp_set_order above. */
int lpbox_bqp_batch_set_order(lpbox_bqp_batch_t *h, int mode);

/* ---- a BATCH of generic BQPs of ANY size through ONE launch chain in lockstep ------------------------------
 * For many problems with a dimension above 2048 (the ones lpbox_bqp_batch_* turns away).  The batch borrows lpbox_bqp_t handles that
 * hold a problem; they stay ordinary handles (lpbox_bqp_solve, the getters) and must outlive the batch.  Every launch of the one-problem
 * chain becomes one launch over a (workgroups, members) grid; each member runs on its own control state, with its own preset,
 * parameters, stop tests and max_iters, and whatever the getters return for a member afterwards is bit for bit what lpbox_bqp_solve
 * returns for it alone.  Members may differ in n, m, l and type.
 * _create makes no device call.  It returns NULL, with status and text in lpbox_last_status / lpbox_last_error and the offending
 * member's index in the text: empty batch or null array -> LPBOX_E_BADARG; a null member or one without a problem -> LPBOX_E_STATE; the
 * same handle twice, or a member on another device than member 0 -> LPBOX_E_BADARG; a member in the reference summation order ->
 * LPBOX_E_UNSUPPORTED (lpbox_bqp_solve per handle runs that order).  _solve checks the members again before anything changes.
 * _solve: uploads (first solve) and initialises every member with the launches of lpbox_bqp_solve, runs the chain, and leaves every
 * member solved: lpbox_bqp_get_vec / _get_scalar on a member return its result; a member's "pcg_resumes" is its own count, its
 * "kernel_ms" and "launches" read 0 (the chain's launches belong to the batch).  iterations[count] may be NULL.
 * LPBOX_BQP_KMAX (read at _create) forces the launch groups per iteration as it does for a handle; LPBOX_BQP_LOCKSTEP_GRAPH=1 replays
 * captured iterations instead of eager launches.
 * Scalars: "count", "launches", "kernel_ms", "kmax", "graph", "graph_entries", "grid_cols" / "grid_y" / "grid_rows" (the x-extents of the
 * launches), "pcg_resumes_<i>" (member i, last solve). */
typedef struct lpbox_bqp_lockstep lpbox_bqp_lockstep_t;
lpbox_bqp_lockstep_t *lpbox_bqp_lockstep_create(lpbox_bqp_t **handles, int count);
void lpbox_bqp_lockstep_destroy(lpbox_bqp_lockstep_t *b);
int lpbox_bqp_lockstep_solve(lpbox_bqp_lockstep_t *b, int *iterations);
int lpbox_bqp_lockstep_get_scalar(lpbox_bqp_lockstep_t *b, const char *name, double *out);

#ifdef __cplusplus
}
#endif
#endif
