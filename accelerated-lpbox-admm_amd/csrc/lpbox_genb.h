// lpbox_genb.h -- internal layout of the BATCH of small generic constrained binary QPs (ADMM_bqp, SEGcpp:1384-1832; see lpbox_gen.h
// for the one-problem path).  One persistent workgroup of GEN_T threads per problem runs the whole loop; the arithmetic -- every
// expression, every summation order -- is that of the kernel chain in lpbox_gen_kernels.hip with 2 slots per thread (chunk 512), so
// a problem gives the same bits on either path.  Not part of the C-ABI.
#pragma once
#include "lpbox_gen.h"

#define GENB_MAXDIM 2048        // max(n, m, l) of a problem: 8 slots of GEN_T threads, 4 chunks of 512

struct GenbProb {               // per-problem descriptor (device memory); the pointers lead into the batch's two pooled arrays
    int n, m, l, eq, ineq;
    GenParams prm;
    double c1;                  // std::pow(n, 1.0 / 2), evaluated on the host like the one-problem path does (reference order: libm's pow)
    // A by rows (every diagonal stored), tmval = 2A + (rho1+rho2) I, adiag[i] = position of the diagonal entry
    const int *aptr, *aidx, *adiag; const double *aval; double *tmval;
    // C (m x n), E (l x n) by rows and by columns; *_sv = the separately scaled transposes rho3 C' / rho4 E'
    GenCsr Cr, Cc, Er, Ec; double *Cc_sv, *Ec_sv; int Cnnz, Ennz;
    const double *x0, *b, *d, *f;
    double *x, *y1, *y2, *z1, *z2, *pdiag, *dinv, *Csq, *Esq, *best;     // n-vectors, touched by their owner thread only
    double *z3;                                                          // m-vector
    double *z4, *y3, *fy, *Ex;                                           // l-vectors
};

// slots = 2, 4 or 8 elements per thread (n <= 512, 1024, 2048 for the largest problem of the batch); lds_doubles = npad + mmax + lmax.
// ref = the reference's summation order (lpbox_bqp_batch_set_order): every sum over a problem's n elements is
// Eigen's redux in index order (lpbox_eigen_redux.h), from staging rows in LDS that genb_lds_bytes adds.
#define GENB_LDS_LIMIT (160 * 1024)   // LDS of one gfx950 workgroup
#define GENB_STATIC_LDS 2048          // bound on the kernels' static LDS (reduction scratch, control state)
size_t genb_lds_bytes(int nmax, int mmax, int lmax, bool ref);
hipError_t genb_launch_init(const GenbProb *probs, GenState *st, int count, int slots, int nmax, bool ref, hipStream_t s);
hipError_t genb_launch_window(const GenbProb *probs, GenState *st, int count, int slots, int window, int nmax, int mmax, int lmax, bool ref,
                              hipStream_t s);
