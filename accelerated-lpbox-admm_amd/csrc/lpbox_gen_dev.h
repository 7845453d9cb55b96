// lpbox_gen_dev.h -- device expressions of ADMM_bqp (SEGcpp:1384-1832) shared by the two kernel files of the GENERIC constrained
// binary-QP path: the kernel chain of one large problem (lpbox_gen_kernels.hip) and the persistent workgroup per small problem
// (lpbox_genb_kernels.hip).  One definition per expression keeps the two bit-identical.  No FMA contraction, IEEE divide / sqrt.
#pragma once
#include "lpbox_gen.h"

namespace {

__device__ __forceinline__ double eigen_res(double tmp) { double r = 0.0; r += 1.0 * tmp; return r; }   // res[i] = 0 + alpha * tmp

// Eigen's RowMajor sparse * dense for one row (SEGh:17): tmp = sum val * ld(idx) over the entries [k, k1) in ascending order, then
// res = 0 + 1.0 * tmp.  The loads of four entries are issued before their (ordered) additions.
template <typename LD>
__device__ __forceinline__ double gen_sparse_dot(const int *idx, const double *vals, int k, int k1, LD ld) {
    double tmp = 0;
    for (; k + 4 <= k1; k += 4) {
        const double v0 = ld(idx[k]), v1 = ld(idx[k + 1]), v2 = ld(idx[k + 2]), v3 = ld(idx[k + 3]);
        tmp += vals[k] * v0; tmp += vals[k + 1] * v1; tmp += vals[k + 2] * v2; tmp += vals[k + 3] * v3;
    }
    for (; k < k1; k++) tmp += vals[k] * ld(idx[k]);
    return eigen_res(tmp);
}

__device__ __forceinline__ double gen_y1(double x, double z1, double rho1) {                 // :1598-1601
    const double t = x + z1 / rho1;
    return t > 1 ? 1 : (t < 0 ? 0 : t);
}
__device__ __forceinline__ double gen_y2_centre(double x, double z2, double rho2) { return (x + z2 / rho2) - 0.5; }   // :1603-1606
__device__ __forceinline__ double gen_y2(double centred, double c1, double c2) { return centred * c1 / c2 + 0.5; }     // :553-558
__device__ __forceinline__ double gen_y3(double f, double Ex, double z4, double rho4) {       // :1609-1613
    const double v = f - Ex - z4 / rho4;
    return v < 0 ? 0 : v;
}
__device__ __forceinline__ double gen_rhs_base(double rho1, double y1, double rho2, double y2, double b, double z1, double z2) {
    return (rho1 * y1 + rho2 * y2) - ((b + z1) + z2);                                         // :1656
}

// The end of an outer iteration `it` from red[0..7) = x.x, |x-y1|^2, |x-y2|^2, x.Ax, b.x, xb.A xb, b.xb (SEGcpp:1742-1794): the
// x / y1 / y2 stop test, the rho / gamma schedule, the objective history with the std stop, the best binary objective.  Sets
// halt = GEN_HALT_STOP on a stop, otherwise advances iter.
__device__ __forceinline__ void gen_finish_iteration(GenState *s, const GenParams &P, const double *red, int it, bool eq, bool ineq) {
    const double xn = sqrt(red[0]);
    const double t0 = (xn < 2.2204e-16) ? 2.2204e-16 : xn;
    s->cvg1 = sqrt(red[1]) / t0; s->cvg2 = sqrt(red[2]) / t0;                                   // :1742-1744
    bool stopped = false;
    if (s->cvg1 <= P.stop_threshold && s->cvg2 <= P.stop_threshold) { s->stop = GEN_STOP_XYY; stopped = true; }   // :1745
    else {
        if ((it + 1) % P.rho_change_step == 0) {                                                     // :1753-1770
            s->prev_rho1 = s->rho1; s->prev_rho2 = s->rho2;
            s->rho1 = P.learning_fact * s->rho1; s->rho2 = P.learning_fact * s->rho2;
            if (eq && ineq) { s->prev_rho3 = s->rho3; s->rho3 = P.learning_fact * s->rho3; }       // update_rho3: type 3 only (:1906, :2045)
            if (ineq) { s->prev_rho4 = s->rho4; s->rho4 = P.learning_fact * s->rho4; }
            const double g = s->gamma_val * P.gamma_factor;
            s->gamma_val = g < 1.0 ? 1.0 : g;
            s->rhoUpdated = 1; s->rcr = P.learning_fact - 1.0;
        }
        s->obj_val = red[3] + red[4];                                                                // :1772
        const int H = P.history_size;
        int hn = s->hist_n;
        if (hn < H) s->hist[hn] = s->obj_val;
        else { for (int k = 0; k < H - 1; k++) s->hist[k] = s->hist[k + 1]; s->hist[H - 1] = s->obj_val; }
        if (hn < 0x3fffffff) hn++;
        s->hist_n = hn;
        if (hn >= H) {                                                                               // :482-507, :574-585
            double mean = 0;
            for (int k = 0; k < H; k++) mean += s->hist[k];
            mean /= (double)H;
            double dev = 0;
            for (int k = 0; k < H; k++) dev += (s->hist[k] - mean) * (s->hist[k] - mean);
            dev /= (double)(H - 1);
            const double sd = (dev == 0) ? 0.0 : sqrt(dev);
            s->std_obj = sd / fabs(s->hist[H - 1]);
        }
        if (s->std_obj <= P.std_threshold) { s->stop = GEN_STOP_OBJSTD; stopped = true; }             // :1777
        else {
            s->cur_obj = red[5] + red[6];                                                            // :1786-1793
            if (s->best_bin_obj >= s->cur_obj) { s->best_bin_obj = s->cur_obj; s->copy_best = 1; }
        }
    }
    if (stopped) s->halt = GEN_HALT_STOP;
    else s->iter = it + 1;
}

}  // namespace
