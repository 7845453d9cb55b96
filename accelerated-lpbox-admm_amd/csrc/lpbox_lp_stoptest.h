// lpbox_lp_stoptest.h -- the two stop tests of an ADMM iteration (LPcpp:931-949, :459-469 / :977), their exact expressions and a
// cheap filter per test that says "the exact value is certainly above the threshold" without forming a square root or a division.
// Host and device: the kernel (lp_window_kernel<512, 1>) skips the exact expressions while a filter fires and forms them from the
// kept operands where the value is read; tests/lp_stop_filter_check.cpp checks the filters against the exact expressions on the CPU.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LPBOX_STOP_HD __host__ __device__ __forceinline__
#else
#define LPBOX_STOP_HD inline
#endif

// A filter compares against threshold^2 * (1 + 2^-30).  Why that margin is safe: sqrt and / are correctly rounded (relative error
// <= 2^-53 each), so the exact expressions below err by less than 4 * 2^-53 relative against the real quotient; the two or three
// multiplications of a filter's right-hand side err by less than 4 * 2^-53 as well (the guards keep every product in the normal
// range).  A filter that fires therefore proves real quotient^2 > T^2 (1 + 2^-30)(1 - 2^-50), i.e. real quotient > T (1 + 2^-32), and the
// computed quotient > T (1 + 2^-32)(1 - 2^-50) > T.  Where a filter does not fire nothing is claimed: the caller runs the exact code.
#define LPBOX_STOP_MARGIN (1.0 + 0x1p-30)

// cvg = sqrt(a) / max(sqrt(c), 2.2204e-16)   (a = |x - y|^2, c = |x|^2)
LPBOX_STOP_HD double lp_cvg_exact(double a, double c) {
    const double xn = sqrt(c);
    const double temp0 = (xn < 2.2204e-16) ? 2.2204e-16 : xn;
    return sqrt(a) / temp0;
}
// true: lp_cvg_exact(a, c) > T for certain.  Needs a, c finite and c >= 2^-100 (sqrt(c) >= 2^-50 > 2.2204e-16: the clamp is
// inactive); a NaN fails every comparison, so it is inconclusive like every other guard case.
LPBOX_STOP_HD bool lp_cvg_certainly_above(double a, double c, double T) {
    const double inf = __builtin_huge_val();
    return a < inf && c < inf && c >= 0x1p-100 && a > ((T * T) * c) * LPBOX_STOP_MARGIN;
}

// std_obj = sd / |h9| with sd = devq == 0 ? 0 : sqrt(devq)   (devq = the sample variance of the objective window, h9 its last value)
LPBOX_STOP_HD double lp_std_exact(double devq, double h9) {
    const double sd = (devq == 0) ? 0.0 : sqrt(devq);
    return sd / fabs(h9);
}
// true: lp_std_exact(devq, h9) > S for certain.  Needs both finite and 2^-400 <= |h9| <= 2^400, so that (S |h9|)^2 stays in the normal
// range for any S in [2^-100, 1]; devq == 0, h9 == 0 and NaN are inconclusive.
LPBOX_STOP_HD bool lp_std_certainly_above(double devq, double h9, double S) {
    const double inf = __builtin_huge_val();
    const double ah = fabs(h9), sh = S * ah;
    return devq < inf && ah >= 0x1p-400 && ah <= 0x1p400 && devq > (sh * sh) * LPBOX_STOP_MARGIN;
}
