// lp_stop_filter_check.cpp -- the stop-test filters of csrc/lpbox_lp_stoptest.h against the exact expressions, as a stand-alone
// program meant to run under the sanitizers of the host compiler (tests/test_lp_stop_filter.py builds and runs it):
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I<csrc> lp_stop_filter_check.cpp
// Claim checked: wherever a filter says "certainly above", the exact expression is above the threshold; on every guard case (zero,
// subnormal, infinity, NaN, a norm below 2^-100, a zero deviation, a last objective outside 2^+-400) the filter is inconclusive.
// Prints one line of counts and "stop filter ok"; any violation is printed and the exit status is 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <random>

#include "lpbox_lp_stoptest.h"

namespace {

constexpr double T = 1e-4, S = 1e-12;      // LP_STOP_THRESHOLD, LP_STD_THRESHOLD (csrc/lpbox_lp.h)
int failures = 0;
long fired_cvg = 0, fired_std = 0, seen_cvg = 0, seen_std = 0;

void fail(const char *what, double u, double v, double exact) {
    if (failures++ < 20) std::printf("FAIL %s: operands %a %a exact %a\n", what, u, v, exact);
}

// soundness of one operand pair; returns what the filter said
bool check_cvg(double a, double c) {
    seen_cvg++;
    const bool above = lp_cvg_certainly_above(a, c, T);
    if (above) {
        fired_cvg++;
        const double e = lp_cvg_exact(a, c);
        if (!(e > T)) fail("cvg filter fired, exact <= T", a, c, e);
    }
    return above;
}
bool check_std(double devq, double h9) {
    seen_std++;
    const bool above = lp_std_certainly_above(devq, h9, S);
    if (above) {
        fired_std++;
        const double e = lp_std_exact(devq, h9);
        if (!(e > S)) fail("std filter fired, exact <= S", devq, h9, e);
    }
    return above;
}
void expect_inconclusive_cvg(double a, double c) {
    if (check_cvg(a, c)) fail("cvg filter fired on a guard case", a, c, lp_cvg_exact(a, c));
}
void expect_inconclusive_std(double devq, double h9) {
    if (check_std(devq, h9)) fail("std filter fired on a guard case", devq, h9, lp_std_exact(devq, h9));
}

double pow2(std::mt19937_64 &g, int lo, int hi) {             // a random double with its exponent uniform in [lo, hi]
    std::uniform_int_distribution<int> e(lo, hi);
    std::uniform_real_distribution<double> m(1.0, 2.0);
    return std::ldexp(m(g), e(g));
}

}  // namespace

int main() {
    std::mt19937_64 g(20240607);
    const double deltas[] = {0.0, 0x1p-52, 0x1p-40, 0x1p-31, 0x1p-30, 0x1p-29};
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double sub = std::numeric_limits<double>::denorm_min() * 1000.0;

    // ---- random operands over the whole guarded range (and beyond it: the guards then decide) ----
    for (int k = 0; k < 1000000; k++) {
        check_cvg(pow2(g, -1074 + 52, 1023), pow2(g, -110, 1023));
        check_std(pow2(g, -1074 + 52, 1023), (k & 1 ? -1.0 : 1.0) * pow2(g, -410, 410));
    }
    // ---- operands at threshold * (1 +- delta): a = T^2 c (1 +- d), devq = (S |h9|)^2 (1 +- d), formed in long double ----
    long near_fired = 0, near_total = 0;
    for (int k = 0; k < 200000; k++) {
        const double c = pow2(g, -100, 900), h9 = (k & 1 ? -1.0 : 1.0) * pow2(g, -400, 399);
        for (double d : deltas)
            for (int sgn = -1; sgn <= 1; sgn += 2) {
                const long double f = 1.0L + sgn * (long double)d;
                const double a = (double)((long double)T * (long double)T * (long double)c * f);
                const long double sh = (long double)S * std::fabs((long double)h9);
                const double devq = (double)(sh * sh * f);
                const bool fa = check_cvg(a, c), fs = check_std(devq, h9);
                near_total += 2; near_fired += fa + fs;
                // not a soundness claim but what makes the filter worth having: well above the margin it fires, at or below the
                // threshold it does not
                if (sgn > 0 && d == 0x1p-29 && !(fa && fs)) fail("filter silent at threshold * (1 + 2^-29)", a, devq, 0.0);
                if ((sgn < 0 || d == 0.0) && (fa || fs)) fail("filter fired at or below the threshold", a, devq, 0.0);
            }
    }
    // ---- guards ----
    const double ok_c = 3.0, ok_a = 1.0, ok_h = -7.5, ok_d = 1.0;
    if (!check_cvg(ok_a, ok_c) || !check_std(ok_d, ok_h)) fail("plain operands far above the threshold must fire", ok_a, ok_c, 0.0);
    for (double a : {0.0, -0.0, sub, -1.0, inf, -inf, nan}) {
        if (a == sub) { check_cvg(a, ok_c); continue; }        // a subnormal numerator is an ordinary small value: sound either way
        expect_inconclusive_cvg(a, ok_c);
    }
    for (double c : {0.0, -0.0, sub, 0x1p-101, std::nextafter(0x1p-100, 0.0), -1.0, inf, -inf, nan}) expect_inconclusive_cvg(ok_a, c);
    expect_inconclusive_cvg(nan, nan);
    expect_inconclusive_cvg(inf, inf);
    if (!check_cvg(1.0, 0x1p-100)) fail("c = 2^-100 is inside the guard", 1.0, 0x1p-100, 0.0);
    for (double d : {0.0, -0.0, -1.0, inf, -inf, nan}) expect_inconclusive_std(d, ok_h);
    for (double h : {0.0, -0.0, sub, -sub, std::nextafter(0x1p-400, 0.0), std::nextafter(0x1p400, inf), -0x1p401, inf, -inf, nan})
        expect_inconclusive_std(ok_d, h);
    expect_inconclusive_std(nan, nan);
    if (!check_std(ok_d, 0x1p-400) || !check_std(0x1p1000, -0x1p400)) fail("|h9| = 2^+-400 is inside the guard", ok_d, 0x1p400, 0.0);

    std::printf("cvg: %ld of %ld fired; std: %ld of %ld fired; near the threshold %ld of %ld fired\n", fired_cvg, seen_cvg, fired_std, seen_std,
                near_fired, near_total);
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("stop filter ok\n");
    return 0;
}
