// CPU check of expm1_nonneg and student_t_variate of pybmc_amd/csrc/bmc_math.h (the same text the
// gfx950 kernels compile) against long double.  tests/test_ppc_t_host.py reads the output:
//   line 1   worst error of expm1_nonneg against expm1l, in units in the last place, over
//            (a) a dense sweep of [0, 710): 4 000 000 uniform arguments and 4 000 000 as 710 U^4,
//            (b) 2^e (1 + j 2^-52), j = -4 .. 4 (2^e (1 + j 2^-53) below the power), e = -1074 .. 9,
//            (c) x = -(2 / nu) log(u) as the variate forms it, u = 2^-U(0, 53) and the exact
//                2^-j, j = 0 .. 53, for nu = 0.06, 0.11, 0.5, 1, 1.5, 2, 4, 10, 50, 1e3, 1e6
//   line 2   expm1_nonneg at 0, 709.78 (value, finite), 710 and 1e300 (infinite: 1)
//   line 3   T_ACCURACY: the largest |t - T| / |T| of the variate against its long-double
//            restatement T for nu = 1.5, 4, 50 and 1e9 (u1 = 2^-U(0, 53) on the 2^-53 grid, U(0, 1]
//            and every 2^-j; u2 = U(0, 1] on the grid), T = 0 demanding t = 0
//   line 4   the variate at u1 = 1 (nu = 4); at nu = 0.06, u1 = 2^-53, u2 = 1 (value, then
//            isfinite); at nu = 0.05, u1 = 2^-53, u2 = 1 (isinf)
//   line 5   nu = 1e9 against Box-Muller z = sqrt(-2 log u1) cos(2 pi u2) of this header: the
//            largest (|t / z - 1| - L / (2 nu)) with L = -log u1, i.e. what is left of the
//            difference after the first-order term of sqrt(expm1(x) / x), x = 2 L / nu
#include "../pybmc_amd/csrc/bmc_math.h"
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <random>

static double ulps(double got, long double want) {
    const double w = (double)want;
    if ((long double)got == want) return 0.0;
    const double u = std::fabs(std::nextafter(w, INFINITY) - w);
    return (double)(fabsl((long double)got - want) / (long double)u);
}

static const long double PI_2 = 1.5707963267948966192313216916397514421L;

// cos(2 pi u) for u in [0, 1] on the 2^-53 grid: 4 u = q + r exactly, the quadrant by hand
static long double cos_2pi(double u) {
    const double t = 4.0 * u, q = std::rint(t);
    const long double x = (long double)(t - q) * PI_2;
    const int iq = (int)q & 3;
    const long double b = (iq & 1) ? sinl(x) : cosl(x);
    return ((iq + 1) & 2) ? -b : b;
}

static long double t_long(double u1, double u2, double nu) {
    const long double n = (long double)nu;
    return sqrtl(n * expm1l(-(2.0L / n) * logl((long double)u1))) * cos_2pi(u2);
}

static double grid(double u) {   // onto (0, 1] in steps of 2^-53
    const double m = std::ceil(std::ldexp(u, 53));
    return std::ldexp(m < 1.0 ? 1.0 : m, -53);
}

int main() {
    std::mt19937_64 g(7);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    double worst[3] = {0.0, 0.0, 0.0};
    for (long i = 0; i < 4000000; ++i) {
        const double a = 710.0 * U(g), v = U(g), b = 710.0 * v * v * v * v;
        worst[0] = std::fmax(worst[0], ulps(bmc::expm1_nonneg(a), expm1l((long double)a)));
        if (b < 709.7) worst[0] = std::fmax(worst[0], ulps(bmc::expm1_nonneg(b), expm1l((long double)b)));
    }
    for (int e = -1074; e <= 9; ++e) {
        for (int j = -4; j <= 4; ++j) {
            double x = std::ldexp(1.0, e);
            for (int s = 0; s < (j < 0 ? -j : j); ++s) x = std::nextafter(x, j < 0 ? 0.0 : INFINITY);
            if (x >= 709.7) continue;
            worst[1] = std::fmax(worst[1], ulps(bmc::expm1_nonneg(x), expm1l((long double)x)));
        }
    }
    const double nus[11] = {0.06, 0.11, 0.5, 1.0, 1.5, 2.0, 4.0, 10.0, 50.0, 1e3, 1e6};
    for (double nu : nus) {
        const double ton = 2.0 / nu;
        for (long i = 0; i < 400000 + 54; ++i) {
            const double u = i < 54 ? std::ldexp(1.0, -(int)i) : grid(std::exp2(-53.0 * U(g)));
            const double x = ton * -bmc::log_normal_arg(u);
            if (x >= 709.7) continue;
            worst[2] = std::fmax(worst[2], ulps(bmc::expm1_nonneg(x), expm1l((long double)x)));
        }
    }
    std::printf("%.4f %.4f %.4f\n", worst[0], worst[1], worst[2]);
    std::printf("%.17g %.17g %d %d %d\n", bmc::expm1_nonneg(0.0), bmc::expm1_nonneg(709.78),
                (int)std::isfinite(bmc::expm1_nonneg(709.78)), (int)std::isinf(bmc::expm1_nonneg(710.0)),
                (int)std::isinf(bmc::expm1_nonneg(1e300)));

    const double tnus[4] = {1.5, 4.0, 50.0, 1e9};
    double acc[4] = {0.0, 0.0, 0.0, 0.0}, bm = -1.0;
    int zero_ok = 1;
    for (int a = 0; a < 4; ++a) {
        const double nu = tnus[a], ton = 2.0 / nu;
        for (long i = 0; i < 1000000 + 54; ++i) {
            const double u1 = i < 54 ? std::ldexp(1.0, -(int)i)
                                     : (i & 1) ? grid(std::exp2(-53.0 * U(g))) : grid(U(g));
            const double u2 = grid(U(g));
            const double t = bmc::student_t_variate(u1, u2, nu, ton);
            const long double T = t_long(u1, u2, nu);
            if (T == 0.0L) {
                zero_ok &= (int)(t == 0.0);
                continue;
            }
            acc[a] = std::fmax(acc[a], (double)(fabsl((long double)t - T) / fabsl(T)));
            if (a == 3 && u1 < 1.0) {
                double z0, z1;
                bmc::box_muller_pair(u1, u2, z0, z1);
                const double L = -(double)logl((long double)u1);
                bm = std::fmax(bm, std::fabs(t / z0 - 1.0) - L / (2.0 * nu));
            }
        }
    }
    std::printf("%.6g %.6g %.6g %.6g %d\n", acc[0], acc[1], acc[2], acc[3], zero_ok);
    const double tiny = std::ldexp(1.0, -53);
    const double t006 = bmc::student_t_variate(tiny, 1.0, 0.06, 2.0 / 0.06);
    std::printf("%.17g %.17g %d %d\n", bmc::student_t_variate(1.0, 0.3, 4.0, 0.5), t006,
                (int)std::isfinite(t006), (int)std::isinf(bmc::student_t_variate(tiny, 1.0, 0.05, 2.0 / 0.05)));
    std::printf("%.6g\n", bm);
    return 0;
}
