// CPU check of log1p_nonneg of pybmc_amd/csrc/bmc_math.h (the same text the gfx950 kernels
// compile): worst error, in units in the last place, against long-double log1pl over
// x = 10^U(-320, 300), x = U(0, 4) and x = 2^U(-60, 10), then the exact values 0, 2^-53, 1 and
// DBL_MAX (value and error each), then NaN and +inf.  tests/test_tscore_host.py reads the output.
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

int main() {
    std::mt19937_64 g(1);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    double worst[3] = {0.0, 0.0, 0.0};
    for (long i = 0; i < 3000000; ++i) {
        const double x[3] = {std::pow(10.0, -320.0 + 620.0 * U(g)), 4.0 * U(g),
                             std::exp2(-60.0 + 70.0 * U(g))};
        for (int j = 0; j < 3; ++j)
            worst[j] = std::fmax(worst[j], ulps(bmc::log1p_nonneg(x[j]), log1pl((long double)x[j])));
    }
    std::printf("%.4f %.4f %.4f\n", worst[0], worst[1], worst[2]);
    const double exact[4] = {0.0, std::ldexp(1.0, -53), 1.0, DBL_MAX};
    for (double x : exact)
        std::printf("%.17g %.4f\n", bmc::log1p_nonneg(x), ulps(bmc::log1p_nonneg(x), log1pl((long double)x)));
    std::printf("%d %d\n", (int)std::isnan(bmc::log1p_nonneg(NAN)),
                (int)std::isfinite(bmc::log1p_nonneg(INFINITY)));
    return 0;
}
