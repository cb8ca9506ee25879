// CPU build of bmc::student_t_cdf (pybmc_amd/csrc/bmc_math.h) for tests/test_loo_predict_t_host.py
// and the device comparison of tests/test_loo_predict_t_gpu.py.
//   loo_predict_t_math_check <in> <out>
// <in>: float64 pairs (z, nu).  <out>: float64 triples (F, steps, f): F = student_t_cdf(z, nu, f),
// steps the continued fraction's steps (student_t_tail), f the density the scoring kernels would
// hand it: exp(C(nu) - (nu + 1)/2 log1p_nonneg(z^2 / nu)) with the long-double C(nu) of
// student_t_cnu (bmc_launch.h, a HIP header: restated here).
//   loo_predict_t_math_check limits      prints "nu_min nu_max max_steps"
#include "../pybmc_amd/csrc/bmc_math.h"

#include <cstdio>
#include <cstring>
#include <vector>

static double cnu(double nu_) {
    const long double nu = (long double)nu_;
    return (double)(lgammal(0.5L * (nu + 1.0L)) - lgammal(0.5L * nu) -
                    0.5L * logl(nu * 3.14159265358979323846264338327950288L));
}

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "limits")) {
        std::printf("%.17g %.17g %d\n", bmc::STUDENT_T_CDF_NU_MIN, bmc::STUDENT_T_CDF_NU_MAX,
                    bmc::STUDENT_T_CDF_MAX_STEPS);
        return 0;
    }
    if (argc != 3) {
        std::fprintf(stderr, "usage: loo_predict_t_math_check <in> <out> | limits\n");
        return 2;
    }
    std::FILE* fi = std::fopen(argv[1], "rb");
    if (!fi) return 1;
    std::vector<double> in;
    double pair[2];
    while (std::fread(pair, 8, 2, fi) == 2) in.insert(in.end(), pair, pair + 2);
    std::fclose(fi);
    std::vector<double> out;
    for (size_t e = 0; e < in.size(); e += 2) {
        const double z = in[e], nu = in[e + 1];
        const double f = exp(fma(-0.5 * (nu + 1.0), bmc::log1p_nonneg((z * z) / nu), cnu(nu)));
        int steps = 0;
        const double az = fabs(z);
        bmc::student_t_tail((az * az) / nu, nu, az < __builtin_inf() ? az * f : 0.0, steps);
        out.push_back(bmc::student_t_cdf(z, nu, f));
        out.push_back((double)steps);
        out.push_back(f);
    }
    std::FILE* fo = std::fopen(argv[2], "wb");
    if (!fo) return 1;
    const bool ok = std::fwrite(out.data(), 8, out.size(), fo) == out.size();
    return std::fclose(fo) == 0 && ok ? 0 : 1;
}
