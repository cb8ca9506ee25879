// Host driver of the nu-grid part of pybmc_amd/csrc/bmc_robust_plan.h for tests/test_robust_nu_plan.py
// (plain g++, no HIP).
//   max                              "ROBUST_MAX_NU_GRID"
//   check nu_init g0:w0 g1:w1 ...    "ok" or the reason
//   table n g0:w0 g1:w1 ...          one line per grid value: "nu shape h c"   (%.17g)
//   consts n nu                      "c rel": c_g at weight 1 and its relative deviation from the long
//                                    double evaluation n (h log h - lgamma h), h = nu / 2
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../pybmc_amd/csrc/bmc_robust_plan.h"

using namespace bmc;

static void pairs(int argc, char** argv, int first, std::vector<double>& grid, std::vector<double>& weight) {
    for (int i = first; i < argc; ++i) {
        const char* colon = std::strchr(argv[i], ':');
        grid.push_back(std::atof(argv[i]));
        weight.push_back(colon ? std::atof(colon + 1) : 1.0);
    }
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string cmd = argv[1];
    std::vector<double> grid, weight;
    if (cmd == "max") {
        std::printf("%d\n", ROBUST_MAX_NU_GRID);
        return 0;
    }
    if (cmd == "check" && argc >= 3) {
        pairs(argc, argv, 3, grid, weight);
        const std::string why = robust_nu_check(grid.data(), weight.data(), (int32_t)grid.size(), std::atoi(argv[2]));
        std::printf("%s\n", why.empty() ? "ok" : why.c_str());
        return 0;
    }
    if (cmd == "table" && argc >= 4) {
        pairs(argc, argv, 3, grid, weight);
        const int G = (int)grid.size();
        std::vector<double> tab(4 * grid.size());
        robust_nu_table(grid.data(), weight.data(), G, std::atoll(argv[2]), tab.data());
        for (int g = 0; g < G; ++g)
            std::printf("%.17g %.17g %.17g %.17g\n", tab[g], tab[G + g], tab[2 * G + g], tab[3 * G + g]);
        return 0;
    }
    if (cmd == "consts" && argc == 4) {
        const int64_t n = std::atoll(argv[2]);
        const double nu = std::atof(argv[3]), one = 1.0;
        double tab[4];
        robust_nu_table(&nu, &one, 1, n, tab);
        const long double h = (long double)nu / 2.0L;
        const long double ref = (long double)n * (h * logl(h) - lgammal(h));
        const long double diff = fabsl((long double)tab[3] - ref);   // h = 1: both are exactly 0
        const long double rel = diff == 0.0L ? 0.0L : diff / fabsl(ref);
        std::printf("%.17g %.6Le\n", tab[3], rel);
        return 0;
    }
    return 2;
}
