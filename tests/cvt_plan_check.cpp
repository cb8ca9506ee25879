// CPU driver of bmc_cvt_plan.h for tests/test_cvt_plan.py (g++, no HIP).
//   cvt_plan_check plan K C T burn thin G budget label...
//       -> per batch "f0-f1 z_len yv_len rows : fold,n_train,rpw,padded,z_off,yv_off,row0 ; ... : chain0+n,..."
//          one batch per line, first line "kept bytes(fold 0) ...bytes(fold F-1)"; "none fold need" when
//          not one fold fits
//   cvt_plan_check check K C T burn thin nu G label...   -> "ok" or the refusal text of cvt_check
//          (G > 0: a grid 1 .. G with unit weights, nu_init = 0 -- or G = 65 to overflow it)
#include "../pybmc_amd/csrc/bmc_cvt_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace bmc;

static std::vector<int64_t> labels_from(int argc, char** argv, int first) {
    std::vector<int64_t> l;
    for (int i = first; i < argc; ++i) l.push_back(std::atoll(argv[i]));
    return l;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    if (!std::strcmp(argv[1], "plan") && argc >= 10) {
        const int k = std::atoi(argv[2]), C = std::atoi(argv[3]);
        const int64_t T = std::atoll(argv[4]), burn = std::atoll(argv[5]), thin = std::atoll(argv[6]);
        const int G = std::atoi(argv[7]);
        const size_t budget = (size_t)std::strtoull(argv[8], nullptr, 10);
        const std::vector<int64_t> l = labels_from(argc, argv, 9);
        const int64_t n = (int64_t)l.size();
        int F = 0;
        for (int64_t v : l) F = v + 1 > F ? (int)v + 1 : F;
        std::vector<int64_t> count;
        if (!cv_check(n, k, F, l.data(), &count).empty()) return 3;
        const int64_t kept = cv_kept_draws(T, burn, thin);
        std::printf("%lld", (long long)kept);
        for (int f = 0; f < F; ++f) std::printf(" %zu", cvt_fold_bytes(n - count[f], k, C, T, burn, kept, G));
        std::printf("\n");
        std::vector<CvtBatch> b;
        int32_t too_big = -1;
        size_t need = 0;
        if (!plan_cvt(F, C, k, count.data(), n, T, burn, kept, G, budget, b, &too_big, &need)) {
            std::printf("none %d %zu\n", too_big, need);
            return 0;
        }
        for (const CvtBatch& x : b) {
            std::printf("%d-%d %lld %lld %lld :", x.f0, x.f1, (long long)x.z_len, (long long)x.yv_len,
                        (long long)x.rows);
            for (size_t i = 0; i < x.folds.size(); ++i) {
                const CvtFold& d = x.folds[i];
                std::printf("%s%d,%lld,%lld,%lld,%lld,%lld,%lld", i ? " ; " : " ", d.fold, (long long)d.n_train,
                            (long long)d.rows_per_wave, (long long)d.rows_padded, (long long)d.z_off,
                            (long long)d.yv_off, (long long)d.row0);
            }
            std::printf(" : ");
            for (size_t i = 0; i < x.launches.size(); ++i)
                std::printf("%s%lld+%d", i ? "," : "", (long long)x.launches[i].chain0, x.launches[i].n_chains);
            std::printf("\n");
        }
        return 0;
    }
    if (!std::strcmp(argv[1], "check") && argc >= 9) {
        const int k = std::atoi(argv[2]), C = std::atoi(argv[3]);
        const int64_t T = std::atoll(argv[4]), burn = std::atoll(argv[5]), thin = std::atoll(argv[6]);
        const double nu = std::atof(argv[7]);
        const int G = std::atoi(argv[8]);
        const std::vector<int64_t> l = labels_from(argc, argv, 9);
        int F = 0;
        for (int64_t v : l) F = v + 1 > F ? (int)v + 1 : F;
        std::vector<double> grid, weight;
        for (int g = 0; g < G; ++g) {
            grid.push_back(1.0 + g);
            weight.push_back(1.0);
        }
        const std::string r = cvt_check((int64_t)l.size(), k, F, l.data(), C, T, burn, thin, nu,
                                        G ? grid.data() : nullptr, G ? weight.data() : nullptr, G, 0);
        std::printf("%s\n", r.empty() ? "ok" : r.c_str());
        return 0;
    }
    return 2;
}
