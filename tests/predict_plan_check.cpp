// CPU check of plan_predict_orderstat (pybmc_amd/csrc/bmc_plan.h), the route of the posterior
// predictive's order statistics.
//   constants                        SEL_BINS, SEL_CAP, SEL_THREADS and the request limits as key=value
//   plan <S> <n_q> <n_cov> <M>       the plan's fields as key=value
//   sweep                            S = 1 .. 16384 x a few (n_q, n_cov) x a few M: the invariants of
//                                    every plan, one "class <select> <vpt> <nsort>" line per class
//                                    seen, then "sweep <plans> <failures>"
#include "../pybmc_amd/csrc/bmc_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <tuple>

using namespace bmc;

// the rules, restated independently of the plan's code
static int want_nsort(int S) {
    int n = 64;
    while (n < S) n *= 2;
    return n;
}
static int want_vpt(int S) {
    for (int v = 8; v <= 32; v += 4)
        if ((int64_t)v * SEL_THREADS >= S) return v;
    return 0;
}

static int check(int S, int n_q, int n_cov, int64_t M) {
    const PredictOrderstatPlan p = plan_predict_orderstat(S, n_q, n_cov, M);
    int bad = 0;
    const bool refuse = S < 1 || S > 16384 || n_q < 0 || n_q > 64 || n_cov < 0 || n_cov > 64 || M < 1;
    if (refuse) {
        bad += p.ok;
    } else {
        const int n_t = 2 * n_q + 2 * n_cov;
        bad += !p.ok;
        bad += p.launch != (n_t > 0);
        bad += p.select != (S >= 2048 && n_t <= 128);
        bad += p.nsort != want_nsort(S) || p.nsort < S;
        bad += p.sort_threads < 128 || p.sort_threads > 1024 || (p.sort_threads & (p.sort_threads - 1));
        bad += p.sort_threads != (p.nsort / 2 < 128 ? 128 : p.nsort / 2 > 1024 ? 1024 : p.nsort / 2);
        // thread t < n_q writes a percentile, thread 64 + c counts interval c
        if (n_q > 0) bad += p.sort_threads < n_q;
        if (n_cov > 0) bad += p.sort_threads < 64 + n_cov;
        if (p.select && n_q > 0) bad += SEL_THREADS < n_q;
        if (p.select && n_cov > 0) bad += SEL_THREADS < 64 + n_cov;
        if (p.select) bad += SEL_THREADS < n_t;          // thread t < n_t places requested rank t
        bad += p.lds_sort != (size_t)p.nsort * 8 || p.lds_sort > LDS_LIMIT;
        bad += p.lds_select > LDS_LIMIT;
        const int64_t first = M < 2048 ? M : 2048;
        if (p.select) {
            bad += p.vpt != want_vpt(S) || (int64_t)p.vpt * SEL_THREADS < S;
            bad += p.vpt > 8 && (int64_t)(p.vpt - 4) * SEL_THREADS >= S;   // no smaller class fits
            bad += p.blocks_select != first;
            bad += p.blocks_sort != (M < 256 ? M : 256);
            // the kernel's carve-up: hist + slot, min / max, wave totals + flag, prefixes, four
            // arrays of n_t words, up to 15 bytes of alignment, n_t lists
            const size_t fixed = (size_t)SEL_BINS * 8 + 16 * 8 + 16 * 4 + (size_t)SEL_THREADS * 4;
            const size_t need = fixed + (size_t)n_t * 16 + 15 + (size_t)n_t * SEL_CAP * 8;
            bad += p.lds_select < need || p.lds_select > need + 16;
        } else {
            bad += p.vpt != 0 || p.blocks_select != 0 || p.lds_select != 0;
            bad += p.blocks_sort != first;
        }
        bad += p.blocks_sort < 1 || p.blocks_sort > M;
    }
    if (bad) std::printf("FAIL S=%d n_q=%d n_cov=%d M=%lld\n", S, n_q, n_cov, (long long)M);
    return bad != 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "constants")) {
        std::printf("SEL_BINS=%d SEL_CAP=%d SEL_THREADS=%d MAX_DRAWS=%d MAX_Q=%d MAX_COV=%d "
                    "SELECT_MIN_DRAWS=%d SELECT_MAX_RANKS=%d MAX_BLOCKS=%lld FALLBACK_BLOCKS=%lld\n",
                    SEL_BINS, SEL_CAP, SEL_THREADS, PREDICT_MAX_DRAWS, PREDICT_MAX_Q, PREDICT_MAX_COV,
                    PREDICT_SELECT_MIN_DRAWS, PREDICT_SELECT_MAX_RANKS, (long long)PREDICT_MAX_BLOCKS,
                    (long long)PREDICT_FALLBACK_BLOCKS);
        return 0;
    }
    if (argc == 6 && !std::strcmp(argv[1], "plan")) {
        const PredictOrderstatPlan p = plan_predict_orderstat(std::atoi(argv[2]), std::atoi(argv[3]),
                                                              std::atoi(argv[4]), std::atoll(argv[5]));
        std::printf("ok=%d launch=%d select=%d vpt=%d nsort=%d sort_threads=%d blocks_select=%lld "
                    "blocks_sort=%lld lds_select=%zu lds_sort=%zu\n",
                    (int)p.ok, (int)p.launch, (int)p.select, p.vpt, p.nsort, p.sort_threads,
                    (long long)p.blocks_select, (long long)p.blocks_sort, p.lds_select, p.lds_sort);
        return 0;
    }
    if (argc == 2 && !std::strcmp(argv[1], "sweep")) {
        const int reqs[][2] = {{6, 21}, {3, 0}, {0, 21}, {1, 0}, {0, 1}, {0, 0}, {43, 21}, {44, 21},
                               {64, 0}, {0, 64}, {64, 64}, {65, 0}, {0, 65}, {-1, 0}};
        const int64_t Ms[] = {0, 1, 70, 255, 256, 257, 2047, 2048, 2049, 50000};
        std::set<std::tuple<int, int, int>> classes;
        long plans = 0, fails = 0;
        for (int S = 0; S <= 16385; ++S)
            for (const auto& r : reqs)
                for (int64_t M : Ms) {
                    ++plans;
                    fails += check(S, r[0], r[1], M);
                    const PredictOrderstatPlan p = plan_predict_orderstat(S, r[0], r[1], M);
                    if (p.ok && p.launch) classes.insert({(int)p.select, p.vpt, p.nsort});
                }
        for (const auto& c : classes)
            std::printf("class %d %d %d\n", std::get<0>(c), std::get<1>(c), std::get<2>(c));
        std::printf("sweep %ld %ld\n", plans, fails);
        return fails != 0;
    }
    std::fprintf(stderr, "usage: predict_plan_check constants | plan <S> <n_q> <n_cov> <M> | sweep\n");
    return 2;
}
