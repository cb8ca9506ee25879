// CPU check of plan_loo_predict (pybmc_amd/csrc/bmc_plan.h), the plan of the leave-one-out
// predictive moments on top of plan_loo (which tests/loo_plan_check.cpp checks).
//   plan <n_points> <n_draws> <k> <n_cu>   the plan's fields as key=value
//   sweep                                  a grid of shapes x CU counts: the shared passes are
//                                          plan_loo's, the fit's LDS holds a value, a tail weight
//                                          and a draw index per slot and fits gfx950's 160 KiB when
//                                          the plan is ok, the draw limit is the stated one, the
//                                          work space is loo_predict_buffers';
//                                          prints "sweep <plans> <failures>" last
#include "../pybmc_amd/csrc/bmc_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace bmc;

static int check(int64_t n, int64_t S, int k, int n_cu) {
    const LooPredictPlan p = plan_loo_predict(n, S, k, n_cu);
    const LooPlan q = plan_loo(n, S, k, n_cu);
    int bad = 0;
    bad += p.loo.tail != q.tail || p.loo.grid_points != q.grid_points || p.loo.cap != q.cap || p.loo.select_passes != q.select_passes ||
           p.loo.matrix_passes != q.matrix_passes || p.loo.ok != q.ok ||
           p.loo.score.point_tiles != q.score.point_tiles ||
           p.loo.score.draw_tiles != q.score.draw_tiles ||
           p.loo.score.tiles_per_split != q.score.tiles_per_split ||
           p.loo.score.splits != q.score.splits || p.loo.score.k_pad != q.score.k_pad;
    // the candidate record: an f64 value and a u32 draw index (every draw index fits)
    bad += p.record_bytes != 12;
    bad += p.ok && S > (int64_t)0xffffffffll;
    // the fit's LDS: cap values, cap / 2 >= M tail weights, cap draw indices
    bad += p.fit_lds != p.loo.cap * 8 + p.loo.cap / 2 * 8 + p.loo.cap * 4;
    bad += p.loo.cap / 2 < p.loo.tail + 1;
    bad += p.ok != (p.fit_lds + LOO_FIT_STATIC_LDS <= LOO_LDS_BYTES);
    bad += p.ok != (p.loo.cap <= LOO_PREDICT_MAX_CAP);
    bad += p.ok != (S <= LOO_PREDICT_MAX_DRAWS);
    bad += p.ok && !p.loo.ok;
    // one more pass over the matrix, only where a select can end in a one-value bucket
    bad += p.bucket_pass != (p.loo.select_passes > 0 ? 1 : 0);
    bad += p.matrix_passes != p.loo.matrix_passes + p.bucket_pass || p.matrix_passes > 12;
    // work space: loo_buffers, then the parts of loo_predict_buffers
    const LooPredictBuffers b = loo_predict_buffers(p, n);
    const size_t n_pad = (size_t)p.loo.score.point_tiles * SCORE_TILE, sp = (size_t)p.loo.score.splits;
    const size_t want[4] = {n_pad * (size_t)p.loo.cap * 4, sp * n_pad * 4 * 8, sp * n_pad * 3 * 8,
                            (size_t)n * 6 * 8};
    const size_t got[4] = {b.candidx, b.pay, b.bucket, b.out};
    size_t total = loo_buffers(q, n).total();
    bad += b.loo.total() != total;
    for (int e = 0; e < 4; ++e) {
        bad += got[e] % 256 != 0 || got[e] < want[e] || got[e] >= want[e] + 256;
        total += got[e];
    }
    bad += total != b.total();
    if (bad)
        std::printf("FAIL n=%lld S=%lld k=%d cu=%d: tail %lld cap %lld lds %lld ok %d\n", (long long)n,
                    (long long)S, k, n_cu, (long long)p.loo.tail, (long long)p.loo.cap,
                    (long long)p.fit_lds, (int)p.ok);
    return bad != 0;
}

int main(int argc, char** argv) {
    if (argc == 6 && !std::strcmp(argv[1], "plan")) {
        const int64_t n = std::atoll(argv[2]);
        const LooPredictPlan p =
            plan_loo_predict(n, std::atoll(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]));
        std::printf("tail=%lld cap=%lld select_passes=%d bucket_pass=%d matrix_passes=%d ok=%d "
                    "splits=%lld fit_lds=%lld record_bytes=%lld max_draws=%lld workspace=%llu\n",
                    (long long)p.loo.tail, (long long)p.loo.cap, p.loo.select_passes, p.bucket_pass,
                    p.matrix_passes, (int)p.ok, (long long)p.loo.score.splits, (long long)p.fit_lds,
                    (long long)p.record_bytes, (long long)LOO_PREDICT_MAX_DRAWS,
                    (unsigned long long)loo_predict_buffers(p, n).total());
        return 0;
    }
    if (argc == 2 && !std::strcmp(argv[1], "sweep")) {
        const int64_t ns[] = {1, 63, 64, 65, 377, 1000, 10000, 40000};
        const int64_t Ss[] = {2,      24,      25,      26,      63,      64,      65,      127,
                              128,    129,     400,     2000,    4097,    12000,   50000,   400000,
                              465124, 465125,  1863225, 1863226, 3200000, 7454720, 7454721, 30000000};
        const int ks[] = {1, 3, 32, 33, 256};
        const int cus[] = {1, 8, 64, 256, 304};
        long plans = 0, fails = 0;
        for (int64_t n : ns)
            for (int64_t S : Ss)
                for (int k : ks)
                    for (int cu : cus) {
                        ++plans;
                        fails += check(n, S, k, cu);
                    }
        for (int64_t S = 2; S <= 70000; ++S) {
            ++plans;
            fails += check(100, S, 3, 256);
        }
        std::printf("sweep %ld %ld\n", plans, fails);
        return fails != 0;
    }
    std::fprintf(stderr, "usage: loo_predict_plan_check plan <n> <S> <k> <n_cu> | sweep\n");
    return 2;
}
