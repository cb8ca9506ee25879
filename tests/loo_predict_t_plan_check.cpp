// CPU check of the fields plan_loo_predict (pybmc_amd/csrc/bmc_plan.h) gains under the Student-t
// likelihood: the phases of the append and the further per-draw constants.  The
// rest of the plan is tests/loo_predict_plan_check.cpp's.
//   plan <n_points> <n_draws> <k> <n_cu>   the t plan's fields as key=value
//   sweep                                  a grid of shapes x CU counts: everything but the new
//                                          fields is the Gaussian plan's; the t plan runs
//                                          LOO_PREDICT_T_PHASES appends, each one more pass over the
//                                          matrix, and holds LOO_PREDICT_T_ROWS doubles per draw
//                                          behind the Gaussian work space, which keeps its layout;
//                                          prints "sweep <plans> <failures>" last
#include "../pybmc_amd/csrc/bmc_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace bmc;

static int check(int64_t n, int64_t S, int k, int n_cu) {
    const LooPredictPlan g = plan_loo_predict(n, S, k, n_cu);
    const LooPredictPlan t = plan_loo_predict(n, S, k, n_cu, true);
    int bad = 0;
    // the Gaussian plan: one append, no further rows (also what the default argument gives)
    const LooPredictPlan d = plan_loo_predict(n, S, k, n_cu, false);
    bad += g.append_phases != 1 || g.draw_rows != 0 || d.append_phases != 1 || d.draw_rows != 0 ||
           d.matrix_passes != g.matrix_passes;
    bad += g.matrix_passes != g.loo.matrix_passes + g.bucket_pass;
    // the t plan: the same passes, cap, LDS and limits
    bad += t.loo.tail != g.loo.tail || t.loo.cap != g.loo.cap || t.loo.grid_points != g.loo.grid_points ||
           t.loo.select_passes != g.loo.select_passes || t.loo.matrix_passes != g.loo.matrix_passes ||
           t.loo.score.splits != g.loo.score.splits || t.loo.score.tiles_per_split != g.loo.score.tiles_per_split ||
           t.loo.score.k_pad != g.loo.score.k_pad || t.fit_lds != g.fit_lds || t.record_bytes != g.record_bytes ||
           t.bucket_pass != g.bucket_pass || t.ok != g.ok;
    bad += t.append_phases != LOO_PREDICT_T_PHASES || t.append_phases != 2;
    bad += t.matrix_passes != g.matrix_passes + (t.append_phases - 1) || t.matrix_passes > 13;
    bad += t.draw_rows != (int64_t)LOO_PREDICT_T_ROWS * S || LOO_PREDICT_T_ROWS != 2;
    // the phases share the payload slots: the work space differs by the rows alone, which lie last
    const LooPredictBuffers bg = loo_predict_buffers(g, n), bt = loo_predict_buffers(t, n);
    bad += bg.tc != 0 || bt.tc % 256 != 0 || bt.tc < (size_t)S * 2 * 8 || bt.tc >= (size_t)S * 2 * 8 + 256;
    bad += bt.candidx != bg.candidx || bt.pay != bg.pay || bt.bucket != bg.bucket || bt.out != bg.out ||
           bt.loo.total() != bg.loo.total();
    bad += bt.total() != bg.total() + bt.tc;
    bad += bt.total() != bt.loo.total() + bt.candidx + bt.pay + bt.bucket + bt.out + bt.tc;
    if (bad)
        std::printf("FAIL n=%lld S=%lld k=%d cu=%d: phases %d rows %lld passes %d\n", (long long)n,
                    (long long)S, k, n_cu, t.append_phases, (long long)t.draw_rows, t.matrix_passes);
    return bad != 0;
}

int main(int argc, char** argv) {
    if (argc == 6 && !std::strcmp(argv[1], "plan")) {
        const int64_t n = std::atoll(argv[2]), S = std::atoll(argv[3]);
        const int k = std::atoi(argv[4]), cu = std::atoi(argv[5]);
        const LooPredictPlan p = plan_loo_predict(n, S, k, cu, true);
        std::printf("append_phases=%d draw_rows=%lld matrix_passes=%d gaussian_matrix_passes=%d "
                    "bucket_pass=%d ok=%d tc_bytes=%llu workspace=%llu\n",
                    p.append_phases, (long long)p.draw_rows, p.matrix_passes,
                    plan_loo_predict(n, S, k, cu).matrix_passes, p.bucket_pass, (int)p.ok,
                    (unsigned long long)loo_predict_buffers(p, n).tc,
                    (unsigned long long)loo_predict_buffers(p, n).total());
        return 0;
    }
    if (argc == 2 && !std::strcmp(argv[1], "sweep")) {
        const int64_t ns[] = {1, 63, 64, 65, 377, 1000, 10000, 40000};
        const int64_t Ss[] = {2,    24,    25,     26,     63,      64,      65,      127,    128,
                              129,  400,   2000,   4097,   12000,   50000,   400000,  465125, 1863225,
                              1863226, 7454720, 30000000};
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
        std::printf("sweep %ld %ld\n", plans, fails);
        return fails != 0;
    }
    std::fprintf(stderr, "usage: loo_predict_t_plan_check plan <n> <S> <k> <n_cu> | sweep\n");
    return 2;
}
