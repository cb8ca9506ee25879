// CPU check of plan_score (pybmc_amd/csrc/bmc_plan.h), the draw-split plan of the pointwise
// log-likelihood kernels.
//   plan <n_points> <n_draws> <k> <n_cu>   the plan's fields as key=value
//   sweep                                  a grid of shapes x CU counts: every draw tile in exactly
//                                          one split, no empty split, the workgroup count bounded;
//                                          prints "sweep <plans> <failures>" last
#include "../pybmc_amd/csrc/bmc_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace bmc;

static int check(int64_t n, int64_t S, int k, int n_cu) {
    const ScorePlan p = plan_score(n, S, k, n_cu);
    int bad = 0;
    bad += p.point_tiles * SCORE_TILE < n || (p.point_tiles - 1) * SCORE_TILE >= n;
    bad += p.draw_tiles * SCORE_TILE < S || (p.draw_tiles - 1) * SCORE_TILE >= S;
    bad += p.k_pad < k || p.k_pad % 16 != 0 || p.k_pad - k >= 16;
    bad += p.splits < 1 || p.tiles_per_split < 1;
    // split j walks [j * tps, min((j + 1) * tps, draw_tiles)): a partition with no empty part
    int64_t covered = 0;
    for (int64_t j = 0; j < p.splits; ++j) {
        const int64_t lo = j * p.tiles_per_split;
        int64_t hi = lo + p.tiles_per_split;
        if (hi > p.draw_tiles) hi = p.draw_tiles;
        if (hi <= lo || lo != covered) ++bad;
        covered = hi;
    }
    bad += covered != p.draw_tiles;
    // no more workgroups than the target asks for (rounding: below twice the target), and a split
    // shorter than SCORE_MIN_TILES only when it is the only way to cover the draws
    const int64_t target = (int64_t)SCORE_GROUPS_PER_CU * n_cu;
    if (p.splits > 1) {
        bad += p.tiles_per_split < SCORE_MIN_TILES;
        bad += (p.splits - 1) * p.point_tiles >= target;
    }
    // few points and many draws must fill the chip
    if (p.point_tiles < n_cu && p.draw_tiles >= (int64_t)SCORE_MIN_TILES * target)
        bad += p.splits * p.point_tiles < n_cu;
    if (bad)
        std::printf("FAIL n=%lld S=%lld k=%d cu=%d: tiles %lld x %lld, %lld splits of %lld\n",
                    (long long)n, (long long)S, k, n_cu, (long long)p.point_tiles,
                    (long long)p.draw_tiles, (long long)p.splits, (long long)p.tiles_per_split);
    return bad != 0;
}

int main(int argc, char** argv) {
    if (argc == 6 && !std::strcmp(argv[1], "plan")) {
        const ScorePlan p = plan_score(std::atoll(argv[2]), std::atoll(argv[3]), std::atoi(argv[4]),
                                       std::atoi(argv[5]));
        std::printf("point_tiles=%lld draw_tiles=%lld tiles_per_split=%lld splits=%lld k_pad=%d\n",
                    (long long)p.point_tiles, (long long)p.draw_tiles, (long long)p.tiles_per_split,
                    (long long)p.splits, p.k_pad);
        return 0;
    }
    if (argc == 2 && !std::strcmp(argv[1], "sweep")) {
        const int64_t ns[] = {1, 63, 64, 65, 377, 1000, 2000, 10000, 16384, 40000, 1000000};
        const int64_t Ss[] = {2, 63, 64, 65, 255, 256, 257, 4097, 12000, 50000, 400000, 3200000};
        const int ks[] = {1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 256};
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
    std::fprintf(stderr, "usage: score_plan_check plan <n> <S> <k> <n_cu> | sweep\n");
    return 2;
}
