// CPU check of plan_loo (pybmc_amd/csrc/bmc_plan.h), the pass and candidate plan of the PSIS-LOO
// kernels.
//   plan <n_points> <n_draws> <k> <n_cu>   the plan's fields as key=value
//   sweep                                  a grid of shapes x CU counts: the tail length is the
//                                          estimator's, the cap holds the tail, the cutoff and a
//                                          sort's scratch, the passes are bounded, every draw is in
//                                          exactly one split, the work space is loo_buffers';
//                                          prints "sweep <plans> <failures>" last
#include "../pybmc_amd/csrc/bmc_plan.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace bmc;

static int check(int64_t n, int64_t S, int k, int n_cu) {
    const LooPlan p = plan_loo(n, S, k, n_cu);
    const ScorePlan q = plan_score(n, S, k, n_cu);
    int bad = 0;
    // the tail: min(floor(S / 5), ceil(3 sqrt(S))), none below 5; the square root in integers
    int64_t t = (int64_t)std::ceil(3.0 * std::sqrt((double)S));
    while ((t - 1) * (t - 1) >= 9 * S) --t;
    while (t * t < 9 * S) ++t;
    int64_t M = S / 5 < t ? S / 5 : t;
    if (M < LOO_MIN_TAIL) M = 0;
    bad += p.tail != M;
    bad += p.tail > 0 && S < 25;
    bad += p.tail == 0 && S >= 25;
    // the grid of the fit: 30 + floor(sqrt(M)) points, none without a tail; a plan that is ok holds
    // them on chip (128 of each array)
    int64_t rt = 0;
    while ((rt + 1) * (rt + 1) <= M) ++rt;
    bad += p.grid_points != (M > 0 ? 30 + rt : 0) || (p.ok && p.grid_points > 128);
    // the cap: a power of two, room for the tail and the cutoff (M + 1) and as much again for the
    // fit's scratch; the plan is refused, not truncated, when that exceeds the LDS sort
    bad += p.cap < p.tail + 1 || p.cap < 2 * (p.tail + 1) || (p.cap & (p.cap - 1)) != 0;
    bad += p.cap < LOO_MIN_CAP || p.cap >= 4 * (p.tail + 1) + 2 * LOO_MIN_CAP;
    bad += p.ok != (p.cap <= LOO_MAX_CAP);
    bad += p.tail + 1 > S && p.tail > 0;   // the cutoff exists
    // passes: bounded for any input; none when every draw is a candidate or nothing is smoothed
    bad += p.select_passes != 0 && p.select_passes != LOO_MAX_SELECT_PASSES;
    bad += p.select_passes * LOO_DIGIT_BITS > 64 + LOO_DIGIT_BITS - 1;
    bad += (p.select_passes == 0) != (p.tail == 0 || S <= p.cap);
    bad += p.matrix_passes != 3 + p.select_passes || p.matrix_passes > 11;
    // every draw in exactly one split: the split plan is plan_score's
    bad += std::memcmp(&p.score, &q, sizeof q) != 0;
    int64_t covered = 0;
    for (int64_t j = 0; j < p.score.splits; ++j) {
        const int64_t lo = j * p.score.tiles_per_split;
        int64_t hi = lo + p.score.tiles_per_split;
        if (hi > p.score.draw_tiles) hi = p.score.draw_tiles;
        if (hi <= lo || lo != covered) ++bad;
        covered = hi;
    }
    bad += covered != p.score.draw_tiles || covered * SCORE_TILE < S;
    // work space: the parts of loo_buffers, each a whole number of 256-byte lines that holds what
    // its comment says
    const LooBuffers b = loo_buffers(p, n);
    const size_t n_pad = (size_t)p.score.point_tiles * SCORE_TILE, sp = (size_t)p.score.splits;
    const size_t want[9] = {sp * n_pad * 24, n_pad * 8, n_pad * 8, n_pad * 16, n_pad * 256 * 4,
                            n_pad * 4, n_pad * (size_t)p.cap * 8, sp * n_pad * 8, (size_t)n * 16};
    const size_t got[9] = {b.range, b.prefix, b.kmin, b.meta, b.hist, b.count, b.cand, b.body, b.out};
    size_t total = 0;
    for (int e = 0; e < 9; ++e) {
        bad += got[e] % 256 != 0 || got[e] < want[e] || got[e] >= want[e] + 256;
        total += got[e];
    }
    bad += total != b.total();
    if (bad)
        std::printf("FAIL n=%lld S=%lld k=%d cu=%d: tail %lld cap %lld passes %d\n", (long long)n,
                    (long long)S, k, n_cu, (long long)p.tail, (long long)p.cap, p.matrix_passes);
    return bad != 0;
}

int main(int argc, char** argv) {
    if (argc == 6 && !std::strcmp(argv[1], "plan")) {
        const int64_t n = std::atoll(argv[2]);
        const LooPlan p = plan_loo(n, std::atoll(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]));
        std::printf("tail=%lld grid=%d cap=%lld select_passes=%d matrix_passes=%d ok=%d splits=%lld "
                    "workspace=%llu\n",
                    (long long)p.tail, p.grid_points, (long long)p.cap, p.select_passes, p.matrix_passes,
                    (int)p.ok,
                    (long long)p.score.splits, (unsigned long long)loo_buffers(p, n).total());
        return 0;
    }
    if (argc == 2 && !std::strcmp(argv[1], "sweep")) {
        const int64_t ns[] = {1, 63, 64, 65, 377, 1000, 10000, 40000};
        const int64_t Ss[] = {2,    24,    25,    26,     63,     64,      65,      127,    128,
                              129,  400,   2000,  4097,   12000,  50000,   400000,  3200000,
                              7454720, 7454721, 30000000};
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
        // every S up to 70 000: the integer tail against the floating-point formula
        for (int64_t S = 2; S <= 70000; ++S) {
            ++plans;
            fails += check(100, S, 3, 256);
        }
        std::printf("sweep %ld %ld\n", plans, fails);
        return fails != 0;
    }
    std::fprintf(stderr, "usage: loo_plan_check plan <n> <S> <k> <n_cu> | sweep\n");
    return 2;
}
