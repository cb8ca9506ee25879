// CPU check of plan_ppc (pybmc_amd/csrc/bmc_plan.h), the plan of the posterior predictive check.
//   plan <n_points> <n_draws> <k> <n_cu>   the plan's fields and buffer bytes as key=value
//   sweep                                  a grid of shapes x CU counts: whole tiles that cover the
//                                          operands and no more, one workgroup per draw tile, the
//                                          buffers as large as the kernels index them, refusals
//                                          exactly outside the documented range, nothing but
//                                          `rounds` depending on the CU count;
//                                          prints "sweep <plans> <failures>" last
#include "../pybmc_amd/csrc/bmc_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace bmc;

static bool should_refuse(int64_t n, int64_t S, int k) {
    return n < 3 || n > ((int64_t)1 << 31) || S < 2 || k < 1 || k > 256;
}

static int check(int64_t n, int64_t S, int k, int n_cu) {
    const PpcPlan p = plan_ppc(n, S, k, n_cu);
    int bad = 0;
    if (should_refuse(n, S, k)) {
        bad += p.ok;
    } else {
        bad += !p.ok;
        bad += p.n_pad != p.point_tiles * 64 || p.n_pad < n || p.n_pad - n >= 64;
        bad += p.S_pad != p.draw_tiles * 64 || p.S_pad < S || p.S_pad - S >= 64;
        bad += p.k_pad < k || p.k_pad % 16 != 0 || p.k_pad - k >= 16;
        bad += p.grid != p.draw_tiles;   // no split over the points
        const int64_t slots = 2 * (int64_t)(n_cu > 0 ? n_cu : 1);
        bad += p.rounds < 1 || p.rounds * slots < p.grid || (p.rounds - 1) * slots >= p.grid;
        const PpcBuffers b = ppc_buffers(p, S);
        bad += b.Ap != (size_t)p.n_pad * p.k_pad * 8 || b.yo != (size_t)p.n_pad * 16;
        bad += b.Tp != (size_t)p.S_pad * p.k_pad * 8 || b.sg != ((size_t)p.S_pad * 3 + p.k_pad + 16) * 8;   // sigma, 1 / sigma, centre; column means
        bad += b.out != (size_t)S * (PPC_STATS + PPC_OBS) * 8;
        bad += b.total() != b.Ap + b.yo + b.Tp + b.sg + b.out;
        // the bits may not depend on the device: everything but `rounds` is the 1-CU plan
        const PpcPlan q = plan_ppc(n, S, k, 1);
        bad += q.point_tiles != p.point_tiles || q.draw_tiles != p.draw_tiles || q.n_pad != p.n_pad ||
               q.S_pad != p.S_pad || q.k_pad != p.k_pad || q.grid != p.grid;
    }
    if (bad)
        std::printf("FAIL n=%lld S=%lld k=%d cu=%d\n", (long long)n, (long long)S, k, n_cu);
    return bad != 0;
}

int main(int argc, char** argv) {
    if (argc == 6 && !std::strcmp(argv[1], "plan")) {
        const int64_t n = std::atoll(argv[2]), S = std::atoll(argv[3]);
        const PpcPlan p = plan_ppc(n, S, std::atoi(argv[4]), std::atoi(argv[5]));
        const PpcBuffers b = p.ok ? ppc_buffers(p, S) : PpcBuffers{};
        std::printf("ok=%d point_tiles=%lld draw_tiles=%lld n_pad=%lld S_pad=%lld k_pad=%d grid=%lld "
                    "rounds=%lld bytes_Ap=%zu bytes_yo=%zu bytes_Tp=%zu bytes_sg=%zu bytes_out=%zu "
                    "bytes_total=%zu\n",
                    (int)p.ok, (long long)p.point_tiles, (long long)p.draw_tiles, (long long)p.n_pad,
                    (long long)p.S_pad, p.k_pad, (long long)p.grid, (long long)p.rounds, b.Ap, b.yo, b.Tp,
                    b.sg, b.out, p.ok ? b.total() : (size_t)0);
        return 0;
    }
    if (argc == 2 && !std::strcmp(argv[1], "sweep")) {
        const int64_t ns[] = {0, 1, 2, 3, 4, 63, 64, 65, 629, 10000, 1000000, ((int64_t)1 << 31),
                              ((int64_t)1 << 31) + 1};
        const int64_t Ss[] = {0, 1, 2, 63, 64, 65, 255, 256, 257, 50000, 400000, 3200000};
        const int ks[] = {0, 1, 3, 15, 16, 17, 32, 33, 256, 257};
        const int cus[] = {0, 1, 8, 64, 256, 304};
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
    std::fprintf(stderr, "usage: ppc_plan_check plan <n> <S> <k> <n_cu> | sweep\n");
    return 2;
}
