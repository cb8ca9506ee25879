// Host driver of pybmc_amd/csrc/bmc_robust_plan.h for tests/test_robust_plan.py (plain g++, no HIP).
//   slabs N k              "rows_per_wave rows_padded tiles pairs kc ldz | r0-r1 r0-r1 r0-r1 r0-r1"
//   launches n_chains      "max_per_launch | c0+n c0+n ..."
//   bytes N k C sweeps     "workspace packed gl"
//   check N k f32 nu C iters burn      "ok" or the reason
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../pybmc_amd/csrc/bmc_robust_plan.h"

using namespace bmc;

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string cmd = argv[1];
    if (cmd == "slabs" && argc == 4) {
        const int64_t n = std::atoll(argv[2]);
        const int k = std::atoi(argv[3]);
        std::printf("%lld %lld %d %d %d %d |", (long long)robust_rows_per_wave(n),
                    (long long)robust_rows_padded(n), robust_tiles(k), robust_tile_pairs(k), robust_kc(k),
                    robust_ldz(k));
        for (int w = 0; w < ROBUST_WAVES; ++w) {
            const RobustSlab s = robust_slab(n, w);
            std::printf(" %lld-%lld", (long long)s.row0, (long long)s.row1);
        }
        std::printf("\n");
        return 0;
    }
    if (cmd == "launches" && argc == 3) {
        std::printf("%d |", ROBUST_MAX_CHAINS_PER_LAUNCH);
        for (const RobustLaunch& l : robust_launches(std::atoi(argv[2]))) std::printf(" %d+%d", l.c0, l.n_chains);
        std::printf("\n");
        return 0;
    }
    if (cmd == "bytes" && argc == 6) {
        const int64_t n = std::atoll(argv[2]);
        const int k = std::atoi(argv[3]), C = std::atoi(argv[4]);
        std::printf("%zu %zu %zu\n", robust_workspace_bytes(n, C), robust_packed_bytes(n, k),
                    robust_gl_bytes(n, C, std::atoll(argv[5])));
        return 0;
    }
    if (cmd == "check" && argc == 9) {
        const std::string why = robust_check(std::atoll(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]),
                                             std::atof(argv[5]), std::atoi(argv[6]), std::atoll(argv[7]),
                                             std::atoll(argv[8]));
        std::printf("%s\n", why.empty() ? "ok" : why.c_str());
        return 0;
    }
    return 2;
}
