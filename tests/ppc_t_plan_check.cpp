// CPU check that the room for the Student-t predictive check's nu rows (ppc_nu_bytes of
// pybmc_amd/csrc/bmc_plan.h) stands beside plan_ppc and ppc_buffers without changing them:
//   <n_points> <n_draws> <k> <n_cu>   the plan's fields and buffer bytes of tests/ppc_plan_check.cpp,
//                                     then bytes_nu and max_nu_values, as key=value
#include "../pybmc_amd/csrc/bmc_plan.h"

#include <cstdio>
#include <cstdlib>

using namespace bmc;

int main(int argc, char** argv) {
    if (argc != 5) return 2;
    const int64_t n = std::atoll(argv[1]), S = std::atoll(argv[2]);
    const PpcPlan p = plan_ppc(n, S, std::atoi(argv[3]), std::atoi(argv[4]));
    const PpcBuffers b = p.ok ? ppc_buffers(p, S) : PpcBuffers{};
    std::printf("ok=%d point_tiles=%lld draw_tiles=%lld n_pad=%lld S_pad=%lld k_pad=%d grid=%lld "
                "rounds=%lld bytes_Ap=%zu bytes_yo=%zu bytes_Tp=%zu bytes_sg=%zu bytes_out=%zu "
                "bytes_total=%zu bytes_nu=%zu max_nu_values=%d\n",
                (int)p.ok, (long long)p.point_tiles, (long long)p.draw_tiles, (long long)p.n_pad,
                (long long)p.S_pad, p.k_pad, (long long)p.grid, (long long)p.rounds, b.Ap, b.yo, b.Tp, b.sg,
                b.out, p.ok ? b.total() : (size_t)0, p.ok ? ppc_nu_bytes(p) : (size_t)0,
                (int)PPC_MAX_NU_VALUES);
    return 0;
}
