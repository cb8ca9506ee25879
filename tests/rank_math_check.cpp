// CPU check of ndtri and rank_key (pybmc_amd/csrc/bmc_math.h), the text the gfx950 kernels compile.
// Doubles are read from stdin as C hex floats, one per token:
//   ndtri   prints ndtri(p) per input, as a hex float
//   keys    prints "<key as 16 hex digits> <rank_unkey(key) as a hex float>" per input
#include "../pybmc_amd/csrc/bmc_math.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

int main(int argc, char** argv) {
    if (argc != 2 || (std::strcmp(argv[1], "ndtri") && std::strcmp(argv[1], "keys"))) {
        std::fprintf(stderr, "usage: rank_math_check ndtri|keys < hex floats\n");
        return 2;
    }
    const bool keys = !std::strcmp(argv[1], "keys");
    char tok[128];
    while (std::scanf("%127s", tok) == 1) {
        const double x = std::strtod(tok, nullptr);
        if (keys) {
            const uint64_t k = bmc::rank_key(x);
            std::printf("%016llx %a\n", (unsigned long long)k, bmc::rank_unkey(k));
        } else {
            std::printf("%a\n", bmc::ndtri(x));
        }
    }
    return 0;
}
