// CPU build of the Box-Muller transform of pybmc_amd/csrc/bmc_math.h (the same text the gfx950
// kernels compile).  Reads pairs of float64 uniforms (u1, u2) from the file named first and
// writes the pairs (z0, z1) of bmc::box_muller_pair to the file named second, both raw
// little-endian float64.  tests/rng_host_build.py drives it; the uniforms come from the host
// restatement of the streams (tests/rng_reference.py), so this file holds no generator.
#include "../pybmc_amd/csrc/bmc_math.h"
#include <cstdio>
#include <vector>

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 3;
    std::vector<double> buf(2 * 65536);
    size_t got;
    while ((got = std::fread(buf.data(), 16, 65536, in)) > 0) {
        for (size_t i = 0; i < got; ++i) {
            double z0, z1;
            bmc::box_muller_pair(buf[2 * i], buf[2 * i + 1], z0, z1);
            buf[2 * i] = z0;
            buf[2 * i + 1] = z1;
        }
        if (std::fwrite(buf.data(), 16, got, out) != got) return 4;
    }
    std::fclose(in);
    return std::fclose(out) == 0 ? 0 : 4;
}
