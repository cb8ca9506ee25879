// CPU build of the Student-t variate of pybmc_amd/csrc/bmc_math.h (the same text the gfx950 kernels
// compile).  Reads triples of float64 (u1, u2, nu) from the file named first and writes
// bmc::student_t_variate(u1, u2, nu, 2 / nu) to the file named second, both raw little-endian
// float64; 2 / nu is rounded once, as the library's host driver rounds it.
// tests/predict_t_host_build.py drives it; the uniforms come from the host restatement of the
// stream (tests/predict_t_reference.py), so this file holds no generator.
#include "../pybmc_amd/csrc/bmc_math.h"
#include <cstdio>
#include <vector>

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 3;
    std::vector<double> buf(3 * 65536), res(65536);
    size_t got;
    while ((got = std::fread(buf.data(), 24, 65536, in)) > 0) {
        for (size_t i = 0; i < got; ++i) {
            const double nu = buf[3 * i + 2];
            res[i] = bmc::student_t_variate(buf[3 * i], buf[3 * i + 1], nu, 2.0 / nu);
        }
        if (std::fwrite(res.data(), 8, got, out) != got) return 4;
    }
    std::fclose(in);
    return std::fclose(out) == 0 ? 0 : 4;
}
