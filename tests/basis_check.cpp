// CPU driver of bmc_basis.h for tests/test_basis_host.py (g++, no HIP).  Arrays are raw float64
// files in DIR: it reads C0 [k][ldc], b0 [ldc], A [k][k], xty [k], dtot [k] and writes its results
// next to them; the status goes to stdout (ok, c0_singular, not_pd, a_singular).
//   basis_check basis DIR k ldc gram  -> prior_basis on the leading block, then chain_basis:
//                                        P, Li, Pb0, lam, W, c1, c2, bols = solve(A, xty), and
//                                        with gram = 1 G, u0, g0 and Wu0 = W u0
//   basis_check fold DIR k F f        -> prior_basis (ldc = k) and fold_setup of fold f of F: every
//                                        array of the FoldArrays, whole (fa_G, fa_WT, ..., fa_scal)
//   basis_check regular DIR k         -> numerically_regular(A, dtot): regular or deficient
#include "../pybmc_amd/csrc/bmc_basis.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

using namespace bmc;

static std::vector<double> load(const std::string& dir, const char* name, size_t count) {
    std::vector<double> v(count);
    FILE* f = std::fopen((dir + "/" + name + ".f64").c_str(), "rb");
    if (!f || std::fread(v.data(), 8, count, f) != count) {
        std::fprintf(stderr, "cannot read %zu doubles of %s\n", count, name);
        std::exit(4);
    }
    std::fclose(f);
    return v;
}

static void store(const std::string& dir, const char* name, const std::vector<double>& v) {
    FILE* f = std::fopen((dir + "/" + name + ".f64").c_str(), "wb");
    if (!f || std::fwrite(v.data(), 8, v.size(), f) != v.size()) {
        std::fprintf(stderr, "cannot write %s\n", name);
        std::exit(4);
    }
    std::fclose(f);
}

static const char* name_of(BasisStatus st) {
    switch (st) {
        case BASIS_OK: return "ok";
        case BASIS_C0_SINGULAR: return "c0_singular";
        case BASIS_NOT_PD: return "not_pd";
        case BASIS_A_SINGULAR: return "a_singular";
    }
    return "?";
}

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const std::string mode = argv[1], dir = argv[2];
    const int k = std::atoi(argv[3]);
    if (k < 1) return 2;
    if (mode == "regular") {
        const std::vector<double> A = load(dir, "A", (size_t)k * k), dtot = load(dir, "dtot", k);
        std::printf("%s\n", numerically_regular(A.data(), dtot.data(), k) ? "regular" : "deficient");
        return 0;
    }
    if (mode == "basis" && argc == 6) {
        const int ldc = std::atoi(argv[4]);
        const bool gram = std::atoi(argv[5]) != 0;
        if (ldc < k) return 2;
        const std::vector<double> C0 = load(dir, "C0", (size_t)k * ldc), b0 = load(dir, "b0", ldc);
        const std::vector<double> A = load(dir, "A", (size_t)k * k), xty = load(dir, "xty", k);
        PriorBasis pb;
        const BasisStatus st = prior_basis(k, C0.data(), ldc, b0.data(), pb);
        std::printf("%s\n", name_of(st));
        if (st != BASIS_OK) return 0;
        ChainBasis cb;
        chain_basis(k, A, xty, pb, gram, cb);
        if (!gram && !(cb.G.empty() && cb.u0.empty() && cb.g0.empty())) return 5;
        store(dir, "P", pb.P);
        store(dir, "Li", pb.Li);
        store(dir, "Pb0", pb.Pb0);
        store(dir, "lam", cb.lam);
        store(dir, "W", cb.W);
        store(dir, "c1", cb.c1);
        store(dir, "c2", cb.c2);
        std::vector<double> bols;     // the least-squares point, as the callers take it
        if (bmc_la::solve(A, xty, k, bols)) store(dir, "bols", bols);
        if (gram) {
            store(dir, "G", cb.G);
            store(dir, "u0", cb.u0);
            store(dir, "g0", cb.g0);
            std::vector<double> Wu0(k);   // each entry one in-order extended-precision sum, rounded once
            for (int i = 0; i < k; ++i) {
                long double s = 0.0L;
                for (int j = 0; j < k; ++j) s += (long double)cb.W[(size_t)i * k + j] * cb.u0[j];
                Wu0[i] = (double)s;
            }
            store(dir, "Wu0", Wu0);
        }
        return 0;
    }
    if (mode == "fold" && argc == 6) {
        const int F = std::atoi(argv[4]), f = std::atoi(argv[5]);
        if (F < 1 || f < 0 || f >= F) return 2;
        const std::vector<double> C0 = load(dir, "C0", (size_t)k * k), b0 = load(dir, "b0", k);
        const std::vector<double> A = load(dir, "A", (size_t)k * k), xty = load(dir, "xty", k);
        const std::vector<double> dtot = load(dir, "dtot", k);
        PriorBasis pb;
        BasisStatus st = prior_basis(k, C0.data(), k, b0.data(), pb);
        FoldArrays fa(F, k);
        if (st == BASIS_OK) st = fold_setup(k, F, f, A, xty, dtot.data(), pb, fa);
        std::printf("%s\n", name_of(st));
        if (st != BASIS_OK) return 0;
        store(dir, "fa_G", fa.G);
        store(dir, "fa_WT", fa.WT);
        store(dir, "fa_lam", fa.lam);
        store(dir, "fa_c1", fa.c1);
        store(dir, "fa_c2", fa.c2);
        store(dir, "fa_u0", fa.u0);
        store(dir, "fa_g0", fa.g0);
        store(dir, "fa_beta", fa.beta);
        store(dir, "fa_scal", fa.scal);
        return 0;
    }
    return 2;
}
