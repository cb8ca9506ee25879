// CPU check of moment_plan and acov_plan (pybmc_amd/csrc/bmc_diag_plan.h), the launch plans of the
// chain-diagnostics kernels.
//   plan <C> <T> <burn> <P> <n_active> <n_lags>
//          "acov ncc nlc MG spg S rps groups bytes" and "moments n_seq ncc S rps bytes" of the shape
//   sweep  C in 1..300, a grid of n in 4..3000 and of n_active in 1..4200, the lag blocks diag_run
//          asks for (64, 128, 256, ... clipped at n) and a few free lag counts: the invariants the
//          kernels rely on; prints "sweep <plans> <failures>"
#include "../pybmc_amd/csrc/bmc_diag_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace bmc;

static long g_fail = 0;
static void fail(const char* what, int32_t C, int64_t n, int32_t a, int64_t nl) {
    if (g_fail++ < 20)
        std::printf("FAIL %s C=%d n=%lld n_active=%d n_lags=%lld\n", what, C, (long long)n, a, (long long)nl);
}

static void check_acov(int32_t C, int64_t n, int32_t na, int64_t nl) {
    const AcovPlan p = acov_plan(C, n, na, nl);
    const int64_t M = 2 * (int64_t)C;
    // every active column in one column group, every lag in one lag chunk
    if ((int64_t)p.ncc * DIAG_CW < na || (int64_t)(p.ncc - 1) * DIAG_CW >= na) fail("ncc", C, n, na, nl);
    if ((int64_t)p.nlc * DIAG_LC < nl || (int64_t)(p.nlc - 1) * DIAG_LC >= nl) fail("nlc", C, n, na, nl);
    // the tile loop steps by DIAG_R from a split's first row
    if (p.rps < DIAG_R || p.rps % DIAG_R) fail("rps", C, n, na, nl);
    // the splits [s rps, min((s + 1) rps, n)) tile [0, n) once, none empty
    if (p.S < 1 || (int64_t)p.S * p.rps < n || (int64_t)(p.S - 1) * p.rps >= n) fail("S", C, n, na, nl);
    int64_t rows = 0;
    for (int32_t s = 0; s < p.S; ++s) {
        const int64_t lo = (int64_t)s * p.rps, hi = lo + p.rps < n ? lo + p.rps : n;
        if (hi <= lo || lo != rows) fail("split", C, n, na, nl);
        rows = hi;
    }
    if (rows != n) fail("rows", C, n, na, nl);
    // the groups [g spg, min((g + 1) spg, 2C)) cover the 2C halves once, none empty
    if (p.spg < 1 || p.MG < 1 || (int64_t)(p.MG - 1) * p.spg >= M || M > (int64_t)p.MG * p.spg)
        fail("groups", C, n, na, nl);
    // one [16][64] f64 slab of partials per workgroup, and a grid that fits blockIdx.x
    const int64_t groups = (int64_t)p.MG * p.ncc * p.nlc * p.S;
    if (acov_groups(p) != groups || groups > 2147483647LL) fail("grid", C, n, na, nl);
    if (acov_scratch_bytes(p) != (size_t)groups * 16 * 64 * 8) fail("bytes", C, n, na, nl);
}

static void check_moments(int32_t n_seq, int32_t P, int64_t n) {
    const MomentPlan p = moment_plan(n_seq, P, n);
    if ((int64_t)p.ncc * 64 < P || (int64_t)(p.ncc - 1) * 64 >= P) fail("m.ncc", n_seq, n, P, 0);
    if (p.S < 1 || p.rps < 1 || (int64_t)p.S * p.rps < n || (int64_t)(p.S - 1) * p.rps >= n)
        fail("m.S", n_seq, n, P, 0);
    int64_t rows = 0;
    for (int32_t s = 0; s < p.S; ++s) {
        const int64_t lo = (int64_t)s * p.rps, hi = lo + p.rps < n ? lo + p.rps : n;
        if (hi <= lo || lo != rows) fail("m.split", n_seq, n, P, 0);
        rows = hi;
    }
    if (rows != n) fail("m.rows", n_seq, n, P, 0);
    // no more splits than started blocks of 256 rows: S = 1, or 256 (S - 1) < n, so that every
    // split but the last holds rps = ceil(n / S) > 128 rows (n = 257 gives 129 + 128)
    if (p.S > 1 && ((int64_t)256 * (p.S - 1) >= n || p.rps <= 128)) fail("m.256", n_seq, n, P, 0);
    if (moment_scratch_bytes(p, n_seq, P) != (size_t)n_seq * p.S * 2 * P * 8) fail("m.bytes", n_seq, n, P, 0);
    // a middle draw (length 1) lies in split 0 alone: rps >= 1 was checked above
}

int main(int argc, char** argv) {
    if (argc == 8 && !std::strcmp(argv[1], "plan")) {
        const int32_t C = std::atoi(argv[2]), P = std::atoi(argv[5]), na = std::atoi(argv[6]);
        const int64_t T = std::atoll(argv[3]), burn = std::atoll(argv[4]), nl = std::atoll(argv[7]);
        const int64_t Tp = T - burn, n = Tp / 2;
        const int32_t n_seq = 2 * C + (Tp & 1 ? C : 0);
        const AcovPlan a = acov_plan(C, n, na, nl);
        const MomentPlan m = moment_plan(n_seq, P, n);
        std::printf("acov %d %d %d %d %d %lld %lld %zu\n", a.ncc, a.nlc, a.MG, a.spg, a.S, (long long)a.rps,
                    (long long)acov_groups(a), acov_scratch_bytes(a));
        std::printf("moments %d %d %d %lld %zu\n", n_seq, m.ncc, m.S, (long long)m.rps,
                    moment_scratch_bytes(m, n_seq, P));
        return 0;
    }
    if (argc == 2 && !std::strcmp(argv[1], "sweep")) {
        std::vector<int64_t> ns;
        for (int64_t n = 4; n <= 3000; n += (n < 140 ? 1 : n < 600 ? 7 : 61)) ns.push_back(n);
        for (int64_t k = 128; k <= 3000; k += 128)
            for (int64_t e = -1; e <= 1; ++e)
                if (k + e <= 3000) ns.push_back(k + e);
        ns.push_back(3000);
        std::vector<int32_t> nas;
        for (int32_t a = 1; a <= 4200; a += (a < 70 ? 1 : a < 400 ? 13 : 211)) nas.push_back(a);
        for (int32_t a : {512, 1024, 2047, 2048, 2049, 4095, 4096, 4097, 4200}) nas.push_back(a);
        long plans = 0;
        for (int32_t C = 1; C <= 300; ++C)
            for (int64_t n : ns) {
                for (int32_t na : nas) {
                    // the blocks of diag_run: 64 lags first, then doubling, clipped at n
                    for (int64_t t0 = 0, L = 64; t0 < n; L *= 2) {
                        const int64_t nl = L < n - t0 ? L : n - t0;
                        check_acov(C, n, na, nl);
                        ++plans;
                        t0 += nl;
                    }
                    if (C % 7 == 1)
                        for (int64_t nl : {1, 63, 65, 512, 131072}) {   // bmc_chain_autocov's free choice
                            check_acov(C, n, na, nl);
                            ++plans;
                        }
                }
                for (int32_t P : {1, 2, 63, 64, 65, 130, 336, 4096, 4200})
                    for (int32_t n_seq : {2 * C, 3 * C}) {
                        check_moments(n_seq, P, n);
                        ++plans;
                    }
            }
        std::printf("sweep %ld %ld\n", plans, g_fail);
        return g_fail != 0;
    }
    std::fprintf(stderr, "usage: diag_plan_check plan <C> <T> <burn> <P> <n_active> <n_lags> | sweep\n");
    return 2;
}
