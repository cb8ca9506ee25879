// CPU driver of bmc_cvpath_plan.h for tests/test_cvpath_plan.py (g++, no HIP).
//   cvpath_plan_check check K comp...                       -> "ok" or the refusal text of cvpath_check
//   cvpath_plan_check plan F C T burn thin budget comp...   -> kept | bytes per candidate | batches
//       a batch: p0-p1/bytes:kmax@chain0+n,...   ("none p need": problem p needs `need` bytes)
//   cvpath_plan_check verify F C T burn thin budget comp... -> "ok ..." after checking every invariant
//   cvpath_plan_check sweep                                 -> random plans through verify
#include "../pybmc_amd/csrc/bmc_cvpath_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace bmc;

// "" when the plan of these arguments holds every invariant, else what is wrong
static std::string verify(int F, int C, const std::vector<int32_t>& comps, int64_t T, int64_t kept,
                          size_t budget, const std::vector<CvPathBatch>& batches) {
    const int m = (int)comps.size(), P = m * F;
    std::vector<int> seen((size_t)P * C, 0);
    std::vector<int64_t> mat, vec;
    cvpath_setup_offsets(F, comps.data(), m, mat, vec);
    int next_p = 0;
    for (const CvPathBatch& b : batches) {
        if (b.p0 != next_p || b.p1 <= b.p0 || b.p1 > P) return "batches do not tile the problems in order";
        next_p = b.p1;
        const int np = b.p1 - b.p0;
        if ((int)b.desc.size() != np) return "descriptor count";
        size_t bytes = 0;
        int64_t xi = 0, gam = 0, u = 0, d = 0;
        for (int q = 0; q < np; ++q) {
            const CvPathDesc& e = b.desc[q];
            const int p = b.p0 + q;
            if (e.cand != p / F || e.fold != p % F || e.k != comps[e.cand]) return "descriptor order";
            if (e.g_off != mat[e.cand] + (int64_t)e.fold * e.k * e.k || e.v_off != vec[e.cand] + (int64_t)e.fold * e.k ||
                e.s_off != (int64_t)p * 4)
                return "set-up offsets";
            if (e.g_off + (int64_t)e.k * e.k > mat[m] || e.v_off + e.k > vec[m]) return "set-up offset out of range";
            // the chain buffers are packed problem after problem, nothing overlapping
            if (e.xi_off != xi || e.gam_off != gam || e.u_off != u || e.d_off != d) return "chain offsets";
            xi += (int64_t)C * T * e.k;
            gam += (int64_t)C * T;
            u += (int64_t)C * T * (e.k + 1);
            d += (int64_t)C * kept * (e.k + 1);
            const size_t pb = cvpath_problem_bytes(e.k, C, T, kept);
            if (pb != cv_chain_bytes(e.k, T, kept) * (size_t)C) return "bytes per problem";
            bytes += pb;
        }
        if (xi != b.xi_len || gam != b.gam_len || u != b.u_len || d != b.d_len) return "buffer lengths";
        if ((size_t)(xi + gam + u + d) * 8 != bytes || bytes != b.bytes) return "batch bytes";
        if (bytes > budget) return "a batch exceeds the budget";
        // (greedy: the next problem would not have fitted)
        if (b.p1 < P && bytes + cvpath_problem_bytes(comps[b.p1 / F], C, T, kept) <= budget)
            return "a batch stops although the next problem fits";
        int last_kmax = 128;
        for (const CvPathLaunch& l : b.launches) {
            if (l.n_chains < 1 || l.n_chains > CV_MAX_CHAINS_PER_LAUNCH) return "launch size";
            if (l.kmax > last_kmax) return "launches are not widest first";
            last_kmax = l.kmax;
            if (l.chain0 < 0 || l.chain0 + l.n_chains > (int64_t)np * C) return "launch outside the batch";
            for (int64_t c = l.chain0; c < l.chain0 + l.n_chains; ++c) {
                const CvPathDesc& e = b.desc[c / C];
                if (cv_kmax(e.k) != l.kmax) return "a launch mixes width classes";
                ++seen[(size_t)(b.p0 + c / C) * C + c % C];
            }
        }
    }
    if (next_p != P) return "problems left out";
    for (int v : seen)
        if (v != 1) return "a chain is launched " + std::to_string(v) + " times";
    return "";
}

static int sweep() {
    long cases = 0, bad = 0, refused = 0;
    unsigned long long st = 2024;
    auto rnd = [&](unsigned mod) {
        st = st * 6364136223846793005ull + 1442695040888963407ull;
        return (unsigned)((st >> 33) % mod);
    };
    for (int rep = 0; rep < 600; ++rep) {
        const int kmax = 1 + (int)rnd(64);
        std::vector<int32_t> comps;
        for (int k = 1; k <= kmax; ++k)
            if (rnd(3) || k == kmax) comps.push_back(k);
        const int F = 2 + (int)rnd(rep % 5 == 0 ? 60 : 6), C = 1 + (int)rnd(rep % 7 == 0 ? 300 : 5);
        const int64_t T = 1 + rnd(50), burn = rnd((unsigned)T), thin = 1 + rnd(3);
        const int64_t kept = cv_kept_draws(T, burn, thin);
        const size_t widest = cvpath_problem_bytes(kmax, C, T, kept);
        const size_t budget = rnd(4) == 0 ? (size_t)1 << 60 : widest / 2 + (size_t)((double)rnd(1u << 20) / (double)(1u << 20) * 3.0 * (double)widest);
        std::vector<CvPathBatch> b;
        int32_t too_big = -1;
        size_t need = 0;
        const bool ok = plan_cvpath(F, C, comps.data(), (int)comps.size(), T, kept, budget, b, &too_big, &need);
        ++cases;
        if (!ok) {
            ++refused;
            // refused exactly when some problem does not fit, and that problem is reported
            if (widest <= budget || !b.empty() || too_big < 0 || need <= budget ||
                need != cvpath_problem_bytes(comps[too_big / F], C, T, kept))
                ++bad;
            continue;
        }
        if (widest > budget || !verify(F, C, comps, T, kept, budget, b).empty()) ++bad;
    }
    std::printf("sweep %ld %ld %ld\n", cases, bad, refused);
    return bad ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    if (!std::strcmp(argv[1], "sweep")) return sweep();
    if (!std::strcmp(argv[1], "check") && argc >= 3) {
        std::vector<int32_t> comps;
        for (int i = 3; i < argc; ++i) comps.push_back(std::atoi(argv[i]));
        const std::string r = cvpath_check(std::atoi(argv[2]), comps.data(), (int32_t)comps.size());
        std::printf("%s\n", r.empty() ? "ok" : r.c_str());
        return 0;
    }
    if ((!std::strcmp(argv[1], "plan") || !std::strcmp(argv[1], "verify")) && argc >= 9) {
        const int F = std::atoi(argv[2]), C = std::atoi(argv[3]);
        const int64_t T = std::atoll(argv[4]), burn = std::atoll(argv[5]), thin = std::atoll(argv[6]);
        const size_t budget = (size_t)std::strtoull(argv[7], nullptr, 10);
        std::vector<int32_t> comps;
        for (int i = 8; i < argc; ++i) comps.push_back(std::atoi(argv[i]));
        const int m = (int)comps.size();
        if (!cvpath_check(comps.back(), comps.data(), m).empty()) return 3;
        const int64_t kept = cv_kept_draws(T, burn, thin);
        std::vector<CvPathBatch> b;
        int32_t too_big = -1;
        size_t need = 0;
        const bool ok = plan_cvpath(F, C, comps.data(), m, T, kept, budget, b, &too_big, &need);
        if (!std::strcmp(argv[1], "verify")) {
            if (!ok) {
                std::printf("refused %d %zu\n", too_big, need);
                return 0;
            }
            const std::string r = verify(F, C, comps, T, kept, budget, b);
            std::printf("%s %zu\n", r.empty() ? "ok" : r.c_str(), b.size());
            return r.empty() ? 0 : 1;
        }
        std::printf("%lld |", (long long)kept);
        for (int j = 0; j < m; ++j) std::printf(" %zu", cvpath_problem_bytes(comps[j], C, T, kept));
        std::printf(" |");
        if (!ok) std::printf(" none %d %zu", too_big, need);
        for (const CvPathBatch& x : b) {
            std::printf(" %d-%d/%zu:", x.p0, x.p1, x.bytes);
            for (size_t i = 0; i < x.launches.size(); ++i)
                std::printf("%s%d@%lld+%d", i ? "," : "", x.launches[i].kmax, (long long)x.launches[i].chain0,
                            x.launches[i].n_chains);
        }
        std::printf("\n");
        return 0;
    }
    return 2;
}
