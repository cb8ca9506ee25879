// CPU driver of bmc_cv_plan.h for tests/test_cv_plan.py (g++, no HIP).
//   cv_plan_check check K F label...            -> "ok" or the refusal text of cv_check
//   cv_plan_check segments F label...           -> offsets | counts | src | gram chunks | rss chunks
//   cv_plan_check batches F C K T burn thin budget -> kept bytes | f0-f1:chain0+n,chain0+n;...
//   cv_plan_check sweep                         -> random labels: every row once, stable, padded
//   cv_plan_check widths                        -> "k cv_ldz cv_tiles cv_kmax" per line, k = 1 .. CV_MAX_K
//   cv_plan_check chunks F label...             -> n_pad | gram chunks | rss chunks (segments without src)
#include "../pybmc_amd/csrc/bmc_cv_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace bmc;

static std::vector<int64_t> labels_from(int argc, char** argv, int first) {
    std::vector<int64_t> l;
    for (int i = first; i < argc; ++i) l.push_back(std::atoll(argv[i]));
    return l;
}

static void print_chunks(const CvChunks& c) {
    for (size_t i = 0; i < c.row0.size(); ++i)
        std::printf("%s%lld+%d", i ? "," : "", (long long)c.row0[i], c.rows[i]);
    std::printf("/");
    for (size_t i = 0; i < c.fold_off.size(); ++i) std::printf("%s%d", i ? "," : "", c.fold_off[i]);
}

static int sweep() {
    long cases = 0, bad = 0;
    unsigned long long st = 12345;
    auto rnd = [&](unsigned m) {
        st = st * 6364136223846793005ull + 1442695040888963407ull;
        return (unsigned)((st >> 33) % m);
    };
    for (int rep = 0; rep < 400; ++rep) {
        const int F = 2 + (int)rnd(rep % 7 == 0 ? 1023 : 12);
        const int64_t n = F + (int64_t)rnd(3000);
        std::vector<int64_t> lab(n);
        for (int64_t i = 0; i < n; ++i) lab[i] = i < F ? i : (int64_t)rnd((unsigned)F);
        if (!cv_check(n, 1, F, lab.data()).empty()) { ++bad; continue; }
        const CvSegments s = cv_segments(n, F, lab.data());
        ++cases;
        bool ok = s.n_pad % CV_ROW_PAD == 0 && s.offset[0] == 0 && s.offset[F] == s.n_pad;
        std::vector<char> seen(n, 0);
        for (int f = 0; f < F && ok; ++f) {
            ok = s.offset[f] % CV_ROW_PAD == 0 && s.offset[f + 1] - s.offset[f] >= s.count[f] &&
                 s.offset[f + 1] - s.offset[f] < s.count[f] + CV_ROW_PAD;
            int64_t prev = -1;
            for (int64_t r = s.offset[f]; r < s.offset[f + 1] && ok; ++r) {
                const int64_t i = s.src[r];
                if (r - s.offset[f] < s.count[f])
                    ok = i > prev && i < n && lab[i] == f && !seen[i] && s.row_fold[r] == f;   // stable
                else
                    ok = i == -1 && s.row_fold[r] == f;
                if (ok && i >= 0) { seen[i] = 1; prev = i; }
            }
            // the chunks of a fold tile its rows exactly, in order
            int64_t at = s.offset[f];
            for (int c = s.gram.fold_off[f]; c < s.gram.fold_off[f + 1] && ok; ++c) {
                ok = s.gram.row0[c] == at && s.gram.rows[c] > 0 && s.gram.rows[c] <= CV_GRAM_CHUNK &&
                     s.gram.rows[c] % CV_ROW_PAD == 0;
                at += s.gram.rows[c];
            }
            ok = ok && at == s.offset[f + 1];
            at = s.offset[f];
            for (int c = s.rss.fold_off[f]; c < s.rss.fold_off[f + 1] && ok; ++c) {
                ok = s.rss.row0[c] == at && s.rss.rows[c] > 0 && s.rss.rows[c] <= CV_RSS_CHUNK;
                at += s.rss.rows[c];
            }
            ok = ok && at == s.offset[f] + s.count[f];
        }
        for (int64_t i = 0; i < n && ok; ++i) ok = seen[i];
        if (!ok) ++bad;
    }
    std::printf("sweep %ld %ld\n", cases, bad);
    return bad ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    if (!std::strcmp(argv[1], "sweep")) return sweep();
    if (!std::strcmp(argv[1], "check") && argc >= 4) {
        const int k = std::atoi(argv[2]), F = std::atoi(argv[3]);
        const std::vector<int64_t> l = labels_from(argc, argv, 4);
        const std::string r = cv_check((int64_t)l.size(), k, F, l.data());
        std::printf("%s\n", r.empty() ? "ok" : r.c_str());
        return 0;
    }
    if (!std::strcmp(argv[1], "widths")) {
        for (int k = 1; k <= CV_MAX_K; ++k) std::printf("%d %d %d %d\n", k, cv_ldz(k), cv_tiles(k), cv_kmax(k));
        return 0;
    }
    if (!std::strcmp(argv[1], "chunks") && argc >= 3) {
        const int F = std::atoi(argv[2]);
        const std::vector<int64_t> l = labels_from(argc, argv, 3);
        if (!cv_check((int64_t)l.size(), 1, F, l.data()).empty()) return 3;
        const CvSegments s = cv_segments((int64_t)l.size(), F, l.data());
        std::printf("%lld | ", (long long)s.n_pad);
        print_chunks(s.gram);
        std::printf(" | ");
        print_chunks(s.rss);
        std::printf("\n");
        return 0;
    }
    if (!std::strcmp(argv[1], "segments") && argc >= 3) {
        const int F = std::atoi(argv[2]);
        const std::vector<int64_t> l = labels_from(argc, argv, 3);
        if (!cv_check((int64_t)l.size(), 1, F, l.data()).empty()) return 3;
        const CvSegments s = cv_segments((int64_t)l.size(), F, l.data());
        for (int f = 0; f <= F; ++f) std::printf("%s%lld", f ? "," : "", (long long)s.offset[f]);
        std::printf(" | ");
        for (int f = 0; f < F; ++f) std::printf("%s%lld", f ? "," : "", (long long)s.count[f]);
        std::printf(" | ");
        for (int64_t r = 0; r < s.n_pad; ++r) std::printf("%s%lld", r ? "," : "", (long long)s.src[r]);
        std::printf(" | ");
        print_chunks(s.gram);
        std::printf(" | ");
        print_chunks(s.rss);
        std::printf("\n");
        return 0;
    }
    if (!std::strcmp(argv[1], "batches") && argc == 9) {
        const int F = std::atoi(argv[2]), C = std::atoi(argv[3]), k = std::atoi(argv[4]);
        const int64_t T = std::atoll(argv[5]), burn = std::atoll(argv[6]), thin = std::atoll(argv[7]);
        const size_t budget = (size_t)std::strtoull(argv[8], nullptr, 10);
        const int64_t kept = cv_kept_draws(T, burn, thin);
        std::vector<CvBatch> b;
        const bool ok = plan_cv_batches(F, C, cv_chain_bytes(k, T, kept), budget, b);
        std::printf("%lld %zu |", (long long)kept, cv_chain_bytes(k, T, kept));
        if (!ok) std::printf(" none");
        for (const CvBatch& x : b) {
            std::printf(" %d-%d:", x.f0, x.f1);
            for (size_t i = 0; i < x.launches.size(); ++i)
                std::printf("%s%lld+%d", i ? "," : "", (long long)x.launches[i].chain0, x.launches[i].n_chains);
        }
        std::printf("\n");
        return 0;
    }
    return 2;
}
