// CPU check of plan_rank (pybmc_amd/csrc/bmc_rank_plan.h), the plan of the rank-normalised diagnostics.
//   plan <C> <iters> <P> <ld> <burn> <n_probs> <cols_per_batch> <budget>
//          the plan's fields as key=value (probabilities 0.5 each; n_probs = 17 makes too many,
//          n_probs = -1 one probability of 1.5)
//   sweep  a grid of shapes x batch requests x budgets: the batches cover every column once, the
//          tiles cover S and no more, the scratch sizes grow with the batch, cols_per_batch is
//          honoured, refusals exactly outside the documented limits; prints "sweep <plans> <failures>"
//   passes <or> <and> [<or> <and> ...]   hex masks per segment -> the live-pass bit mask
//   orderstat <S> <p as hex float>       index and weight (hex float) of the quantile
#include "../pybmc_amd/csrc/bmc_rank_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace bmc;

static bool should_refuse(int64_t C, int64_t iters, int64_t P, int64_t ld, int64_t burn, int n_probs) {
    if (C < 1 || C > 65536 || P < 1 || P > 65536 || ld < P || burn < 0) return true;
    const int64_t n = (iters - burn) / 2;
    if (iters - burn < 8 || n < 4) return true;
    if (2 * C * n > 2147483647LL) return true;
    return n_probs < 0 || n_probs > 16;
}

static int check(int32_t C, int64_t iters, int32_t P, int64_t burn, int n_probs, int32_t cpb, size_t budget) {
    std::vector<double> probs(n_probs > 0 ? n_probs : 1, 0.5);
    const RankPlan p = plan_rank(C, iters, P, P, burn, probs.data(), n_probs, cpb, budget);
    int bad = 0;
    if (should_refuse(C, iters, P, P, burn, n_probs)) {
        bad += p.ok || p.why.empty();
    } else if (!p.ok) {
        // the one allowed refusal of valid arguments: auto batching and not even one column fits
        RankPlan one;
        one.S = 2 * (int64_t)C * ((iters - burn) / 2);
        one.tiles = (one.S + RANK_TILE - 1) / RANK_TILE;
        rank_scratch(one, 1);
        bad += cpb != 0 || one.bytes_total <= budget;
    } else {
        bad += p.n != (iters - burn) / 2 || p.S != 2 * (int64_t)C * p.n;
        bad += p.tiles * RANK_TILE < p.S || (p.tiles - 1) * RANK_TILE >= p.S;
        bad += p.cols_per_batch < 1 || p.cols_per_batch > P;
        if (cpb > 0) bad += p.cols_per_batch != (cpb < P ? cpb : P) && p.tiles * RANK_ITEMS * cpb <= RANK_MAX_BLOCKS;
        if (cpb == 0) bad += p.bytes_total > budget;
        bad += p.tiles * RANK_ITEMS * p.cols_per_batch > RANK_MAX_BLOCKS;
        // every column in exactly one batch, in order
        int32_t next = 0;
        for (int32_t b = 0; b < p.n_batches; ++b) {
            int32_t c0, nc;
            rank_batch(p, P, b, &c0, &nc);
            bad += c0 != next || nc < 1 || nc > p.cols_per_batch;
            next = c0 + nc;
        }
        bad += next != P;
        // sizes: as large as the kernels index them, and monotone in the batch
        bad += p.bytes_keys != (size_t)p.cols_per_batch * p.S * 8 || p.bytes_idx != (size_t)p.cols_per_batch * p.S * 4;
        bad += p.bytes_hist != (size_t)p.cols_per_batch * p.tiles * 256 * 4;
        bad += p.bytes_derived != (size_t)p.S * 4 * p.cols_per_batch * 8;
        bad += p.bytes_total != 2 * p.bytes_keys + 2 * p.bytes_idx + p.bytes_hist + p.bytes_derived + p.bytes_small;
        RankPlan a = p, b = p;
        for (int64_t pb = 1; pb < 6; ++pb) {
            rank_scratch(a, pb);
            rank_scratch(b, pb + 1);
            bad += b.bytes_keys <= a.bytes_keys || b.bytes_idx <= a.bytes_idx || b.bytes_hist <= a.bytes_hist ||
                   b.bytes_derived <= a.bytes_derived || b.bytes_small <= a.bytes_small ||
                   b.bytes_total <= a.bytes_total;
        }
    }
    if (bad)
        std::printf("FAIL C=%d iters=%lld P=%d burn=%lld n_probs=%d cpb=%d budget=%zu\n", C, (long long)iters, P,
                    (long long)burn, n_probs, cpb, budget);
    return bad != 0;
}

int main(int argc, char** argv) {
    if (argc == 10 && !std::strcmp(argv[1], "plan")) {
        int n_probs = std::atoi(argv[7]);
        std::vector<double> probs(17, 0.5);
        if (n_probs == -1) probs[0] = 1.5, n_probs = 1;
        const RankPlan p = plan_rank(std::atoi(argv[2]), std::atoll(argv[3]), std::atoi(argv[4]),
                                     std::atoll(argv[5]), std::atoll(argv[6]), probs.data(), n_probs,
                                     std::atoi(argv[8]), (size_t)std::strtoull(argv[9], nullptr, 10));
        std::printf("ok=%d n=%lld S=%lld tiles=%lld tile=%d passes=%d cols_per_batch=%d n_batches=%d bytes_keys=%zu "
                    "bytes_idx=%zu bytes_hist=%zu bytes_derived=%zu bytes_small=%zu bytes_total=%zu\n",
                    (int)p.ok, (long long)p.n, (long long)p.S, (long long)p.tiles, RANK_TILE, p.passes,
                    p.cols_per_batch, p.n_batches, p.bytes_keys, p.bytes_idx, p.bytes_hist, p.bytes_derived,
                    p.bytes_small, p.bytes_total);
        if (!p.ok) std::printf("why=%s\n", p.why.c_str());
        return 0;
    }
    if (argc == 2 && !std::strcmp(argv[1], "sweep")) {
        const int32_t Cs[] = {0, 1, 2, 64, 65536, 65537};
        const int64_t its[] = {7, 8, 9, 2047, 2048, 2049, 4097, 50000, 32768, 32770};
        const int32_t Ps[] = {0, 1, 5, 33, 65536, 65537};
        const int64_t burns[] = {-1, 0, 1, 100};
        const int nps[] = {0, 1, 3, 16, 17};
        const int32_t cpbs[] = {0, 1, 2, 7, 100000};
        const size_t budgets[] = {(size_t)1 << 20, (size_t)1 << 30, (size_t)200 << 30};
        long plans = 0, fails = 0;
        for (int32_t C : Cs)
            for (int64_t it : its)
                for (int32_t P : Ps)
                    for (int64_t burn : burns)
                        for (int np : nps)
                            for (int32_t cpb : cpbs)
                                for (size_t budget : budgets) {
                                    ++plans;
                                    fails += check(C, it, P, burn, np, cpb, budget);
                                }
        std::printf("sweep %ld %ld\n", plans, fails);
        return fails != 0;
    }
    if (argc >= 4 && argc % 2 == 0 && !std::strcmp(argv[1], "passes")) {
        std::vector<uint64_t> oa;
        for (int i = 2; i < argc; ++i) oa.push_back(std::strtoull(argv[i], nullptr, 16));
        std::printf("%u\n", rank_live_passes(oa.data(), (int32_t)(oa.size() / 2)));
        return 0;
    }
    if (argc == 4 && !std::strcmp(argv[1], "orderstat")) {
        int32_t index;
        double weight;
        rank_order_stat(std::atoll(argv[2]), std::strtod(argv[3], nullptr), &index, &weight);
        std::printf("%d %a\n", index, weight);
        return 0;
    }
    std::fprintf(stderr, "usage: rank_plan_check plan ... | sweep | passes ... | orderstat <S> <p>\n");
    return 2;
}
