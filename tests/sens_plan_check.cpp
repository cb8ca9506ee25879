// CPU check of the plan of the power-scaling sensitivity (pybmc_amd/csrc/bmc_sens_plan.h).
//   const   the geometry constants as key=value (what the GPU tests size their cases from)
//   tail <S>            tail length M and grid points of the fit
//   tails               binary int64 S values on stdin -> three int32 per S on stdout: psis_tail_length(S),
//                       psis_grid_points of it, plan_loo(...).tail (the rule of bmc_psis_plan.h as both
//                       plans see it; tests/test_sens_plan.py holds them to integer arithmetic of its own)
//   plan <S> <n_cols> <W> <cols_per_batch> <budget>   the plan's fields as key=value
//   sweep   S = 1 .. a few thousand and the limits x columns x batch requests x budgets: the tail is
//           min(S / 5, ceil(3 sqrt S)) in exact arithmetic, the grid fits on chip, the padded segment
//           is even and one pad at most, the chunks cover S once and in order, the batches cover
//           every column once, the scratch is what the kernels index, refusals exactly outside the
//           limits; prints "sweep <plans> <failures>"
//   check <n> <k> <S> <n_models> <n_alphas> <alpha as double> <components>   the refusal text, or "ok"
#include "../pybmc_amd/csrc/bmc_plan.h"
#include "../pybmc_amd/csrc/bmc_sens_plan.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace bmc;

// M by its definition, without the header's integer root: the largest r with (r - 1)^2 < 9 S
static int64_t tail_by_definition(int64_t S) {
    __int128 v = (__int128)9 * S;
    int64_t r = (int64_t)std::sqrt((long double)v);
    while ((__int128)r * r < v) ++r;
    while (r > 0 && (__int128)(r - 1) * (r - 1) >= v) --r;
    return S / 5 < r ? S / 5 : r;
}

static int check_shape(int64_t S) {
    int bad = 0;
    const int64_t M = sens_tail_length(S);
    bad += M != tail_by_definition(S);
    bad += M != psis_tail_length(S) || SENS_MIN_TAIL != PSIS_MIN_TAIL;   // the one rule under the plan's names
    bad += M < 0 || (S >= 1 && M >= S && M > 0);
    if (M >= SENS_MIN_TAIL) {
        const int32_t mg = sens_grid_points(M);
        const int64_t rt = mg - 30;
        bad += rt * rt > M || (rt + 1) * (rt + 1) <= M || mg > SENS_MAX_GRID;
        bad += M + 1 > S;   // the cutoff is a draw below the tail
    }
    const int64_t Sp = sens_padded(S);
    bad += (Sp & 1) != 0 || Sp < S || Sp > S + 1 || Sp > RANK_MAX_S;
    // the chunks: in order, no gap, no overlap, none empty, none past S
    const int64_t chunks = sens_chunks(S);
    int64_t next = 0;
    const int64_t step = chunks > 64 ? chunks / 61 : 1;   // every chunk of small S, a sample of large S
    for (int64_t c = 0; c < chunks; c += step) {
        int64_t first;
        int32_t count;
        sens_chunk(S, c, &first, &count);
        bad += first != c * SENS_CHUNK || count < 1 || count > SENS_CHUNK || first + count > S;
        if (step == 1) {
            bad += first != next;
            next = first + count;
        }
    }
    if (step == 1) bad += next != S;
    {
        int64_t first;
        int32_t count;
        sens_chunk(S, chunks - 1, &first, &count);
        bad += first + count != S;
    }
    return bad;
}

static int check_plan(int64_t S, int32_t n_cols, int32_t W, int32_t cpb, size_t budget) {
    const SensPlan p = plan_sens(S, n_cols, W, cpb, budget);
    const bool refuse = S < 2 || S > SENS_MAX_S || n_cols < 1 || n_cols > 65536 || W < 1 ||
                        W > SENS_COMPONENTS * SENS_MAX_ALPHAS || cpb < 0;
    int bad = 0;
    if (refuse) return p.ok || p.why.empty();
    if (!p.ok) {
        SensPlan one;
        one.S = S, one.S_pad = sens_padded(S), one.W = W;
        one.tiles = (one.S_pad + RANK_TILE - 1) / RANK_TILE;
        one.chunks = sens_chunks(S);
        sens_scratch(one, 1);
        return cpb != 0 || one.bytes_total <= budget;
    }
    bad += p.S != S || p.S_pad != sens_padded(S) || p.M != sens_tail_length(S) || p.W != W;
    bad += p.tiles * RANK_TILE < p.S_pad || (p.tiles - 1) * RANK_TILE >= p.S_pad;
    bad += p.chunks * SENS_CHUNK < S || (p.chunks - 1) * SENS_CHUNK >= S;
    bad += p.cols_per_batch < 1 || p.cols_per_batch > n_cols || p.cols_per_batch > SENS_MAX_BATCH;
    const int64_t cap = RANK_MAX_BLOCKS / (p.tiles * RANK_ITEMS);
    if (cpb > 0 && cpb <= cap && cpb <= SENS_MAX_BATCH) bad += p.cols_per_batch != (cpb < n_cols ? cpb : n_cols);
    if (cpb == 0) bad += p.bytes_total > budget;
    if (cap >= 1) bad += p.tiles * RANK_ITEMS * p.cols_per_batch > RANK_MAX_BLOCKS;
    int32_t next = 0;
    for (int32_t b = 0; b < p.n_batches; ++b) {
        int32_t c0, nc;
        sens_batch(p, n_cols, b, &c0, &nc);
        bad += c0 != next || nc < 1 || nc > p.cols_per_batch;
        next = c0 + nc;
    }
    bad += next != n_cols;
    const size_t Pb = (size_t)p.cols_per_batch;
    bad += p.bytes_keys != Pb * (size_t)p.S_pad * 8 || p.bytes_idx != Pb * (size_t)p.S_pad * 4;
    bad += p.bytes_hist != Pb * (size_t)p.tiles * 256 * 4 || p.bytes_small < Pb * 20;
    bad += p.bytes_part != Pb * (size_t)W * (size_t)p.chunks * SENS_PART * 8;
    bad += p.bytes_offs != Pb * (size_t)W * (size_t)p.chunks * 8;
    bad += p.bytes_total != 2 * p.bytes_keys + 2 * p.bytes_idx + p.bytes_hist + p.bytes_small + p.bytes_part + p.bytes_offs;
    if (p.cols_per_batch > 1) {
        SensPlan q = p;
        sens_scratch(q, p.cols_per_batch - 1);
        bad += q.bytes_total >= p.bytes_total;
    }
    return bad;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "const")) {
        printf("chunk=%d block=%d items=%d sort_tile=%d max_alphas=%d min_tail=%d max_grid=%d wg=%d\n", SENS_CHUNK,
               SENS_BLOCK, SENS_ITEMS, RANK_TILE, SENS_MAX_ALPHAS, SENS_MIN_TAIL, SENS_MAX_GRID, SENS_WG);
        return 0;
    }
    if (argc == 3 && !strcmp(argv[1], "tail")) {
        const int64_t M = sens_tail_length(atoll(argv[2]));
        printf("M=%lld grid=%d\n", (long long)M, M >= SENS_MIN_TAIL ? sens_grid_points(M) : 0);
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "tails")) {
        std::vector<int64_t> in(1 << 16);
        std::vector<int32_t> out(3 * in.size());
        size_t got;
        while ((got = fread(in.data(), 8, in.size(), stdin)) > 0) {
            for (size_t i = 0; i < got; ++i) {
                const int64_t M = psis_tail_length(in[i]);
                out[3 * i] = (int32_t)M;
                out[3 * i + 1] = psis_grid_points(M);
                out[3 * i + 2] = (int32_t)plan_loo(100, in[i], 3, 256).tail;
            }
            if (fwrite(out.data(), 4, 3 * got, stdout) != 3 * got) return 1;
        }
        return 0;
    }
    if (argc == 7 && !strcmp(argv[1], "plan")) {
        const SensPlan p = plan_sens(atoll(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]),
                                     (size_t)strtoull(argv[6], nullptr, 10));
        printf("ok=%d S_pad=%lld tiles=%lld chunks=%lld M=%lld grid=%d cols_per_batch=%d n_batches=%d total=%zu why=%s\n",
               (int)p.ok, (long long)p.S_pad, (long long)p.tiles, (long long)p.chunks, (long long)p.M, p.grid_points,
               p.cols_per_batch, p.n_batches, p.bytes_total, p.why.c_str());
        return 0;
    }
    if (argc == 9 && !strcmp(argv[1], "check")) {
        const int n_alphas = atoi(argv[6]);
        const std::vector<double> alphas(n_alphas > 0 && n_alphas < 1000 ? n_alphas : 1, atof(argv[7]));
        const std::string why = sens_check(atoll(argv[2]), atoi(argv[3]), atoll(argv[4]), atoi(argv[5]),
                                           alphas.data(), n_alphas, (uint32_t)atoi(argv[8]));
        printf("%s\n", why.empty() ? "ok" : why.c_str());
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "sweep")) {
        long plans = 0, failures = 0;
        std::vector<int64_t> Ss;
        for (int64_t S = 1; S <= 5000; ++S) Ss.push_back(S);
        for (int64_t S : {(int64_t)RANK_TILE - 1, (int64_t)RANK_TILE, (int64_t)RANK_TILE + 1, (int64_t)3200000,
                          (int64_t)7400001, (int64_t)1 << 30, SENS_MAX_S - 1, SENS_MAX_S})
            Ss.push_back(S);
        for (int64_t S : Ss) {
            failures += check_shape(S);
            const bool all = S <= 40 || S % 257 == 0 || S > 5000 || (S >= SENS_CHUNK - 1 && S <= SENS_CHUNK + 1) ||
                             (S >= RANK_TILE - 1 && S <= RANK_TILE + 1);
            if (!all) continue;
            for (int32_t n_cols : {1, 4, 33, 65536})
                for (int32_t W : {1, 4, 264})
                    for (int32_t cpb : {0, 1, 5, 70000})
                        for (size_t budget : {(size_t)1 << 12, (size_t)1 << 26, (size_t)200 << 30}) {
                            failures += check_plan(S, n_cols, W, cpb, budget);
                            ++plans;
                        }
        }
        // outside the limits
        failures += check_plan(0, 4, 4, 0, (size_t)1 << 30) + check_plan(1, 4, 4, 0, (size_t)1 << 30);
        failures += check_plan(SENS_MAX_S + 1, 4, 4, 0, (size_t)1 << 40);
        failures += check_plan(100, 0, 4, 0, (size_t)1 << 30) + check_plan(100, 65537, 4, 0, (size_t)1 << 30);
        failures += check_plan(100, 4, 0, 0, (size_t)1 << 30) + check_plan(100, 4, 265, 0, (size_t)1 << 30);
        failures += check_plan(100, 4, 4, -1, (size_t)1 << 30);
        plans += 8;
        printf("sweep %ld %ld\n", plans, failures);
        return failures != 0;
    }
    fprintf(stderr, "usage: sens_plan_check const | tail S | tails | plan ... | check ... | sweep\n");
    return 2;
}
