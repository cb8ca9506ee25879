// CPU check of the Student-t forms of the power-scaling sensitivity: the validator and the plan of
// pybmc_amd/csrc/bmc_sens_plan.h, and what the tile kernel needs of bmc_math.h for a padded point.
//   const   the limits as key=value
//   zero    a padded point adds exactly 0: log1p_nonneg(0.0) is +0.0 and 0 g is 0 for finite g
//           (the text the gfx950 kernels compile); prints "zero <failures>"
//   check <n> <k> <S> <n_models> <n_alphas> <alpha> <components> <per_draw> <n_values> <nu> <log prior | none>
//           the refusal text, or "ok"; the table holds n_values copies of nu (and of the log prior)
//   plan <S> <n_cols> <W> <cols_per_batch> <budget>   plan_sens_t's fields as key=value
//   sweep   plan_sens_t is plan_sens up to its 264 vectors, plans 265 .. 340 by the same rules and
//           refuses 341; prints "sweep <plans> <failures>"
#include "../pybmc_amd/csrc/bmc_math.h"
#include "../pybmc_amd/csrc/bmc_plan.h"
#include "../pybmc_amd/csrc/bmc_sens_plan.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace bmc;

static bool same(const SensPlan& a, const SensPlan& b) {
    return a.ok == b.ok && a.why == b.why && a.S == b.S && a.S_pad == b.S_pad && a.tiles == b.tiles &&
           a.chunks == b.chunks && a.M == b.M && a.grid_points == b.grid_points && a.W == b.W &&
           a.cols_per_batch == b.cols_per_batch && a.n_batches == b.n_batches && a.bytes_keys == b.bytes_keys &&
           a.bytes_idx == b.bytes_idx && a.bytes_hist == b.bytes_hist && a.bytes_small == b.bytes_small &&
           a.bytes_part == b.bytes_part && a.bytes_offs == b.bytes_offs && a.bytes_total == b.bytes_total;
}

// a plan above plan_sens's bound: the rules of tests/sens_plan_check.cpp's check_plan
static int check_wide(int64_t S, int32_t n_cols, int32_t W, int32_t cpb, size_t budget) {
    const SensPlan p = plan_sens_t(S, n_cols, W, cpb, budget);
    if (W > SENS_T_MAX_W) return p.ok || p.why.empty();
    if (!p.ok) {
        SensPlan one;
        one.S = S, one.S_pad = sens_padded(S), one.W = W;
        one.tiles = (one.S_pad + RANK_TILE - 1) / RANK_TILE;
        one.chunks = sens_chunks(S);
        sens_scratch(one, 1);
        return cpb != 0 || one.bytes_total <= budget;
    }
    int bad = 0;
    bad += p.S != S || p.S_pad != sens_padded(S) || p.M != sens_tail_length(S) || p.W != W;
    bad += p.chunks != sens_chunks(S) || p.tiles != (p.S_pad + RANK_TILE - 1) / RANK_TILE;
    bad += p.cols_per_batch < 1 || p.cols_per_batch > n_cols || p.cols_per_batch > SENS_MAX_BATCH;
    if (cpb == 0) bad += p.bytes_total > budget;
    const int64_t cap = RANK_MAX_BLOCKS / (p.tiles * RANK_ITEMS);
    if (cpb > 0 && cpb <= cap && cpb <= SENS_MAX_BATCH) bad += p.cols_per_batch != (cpb < n_cols ? cpb : n_cols);
    int32_t next = 0;
    for (int32_t b = 0; b < p.n_batches; ++b) {
        int32_t c0, nc;
        sens_batch(p, n_cols, b, &c0, &nc);
        bad += c0 != next || nc < 1 || nc > p.cols_per_batch;
        next = c0 + nc;
    }
    bad += next != n_cols;
    const size_t Pb = (size_t)p.cols_per_batch;
    bad += p.bytes_part != Pb * (size_t)W * (size_t)p.chunks * SENS_PART * 8;
    bad += p.bytes_offs != Pb * (size_t)W * (size_t)p.chunks * 8;
    bad += p.bytes_total != 2 * p.bytes_keys + 2 * p.bytes_idx + p.bytes_hist + p.bytes_small + p.bytes_part + p.bytes_offs;
    return bad;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "const")) {
        printf("components=%d gaussian_components=%d logdens=%d max_nu_values=%d max_w=%d gaussian_max_w=%d\n",
               SENS_T_COMPONENTS, SENS_COMPONENTS, SENS_T_LOGDENS, SENS_MAX_NU_VALUES, SENS_T_MAX_W,
               SENS_COMPONENTS * SENS_MAX_ALPHAS);
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "zero")) {
        int bad = 0;
        const double z = log1p_nonneg(0.0);
        bad += !(z == 0.0) || std::signbit(z);
        for (double g : {0.0, 4.9406564584124654e-324, 1e-300, 0.25, 1.0, 3.7e19, 1.79769313486231570815e308}) {
            volatile double e = 0.0;   // (the residual of a padded point, not folded by the compiler)
            const double x = (e * e) * g;
            bad += !(x == 0.0) || std::signbit(x);
            bad += !(log1p_nonneg(x) == 0.0);
            double sum = 1.2345;   // and adding it leaves a running sum as it was
            sum += log1p_nonneg(x);
            bad += sum != 1.2345;
        }
        // (a NaN or infinite g: the draw has no log density, sens_logdens_t_kernel writes NaN)
        bad += !std::isnan(log1p_nonneg((0.0 * 0.0) * INFINITY)) || !std::isnan(log1p_nonneg(NAN));
        printf("zero %d\n", bad);
        return bad != 0;
    }
    if (argc == 13 && !strcmp(argv[1], "check")) {
        const int n_alphas = atoi(argv[6]), n_values = atoi(argv[10]);
        const std::vector<double> alphas(n_alphas > 0 && n_alphas < 1000 ? n_alphas : 1, atof(argv[7]));
        const size_t V = n_values > 0 && n_values < 100000 ? n_values : 1;
        const std::vector<double> values(V, atof(argv[11])), lp(V, atof(argv[12]));
        const bool prior = strcmp(argv[12], "none") != 0;
        const std::string why =
            sens_t_check(atoll(argv[2]), atoi(argv[3]), atoll(argv[4]), atoi(argv[5]), alphas.data(), n_alphas,
                         (uint32_t)atoi(argv[8]), atoi(argv[9]) != 0, values.data(), n_values,
                         prior ? lp.data() : nullptr);
        printf("%s\n", why.empty() ? "ok" : why.c_str());
        return 0;
    }
    if (argc == 7 && !strcmp(argv[1], "plan")) {
        const SensPlan p = plan_sens_t(atoll(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]),
                                       (size_t)strtoull(argv[6], nullptr, 10));
        printf("ok=%d W=%d cols_per_batch=%d n_batches=%d part=%zu offs=%zu total=%zu why=%s\n", (int)p.ok, p.W,
               p.cols_per_batch, p.n_batches, p.bytes_part, p.bytes_offs, p.bytes_total, p.why.c_str());
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "sweep")) {
        long plans = 0, failures = 0;
        for (int64_t S : {(int64_t)0, (int64_t)1, (int64_t)2, (int64_t)25, (int64_t)SENS_CHUNK + 1, (int64_t)3200001,
                          SENS_MAX_S, SENS_MAX_S + 1})
            for (int32_t n_cols : {0, 1, 5, 34, 65536, 65537})
                for (int32_t cpb : {-1, 0, 1, 5, 70000})
                    for (size_t budget : {(size_t)1 << 12, (size_t)1 << 26, (size_t)200 << 30}) {
                        for (int32_t W : {0, 1, 4, 264}) {
                            failures += !same(plan_sens_t(S, n_cols, W, cpb, budget),
                                              plan_sens(S, n_cols, W, cpb, budget));
                            ++plans;
                        }
                        const bool inside = S >= 2 && S <= SENS_MAX_S && n_cols >= 1 && n_cols <= 65536 && cpb >= 0;
                        for (int32_t W : {265, 330, 340, 341}) {
                            if (inside) failures += check_wide(S, n_cols, W, cpb, budget);
                            else failures += plan_sens_t(S, n_cols, W, cpb, budget).ok;
                            ++plans;
                        }
                    }
        printf("sweep %ld %ld\n", plans, failures);
        return failures != 0;
    }
    fprintf(stderr, "usage: sens_t_plan_check const | zero | check ... | plan ... | sweep\n");
    return 2;
}
