// Host-only plan of the power-scaling sensitivity (bmc_power_sensitivity): the
// argument limits, the sort segment (the rank sort's geometry on a segment padded to an even
// length), the chunks of the weight scan, the split of the columns into batches that fit the device
// memory, and the scratch sizes; the tail of the Pareto fit is bmc_psis_plan.h's.  Below them the
// validator and the plan of the Student-t forms (bmc_power_sensitivity_t / _tv).  No HIP types:
// tests/sens_plan_check.cpp and tests/sens_t_plan_check.cpp compile it with g++.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#include "bmc_psis_plan.h"
#include "bmc_rank_plan.h"

namespace bmc {

constexpr int SENS_BLOCK = 256;                          // threads of a scan workgroup
constexpr int SENS_ITEMS = 8;                            // consecutive sorted draws per thread
constexpr int SENS_CHUNK = 2048;                         // sorted draws per scan chunk
static_assert(SENS_CHUNK == SENS_BLOCK * SENS_ITEMS, "a chunk is one workgroup's draws");
constexpr int SENS_WG = 4;                               // weight vectors carried together by the scan
constexpr int SENS_PART = 6;                             // partial sums of a (column, vector, chunk)
constexpr int SENS_MAX_ALPHAS = 66;                        // a grid of 64 and the two of the sensitivity
constexpr int SENS_COMPONENTS = 4;                       // prior, likelihood, prior_beta, prior_sigma2
constexpr int SENS_LOGDENS = 3;                          // lp_beta, lp_sigma2, loglik
constexpr int SENS_MAX_GRID = 512;                       // grid points of the fit held on chip
constexpr int SENS_TILE = 64;                            // draws / points of an MFMA tile (SCORE_TILE)
constexpr int32_t SENS_MAX_K = 256, SENS_MAX_MODELS = 4096;
constexpr int64_t SENS_MAX_S = RANK_MAX_S - 1;           // the padded segment still has u32 indices
constexpr int32_t SENS_MAX_BATCH = 65535;               // columns of a batch: the y extent of a grid
constexpr int64_t SENS_MAX_POINTS = (int64_t)1 << 31;

// the plan's own names of the one tail rule (bmc_psis_plan.h)
constexpr int SENS_MIN_TAIL = PSIS_MIN_TAIL;
inline int64_t sens_tail_length(int64_t S) { return psis_tail_length(S); }
inline int32_t sens_grid_points(int64_t M) { return psis_grid_points(M); }

// the sort segment of a column: S draws and, when S is odd, one pad key that sorts last
inline int64_t sens_padded(int64_t S) { return S + (S & 1); }
inline int64_t sens_chunks(int64_t S) { return (S + SENS_CHUNK - 1) / SENS_CHUNK; }
// first sorted position and length of chunk c < sens_chunks(S)
inline void sens_chunk(int64_t S, int64_t c, int64_t* first, int32_t* count) {
    *first = c * SENS_CHUNK;
    const int64_t left = S - *first;
    *count = (int32_t)(left < SENS_CHUNK ? left : SENS_CHUNK);
}

struct SensPlan {
    bool ok = false;
    std::string why;
    int64_t S = 0, S_pad = 0;        // draws, sort segment
    int64_t tiles = 0, chunks = 0;   // sort tiles and scan chunks per column
    int64_t M = 0;                   // tail length
    int32_t grid_points = 0;         // of the fit (0: no fit)
    int32_t W = 0;                   // weight vectors: components x alphas
    int32_t cols_per_batch = 0, n_batches = 0;
    // device bytes of one batch of cols_per_batch columns
    size_t bytes_keys = 0, bytes_idx = 0, bytes_hist = 0, bytes_small = 0;
    size_t bytes_part = 0;           // [Pb][W][chunks][SENS_PART] f64
    size_t bytes_offs = 0;           // [Pb][W][chunks] f64: chunk sums, then their exclusive scan
    size_t bytes_total = 0;
};

inline void sens_scratch(SensPlan& p, int64_t Pb) {
    p.bytes_keys = (size_t)Pb * (size_t)p.S_pad * 8;
    p.bytes_idx = (size_t)Pb * (size_t)p.S_pad * 4;
    p.bytes_hist = (size_t)Pb * (size_t)p.tiles * RANK_DIGITS * 4;
    p.bytes_small = (size_t)Pb * (2 * 8 + 4 + 4);
    p.bytes_part = (size_t)Pb * (size_t)p.W * (size_t)p.chunks * SENS_PART * 8;
    p.bytes_offs = (size_t)Pb * (size_t)p.W * (size_t)p.chunks * 8;
    p.bytes_total = 2 * p.bytes_keys + 2 * p.bytes_idx + p.bytes_hist + p.bytes_small + p.bytes_part +
                    p.bytes_offs;
}

// "" when the arguments are inside the limits of bmc_power_sensitivity, else the reason
inline std::string sens_check(int64_t n_points, int32_t k, int64_t S, int32_t n_models,
                              const double* alphas, int32_t n_alphas, uint32_t components) {
    if (n_points < 1 || n_points > SENS_MAX_POINTS) return "n_points must be between 1 and 2^31";
    if (k < 1 || k > SENS_MAX_K) return "k must be between 1 and 256";
    if (S < 2 || S > SENS_MAX_S) return "n_draws must be between 2 and 2^31 - 2";
    if (n_models < 0 || n_models > SENS_MAX_MODELS) return "n_models must be between 0 and 4096";
    if (n_alphas < 1 || n_alphas > SENS_MAX_ALPHAS || !alphas) return "need between 1 and 66 alphas";
    for (int32_t i = 0; i < n_alphas; ++i)
        if (!(alphas[i] > 0.0) || alphas[i] == 1.0 || !(alphas[i] <= 1.79769313486231570815e308))
            return "alpha " + std::to_string(i) + " must be positive, finite and not 1";
    if (components == 0 || components >= (1u << SENS_COMPONENTS))
        return "components must be a non-empty mask of prior (1), likelihood (2), prior_beta (4), "
               "prior_sigma2 (8)";
    return "";
}

inline int32_t sens_count_components(uint32_t components) {
    int32_t n = 0;
    for (int b = 0; b < SENS_COMPONENTS; ++b) n += (components >> b) & 1;
    return n;
}

// cols_per_batch = 0: as many columns as `budget` bytes hold; > 0: that many (clipped to n_cols)
inline SensPlan plan_sens(int64_t S, int32_t n_cols, int32_t W, int32_t cols_per_batch, size_t budget) {
    SensPlan p;
    if (S < 2 || S > SENS_MAX_S) p.why = "n_draws must be between 2 and 2^31 - 2";
    else if (n_cols < 1 || n_cols > RANK_MAX_COLS) p.why = "need between 1 and 65536 columns";
    else if (W < 1 || W > SENS_COMPONENTS * SENS_MAX_ALPHAS) p.why = "need between 1 and 264 weight vectors";
    else if (cols_per_batch < 0) p.why = "cols_per_batch must be >= 0";
    if (!p.why.empty()) return p;
    p.S = S;
    p.S_pad = sens_padded(S);
    p.tiles = (p.S_pad + RANK_TILE - 1) / RANK_TILE;
    p.chunks = sens_chunks(S);
    p.M = sens_tail_length(S);
    p.grid_points = p.M >= SENS_MIN_TAIL ? sens_grid_points(p.M) : 0;
    p.W = W;
    int64_t launch_cap = RANK_MAX_BLOCKS / (p.tiles * RANK_ITEMS);
    if (launch_cap > SENS_MAX_BATCH) launch_cap = SENS_MAX_BATCH;
    int64_t Pb = cols_per_batch;
    if (Pb == 0) {
        sens_scratch(p, 1);
        if (p.bytes_total > budget) {
            p.why = "one column needs " + std::to_string(p.bytes_total) + " bytes of device memory; " +
                    std::to_string(budget) + " are free";
            return p;
        }
        Pb = (int64_t)(budget / p.bytes_total);
    }
    if (Pb > n_cols) Pb = n_cols;
    if (Pb > launch_cap) Pb = launch_cap;
    if (Pb < 1) Pb = 1;
    p.cols_per_batch = (int32_t)Pb;
    p.n_batches = (int32_t)((n_cols + Pb - 1) / Pb);
    sens_scratch(p, Pb);
    p.ok = true;
    return p;
}

// ---- the Student-t forms (bmc_power_sensitivity_t / _tv) -----------------------
// A fifth component, the prior of nu, and a fourth log density, lp_nu: only a _tv call that was
// given nu_log_prior has them.  The table of distinct nu has the limits of bmc_pointwise_loglik_tv.
constexpr int SENS_T_COMPONENTS = 5;                     // SENS_COMPONENTS' four, then prior_nu
constexpr int SENS_T_LOGDENS = 4;                        // SENS_LOGDENS' three, then lp_nu
constexpr int32_t SENS_MAX_NU_VALUES = 4096;             // distinct nu of a call (PPC_MAX_NU_VALUES)
constexpr int32_t SENS_T_MAX_W = SENS_T_COMPONENTS * (SENS_MAX_ALPHAS + 2);

inline bool sens_positive_finite(double v) { return v > 0.0 && v <= 1.79769313486231570815e308; }

inline int32_t sens_t_count_components(uint32_t components) {
    int32_t n = 0;
    for (int b = 0; b < SENS_T_COMPONENTS; ++b) n += (components >> b) & 1;
    return n;
}

// "" when the arguments are inside the limits of the Student-t forms, else the reason.  A fixed nu
// is a table of one value without an index (per_draw false); nu_log_prior may be NULL.
inline std::string sens_t_check(int64_t n_points, int32_t k, int64_t S, int32_t n_models,
                                const double* alphas, int32_t n_alphas, uint32_t components, bool per_draw,
                                const double* nu_values, int32_t n_values, const double* nu_log_prior) {
    // (the shape and the alphas by the Gaussian form's rules; the mask has its own below)
    const std::string base = sens_check(n_points, k, S, n_models, alphas, n_alphas, 1u);
    if (!base.empty()) return base;
    const bool wide = components >= (1u << SENS_COMPONENTS);
    if (components == 0 || components >= (1u << SENS_T_COMPONENTS))
        return "components must be a non-empty mask of prior (1), likelihood (2), prior_beta (4), "
               "prior_sigma2 (8), prior_nu (16)";
    if (!nu_values) return per_draw ? "nu_values and nu_index must not be NULL" : "nu must be positive and finite";
    if (n_values < 1 || n_values > SENS_MAX_NU_VALUES) return "n_values must be between 1 and 4096";
    for (int32_t v = 0; v < n_values; ++v)
        if (!sens_positive_finite(nu_values[v]))
            return per_draw ? "nu_values must be positive and finite" : "nu must be positive and finite";
    if (nu_log_prior)
        for (int32_t v = 0; v < n_values; ++v)
            if (!(nu_log_prior[v] >= -1.79769313486231570815e308 && nu_log_prior[v] <= 1.79769313486231570815e308))
                return "nu_log_prior must be finite";
    if (wide && !(per_draw && nu_log_prior)) return "the component prior_nu (16) needs nu_log_prior";
    if (sens_t_count_components(components) * n_alphas > SENS_T_MAX_W)
        return "need between 1 and 340 weight vectors";
    return "";
}

// plan_sens at the weight-vector bound of the Student-t forms
inline SensPlan plan_sens_t(int64_t S, int32_t n_cols, int32_t W, int32_t cols_per_batch, size_t budget) {
    if (W <= SENS_COMPONENTS * SENS_MAX_ALPHAS) return plan_sens(S, n_cols, W, cols_per_batch, budget);
    // the checks and the segment of plan_sens with one vector, then the batch at the real W
    SensPlan p = plan_sens(S, n_cols, 1, cols_per_batch, budget);
    if (!p.ok) return p;
    p.ok = false;
    if (W > SENS_T_MAX_W) {
        p.why = "need between 1 and 340 weight vectors";
        return p;
    }
    p.W = W;
    int64_t launch_cap = RANK_MAX_BLOCKS / (p.tiles * RANK_ITEMS);
    if (launch_cap > SENS_MAX_BATCH) launch_cap = SENS_MAX_BATCH;
    int64_t Pb = cols_per_batch;
    if (Pb == 0) {
        sens_scratch(p, 1);
        if (p.bytes_total > budget) {
            p.why = "one column needs " + std::to_string(p.bytes_total) + " bytes of device memory; " +
                    std::to_string(budget) + " are free";
            return p;
        }
        Pb = (int64_t)(budget / p.bytes_total);
    }
    if (Pb > n_cols) Pb = n_cols;
    if (Pb > launch_cap) Pb = launch_cap;
    if (Pb < 1) Pb = 1;
    p.cols_per_batch = (int32_t)Pb;
    p.n_batches = (int32_t)((n_cols + Pb - 1) / Pb);
    sens_scratch(p, Pb);
    p.ok = true;
    return p;
}

inline void sens_batch(const SensPlan& p, int32_t n_cols, int32_t b, int32_t* col0, int32_t* n) {
    *col0 = b * p.cols_per_batch;
    *n = n_cols - *col0 < p.cols_per_batch ? n_cols - *col0 : p.cols_per_batch;
}

}  // namespace bmc
