// Host-only plan of the Student-t (outlier-robust) Gibbs sampler (bmc_robust_run):
// the row slab of every wave, the MFMA tile count and the kernel width for a given (N, k), the
// workspace and replay-buffer sizes, the split of n_chains into launches and the argument checks.
// No HIP types: tests/robust_plan_check.cpp compiles it with g++.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace bmc {

constexpr int ROBUST_MAX_K = 32;                    // two 16-column MFMA tiles; one lane per Cholesky row
constexpr int ROBUST_WAVES = 4;                     // one workgroup of 256 threads per chain
constexpr int ROBUST_THREADS = 64 * ROBUST_WAVES;
constexpr int ROBUST_ROW_STEP = 4;                  // rows per v_mfma_f64_16x16x4_f64 k-step
constexpr int ROBUST_MAX_CHAINS_PER_LAUNCH = 1024;  // workgroups of one launch (chains never wait for
                                                    // each other: any split gives the same bits)

// 16-column tiles of X in the weighted Gram (y is not a column: X'Ly is summed beside the tiles)
inline int robust_tiles(int k) { return k <= 16 ? 1 : 2; }
inline int robust_ldz(int k) { return 16 * robust_tiles(k); }
// the instantiation of robust_chain_kernel: rows of the register-resident Cholesky factor
inline int robust_kc(int k) { return k <= 4 ? 4 : k <= 8 ? 8 : k <= 16 ? 16 : 32; }
// upper-triangle tile pairs: MFMAs per k-step
inline int robust_tile_pairs(int k) { return robust_tiles(k) * (robust_tiles(k) + 1) / 2; }

// Wave w owns the contiguous rows [w * rows_per_wave, min(N, (w + 1) * rows_per_wave)): whole
// k-steps, the same number for every wave, fixed by N alone.
inline int64_t robust_rows_per_wave(int64_t n) {
    const int64_t steps = (n + ROBUST_ROW_STEP - 1) / ROBUST_ROW_STEP;
    return (steps + ROBUST_WAVES - 1) / ROBUST_WAVES * ROBUST_ROW_STEP;
}
// rows of the packed, zero-padded copy of X that the Gram pass reads
inline int64_t robust_rows_padded(int64_t n) { return robust_rows_per_wave(n) * ROBUST_WAVES; }
struct RobustSlab {
    int64_t row0, row1;   // [row0, row1); empty when row0 == row1
};
inline RobustSlab robust_slab(int64_t n, int wave) {
    const int64_t rpw = robust_rows_per_wave(n);
    int64_t r0 = wave * rpw, r1 = r0 + rpw;
    if (r0 > n) r0 = n;
    if (r1 > n) r1 = n;
    return RobustSlab{r0, r1};
}

// per-chain row state [n_chains][N][2] f64: the residual r_n and the weight lambda_n
inline size_t robust_workspace_bytes(int64_t n, int32_t n_chains) {
    return (size_t)n_chains * (size_t)n * 2 * sizeof(double);
}
// the packed operand: [rows_padded][ldz] of X, then [rows_padded] of y
inline size_t robust_packed_bytes(int64_t n, int32_t k) {
    return (size_t)robust_rows_padded(n) * (size_t)(robust_ldz(k) + 1) * sizeof(double);
}
// replay mode: the caller's gl [n_chains][burn + iters][N]
inline size_t robust_gl_bytes(int64_t n, int32_t n_chains, int64_t sweeps) {
    return (size_t)n_chains * (size_t)sweeps * (size_t)n * sizeof(double);
}

struct RobustLaunch {
    int32_t c0, n_chains;
};
inline std::vector<RobustLaunch> robust_launches(int32_t n_chains) {
    std::vector<RobustLaunch> out;
    for (int32_t c = 0; c < n_chains; c += ROBUST_MAX_CHAINS_PER_LAUNCH)
        out.push_back(RobustLaunch{c, n_chains - c < ROBUST_MAX_CHAINS_PER_LAUNCH
                                          ? n_chains - c : ROBUST_MAX_CHAINS_PER_LAUNCH});
    return out;
}

// "" when the arguments describe a valid run, else the reason
inline std::string robust_check(int64_t n, int32_t k, int f32, double nu, int32_t n_chains,
                                int64_t iters, int64_t burn) {
    if (n < 1) return "need N >= 1";
    if (n >= ((int64_t)1 << 32)) return "N must be < 2^32 (the row is one Philox counter word)";
    if (k < 1 || k > ROBUST_MAX_K)
        return "the Student-t sampler supports 1 <= k <= " + std::to_string(ROBUST_MAX_K) +
               " columns; got " + std::to_string(k);
    if (f32) return "the Student-t sampler needs a problem stored in float64 (dtype BMC_F64)";
    if (!(nu > 0) || !std::isfinite(nu)) return "nu must be positive and finite";
    if (n_chains < 1) return "need n_chains >= 1";
    if (iters < 0) return "need iters >= 0";
    if (burn < 0) return "Burn-in iterations must be non-negative.";
    if (burn + iters >= 0xffffffffll) return "burn + iters must be < 2^32 - 1";
    return "";
}

// ---- nu on a grid (bmc_robust_run_nu) --------------------------------------------------
constexpr int ROBUST_MAX_NU_GRID = 64;              // one lane of wave 0 per grid value

// "" when (grid, weight, nu_init) describe a valid discrete prior, else the reason
inline std::string robust_nu_check(const double* grid, const double* weight, int32_t n_grid,
                                   int32_t nu_init) {
    if (n_grid < 1 || n_grid > ROBUST_MAX_NU_GRID)
        return "the nu grid needs 1 <= n_grid <= " + std::to_string(ROBUST_MAX_NU_GRID) + " values; got " +
               std::to_string(n_grid);
    if (!grid || !weight) return "nu_grid and nu_weight must not be NULL";
    bool any = false;
    for (int32_t g = 0; g < n_grid; ++g) {
        if (!(grid[g] > 0) || !std::isfinite(grid[g])) return "the nu grid must be positive and finite";
        if (g > 0 && !(grid[g] > grid[g - 1])) return "the nu grid must be strictly increasing";
        if (!(weight[g] >= 0) || !std::isfinite(weight[g]))
            return "the nu prior weights must be non-negative and finite";
        any = any || weight[g] > 0;
    }
    if (!any) return "at least one nu prior weight must be positive";
    if (nu_init < 0 || nu_init >= n_grid) return "nu_init must index the nu grid";
    if (!(weight[nu_init] > 0)) return "nu_init must have a positive prior weight";
    return "";
}

// The four rows [4][n_grid] that the kernel keeps in LDS: nu_g, the shape (nu_g + 1) / 2 of the weight
// variates, h_g = nu_g / 2 and c_g = n (h_g log h_g - lgamma(h_g)) + log w_g (-inf where w_g = 0).
// log p(nu_g | lambda) = h_g T + c_g + const with T = sum_n (log lambda_n - lambda_n).
inline void robust_nu_table(const double* grid, const double* weight, int32_t n_grid, int64_t n,
                            double* table) {
    for (int32_t g = 0; g < n_grid; ++g) {
        const double nu = grid[g], h = nu / 2.0;
        table[g] = nu;
        table[n_grid + g] = (nu + 1.0) / 2.0;
        table[2 * n_grid + g] = h;
        table[3 * n_grid + g] = weight[g] > 0
                                    ? (double)n * (h * std::log(h) - std::lgamma(h)) + std::log(weight[g])
                                    : -HUGE_VAL;
    }
}

}  // namespace bmc
