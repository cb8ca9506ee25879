// Host-only plan of the rank-normalised diagnostics (bmc_rank_diagnostics): the
// argument limits, the sort geometry (tile, tiles per segment, passes), the split of the columns
// into batches that fit the device memory, and the scratch sizes of one batch.  No HIP types:
// tests/rank_plan_check.cpp compiles it with g++.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

namespace bmc {

constexpr int RANK_BLOCK = 256;                         // threads of a sort workgroup (4 waves)
constexpr int RANK_ITEMS = 16;                          // keys per thread
constexpr int RANK_TILE = RANK_BLOCK * RANK_ITEMS;      // keys per tile: 4096
constexpr int RANK_DIGIT_BITS = 8, RANK_DIGITS = 1 << RANK_DIGIT_BITS;
constexpr int RANK_PASSES = 64 / RANK_DIGIT_BITS;       // LSD passes over a 64-bit key
constexpr int RANK_MAX_PROBS = 16;
constexpr int RANK_Q_INTERNAL = 3;                      // q05, q50, q95: always computed
constexpr int RANK_Q_SLOTS = RANK_MAX_PROBS + RANK_Q_INTERNAL;
constexpr int RANK_SERIES = 4;                          // z(x), z(f), 1[x <= q05], 1[x <= q95]
constexpr int64_t RANK_MAX_S = 2147483647;              // split draws of a column: u32 indices, i32 ranks
constexpr int32_t RANK_MAX_CHAINS = 65536, RANK_MAX_COLS = 65536;
constexpr int64_t RANK_MAX_BLOCKS = (int64_t)1 << 30;   // workgroups of one launch (tiles x columns)

struct RankPlan {
    bool ok = false;
    std::string why;          // the refusal when !ok
    int64_t n = 0, S = 0;     // draws per split half-chain, split draws per column (2 C n)
    int64_t tiles = 0;        // sort tiles per segment: ceil(S / RANK_TILE)
    int32_t passes = RANK_PASSES;     // at most (constant digits are skipped at run time)
    int32_t cols_per_batch = 0, n_batches = 0;
    // device bytes of one batch of cols_per_batch columns
    size_t bytes_keys = 0;    // ONE of the two key buffers: [Pb][S] u64
    size_t bytes_idx = 0;     // ONE of the two index buffers: [Pb][S] u32
    size_t bytes_hist = 0;    // per-tile digit counts, then offsets: [Pb][tiles][256] u32
    size_t bytes_derived = 0; // [Pb][C][2n][4] f64: a column's four derived series in the samplers' layout
    size_t bytes_small = 0;   // quantiles [Pb][RANK_Q_SLOTS] f64, OR / AND masks [Pb][2] u64, flags [Pb] u32
    size_t bytes_total = 0;
};

// bytes of a batch of Pb columns (monotone in Pb)
inline void rank_scratch(RankPlan& p, int64_t Pb) {
    p.bytes_keys = (size_t)Pb * (size_t)p.S * 8;
    p.bytes_idx = (size_t)Pb * (size_t)p.S * 4;
    p.bytes_hist = (size_t)Pb * (size_t)p.tiles * RANK_DIGITS * 4;
    p.bytes_derived = (size_t)p.S * RANK_SERIES * (size_t)Pb * 8;
    p.bytes_small = (size_t)Pb * (RANK_Q_SLOTS * 8 + 2 * 8 + 4);
    p.bytes_total = 2 * p.bytes_keys + 2 * p.bytes_idx + p.bytes_hist + p.bytes_derived + p.bytes_small;
}

// "" when the arguments are inside the limits of bmc_rank_diagnostics, else the reason
inline std::string rank_check(int32_t C, int64_t iters, int32_t P, int64_t ld, int64_t burn,
                              const double* probs, int32_t n_probs) {
    if (C < 1 || C > RANK_MAX_CHAINS) return "n_chains must be between 1 and 65536";
    if (P < 1 || P > RANK_MAX_COLS) return "n_cols must be between 1 and 65536";
    if (ld < P) return "ld must be >= n_cols";
    if (burn < 0) return "burn must be >= 0";
    if (iters - burn < 8)
        return "need n = (iters - burn) / 2 >= 4 draws per split half-chain (iters = " +
               std::to_string(iters) + ", burn = " + std::to_string(burn) + ")";
    const int64_t n = (iters - burn) / 2;
    if (n > RANK_MAX_S / (2 * (int64_t)C))
        return "too many split draws per column: 2 * n_chains * n must be <= 2^31 - 1";
    if (n_probs < 0 || n_probs > RANK_MAX_PROBS || (n_probs > 0 && !probs))
        return "need between 1 and 16 probabilities";
    for (int32_t i = 0; i < n_probs; ++i)
        if (!(probs[i] >= 0.0 && probs[i] <= 1.0))
            return "probability " + std::to_string(i) + " is outside [0, 1]";
    return "";
}

// cols_per_batch = 0: as many columns as `budget` bytes hold (at least one must fit); > 0: that
// many (clipped to P), whatever the budget.  n_probs = 0 is allowed here (bmc_rank_normalize).
inline RankPlan plan_rank(int32_t C, int64_t iters, int32_t P, int64_t ld, int64_t burn,
                          const double* probs, int32_t n_probs, int32_t cols_per_batch, size_t budget) {
    RankPlan p;
    p.why = rank_check(C, iters, P, ld, burn, probs, n_probs);
    if (p.why.empty() && cols_per_batch < 0) p.why = "cols_per_batch must be >= 0";
    if (!p.why.empty()) return p;
    p.n = (iters - burn) / 2;
    p.S = 2 * (int64_t)C * p.n;
    p.tiles = (p.S + RANK_TILE - 1) / RANK_TILE;
    const int64_t launch_cap = RANK_MAX_BLOCKS / (p.tiles * RANK_ITEMS);   // gather: S / 256 blocks per column
    int64_t Pb = cols_per_batch;
    if (Pb == 0) {
        rank_scratch(p, 1);
        if (p.bytes_total > budget) {
            p.why = "one column needs " + std::to_string(p.bytes_total) + " bytes of device memory; " +
                    std::to_string(budget) + " are free";
            return p;
        }
        Pb = (int64_t)(budget / p.bytes_total);
    }
    if (Pb > P) Pb = P;
    if (Pb > launch_cap) Pb = launch_cap;
    if (Pb < 1) Pb = 1;
    p.cols_per_batch = (int32_t)Pb;
    p.n_batches = (int32_t)((P + Pb - 1) / Pb);
    rank_scratch(p, Pb);
    p.ok = true;
    return p;
}

// columns [col0, col0 + n_cols) of batch b < n_batches
inline void rank_batch(const RankPlan& p, int32_t P, int32_t b, int32_t* col0, int32_t* n_cols) {
    *col0 = b * p.cols_per_batch;
    *n_cols = P - *col0 < p.cols_per_batch ? P - *col0 : p.cols_per_batch;
}

// Bit d set: digit d (bits 8d .. 8d+7) differs between two keys of some segment, whose OR and AND
// over its keys are or_and[2 j], or_and[2 j + 1].  A clear bit is a pass that would move nothing.
inline uint32_t rank_live_passes(const uint64_t* or_and, int32_t n_segments) {
    uint64_t vary = 0;
    for (int32_t j = 0; j < n_segments; ++j) vary |= or_and[2 * j] ^ or_and[2 * j + 1];
    uint32_t live = 0;
    for (int d = 0; d < RANK_PASSES; ++d)
        if ((vary >> (RANK_DIGIT_BITS * d)) & (RANK_DIGITS - 1)) live |= 1u << d;
    return live;
}

// numpy's method="linear": virtual index (S - 1) p in f64, its floor and fraction (the rule of
// _lib.order_stat_plan)
inline void rank_order_stat(int64_t S, double p, int32_t* index, double* weight) {
    const double vi = (double)(S - 1) * p;
    double lo = (double)(int64_t)vi;   // vi >= 0: truncation is the floor
    double g = vi - lo;
    if (lo >= (double)(S - 1)) lo = (double)(S - 1), g = 0.0;
    *index = (int32_t)lo;
    *weight = g;
}

}  // namespace bmc
