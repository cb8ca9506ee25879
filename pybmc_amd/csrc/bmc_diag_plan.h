// Host-only plans of the chain-diagnostics kernels (kernels_diag.hip): the tile
// constants, how the moments pass splits a sequence's rows, and how the autocovariance pass splits
// sequences, columns, lags and rows over workgroups, with the scratch sizes of both.  No HIP
// types: tests/diag_plan_check.cpp compiles it with g++.
#pragma once
#include <cstddef>
#include <cstdint>

namespace bmc {

constexpr int DIAG_THREADS = 256;
constexpr int DIAG_R = 128;    // rows of one acov tile
constexpr int DIAG_CW = 16;    // columns of one acov workgroup (4 per wave)
constexpr int DIAG_LC = 64;    // lags of one acov workgroup (one per lane)
constexpr int DIAG_TARGET_GROUPS = 2048;

inline int64_t diag_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// diag_moments_kernel: grid n_seq * ncc * S; column chunk cc holds columns [64 cc, 64 cc + 64),
// row split s rows [s rps, min((s + 1) rps, len)) of its sequence (len = n, or 1 for a middle draw)
struct MomentPlan {
    int32_t ncc, S;
    int64_t rps;
};
inline MomentPlan moment_plan(int32_t n_seq, int32_t P, int64_t n) {
    MomentPlan p;
    p.ncc = (int32_t)diag_cdiv(P, 64);
    const int64_t units = (int64_t)n_seq * p.ncc;
    int64_t S = diag_cdiv(DIAG_TARGET_GROUPS, units);
    const int64_t smax = diag_cdiv(n, 256);   // at least 256 rows per split
    S = S < 1 ? 1 : (S > smax ? smax : S);
    p.rps = diag_cdiv(n, S);
    p.S = (int32_t)diag_cdiv(n, p.rps);
    return p;
}
inline size_t moment_scratch_bytes(const MomentPlan& p, int32_t n_seq, int32_t P) {
    return (size_t)n_seq * p.S * 2 * P * sizeof(double);
}

// diag_acov_kernel: grid MG * ncc * nlc * S; group g sequences [g spg, min((g + 1) spg, 2C)),
// column group cc active columns [16 cc, 16 cc + 16), lag chunk lc lags [t0 + 64 lc, + 64),
// row split s rows [s rps, min((s + 1) rps, n)) in tiles of DIAG_R (rps is a multiple of it)
struct AcovPlan {
    int32_t ncc, nlc, MG, spg, S;
    int64_t rps;
};
inline AcovPlan acov_plan(int32_t C, int64_t n, int32_t n_active, int64_t n_lags) {
    AcovPlan p;
    const int32_t M = 2 * C;
    p.ncc = (int32_t)diag_cdiv(n_active, DIAG_CW);
    p.nlc = (int32_t)diag_cdiv(n_lags, DIAG_LC);
    const int64_t units = (int64_t)p.ncc * p.nlc;
    const int64_t tiles = diag_cdiv(n, DIAG_R);
    int64_t MG = 1, S = 1;
    if (units < DIAG_TARGET_GROUPS) {
        const int64_t want = diag_cdiv(DIAG_TARGET_GROUPS, units);
        MG = want < M ? want : M;
        S = diag_cdiv(want, MG);
        S = S > tiles ? tiles : S;
    }
    p.spg = (int32_t)diag_cdiv(M, MG);
    p.MG = (int32_t)diag_cdiv(M, p.spg);
    const int64_t tps = diag_cdiv(tiles, S);   // tiles per split
    p.rps = tps * DIAG_R;
    p.S = (int32_t)diag_cdiv(tiles, tps);
    return p;
}
inline int64_t acov_groups(const AcovPlan& p) { return (int64_t)p.MG * p.ncc * p.nlc * p.S; }
inline size_t acov_scratch_bytes(const AcovPlan& p) {
    return (size_t)acov_groups(p) * DIAG_CW * DIAG_LC * sizeof(double);
}

}  // namespace bmc
