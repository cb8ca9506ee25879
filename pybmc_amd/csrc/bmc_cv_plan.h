// Host-only plan of exact K-fold / leave-group-out cross-validation (bmc_kfold_cv):
// label validation, the fold-ordered row layout and its chunk tables, the kernel width, the split
// of the F x C chains into batches that fit the device memory and launches of at most 2048 one-wave
// chains, and the memory estimate.  No HIP types: tests/cv_plan_check.cpp compiles it with g++.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace bmc {

constexpr int CV_MAX_K = 64;                      // one lane per coefficient (gibbs_gram_kernel)
constexpr int CV_MIN_FOLDS = 2, CV_MAX_FOLDS = 1024;
constexpr int CV_MAX_CHAINS_PER_LAUNCH = 2048;    // the bound of the other one-wave launches
constexpr int CV_ROW_PAD = 4;                     // rows per v_mfma_f64_16x16x4_f64 k-step
constexpr int CV_GRAM_CHUNK = 512;                // rows per Gram partial (a multiple of CV_ROW_PAD)
constexpr int CV_RSS_CHUNK = 64;                  // rows per block-rss partial
// cv_gather_kernel and cv_unrotate_kernel are grid-stride loops: at most CV_STRIDE_BLOCKS blocks of
// CV_STRIDE_THREADS threads, so a launch of more elements than their product makes a second trip
constexpr int CV_STRIDE_THREADS = 256;
constexpr int CV_STRIDE_BLOCKS = 8192;

// columns of the gathered matrix [A | y | 0-pad]: whole 16-column MFMA tiles
inline int cv_ldz(int k) { return (k + 1 + 15) / 16 * 16; }
inline int cv_tiles(int k) { return cv_ldz(k) / 16; }
// the instantiation of cv_gram_kernel / cv_block_rss_kernel
inline int cv_kmax(int k) { return k <= 8 ? 8 : k <= 16 ? 16 : k <= 32 ? 32 : 64; }

// Rows of one fold cut into pieces of at most `chunk` rows
struct CvChunks {
    std::vector<int64_t> row0;      // first (padded-layout) row of the chunk
    std::vector<int32_t> rows;      // its rows
    std::vector<int32_t> fold_off;  // [F + 1]: chunks of fold f are fold_off[f] .. fold_off[f + 1] - 1
};

struct CvSegments {
    int32_t F = 0;
    int64_t n = 0, n_pad = 0;
    std::vector<int64_t> count;    // [F] rows of fold f
    std::vector<int64_t> offset;   // [F + 1] first row of fold f in the padded layout (multiples of 4)
    std::vector<int64_t> src;      // [n_pad] source row of a gathered row, -1: padding (zero row)
    std::vector<int32_t> row_fold; // [n_pad] fold of a gathered row (padding: the fold it pads)
    CvChunks gram, rss;            // gram: padded rows, CV_GRAM_CHUNK; rss: true rows, CV_RSS_CHUNK
};

// "" when (n, k, F, labels) describe a valid cross-validation, else the reason (naming the fold).
// A fold must hold a row, and its training set (all other rows) at least k.
inline std::string cv_check(int64_t n, int32_t k, int32_t F, const int64_t* labels,
                            std::vector<int64_t>* count_out = nullptr) {
    if (n < 1) return "need n >= 1";
    if (k < 1 || k > CV_MAX_K)
        return "k must be between 1 and " + std::to_string(CV_MAX_K) + "; got " + std::to_string(k);
    if (F < CV_MIN_FOLDS || F > CV_MAX_FOLDS)
        return "n_folds must be between " + std::to_string(CV_MIN_FOLDS) + " and " +
               std::to_string(CV_MAX_FOLDS) + "; got " + std::to_string(F);
    if (!labels) return "fold labels must not be NULL";
    std::vector<int64_t> count(F, 0);
    for (int64_t i = 0; i < n; ++i) {
        if (labels[i] < 0 || labels[i] >= F)
            return "fold label " + std::to_string(labels[i]) + " of row " + std::to_string(i) +
                   " is outside 0 .. " + std::to_string(F - 1);
        ++count[labels[i]];
    }
    for (int32_t f = 0; f < F; ++f) {
        if (count[f] == 0) return "fold " + std::to_string(f) + " is empty";
        if (n - count[f] < k)
            return "fold " + std::to_string(f) + ": its training set has " + std::to_string(n - count[f]) +
                   " rows, fewer than k = " + std::to_string(k);
    }
    if (count_out) count_out->swap(count);
    return "";
}

inline void cv_cut(const std::vector<int64_t>& offset, const std::vector<int64_t>& rows_of, int chunk,
                   CvChunks& out) {
    const int32_t F = (int32_t)rows_of.size();
    out.fold_off.assign(F + 1, 0);
    for (int32_t f = 0; f < F; ++f) {
        for (int64_t r = 0; r < rows_of[f]; r += chunk) {
            out.row0.push_back(offset[f] + r);
            out.rows.push_back((int32_t)(rows_of[f] - r < chunk ? rows_of[f] - r : chunk));
        }
        out.fold_off[f + 1] = (int32_t)out.row0.size();
    }
}

// The stable permutation into fold order (rows of a fold keep their order), each fold padded with
// zero rows to a multiple of CV_ROW_PAD.  Labels must have passed cv_check.
inline CvSegments cv_segments(int64_t n, int32_t F, const int64_t* labels) {
    CvSegments s;
    s.F = F;
    s.n = n;
    s.count.assign(F, 0);
    for (int64_t i = 0; i < n; ++i) ++s.count[labels[i]];
    s.offset.assign(F + 1, 0);
    std::vector<int64_t> padded(F);
    for (int32_t f = 0; f < F; ++f) {
        padded[f] = (s.count[f] + CV_ROW_PAD - 1) / CV_ROW_PAD * CV_ROW_PAD;
        s.offset[f + 1] = s.offset[f] + padded[f];
    }
    s.n_pad = s.offset[F];
    s.src.assign(s.n_pad, -1);
    s.row_fold.assign(s.n_pad, 0);
    for (int32_t f = 0; f < F; ++f)
        for (int64_t r = s.offset[f]; r < s.offset[f + 1]; ++r) s.row_fold[r] = f;
    std::vector<int64_t> next(s.offset.begin(), s.offset.end() - 1);
    for (int64_t i = 0; i < n; ++i) s.src[next[labels[i]]++] = i;
    cv_cut(s.offset, padded, CV_GRAM_CHUNK, s.gram);
    cv_cut(s.offset, s.count, CV_RSS_CHUNK, s.rss);
    return s;
}

// ---- chains -> batches -> launches -----------------------------------------------------------------
// Chain (f, c) has the global index f * C + c.  A batch is a run of whole folds whose variates,
// rotated draws and kept draws are on the device together; its chains go out in launches of at
// most CV_MAX_CHAINS_PER_LAUNCH (a fold's chains may straddle two launches).
struct CvLaunch {
    int64_t chain0;     // global index of the first chain
    int32_t n_chains;
};
struct CvBatch {
    int32_t f0, f1;     // folds [f0, f1)
    std::vector<CvLaunch> launches;
};

inline int64_t cv_kept_draws(int64_t T, int64_t burn, int64_t thin) {
    return T > burn ? (T - burn + thin - 1) / thin : 0;
}

// device bytes of one chain: xi [T][k], gamma [T], rotated draws [T][k+1], kept draws [kept][k+1]
inline size_t cv_chain_bytes(int32_t k, int64_t T, int64_t kept) {
    return ((size_t)T * k + (size_t)T + (size_t)T * (k + 1) + (size_t)kept * (k + 1)) * 8;
}

// false: not even one fold's chains fit `budget` bytes (the caller: what is free once the gathered
// matrix, the fold tables and the per-fold set-up are on the device)
inline bool plan_cv_batches(int32_t F, int32_t C, size_t chain_bytes, size_t budget,
                            std::vector<CvBatch>& out) {
    out.clear();
    const size_t fold_bytes = chain_bytes * (size_t)C;
    if (fold_bytes == 0 || fold_bytes > budget) return false;
    size_t per = budget / fold_bytes;
    if (per > (size_t)F) per = (size_t)F;
    for (int32_t f0 = 0; f0 < F; f0 += (int32_t)per) {
        CvBatch b;
        b.f0 = f0;
        b.f1 = f0 + (int32_t)per < F ? f0 + (int32_t)per : F;
        const int64_t c0 = (int64_t)b.f0 * C, c1 = (int64_t)b.f1 * C;
        for (int64_t c = c0; c < c1; c += CV_MAX_CHAINS_PER_LAUNCH)
            b.launches.push_back(CvLaunch{c, (int32_t)(c1 - c < CV_MAX_CHAINS_PER_LAUNCH
                                                           ? c1 - c : CV_MAX_CHAINS_PER_LAUNCH)});
        out.push_back(b);
    }
    return true;
}

}  // namespace bmc
