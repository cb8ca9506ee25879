// Host-only plan of exact K-fold cross-validation under the Student-t likelihood (bmc_kfold_cv_t,
// bmc_kfold_cv_tv): the descriptor of every fold's packed training rows, the
// chains' blocks of row state, the batches of whole folds that fit a byte budget, their launches of
// at most ROBUST_MAX_CHAINS_PER_LAUNCH workgroups, the memory estimate and the argument checks.
// No HIP types: tests/cvt_plan_check.cpp compiles it with g++.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "bmc_cv_plan.h"
#include "bmc_robust_plan.h"

namespace bmc {

// Fold f of a batch.  Offsets are in doubles from the start of the batch's block of that kind: the
// packed rows Z [rows_padded][ldz] of every fold of the batch lie one after the other, then every
// fold's yv [rows_padded]; chain (f, c) owns rows row0 + c * n_train .. + n_train of the batch's ws
// ([.][2]) and wsum.
struct CvtFold {
    int32_t fold;
    int64_t n_train, rows_per_wave, rows_padded;
    int64_t z_off, yv_off;   // doubles
    int64_t row0;            // rows
};
struct CvtLaunch {
    int64_t chain0;          // local to the batch: chain (f, c) is (f - f0) * C + c
    int32_t n_chains;
};
struct CvtBatch {
    int32_t f0, f1;          // folds [f0, f1)
    std::vector<CvtFold> folds;
    std::vector<CvtLaunch> launches;
    int64_t z_len, yv_len;   // doubles of all packed rows and targets
    int64_t rows;            // rows of ws / wsum of all chains
};

// sweeps a chain keeps on the device: those after burn; every thin-th of them is a kept draw
inline int64_t cvt_sweeps_after_burn(int64_t T, int64_t burn) { return T > burn ? T - burn : 0; }

// Device bytes of fold f's part of a batch: the replicated rows (Z and yv); per chain xi [T][k], the
// sigma2 variates [T], the row state ws [n_train][2], the mean weights [n_train], the draws after
// burn [T - burn][k + 1] and the kept draws [kept][k + 1]; with nu on a grid the fold's table
// [4][n_grid] and per chain the indices after burn and the kept ones (int32).
inline size_t cvt_fold_bytes(int64_t n_train, int32_t k, int32_t C, int64_t T, int64_t burn, int64_t kept,
                             int32_t n_grid) {
    const size_t Ta = (size_t)cvt_sweeps_after_burn(T, burn);
    size_t chain = ((size_t)T * k + (size_t)T + (size_t)n_train * 3 + Ta * (k + 1) + (size_t)kept * (k + 1)) * 8;
    size_t fold = robust_packed_bytes(n_train, k);
    if (n_grid > 0) {
        chain += (Ta + (size_t)kept) * 4;
        fold += (size_t)4 * n_grid * 8;
    }
    return fold + chain * (size_t)C;
}

// Batches of whole folds under `budget` bytes, greedily in fold order.  false: fold *too_big alone
// needs *need bytes, more than the budget.
inline bool plan_cvt(int32_t F, int32_t C, int32_t k, const int64_t* count, int64_t n, int64_t T,
                     int64_t burn, int64_t kept, int32_t n_grid, size_t budget, std::vector<CvtBatch>& out,
                     int32_t* too_big = nullptr, size_t* need = nullptr) {
    out.clear();
    const int64_t ldz = robust_ldz(k);
    size_t used = 0;
    for (int32_t f = 0; f < F; ++f) {
        const int64_t nt = n - count[f];
        const size_t bytes = cvt_fold_bytes(nt, k, C, T, burn, kept, n_grid);
        if (bytes > budget) {
            if (too_big) *too_big = f;
            if (need) *need = bytes;
            out.clear();
            return false;
        }
        if (out.empty() || used + bytes > budget) {
            CvtBatch b;
            b.f0 = b.f1 = f;
            b.z_len = b.yv_len = b.rows = 0;
            out.push_back(b);
            used = 0;
        }
        CvtBatch& b = out.back();
        CvtFold d;
        d.fold = f;
        d.n_train = nt;
        d.rows_per_wave = robust_rows_per_wave(nt);
        d.rows_padded = robust_rows_padded(nt);
        d.z_off = b.z_len;
        d.yv_off = b.yv_len;
        d.row0 = b.rows;
        b.z_len += d.rows_padded * ldz;
        b.yv_len += d.rows_padded;
        b.rows += nt * C;
        b.folds.push_back(d);
        b.f1 = f + 1;
        used += bytes;
    }
    for (CvtBatch& b : out) {
        const int64_t nch = (int64_t)(b.f1 - b.f0) * C;
        for (int64_t c = 0; c < nch; c += ROBUST_MAX_CHAINS_PER_LAUNCH)
            b.launches.push_back(CvtLaunch{c, (int32_t)(nch - c < ROBUST_MAX_CHAINS_PER_LAUNCH
                                                            ? nch - c : ROBUST_MAX_CHAINS_PER_LAUNCH)});
    }
    return true;
}

// "" when the arguments describe a valid call, else the reason: the rules of bmc_kfold_cv at
// k <= ROBUST_MAX_K, then those of the Student-t sampler for every training set.  grid != NULL: nu on
// a grid (nu is not read).
inline std::string cvt_check(int64_t n, int32_t k, int32_t F, const int64_t* labels, int32_t C, int64_t iters,
                             int64_t burn, int64_t thin, double nu, const double* grid, const double* weight,
                             int32_t n_grid, int32_t nu_init, std::vector<int64_t>* count_out = nullptr) {
    if (k > ROBUST_MAX_K)
        return "the Student-t sampler supports 1 <= k <= " + std::to_string(ROBUST_MAX_K) + " columns; got " +
               std::to_string(k);
    std::vector<int64_t> count;
    std::string bad = cv_check(n, k, F, labels, &count);
    if (!bad.empty()) return bad;
    if (C < 1 || C > 65535) return "n_chains must be between 1 and 65535";
    if (iters < 1 || iters >= 0xffffffffll) return "iters must be between 1 and 2^32 - 2";
    if (burn < 0 || burn >= iters || thin < 1) return "need 0 <= burn < iters and thin >= 1";
    if ((int64_t)C * cv_kept_draws(iters, burn, thin) < 2) return "need at least 2 draws per fold after burn and thin";
    if (grid || weight || n_grid != 0) {
        bad = robust_nu_check(grid, weight, n_grid, nu_init);
        if (!bad.empty()) return bad;
        nu = grid[nu_init];
    }
    bad = robust_check(n, k, 0, nu, C, iters - burn, burn);
    if (!bad.empty()) return bad;
    if (count_out) count_out->swap(count);
    return "";
}

}  // namespace bmc
