// Launchers of the Student-t (outlier-robust) Gibbs sampler (kernels_robust.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmc_launch.h"
#include "bmc_robust_plan.h"

namespace bmc {

struct RobustArgs {
    const double* Z;      // [rows_padded][ldz]: X row-major, zero-padded columns and rows
    const double* yv;     // [rows_padded]: y, zero-padded
    int64_t n;            // true rows
    int32_t k;
    int64_t rows_per_wave;   // robust_rows_per_wave(n)
    const double* P;      // [k][k] prior precision inv(C0) (its lower triangle is read)
    const double* Pb0;    // [k] P b0
    double nu, shape_l;   // degrees of freedom; (nu + 1) / 2
    double nu0_s20, sigma2_init;
    int64_t iters, burn;
    int32_t n_chains;
    // per-chain arrays, chain 0 of the launch first
    const uint64_t* seeds;   // device RNG: the keys of the STREAM_ROBUST variates; NULL in replay mode
    const double* xi;     // [C][burn + iters][k]
    const double* gam;    // [C][burn + iters]
    const double* gl;     // replay mode: [C][burn + iters][n]
    double* ws;           // [C][n][2]: r_n, lambda_n
    double* samples;      // [C][iters][k + 1]
    double* wsum;         // [C][n]: mean of lambda_n over the kept sweeps
    int32_t* status;      // [C]: 1 = a Cholesky pivot was not positive and finite
    // nu on a grid (launch_robust_nu only; the fixed-nu kernels read none of these)
    const double* nu_tab; // [4][n_grid]: robust_nu_table
    int32_t n_grid, nu_init;
    const double* u_nu;   // replay mode: [C][burn + iters] uniforms of the pick; NULL in device RNG mode
    const int32_t* nu_path;  // replay mode: [C][burn + iters] the index in force after each sweep
    int32_t* nu_idx;      // [C][iters]: the index picked in each kept sweep
    double* tstat;        // [C][iters]: T_t = sum_n (log lambda_n - lambda_n), or NULL
};

// The folded form (bmc_kfold_cv_t): chains of DIFFERENT problems in one launch.
// One entry per fold of the batch, device memory:
struct RobustFold {
    const double* Z;       // [robust_rows_padded(n)][ldz]: the fold's training rows, packed as above
    const double* yv;      // [robust_rows_padded(n)]
    const double* nu_tab;  // [4][n_grid]: robust_nu_table at THIS n (nu on a grid only)
    int64_t n;             // training rows
    int64_t rows_per_wave; // robust_rows_per_wave(n)
    double sigma2_init;    // the OLS start value of the training rows
};
// Launch-wide: k, the prior, nu, the sweeps.  Per chain of the launch: its fold, the first row of its
// block of ws ([n][2]) and wsum ([n]) -- n differs between folds -- and, at the chain's index as in
// RobustArgs, seeds, xi, gam, samples, status, nu_idx and tstat.  Device RNG only.
struct RobustFoldedArgs {
    const RobustFold* fold;        // [folds of the batch]
    const int32_t* fold_of_chain;  // [C]: index into fold
    const int64_t* row0;           // [C]: rows, from ws / wsum
    int32_t k;
    const double* P;
    const double* Pb0;
    double nu, shape_l;
    double nu0_s20;
    int64_t iters, burn;
    int32_t n_chains;
    const uint64_t* seeds;
    const double* xi;      // [C][burn + iters][k]
    const double* gam;     // [C][burn + iters]: shape (nu0 + n of the chain's fold) / 2
    double* ws;
    double* samples;       // [C][iters][k + 1]
    double* wsum;
    int32_t* status;
    int32_t n_grid, nu_init;   // n_grid = 0: nu fixed
    int32_t* nu_idx;       // [C][iters]
    double* tstat;         // [C][iters] or NULL
};
// one workgroup per chain, a.n_chains <= ROBUST_MAX_CHAINS_PER_LAUNCH; a.n_grid > 0 draws nu
hipError_t launch_robust_folded(const RobustFoldedArgs& a, hipStream_t s);
// out[ch][s][0 .. width) = in[ch][s * thin][0 .. width), s < kept, of chains that hold rows_in rows
hipError_t launch_robust_thin(const double* in, int64_t chains, int64_t rows_in, int64_t thin, int64_t kept,
                              int32_t width, double* out, hipStream_t s);
hipError_t launch_robust_thin_idx(const int32_t* in, int64_t chains, int64_t rows_in, int64_t thin, int64_t kept,
                                  int32_t* out, hipStream_t s);

// panels (f64) -> Z, yv
hipError_t launch_robust_pack(const Panels& P, double* Z, double* yv, hipStream_t s);
// one workgroup per chain, a.n_chains <= ROBUST_MAX_CHAINS_PER_LAUNCH
hipError_t launch_robust(const RobustArgs& a, hipStream_t s);
// the same with nu drawn from its grid every sweep, 1 <= a.n_grid <= ROBUST_MAX_NU_GRID
hipError_t launch_robust_nu(const RobustArgs& a, hipStream_t s);

}  // namespace bmc
