// Launchers of kernels_cv.hip: exact K-fold / leave-group-out cross-validation.
// Every pointer is device memory; the layouts are those of bmc_cv_plan.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmc_cv_plan.h"
#include "bmc_cvpath_plan.h"

namespace bmc {

// Z[r][j] (n_pad x ldz, row-major) = [A | y | 0] of source row src[r], a zero row where src[r] < 0;
// ys[r] = the y of that row.  A: element (i, j) at i*lda + j, or j*lda + i when col_major.
hipError_t launch_cv_gather(const double* A, const double* y, int64_t lda, int col_major, int32_t k,
                            const int64_t* src, int64_t n_pad, double* Z, double* ys, hipStream_t s);

// Gram [A y]'[A y] of every fold's own rows: gram[f] is (k+1) x (k+1), row-major, symmetric.
// chunk_row0 / chunk_rows / fold_off: CvSegments::gram; partial: n_chunks * pairs * 256 doubles,
// pairs = tiles (tiles + 1) / 2.
hipError_t launch_cv_fold_gram(const double* Z, int32_t k, int32_t n_folds, const int64_t* chunk_row0,
                               const int32_t* chunk_rows, int32_t n_chunks, const int32_t* fold_off,
                               double* partial, double* gram, hipStream_t s);

// partial[c][b] = sum over the rows i of chunk c of (y_i - a_i . beta_b)^2, b < nb, rows in order
// (chunks: CvSegments::rss; beta [nb][k]).
hipError_t launch_cv_block_rss(const double* Z, int32_t k, const double* beta, int32_t nb,
                               const int64_t* chunk_row0, const int32_t* chunk_rows, int32_t n_chunks,
                               double* partial, hipStream_t s);

// The body of gibbs_gram_kernel for chains of DIFFERENT problems: chain blockIdx.x of the launch
// is the global chain chain0 + blockIdx.x, of fold (chain0 + blockIdx.x) / chains_per_fold, and
// its variates and draws are the chain local0 + blockIdx.x of xi, gam and uout.
struct CvGramArgs {
    int32_t k, chains_per_fold;
    int64_t chain0, local0;
    const double* G;      // [F][k][k]  W'AW of the fold's training rows
    const double* lam;    // [F][k]
    const double* c1;     // [F][k]
    const double* c2;     // [F][k]
    const double* u0;     // [F][k]
    const double* g0;     // [F][k]
    const double* scal;   // [F][4]: rss0, sigma2_init, nu0 * sigma20, unused
    const double* xi;     // [chains of the batch][T][k]
    const double* gam;    // [chains of the batch][T]
    double* uout;         // [chains of the batch][T][k+1]
    int64_t iters;
    int32_t n_chains;     // chains in THIS launch
};
hipError_t launch_cv_gram(const CvGramArgs& a, hipStream_t s);

// out[ch][s][0..k) = W_f u[ch][burn + s*thin][0..k), out[ch][s][k] = u[..][k], s < kept, for the
// `chains` chains of a batch whose first fold is fold0 (f = fold0 + ch / chains_per_fold);
// WT [F][k][k] holds every W transposed, as launch_unrotate takes it.
hipError_t launch_cv_unrotate(const double* u, const double* WT, int32_t k, int32_t chains_per_fold,
                              int32_t fold0, int64_t chains, int64_t T, int64_t burn, int64_t thin,
                              int64_t kept, double* out, hipStream_t s);

// bbar[fold0 + b][j] = mean over the S = chains_per_fold * kept pooled draws of fold b of the
// batch of coefficient j < k (fixed order)
hipError_t launch_cv_colmean(const double* draws, int32_t k, int64_t S, int32_t folds, int32_t fold0,
                             double* bbar, hipStream_t s);

// mean[r] = Z[r][0..k) . bbar[row_fold[r]]; ldz the leading dimension of Z (cv_ldz of the width it
// was gathered at)
hipError_t launch_cv_mean(const double* Z, int32_t ldz, int32_t k, const int32_t* row_fold,
                          const double* bbar, int64_t n_pad, double* mean, hipStream_t s);

// The chains of a component path (bmc_cv_path; the plan in bmc_cvpath_plan.h): block b of the launch
// is local chain l = chain0 + b of the batch, chain l % chains_per_problem of problem
// l / chains_per_problem, and runs the body of cv_gram_kernel<kmax> on what desc[] names.  Every
// chain of a launch has cv_kmax(k) == kmax.
struct CvPathArgs {
    const CvPathDesc* desc;   // [problems of the batch], device
    int32_t chains_per_problem, kmax;
    int64_t chain0;
    const double *G, *lam, *c1, *c2, *u0, *g0, *scal;   // set-up arrays of all problems
    const double *xi, *gam;   // the batch's variates
    double* uout;             // the batch's rotated draws
    int64_t iters;
    int32_t n_chains;         // chains in THIS launch
};
hipError_t launch_cv_path(const CvPathArgs& a, hipStream_t s);

}  // namespace bmc
