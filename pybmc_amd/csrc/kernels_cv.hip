// gfx950 kernels of exact K-fold / leave-group-out cross-validation (bmc_kfold_cv).
//
// The rows are gathered once into fold order, [A | y | 0-pad] per row, every fold padded with zero
// rows to whole MFMA k-steps.  From that one matrix:
//   * cv_fold_gram_kernel   the Gram [A y]'[A y] of every fold's OWN rows with
//                           v_mfma_f64_16x16x4_f64, upper-triangle tiles, fixed-order partial sums
//                           (the host takes total - own: the training statistics of every fold);
//   * cv_block_rss_kernel   R[b][chunk] = sum over the chunk's rows of (y_i - a_i . beta_b)^2 for all
//                           coefficient vectors at once: non-negative sums, nothing cancels;
//   * cv_gram_kernel        gibbs_gram_kernel for F x C chains of F different problems, one wave
//                           per chain, every per-problem quantity indexed by the chain's fold;
//   * cv_path_kernel        the same chain body for problems of different widths (the component
//                           path, bmc_cv_path): each chain finds its problem through a descriptor;
//   * cv_unrotate_kernel    the kept draws back in the coefficient basis, per-fold W;
//   * cv_colmean_kernel, cv_mean_kernel   the held-out predictive mean a_i . mean_s beta_s.
// The held-out log predictive densities come from the score kernels (kernels_waic.hip) on a fold's
// row segment and draws.
#include "bmc_cv.h"
#include "bmc_dev.h"

namespace bmc {

namespace {

using f64x4 = __attribute__((ext_vector_type(4))) double;

// ---- draw and sigma2 step ---------------------------------------------------------------------------
// The arithmetic of draw_u and sigma2_step of kernels_gibbs.hip, operation for operation (that file
// explains it): a cross-validation chain must be the chain the loop kernels run on the same rows.
__device__ __forceinline__ double rsqrt_pos(double x) {
    const double y0 = __builtin_amdgcn_rsq(x);
    const double e = fma(-x * y0, y0, 1.0);
    return fma(y0 * e, fma(e, 0.375, 0.5), y0);
}
__device__ __forceinline__ double draw_u(double lam, double c1, double c2, double xi, double sp,
                                         double g) {
    const double D = fma(lam, g, sp);
    const double r = rsqrt_pos(D);
    const double rs = rsqrt_pos(sp);
    const double m = fma(c2, g, c1 * sp);
    return fma(r * r, m, ((sp * rs) * r) * xi);
}
struct Sigma2 {
    double sp, g;   // sigma2 = sp / g
};
__device__ __forceinline__ Sigma2 sigma2_step(double nu0_s20, double rss, double gam_t) {
    const double scale_post = (nu0_s20 + rss) * 0.5;
    const bool floor_hit = scale_post < 1e-6 * gam_t;
    return Sigma2{floor_hit ? 1e-6 : scale_post, floor_hit ? 1.0 : gam_t};
}

// ---- gather -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cv_gather_kernel(const double* __restrict__ A,
                                                        const double* __restrict__ y, int64_t lda,
                                                        int col_major, int32_t k,
                                                        const int64_t* __restrict__ src, int64_t n_pad,
                                                        int32_t ldz, double* __restrict__ Z,
                                                        double* __restrict__ ys) {
    const int64_t total = n_pad * ldz;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const int64_t r = e / ldz;
        const int32_t j = (int32_t)(e - r * ldz);
        const int64_t i = src[r];
        double v = 0.0;
        if (i >= 0 && j <= k) v = j == k ? y[i] : (col_major ? A[(int64_t)j * lda + i] : A[i * lda + j]);
        Z[e] = v;
        if (j == k) ys[r] = v;
    }
}

// ---- Gram of every fold's own rows --------------------------------------------------------------------
// One wave per chunk of at most CV_GRAM_CHUNK rows of one fold (a multiple of 4: the padding rows
// are zero), all tile pairs: every row is read once.  Per k-step of 4 rows lane l loads
// Z[row0 + (l >> 4)][16 t + (l & 15)] for every column tile t -- that one value is both the A operand
// of tile row t (A[i = l & 15][k = l >> 4]) and the B operand of tile column t
// (B[k = l >> 4][j = l & 15]) -- and issues one MFMA per pair (ti, tj >= ti).  D: col = l & 15,
// row = (l >> 4) + 4 reg.  partial[chunk][pair][16 x 16].
template <int NT>
__global__ __launch_bounds__(64) void cv_fold_gram_kernel(const double* __restrict__ Z, int32_t ldz,
                                                          const int64_t* __restrict__ chunk_row0,
                                                          const int32_t* __restrict__ chunk_rows,
                                                          double* __restrict__ partial) {
    constexpr int NP = NT * (NT + 1) / 2;
    const int lane = threadIdx.x, kq = lane >> 4, cl = lane & 15;
    const int64_t row0 = chunk_row0[blockIdx.x];
    const int32_t nr = chunk_rows[blockIdx.x];
    f64x4 acc[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) acc[p] = f64x4{0.0, 0.0, 0.0, 0.0};
    const double* z = Z + (row0 + kq) * ldz + cl;
    for (int32_t r = 0; r < nr; r += 4) {
        double v[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) v[t] = z[(int64_t)r * ldz + 16 * t];
        int p = 0;
#pragma unroll
        for (int ti = 0; ti < NT; ++ti)
#pragma unroll
            for (int tj = ti; tj < NT; ++tj, ++p)
                acc[p] = __builtin_amdgcn_mfma_f64_16x16x4f64(v[ti], v[tj], acc[p], 0, 0, 0);
    }
    double* out = partial + (size_t)blockIdx.x * NP * 256;
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int i = 0; i < 4; ++i) out[(size_t)p * 256 + (kq + 4 * i) * 16 + cl] = acc[p][i];
}

// gram[f][i][j], i, j <= k: the chunks of fold f added in chunk order; element (i, j) and its mirror
// are the same sum.  One workgroup per fold.
__global__ __launch_bounds__(256) void cv_fold_gram_reduce_kernel(const double* __restrict__ partial,
                                                                  const int32_t* __restrict__ fold_off,
                                                                  int32_t nt, int32_t ka,
                                                                  double* __restrict__ gram) {
    const int f = blockIdx.x, np = nt * (nt + 1) / 2;
    const int32_t c0 = fold_off[f], c1 = fold_off[f + 1];
    for (int e = threadIdx.x; e < ka * ka; e += blockDim.x) {
        const int i = e / ka, j = e - i * ka;
        const int a = i < j ? i : j, b = i < j ? j : i;
        const int ti = a >> 4, tj = b >> 4;
        const int p = ti * nt - ti * (ti - 1) / 2 + (tj - ti);
        const int idx = (a & 15) * 16 + (b & 15);
        double s = 0.0;
        for (int32_t c = c0; c < c1; ++c) s += partial[((size_t)c * np + p) * 256 + idx];
        gram[(size_t)f * ka * ka + e] = s;
    }
}

// ---- block sums of squared residuals ------------------------------------------------------------------
// Lane = coefficient vector b (its k coefficients in registers), the rows of the chunk one after the
// other (wave-uniform addresses: the row is read once and broadcast).  Per row the residual is the
// chain acc = y, acc = fma(-x_j, beta_j, acc), j ascending, as in the loop kernels; rows are added
// into two accumulators in row order.
template <int KMAX>
__global__ __launch_bounds__(64) void cv_block_rss_kernel(const double* __restrict__ Z, int32_t ldz,
                                                          int32_t k, const double* __restrict__ beta,
                                                          int32_t nb,
                                                          const int64_t* __restrict__ chunk_row0,
                                                          const int32_t* __restrict__ chunk_rows,
                                                          double* __restrict__ partial) {
    const int b = blockIdx.y * 64 + threadIdx.x;
    const bool have = b < nb;
    double bj[KMAX];
#pragma unroll
    for (int j = 0; j < KMAX; ++j) bj[j] = (have && j < k) ? beta[(size_t)b * k + j] : 0.0;
    const int64_t row0 = chunk_row0[blockIdx.x];
    const int32_t nr = chunk_rows[blockIdx.x];
    double part0 = 0.0, part1 = 0.0;
    for (int32_t r = 0; r < nr; ++r) {
        const double* z = Z + (row0 + r) * ldz;
        double acc = z[k];
#pragma unroll
        for (int j = 0; j < KMAX; ++j)
            if (j < k) acc = fma(-z[j], bj[j], acc);
        if (r & 1) part1 = fma(acc, acc, part1);
        else part0 = fma(acc, acc, part0);
    }
    if (have) partial[(size_t)blockIdx.x * nb + b] = part0 + part1;
}

// ---- all chains of all folds ----------------------------------------------------------------------------
// gibbs_gram_kernel (kernels_gibbs.hip explains the iteration, the 64-row output staging and the
// deferred sigma roots) for ONE chain of width K <= KMAX, one wave: its variates xi [T][K] and gam
// [T], its rotated draws uout [T][K+1], and its problem's G [K][K], k-vectors and scal (rss0,
// sigma2_init, nu0 * sigma20).  The body of cv_gram_kernel and cv_path_kernel: a chain of the
// component path is the chain bmc_kfold_cv runs on the leading columns, operation for operation.
template <int KMAX>
__device__ __forceinline__ void cv_chain(const int K, const int64_t T_it, const double* __restrict__ xi,
                                         const double* __restrict__ gam, double* __restrict__ uout,
                                         const double* __restrict__ Gf, const double* __restrict__ lamv,
                                         const double* __restrict__ c1v, const double* __restrict__ c2v,
                                         const double* __restrict__ u0v, const double* __restrict__ g0v,
                                         const double* __restrict__ scal) {
    __shared__ double d_lds[64];
    __shared__ double rows[64 * (KMAX + 1)];
    const int lane = threadIdx.x;
    const bool act = lane < K;
    double grow[KMAX];   // row `lane` of G
#pragma unroll
    for (int i = 0; i < KMAX; ++i) grow[i] = (act && i < K) ? Gf[(size_t)lane * K + i] : 0.0;
    const double lam = act ? lamv[lane] : 0.0, c1 = act ? c1v[lane] : 0.0;
    const double c2 = act ? c2v[lane] : 0.0, u0 = act ? u0v[lane] : 0.0;
    const double g0x2 = act ? 2.0 * g0v[lane] : 0.0;
    const double rss0 = scal[0], sigma2_init = scal[1];
    const double nu0_s20 = scal[2];
    d_lds[lane] = 0.0;
    double sp_eff = sigma2_init, g_eff = 1.0;
    double sp_cap = 1.0, g_cap = 1.0;   // lane i: the (sp, g) pair behind staged row i
    double xi_next = (act && T_it > 0) ? xi[lane] : 0.0;
    double gam_next = T_it > 0 ? gam[0] : 1.0;
    const int K1 = K + 1;
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): see gibbs_wave_kernel
    for (int64_t t = 0; t < T_it; ++t) {
        const int slot = (int)(t & 63);
        const double u = draw_u(lam, c1, c2, xi_next, sp_eff, g_eff);
        const double gam_t = gam_next;
        {
            const int64_t tn = t + 1 < T_it ? t + 1 : t;
            xi_next = act ? xi[tn * K + lane] : 0.0;
            gam_next = gam[tn];
        }
        if (act) rows[slot * K1 + lane] = u;
        const double d = u - u0;
        d_lds[lane] = d;
        double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
#pragma unroll
        for (int i = 0; i < KMAX; i += 4) {
            acc0 = fma(grow[i], d_lds[i], acc0);
            acc1 = fma(grow[i + 1], d_lds[i + 1], acc1);
            acc2 = fma(grow[i + 2], d_lds[i + 2], acc2);
            acc3 = fma(grow[i + 3], d_lds[i + 3], acc3);
        }
        const double gd = (acc0 + acc1) + (acc2 + acc3);
        const double q = wave_sum(d * (gd - g0x2));
        double rss = rss0 + q;
        rss = rss > 0.0 ? rss : 0.0;
        const Sigma2 s2 = sigma2_step(nu0_s20, rss, gam_t);
        sp_eff = s2.sp;
        g_eff = s2.g;
        const bool mine = lane == slot;
        sp_cap = mine ? sp_eff : sp_cap;
        g_cap = mine ? g_eff : g_cap;
        if (slot == 63 || t + 1 == T_it) {
            const int nrows = slot + 1;
            const double sig = sqrt(sp_cap / g_cap);
            if (lane < nrows) rows[lane * K1 + K] = sig;
            double* dst = uout + (t - slot) * K1;
            for (int idx = lane; idx < nrows * K1; idx += 64) dst[idx] = rows[idx];
        }
    }
}

// F x C chains of F problems of one width: every per-problem quantity is the chain's fold's; the
// base pointers are formed once, in front of the loop.
template <int KMAX>
__global__ __launch_bounds__(64) void cv_gram_kernel(CvGramArgs a) {
    const int K = a.k;
    if ((int)blockIdx.x >= a.n_chains) return;
    const int64_t fold = (a.chain0 + blockIdx.x) / a.chains_per_fold;
    const int64_t local = a.local0 + blockIdx.x;
    const int64_t T_it = a.iters;
    const int64_t fk = fold * K;
    cv_chain<KMAX>(K, T_it, a.xi + local * T_it * K, a.gam + local * T_it, a.uout + local * T_it * (K + 1),
                   a.G + fk * K, a.lam + fk, a.c1 + fk, a.c2 + fk, a.u0 + fk, a.g0 + fk, a.scal + fold * 4);
}

// The chains of a component path: problems of DIFFERENT widths within one width class, each
// found through its descriptor (bmc_cvpath_plan.h).
template <int KMAX>
__global__ __launch_bounds__(64) void cv_path_kernel(CvPathArgs a) {
    if ((int)blockIdx.x >= a.n_chains) return;
    const int64_t l = a.chain0 + blockIdx.x;
    const int64_t p = l / a.chains_per_problem, c = l - p * a.chains_per_problem;
    const CvPathDesc d = a.desc[p];
    const int K = d.k;
    const int64_t T_it = a.iters;
    cv_chain<KMAX>(K, T_it, a.xi + d.xi_off + c * T_it * K, a.gam + d.gam_off + c * T_it,
                   a.uout + d.u_off + c * T_it * (K + 1), a.G + d.g_off, a.lam + d.v_off, a.c1 + d.v_off,
                   a.c2 + d.v_off, a.u0 + d.v_off, a.g0 + d.v_off, a.scal + d.s_off);
}

// ---- kept draws in the coefficient basis ------------------------------------------------------------------
// unrotate_kernel (kernels_setup.hip) with the fold's W' and the burn / thin selection: fixed i
// order, so a draw has the bits launch_unrotate gives it under the same W.
__global__ __launch_bounds__(256) void cv_unrotate_kernel(const double* __restrict__ u,
                                                          const double* __restrict__ WT, int32_t K,
                                                          int32_t chains_per_fold, int32_t fold0,
                                                          int64_t chains, int64_t T, int64_t burn,
                                                          int64_t thin, int64_t kept,
                                                          double* __restrict__ out) {
    const int64_t total = chains * kept * (K + 1);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const int64_t r = e / (K + 1);
        const int32_t j = (int32_t)(e - r * (K + 1));
        const int64_t ch = r / kept, s = r - ch * kept;
        const double* ur = u + (ch * T + burn + s * thin) * (K + 1);
        double v;
        if (j == K) {
            v = ur[K];
        } else {
            const double* wt = WT + (size_t)(fold0 + ch / chains_per_fold) * K * K;
            v = 0.0;
            for (int i = 0; i < K; ++i) v = fma(wt[(size_t)i * K + j], ur[i], v);
        }
        out[e] = v;
    }
}

// ---- held-out predictive mean -----------------------------------------------------------------------------
// Workgroup (j, b): the mean of coefficient j over the S pooled draws of fold b of the batch.  Thread
// t adds draws t, t + 256, .. in order; the 256 partial sums meet in a fixed tree through LDS.
__global__ __launch_bounds__(256) void cv_colmean_kernel(const double* __restrict__ draws, int32_t K,
                                                         int64_t S, int32_t fold0,
                                                         double* __restrict__ bbar) {
    __shared__ double part[256];
    const int j = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    const double* d = draws + (size_t)b * S * (K + 1) + j;
    double s = 0.0;
    for (int64_t i = t; i < S; i += 256) s += d[i * (K + 1)];
    part[t] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) part[t] += part[t + w];
        __syncthreads();
    }
    if (t == 0) bbar[(size_t)(fold0 + b) * K + j] = part[0] / (double)S;
}

__global__ __launch_bounds__(256) void cv_mean_kernel(const double* __restrict__ Z, int32_t ldz,
                                                      int32_t K, const int32_t* __restrict__ row_fold,
                                                      const double* __restrict__ bbar, int64_t n_pad,
                                                      double* __restrict__ mean) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_pad) return;
    const double* z = Z + r * ldz;
    const double* b = bbar + (size_t)row_fold[r] * K;
    double m = 0.0;
    for (int j = 0; j < K; ++j) m = fma(z[j], b[j], m);
    mean[r] = m;
}

unsigned blocks_for(int64_t total, int per, int64_t most) {
    int64_t b = (total + per - 1) / per;
    if (b > most) b = most;
    return (unsigned)(b < 1 ? 1 : b);
}

}  // namespace

hipError_t launch_cv_gather(const double* A, const double* y, int64_t lda, int col_major, int32_t k,
                            const int64_t* src, int64_t n_pad, double* Z, double* ys, hipStream_t s) {
    if (k < 1 || k > CV_MAX_K || n_pad < 1) return hipErrorInvalidValue;
    const int32_t ldz = cv_ldz(k);
    hipLaunchKernelGGL(cv_gather_kernel, dim3(blocks_for(n_pad * ldz, CV_STRIDE_THREADS, CV_STRIDE_BLOCKS)),
                       dim3(256), 0, s, A, y, lda, col_major, k, src, n_pad, ldz, Z, ys);
    return hipGetLastError();
}

hipError_t launch_cv_fold_gram(const double* Z, int32_t k, int32_t n_folds, const int64_t* chunk_row0,
                               const int32_t* chunk_rows, int32_t n_chunks, const int32_t* fold_off,
                               double* partial, double* gram, hipStream_t s) {
    if (k < 1 || k > CV_MAX_K || n_chunks < 1 || n_folds < 1) return hipErrorInvalidValue;
    const int32_t ldz = cv_ldz(k), nt = cv_tiles(k);
    const dim3 grid((unsigned)n_chunks), block(64);
    switch (nt) {
    case 1: hipLaunchKernelGGL(cv_fold_gram_kernel<1>, grid, block, 0, s, Z, ldz, chunk_row0, chunk_rows, partial); break;
    case 2: hipLaunchKernelGGL(cv_fold_gram_kernel<2>, grid, block, 0, s, Z, ldz, chunk_row0, chunk_rows, partial); break;
    case 3: hipLaunchKernelGGL(cv_fold_gram_kernel<3>, grid, block, 0, s, Z, ldz, chunk_row0, chunk_rows, partial); break;
    case 4: hipLaunchKernelGGL(cv_fold_gram_kernel<4>, grid, block, 0, s, Z, ldz, chunk_row0, chunk_rows, partial); break;
    default: hipLaunchKernelGGL(cv_fold_gram_kernel<5>, grid, block, 0, s, Z, ldz, chunk_row0, chunk_rows, partial); break;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(cv_fold_gram_reduce_kernel, dim3((unsigned)n_folds), dim3(256), 0, s, partial,
                       fold_off, nt, k + 1, gram);
    return hipGetLastError();
}

hipError_t launch_cv_block_rss(const double* Z, int32_t k, const double* beta, int32_t nb,
                               const int64_t* chunk_row0, const int32_t* chunk_rows, int32_t n_chunks,
                               double* partial, hipStream_t s) {
    if (k < 1 || k > CV_MAX_K || nb < 1 || n_chunks < 1) return hipErrorInvalidValue;
    const int32_t ldz = cv_ldz(k);
    const dim3 grid((unsigned)n_chunks, (unsigned)((nb + 63) / 64)), block(64);
    switch (cv_kmax(k)) {
    case 8: hipLaunchKernelGGL(cv_block_rss_kernel<8>, grid, block, 0, s, Z, ldz, k, beta, nb, chunk_row0, chunk_rows, partial); break;
    case 16: hipLaunchKernelGGL(cv_block_rss_kernel<16>, grid, block, 0, s, Z, ldz, k, beta, nb, chunk_row0, chunk_rows, partial); break;
    case 32: hipLaunchKernelGGL(cv_block_rss_kernel<32>, grid, block, 0, s, Z, ldz, k, beta, nb, chunk_row0, chunk_rows, partial); break;
    default: hipLaunchKernelGGL(cv_block_rss_kernel<64>, grid, block, 0, s, Z, ldz, k, beta, nb, chunk_row0, chunk_rows, partial); break;
    }
    return hipGetLastError();
}

hipError_t launch_cv_gram(const CvGramArgs& a, hipStream_t s) {
    if (a.k < 1 || a.k > CV_MAX_K || a.n_chains < 1 || a.n_chains > CV_MAX_CHAINS_PER_LAUNCH ||
        a.chains_per_fold < 1)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)a.n_chains), block(64);
    switch (cv_kmax(a.k)) {
    case 8: hipLaunchKernelGGL(cv_gram_kernel<8>, grid, block, 0, s, a); break;
    case 16: hipLaunchKernelGGL(cv_gram_kernel<16>, grid, block, 0, s, a); break;
    case 32: hipLaunchKernelGGL(cv_gram_kernel<32>, grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL(cv_gram_kernel<64>, grid, block, 0, s, a); break;
    }
    return hipGetLastError();
}

hipError_t launch_cv_unrotate(const double* u, const double* WT, int32_t k, int32_t chains_per_fold,
                              int32_t fold0, int64_t chains, int64_t T, int64_t burn, int64_t thin,
                              int64_t kept, double* out, hipStream_t s) {
    if (chains < 1 || kept < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cv_unrotate_kernel,
                       dim3(blocks_for(chains * kept * (k + 1), CV_STRIDE_THREADS, CV_STRIDE_BLOCKS)), dim3(256),
                       0, s, u, WT, k, chains_per_fold, fold0, chains, T, burn, thin, kept, out);
    return hipGetLastError();
}

hipError_t launch_cv_colmean(const double* draws, int32_t k, int64_t S, int32_t folds, int32_t fold0,
                             double* bbar, hipStream_t s) {
    if (folds < 1 || S < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cv_colmean_kernel, dim3((unsigned)k, (unsigned)folds), dim3(256), 0, s, draws, k, S,
                       fold0, bbar);
    return hipGetLastError();
}

hipError_t launch_cv_mean(const double* Z, int32_t ldz, int32_t k, const int32_t* row_fold,
                          const double* bbar, int64_t n_pad, double* mean, hipStream_t s) {
    if (k < 1 || ldz < k) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cv_mean_kernel, dim3(blocks_for(n_pad, 256, (int64_t)1 << 30)), dim3(256), 0, s, Z,
                       ldz, k, row_fold, bbar, n_pad, mean);
    return hipGetLastError();
}

hipError_t launch_cv_path(const CvPathArgs& a, hipStream_t s) {
    if (!a.desc || a.n_chains < 1 || a.n_chains > CV_MAX_CHAINS_PER_LAUNCH || a.chains_per_problem < 1 ||
        a.chain0 < 0 || a.iters < 1)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)a.n_chains), block(64);
    switch (a.kmax) {
    case 8: hipLaunchKernelGGL(cv_path_kernel<8>, grid, block, 0, s, a); break;
    case 16: hipLaunchKernelGGL(cv_path_kernel<16>, grid, block, 0, s, a); break;
    case 32: hipLaunchKernelGGL(cv_path_kernel<32>, grid, block, 0, s, a); break;
    case 64: hipLaunchKernelGGL(cv_path_kernel<64>, grid, block, 0, s, a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace bmc
