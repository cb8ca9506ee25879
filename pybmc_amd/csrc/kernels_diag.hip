// Convergence diagnostics of sampled chains (split R-hat, ESS):
//   diag_moments         per split half-chain and column: mean and centred sum of squares,
//                        per row-split of the sequence (two passes over the split's rows)
//   diag_moments_merge   the row-splits of each sequence merged in a fixed order (Chan et al.)
//   diag_acov            sum_i d_i d_{i+t} for one block of lags, a tile of rows staged in LDS
//   diag_acov_reduce     the per-workgroup partials summed in a fixed order, averaged over the
//                        sequences: a(t) = mean_m acov_m(t), [n_active][lags] back to the host
// Input: samples [C][iters][ld] f64, column j < P (the samplers' layout: rows contiguous).
// No atomics anywhere: every sum has one fixed order, so two calls return the same bits.
// The launch plans (row splits, sequence groups, scratch sizes) are host-only: bmc_diag_plan.h.
#include "bmc_diag_plan.h"
#include "bmc_launch.h"

namespace bmc {

namespace {

// Sequence m: m < 2C is half (m & 1) of chain m >> 1 (n draws); 2C <= m < 3C is the middle draw
// of chain m - 2C when T' = iters - burn is odd (one draw: it counts for mean and sd only).
// Returns the first row in the flattened [C * iters] row space and the length.
__device__ inline int64_t seq_start(const DiagShape& d, int32_t m, int64_t& len) {
    if (m < 2 * d.C) {
        len = d.n;
        return (int64_t)(m >> 1) * d.iters + d.burn + (m & 1) * d.half_off;
    }
    len = 1;
    return (int64_t)(m - 2 * d.C) * d.iters + d.burn + d.n;
}

// Every value is taken relative to the column's first kept draw of chain 0: the estimator is
// shift-invariant, and the per-sequence means then carry no rounding of the column's magnitude
// (a column at 1e4 with sd 1e-2 would otherwise lose ~1e-12 of each mean, enough to move B/n).
__device__ inline double diag_shift(const DiagShape& d, int32_t col) {
    return d.x[d.burn * d.ld + col];
}

__device__ inline double wave_bcast(double v, int lane) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), lane);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
    return __hiloint2double(hi, lo);
}

// grid: n_seq * ncc * S; block (m, cc, s), s fastest.  Lane = column cc*64 + lane (a whole row
// per wave-instruction), wave w takes rows lo + w, lo + w + 4, ...
__global__ __launch_bounds__(DIAG_THREADS) void diag_moments_kernel(
    DiagShape d, int32_t ncc, int32_t S, int64_t rps, double* __restrict__ part) {
    __shared__ double red[4][64];
    __shared__ double mean_s[64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int32_t s = blockIdx.x % S;
    const int32_t cc = (blockIdx.x / S) % ncc;
    const int32_t m = blockIdx.x / S / ncc;
    const int32_t col = cc * 64 + lane;
    const bool valid = col < d.P;
    int64_t len;
    const int64_t start = seq_start(d, m, len);
    const int64_t lo = (int64_t)s * rps;
    const int64_t hi = lo + rps < len ? lo + rps : len;
    const int64_t cnt = hi > lo ? hi - lo : 0;
    const double* base = d.x + start * d.ld + (valid ? col : 0);
    const double sh = valid ? diag_shift(d, col) : 0.0;

    double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    int64_t r = lo + w;
    if (valid) {
        for (; r + 12 < hi; r += 16) {
            a0 += base[r * d.ld] - sh;
            a1 += base[(r + 4) * d.ld] - sh;
            a2 += base[(r + 8) * d.ld] - sh;
            a3 += base[(r + 12) * d.ld] - sh;
        }
        for (; r < hi; r += 4) a0 += base[r * d.ld] - sh;
    }
    red[w][lane] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (w == 0) {
        const double tot = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
        mean_s[lane] = cnt ? tot / (double)cnt : 0.0;
    }
    __syncthreads();
    const double ms = mean_s[lane];
    a0 = a1 = a2 = a3 = 0;
    r = lo + w;
    if (valid) {
        for (; r + 12 < hi; r += 16) {
            const double d0 = (base[r * d.ld] - sh) - ms, d1 = (base[(r + 4) * d.ld] - sh) - ms;
            const double d2 = (base[(r + 8) * d.ld] - sh) - ms, d3 = (base[(r + 12) * d.ld] - sh) - ms;
            a0 = fma(d0, d0, a0);
            a1 = fma(d1, d1, a1);
            a2 = fma(d2, d2, a2);
            a3 = fma(d3, d3, a3);
        }
        for (; r < hi; r += 4) {
            const double d0 = (base[r * d.ld] - sh) - ms;
            a0 = fma(d0, d0, a0);
        }
    }
    __syncthreads();
    red[w][lane] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (w == 0 && valid) {
        const double tot = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
        double* o = part + ((int64_t)m * S + s) * 2 * d.P;
        o[col] = ms;
        o[d.P + col] = tot;
    }
}

// one thread per (sequence, column): the S row-splits merged in order (count, mean, M2)
__global__ __launch_bounds__(DIAG_THREADS) void diag_moments_merge_kernel(
    DiagShape d, int32_t S, int64_t rps, const double* __restrict__ part,
    double* __restrict__ mean, double* __restrict__ m2) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)d.n_seq * d.P) return;
    const int32_t m = (int32_t)(e / d.P), col = (int32_t)(e % d.P);
    int64_t len;
    (void)seq_start(d, m, len);
    double na = 0, mu = 0, M2 = 0;
    for (int32_t s = 0; s < S; ++s) {
        const int64_t lo = (int64_t)s * rps;
        const int64_t hi = lo + rps < len ? lo + rps : len;
        if (hi <= lo) break;
        const double nb = (double)(hi - lo);
        const double* p = part + ((int64_t)m * S + s) * 2 * d.P;
        const double mb = p[col], M2b = p[d.P + col];
        if (na == 0) {
            na = nb, mu = mb, M2 = M2b;
            continue;
        }
        const double nt = na + nb, delta = mb - mu;
        mu += delta * (nb / nt);
        M2 += M2b + delta * delta * (na * nb / nt);
        na = nt;
    }
    mean[e] = mu;
    m2[e] = M2;
    if (m == 0) mean[(int64_t)d.n_seq * d.P + col] = diag_shift(d, col);
}

// grid: MG * ncc * nlc * S; block (g, cc, lc, s), s fastest.  Sequences g*spg .. of the 2C
// halves, columns cols[cc*16 ..], lags tc = t0 + lc*64 + lane, rows of split s in tiles of R.
// Per tile: b rows [r0 + tc, r0 + tc + R + 64) and a rows [r0, r0 + R), centred, column-major in
// LDS (lane-contiguous b reads: no bank conflict); a value broadcast by readlane.
__global__ __launch_bounds__(DIAG_THREADS) void diag_acov_kernel(
    DiagShape d, const double* __restrict__ mean, const int32_t* __restrict__ cols,
    int32_t n_active, int32_t ncc, int64_t t0, int32_t nlc, int32_t spg, int32_t S, int64_t rps,
    double* __restrict__ partial) {
    __shared__ double as[DIAG_CW][DIAG_R + 1];
    __shared__ double bs[DIAG_CW][DIAG_R + DIAG_LC + 1];
    __shared__ int32_t col_s[DIAG_CW];
    __shared__ double mu_s[DIAG_CW], sh_s[DIAG_CW];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int32_t b = blockIdx.x;
    const int32_t s = b % S;
    b /= S;
    const int32_t lc = b % nlc;
    b /= nlc;
    const int32_t cc = b % ncc;
    const int32_t g = b / ncc;
    const int64_t tc = t0 + (int64_t)lc * DIAG_LC;
    const int64_t n = d.n;
    const int64_t lo = (int64_t)s * rps;
    const int64_t hi = lo + rps < n ? lo + rps : n;
    const int32_t m_end = (g + 1) * spg < 2 * d.C ? (g + 1) * spg : 2 * d.C;

    double acc[4] = {0, 0, 0, 0};
    for (int32_t m = g * spg; m < m_end; ++m) {
        int64_t len;
        const int64_t start = seq_start(d, m, len);
        __syncthreads();   // (the previous sequence's last tile is read)
        if (threadIdx.x < DIAG_CW) {
            const int32_t a = cc * DIAG_CW + threadIdx.x;
            const int32_t gc = a < n_active ? cols[a] : -1;
            col_s[threadIdx.x] = gc;
            mu_s[threadIdx.x] = gc >= 0 ? mean[(int64_t)m * d.P + gc] : 0.0;
            sh_s[threadIdx.x] = gc >= 0 ? diag_shift(d, gc) : 0.0;
        }
        __syncthreads();
        const double* xs = d.x + start * d.ld;
        for (int64_t r0 = lo; r0 < hi; r0 += DIAG_R) {
            if (r0 > lo) __syncthreads();
            for (int e = threadIdx.x; e < (DIAG_R + DIAG_LC) * DIAG_CW; e += DIAG_THREADS) {
                const int c = e & (DIAG_CW - 1), i = e / DIAG_CW;
                const int64_t r = r0 + tc + i;
                const int32_t gc = col_s[c];
                bs[c][i] = (gc >= 0 && r < n) ? (xs[r * d.ld + gc] - sh_s[c]) - mu_s[c] : 0.0;
            }
            if (tc == 0) {
                __syncthreads();
                for (int e = threadIdx.x; e < DIAG_R * DIAG_CW; e += DIAG_THREADS) {
                    const int c = e & (DIAG_CW - 1), i = e / DIAG_CW;
                    as[c][i] = r0 + i < hi ? bs[c][i] : 0.0;
                }
            } else {
                for (int e = threadIdx.x; e < DIAG_R * DIAG_CW; e += DIAG_THREADS) {
                    const int c = e & (DIAG_CW - 1), i = e / DIAG_CW;
                    const int64_t r = r0 + i;
                    const int32_t gc = col_s[c];
                    as[c][i] = (gc >= 0 && r < hi) ? (xs[r * d.ld + gc] - sh_s[c]) - mu_s[c] : 0.0;
                }
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c = w + 4 * q;
                if (col_s[c] < 0) continue;   // (wave-uniform)
                double sacc = acc[q];
                for (int i0 = 0; i0 < DIAG_R; i0 += 64) {
                    const double av = as[c][i0 + lane];
                    const double* bp = &bs[c][i0 + lane];
#pragma unroll
                    for (int r = 0; r < 64; ++r) sacc = fma(wave_bcast(av, r), bp[r], sacc);
                }
                acc[q] = sacc;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
        partial[((int64_t)blockIdx.x * DIAG_CW + w + 4 * q) * DIAG_LC + lane] = acc[q];
}

// grid: n_active * nlc; block (a, lc).  Wave w sums the partials of groups q = w, w+4, ... in
// order, then the four waves in order; out[a][lc*64 + lane] = sum / n / (2C).
__global__ __launch_bounds__(DIAG_THREADS) void diag_acov_reduce_kernel(
    const double* __restrict__ partial, int32_t nlc, int32_t ncc, int32_t MG, int32_t S,
    double n, double M, double* __restrict__ out) {
    __shared__ double red[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int32_t lc = blockIdx.x % nlc, a = blockIdx.x / nlc;
    const int32_t cc = a / DIAG_CW, c = a % DIAG_CW;
    double sum = 0;
    for (int32_t q = w; q < MG * S; q += 4) {
        const int32_t g = q / S, s = q % S;
        const int64_t wg = s + (int64_t)S * (lc + (int64_t)nlc * (cc + (int64_t)ncc * g));
        sum += partial[(wg * DIAG_CW + c) * DIAG_LC + lane];
    }
    red[w][lane] = sum;
    __syncthreads();
    if (w == 0)
        out[((int64_t)a * nlc + lc) * DIAG_LC + lane] =
            (((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane]) / n / M;
}

}  // namespace

size_t diag_moments_scratch(const DiagShape& d) {
    return moment_scratch_bytes(moment_plan(d.n_seq, d.P, d.n), d.n_seq, d.P);
}

hipError_t launch_diag_moments(const DiagShape& d, double* scratch, double* mean, double* m2,
                               hipStream_t s) {
    const MomentPlan p = moment_plan(d.n_seq, d.P, d.n);
    hipLaunchKernelGGL(diag_moments_kernel, dim3((unsigned)((int64_t)d.n_seq * p.ncc * p.S)),
                       dim3(DIAG_THREADS), 0, s, d, p.ncc, p.S, p.rps, scratch);
    const int64_t total = (int64_t)d.n_seq * d.P;
    hipLaunchKernelGGL(diag_moments_merge_kernel, dim3((unsigned)diag_cdiv(total, DIAG_THREADS)),
                       dim3(DIAG_THREADS), 0, s, d, p.S, p.rps, (const double*)scratch, mean, m2);
    return hipGetLastError();
}

size_t diag_acov_scratch(const DiagShape& d, int32_t n_active, int64_t n_lags) {
    return acov_scratch_bytes(acov_plan(d.C, d.n, n_active, n_lags));
}

hipError_t launch_diag_acov(const DiagShape& d, const double* mean, const int32_t* cols,
                            int32_t n_active, int64_t t0, int64_t n_lags, double* scratch,
                            double* acov_out, hipStream_t s) {
    const AcovPlan p = acov_plan(d.C, d.n, n_active, n_lags);
    hipLaunchKernelGGL(diag_acov_kernel, dim3((unsigned)acov_groups(p)), dim3(DIAG_THREADS), 0, s, d,
                       mean, cols, n_active, p.ncc, t0, p.nlc, p.spg, p.S, p.rps, scratch);
    hipLaunchKernelGGL(diag_acov_reduce_kernel, dim3((unsigned)((int64_t)n_active * p.nlc)),
                       dim3(DIAG_THREADS), 0, s, (const double*)scratch, p.nlc, p.ncc, p.MG, p.S,
                       (double)d.n, (double)(2 * d.C), acov_out);
    return hipGetLastError();
}

}  // namespace bmc
