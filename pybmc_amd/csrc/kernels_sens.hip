// Power-scaling sensitivity of a sampled fit: the prior or
// the likelihood raised to a power alpha near 1, the draws importance-reweighted with Pareto
// smoothing, the shift of every marginal measured by the cumulative Jensen-Shannon distance.
//   pad_points        A (either layout), y -> whole 64-point tiles and 16-column slabs, zero padded
//                     (launch_pad_points of kernels_waic.hip, called by the entry point)
//   sens_pad_draws    theta -> the coefficients in whole 64-draw tiles and 16-column slabs (pad_rows
//                     of bmc_score_tile.h)
//   sens_rss_tile     workgroup = 64 draws x ALL point tiles (the layout of ppc_tile_kernel):
//                     sum_i (y_i - a_i . beta_s)^2 on the f64 matrix cores, one fixed order.  Run
//                     twice: on the data (the likelihood) and on (L^-1, L^-1 b0), whose "residual
//                     sum" is the prior's quadratic form (beta - b0)' C0^-1 (beta - b0)
//   sens_logdens      lp_beta, lp_sigma2, loglik per draw and the component vectors
//   sens_consts_t / sens_tsum_tile / sens_logdens_t
//                     the same three under the Student-t likelihood, nu fixed or one per draw:
//                     the walk of sens_rss_tile with sum_i log1p(g_s r_is^2) in place of the
//                     squares, and a fourth log density, the prior of nu
//   sens_omega        the model-weight columns beta . Vt + 1 / M
//   sens_gather       a column -> (key, index) pairs of an even-length segment, OR / AND masks of
//                     the real keys, non-finite flag (launch_key_gather: the gather of
//                     kernels_rank.hip over a SensSource), then sens_pad_key: one pad key that
//                     sorts last when S is odd
//   sens_psis         workgroup = (component, alpha): tail of the sorted log density, generalised
//                     Pareto fit (bmc_psis.h, shared with loo_fit_kernel), smoothed tail,
//                     normalising sum -> weights [S][W], pareto_k
//   sens_chunk_sum / sens_chunk_scan / sens_cjs / sens_finish
//                     the weights gathered along a sorted column, prefix-summed (chunk sums, a
//                     serial scan of the chunks, then the chunk again from its offset), the
//                     integrals of the distance and the weighted moments
// The sort itself is launch_rank_sort_pass (kernels_rank.hip), unchanged.
// No float atomics: every sum has one order that depends on S alone, so two calls, any batching
// of the columns and any grid of alphas return the same bits.
#include "bmc_dev.h"
#include "bmc_launch.h"
#include "bmc_plan.h"
#include "bmc_psis.h"
#include "bmc_score_tile.h"

namespace bmc {

namespace {

static_assert(SENS_TILE == SCORE_TILE, "the plan's tile is the score tile");
constexpr double LN2 = 0.69314718055994530942;

__global__ __launch_bounds__(256) void sens_pad_draws_kernel(const double* __restrict__ theta, int64_t S,
                                                             int64_t ldt, int32_t k, int64_t S_pad,
                                                             int32_t k_pad, double* __restrict__ Tp) {
    pad_rows(theta, S, ldt, k, S_pad, k_pad, Tp);
}

// grid: one workgroup per draw tile.  A padded point has a zero row and a zero target: it adds
// exactly 0.  A wave owns 16 draws, a lane 4 draws x 4 points of every tile; the running sum of
// each draw stays in the lane's registers over the walk and the 16 lanes that share the draws
// meet once, in a tree, at the end.
__global__ __launch_bounds__(256, 2) void sens_rss_tile_kernel(
    const double* __restrict__ Tp, const double* __restrict__ Ap, const double* __restrict__ yo,
    int64_t n_pad, int32_t k, int32_t k_pad, int64_t point_tiles, int64_t S, double* __restrict__ rss) {
    __shared__ double As[SC_LDS_DOUBLES];
    __shared__ double Bs[SC_LDS_DOUBLES];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int cl = lane & 15, kq = lane >> 4;
    const int64_t d0 = (int64_t)blockIdx.x * SC_TM;
    double ee[4] = {0.0, 0.0, 0.0, 0.0};
    score_tile_loop(Tp, Ap, n_pad, (int64_t)k_pad, k, k_pad, d0, 0, point_tiles, As, Bs,
                    [&](int64_t i0, const f64x4(&acc)[4]) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const double yv = yo[i0 + cl + 16 * t];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double e = yv - acc[t][r];
                ee[r] = fma(e, e, ee[r]);
            }
        }
    });
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        double v = ee[r];
#pragma unroll
        for (int bit = 1; bit < 16; bit <<= 1) v += __shfl_xor(v, bit);
        const int64_t d = d0 + 16 * wave + kq + 4 * r;
        if (cl == 0 && d < S) rss[d] = v;
    }
}

// one thread per draw.  A draw with a non-finite coefficient or without a finite sigma > 0 has
// no log density: all three are NaN.
__global__ __launch_bounds__(256) void sens_logdens_kernel(
    const double* __restrict__ theta, int64_t S, int64_t ldt, int32_t k, const double* __restrict__ rss_lik,
    const double* __restrict__ rss_q, double n_points, double nu0, double sigma20, uint32_t components,
    double* __restrict__ lp, double* __restrict__ comps) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const double* th = theta + s * ldt;
    const double sigma = th[k];
    bool ok = is_finite(sigma) && sigma > 0.0;
    for (int32_t j = 0; j < k; ++j) ok = ok && is_finite(th[j]);
    const double nan = __builtin_nan("");
    double lb = nan, ls = nan, ll = nan;
    if (ok) {
        const double s2 = sigma * sigma;
        lb = -0.5 * rss_q[s];
        ls = -(nu0 / 2.0 + 1.0) * log(s2) - nu0 * sigma20 / (2.0 * s2);
        ll = -(n_points / 2.0) * (2.0 * HALF_LOG_2PI) - n_points * log(sigma) - rss_lik[s] / (2.0 * s2);
    }
    lp[s] = lb;
    lp[S + s] = ls;
    lp[2 * S + s] = ll;
    const double v[SENS_COMPONENTS] = {lb + ls, ll, lb, ls};
    int c = 0;
#pragma unroll
    for (int b = 0; b < SENS_COMPONENTS; ++b)
        if ((components >> b) & 1) comps[(int64_t)(c++) * S + s] = v[b];
}

// ---- the Student-t likelihood (SensLogdensArgs::per_draw) ----------------------
// one thread per draw: tc[0] = g = 1 / (nu sigma^2), tc[1] = hn = (nu + 1)/2, tc[2] = c = C(nu) -
// log sigma (the constants of score_consts_tv_kernel), tc[3] = nu, tc[4] = the log prior of nu, at
// the draw's own nu from tab [3][n_nu] = (C(nu), nu, log prior).  index NULL: entry 0 for every
// draw (a fixed nu is a table of one value); an index out of range is clamped and reported.
__global__ __launch_bounds__(256) void sens_consts_t_kernel(const double* __restrict__ theta, int64_t S,
                                                            int64_t ldt, int32_t k,
                                                            const double* __restrict__ tab, int32_t n_nu,
                                                            const int32_t* __restrict__ index,
                                                            int32_t* __restrict__ flag,
                                                            double* __restrict__ tc) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const int32_t iv = nu_index_clamped(index ? index[s] : 0, n_nu, flag);
    const double cnu = tab[iv], nu = tab[n_nu + iv];
    const double sg = theta[s * ldt + k];
    tc[s] = 1.0 / (nu * sg * sg);
    tc[S + s] = 0.5 * (nu + 1.0);
    tc[2 * S + s] = cnu - log(sg);
    tc[3 * S + s] = nu;
    tc[4 * S + s] = tab[2 * n_nu + iv];
}

// sens_rss_tile_kernel's walk with the Student-t term in place of the square: tsum[d] = sum_i
// log1p(g_d (y_i - a_i . beta_d)^2), g [S] = 1 / (nu_d sigma_d^2).  A padded point has e = 0 and
// adds log1p_nonneg(0 g) = 0 exactly for a finite g (tests/sens_t_plan_check.cpp); a draw with a NaN
// or infinite g has no log density anyway (sens_logdens_t_kernel).  One order of summation per
// (n, S), no atomics; the same code for a fixed nu and a nu per draw.
__global__ __launch_bounds__(256, 2) void sens_tsum_tile_kernel(
    const double* __restrict__ Tp, const double* __restrict__ Ap, const double* __restrict__ yo,
    int64_t n_pad, int32_t k, int32_t k_pad, int64_t point_tiles, int64_t S, const double* __restrict__ g,
    double* __restrict__ tsum) {
    __shared__ double As[SC_LDS_DOUBLES];
    __shared__ double Bs[SC_LDS_DOUBLES];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int cl = lane & 15, kq = lane >> 4;
    const int64_t d0 = (int64_t)blockIdx.x * SC_TM;
    double gr[4], tt[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t d = d0 + 16 * wave + kq + 4 * r;
        gr[r] = g[d < S ? d : S - 1];   // (a draw past S: its sum is dropped below)
    }
    score_tile_loop(Tp, Ap, n_pad, (int64_t)k_pad, k, k_pad, d0, 0, point_tiles, As, Bs,
                    [&](int64_t i0, const f64x4(&acc)[4]) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const double yv = yo[i0 + cl + 16 * t];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double e = yv - acc[t][r];
                tt[r] += log1p_nonneg((e * e) * gr[r]);
            }
        }
    });
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        double v = tt[r];
#pragma unroll
        for (int bit = 1; bit < 16; bit <<= 1) v += __shfl_xor(v, bit);
        const int64_t d = d0 + 16 * wave + kq + 4 * r;
        if (cl == 0 && d < S) tsum[d] = v;
    }
}

// sens_logdens_kernel under the Student-t likelihood: lp_beta and lp_sigma2 by its own expressions
// (the same bits), loglik = n c - hn tsum, lp_nu from the staged row; the same NaN rule, for all four.
__global__ __launch_bounds__(256) void sens_logdens_t_kernel(
    const double* __restrict__ theta, int64_t S, int64_t ldt, int32_t k, const double* __restrict__ tsum,
    const double* __restrict__ rss_q, const double* __restrict__ tc, double n_points, double nu0,
    double sigma20, uint32_t components, double* __restrict__ lp, double* __restrict__ comps) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const double* th = theta + s * ldt;
    const double sigma = th[k];
    bool ok = is_finite(sigma) && sigma > 0.0;
    for (int32_t j = 0; j < k; ++j) ok = ok && is_finite(th[j]);
    const double nan = __builtin_nan("");
    double lb = nan, ls = nan, ll = nan, ln = nan;
    if (ok) {
        const double s2 = sigma * sigma;
        lb = -0.5 * rss_q[s];
        ls = -(nu0 / 2.0 + 1.0) * log(s2) - nu0 * sigma20 / (2.0 * s2);
        ll = n_points * tc[2 * S + s] - tc[S + s] * tsum[s];
        ln = tc[4 * S + s];
    }
    lp[s] = lb;
    lp[S + s] = ls;
    lp[2 * S + s] = ll;
    lp[3 * S + s] = ln;
    const double v[SENS_T_COMPONENTS] = {(lb + ls) + ln, ll, lb, ls, ln};
    int c = 0;
#pragma unroll
    for (int b = 0; b < SENS_T_COMPONENTS; ++b)
        if ((components >> b) & 1) comps[(int64_t)(c++) * S + s] = v[b];
}

// one thread per (draw, model)
__global__ __launch_bounds__(256) void sens_omega_kernel(const double* __restrict__ theta, int64_t S,
                                                         int64_t ldt, int32_t k, const double* __restrict__ Vt,
                                                         int32_t M, double* __restrict__ omega) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= S * M) return;
    const int64_t s = e / M;
    const int32_t m = (int32_t)(e - s * M);
    const double* th = theta + s * ldt;
    double acc = 0.0;
    for (int32_t j = 0; j < k; ++j) acc = fma(th[j], Vt[(int64_t)j * M + m], acc);
    omega[e] = acc + 1.0 / (double)M;
}

// The pad of an odd-length segment: a key not below any real key that agrees with them on every
// digit they share, so that it adds no live pass; it starts last and a stable sort leaves it there.
__global__ void sens_pad_key_kernel(int32_t Pb, int64_t S, int64_t S_pad, const uint64_t* __restrict__ or_and,
                                    uint64_t* __restrict__ keys, uint32_t* __restrict__ idx) {
    const int32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= Pb || S_pad == S) return;
    const uint64_t o = or_and[2 * j], vary = o ^ or_and[2 * j + 1];
    uint64_t pad = o;
    for (int d = 0; d < RANK_PASSES; ++d)
        if ((vary >> (RANK_DIGIT_BITS * d)) & (RANK_DIGITS - 1))
            pad |= (uint64_t)(RANK_DIGITS - 1) << (RANK_DIGIT_BITS * d);
    keys[(int64_t)j * S_pad + S] = pad;
    idx[(int64_t)j * S_pad + S] = (uint32_t)S;
}

// [lo, hi): the run of keys equal to k[p] inside k[0, n)
__device__ __forceinline__ void run_of(const uint64_t* __restrict__ k, int64_t n, int64_t p, int64_t* lo,
                                       int64_t* hi) {
    const uint64_t v = k[p];
    int64_t a = 0, b = p;
    while (a < b) {
        const int64_t mid = a + ((b - a) >> 1);
        if (k[mid] < v) a = mid + 1; else b = mid;
    }
    *lo = a;
    a = p + 1, b = n;
    while (a < b) {
        const int64_t mid = a + ((b - a) >> 1);
        if (k[mid] <= v) a = mid + 1; else b = mid;
    }
    *hi = a;
}

// grid: W = components x alphas, workgroup w = c * n_alphas + a.  keys / idx: the sorted segment of
// every component, S_pad apart.  lw = (alpha - 1) lp shifted to a largest of 0; in ascending lw
// with ties in draw order (a stable sort of lw) the last M are the tail.  For alpha > 1 that is
// the sorted segment as it lies; for alpha < 1 it is the segment read backwards with every run of
// equal values turned round again (position p of a run [a, b) stands for a + b - 1 - p).
// xs: M doubles of scratch per workgroup.
__global__ __launch_bounds__(256) void sens_psis_kernel(
    const uint64_t* __restrict__ keys, const uint32_t* __restrict__ idx, int64_t S, int64_t S_pad, int32_t M,
    int32_t mg, int32_t n_alphas, const double* __restrict__ alphas, double* __restrict__ xs_all,
    double* __restrict__ Wt, double* __restrict__ khat_out) {
    __shared__ double red[256];
    __shared__ double g_theta[SENS_MAX_GRID], g_l[SENS_MAX_GRID], g_w[SENS_MAX_GRID];
    const int tid = threadIdx.x;
    const int32_t w = blockIdx.x, W = gridDim.x;
    const int32_t c = w / n_alphas;
    const double alpha = alphas[w - c * n_alphas];
    const uint64_t* k = keys + (int64_t)c * S_pad;
    const uint32_t* ix = idx + (int64_t)c * S_pad;
    double* xs = xs_all + (int64_t)w * (M > 0 ? M : 1);
    const bool up = alpha > 1.0;
    const double am1 = alpha - 1.0;
    const double inf = __builtin_inf();
    // sorted position of the u-th most extreme draw (u = 0: the largest lw)
    auto pos = [&](int64_t u) { return up ? S - 1 - u : u; };
    const double mx = am1 * rank_unkey(k[pos(0)]);
    auto lw_at = [&](int64_t p) { return am1 * rank_unkey(k[p]) - mx; };

    bool smooth = false;
    double ecut = 0.0;
    PsisFit fit{inf, 0.0, false};
    if (M >= PSIS_MIN_TAIL) {
        // ascending tail: lt[j] = lw of u = M - 1 - j; the cutoff is u = M
        smooth = lw_at(pos(M - 1)) != lw_at(pos(0));
        ecut = exp(lw_at(pos(M)));
    }
    if (smooth) {
        for (int j = tid; j < M; j += 256) xs[j] = exp(lw_at(pos(M - 1 - j))) - ecut;
        __syncthreads();
        // mg = psis_grid_points(M) <= SENS_MAX_GRID grid points
        fit = psis_fit(xs, M, mg, red, g_theta, g_l, g_w);
        if (!fit.finite) {
            fit.khat = inf;
            smooth = false;
        }
    }
    // the tail's weights exp(lw), smoothed and truncated at 0, into xs; then the sum over all draws
    double part = 0.0;
    if (smooth) {
        for (int j = tid; j < M; j += 256) {
            double lw = psis_smoothed_lw(j, M, fit, ecut);
            lw = lw > 0.0 ? 0.0 : lw;
            const double e = exp(lw);
            xs[j] = e;
            part += e;
        }
    }
    const int64_t n_tail = smooth ? M : 0;
    for (int64_t u = n_tail + tid; u < S; u += 256) part += exp(lw_at(pos(u)));
    __syncthreads();
    const double sum = block_sum(part, red);

    // which draw takes rank u: runs are turned round up to the end of the run that holds u = M - 1
    int64_t turn_end = 0;
    if (!up && smooth) {
        int64_t lo;
        run_of(k, S, M - 1, &lo, &turn_end);
    }
    for (int64_t u = tid; u < S; u += 256) {
        int64_t p = pos(u);
        const double e = u < n_tail ? xs[M - 1 - u] : exp(lw_at(p));
        if (u < turn_end) {
            int64_t lo, hi;
            run_of(k, S, p, &lo, &hi);
            p = lo + hi - 1 - p;
        }
        Wt[(int64_t)ix[p] * W + w] = e / sum;
    }
    if (tid == 0) khat_out[w] = fit.khat;
}

// The weights of a thread's SENS_ITEMS consecutive sorted draws, SENS_WG vectors from w0
__device__ __forceinline__ void load_weights(const double* __restrict__ Wt, const uint32_t (&d)[SENS_ITEMS],
                                             int n_mine, int32_t W, int32_t w0,
                                             double (&wv)[SENS_ITEMS][SENS_WG]) {
#pragma unroll
    for (int i = 0; i < SENS_ITEMS; ++i)
#pragma unroll
        for (int g = 0; g < SENS_WG; ++g)
            wv[i][g] = (i < n_mine && w0 + g < W) ? Wt[(int64_t)d[i] * W + w0 + g] : 0.0;
}

// grid: (chunks, Pb).  offs[jb][w][chunk] = the chunk's sum of weights: thread sums in position
// order, then a tree over the threads.
__global__ __launch_bounds__(SENS_BLOCK) void sens_chunk_sum_kernel(
    const uint32_t* __restrict__ idx, int64_t S, int64_t S_pad, int32_t W, const double* __restrict__ Wt,
    int64_t chunks, double* __restrict__ offs) {
    __shared__ double red[SENS_BLOCK];
    const int64_t chunk = blockIdx.x, jb = blockIdx.y;
    const int64_t p0 = chunk * SENS_CHUNK + (int64_t)threadIdx.x * SENS_ITEMS;
    const int64_t left = S - p0;
    const int n_mine = left >= SENS_ITEMS ? SENS_ITEMS : (left > 0 ? (int)left : 0);
    uint32_t d[SENS_ITEMS];
#pragma unroll
    for (int i = 0; i < SENS_ITEMS; ++i) d[i] = i < n_mine ? idx[jb * S_pad + p0 + i] : 0u;
    for (int32_t w0 = 0; w0 < W; w0 += SENS_WG) {
        double wv[SENS_ITEMS][SENS_WG];
        load_weights(Wt, d, n_mine, W, w0, wv);
#pragma unroll
        for (int g = 0; g < SENS_WG; ++g) {
            double s = 0.0;
#pragma unroll
            for (int i = 0; i < SENS_ITEMS; ++i) s += wv[i][g];
            const double tot = block_sum(s, red);
            if (threadIdx.x == 0 && w0 + g < W) offs[(jb * W + w0 + g) * chunks + chunk] = tot;
        }
    }
}

// one thread per (column, vector): the chunk sums -> their exclusive scan, in chunk order
__global__ void sens_chunk_scan_kernel(int64_t n_rows, int64_t chunks, double* __restrict__ offs) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    double* o = offs + r * chunks;
    double run = 0.0;
    for (int64_t c = 0; c < chunks; ++c) {
        const double v = o[c];
        o[c] = run;
        run += v;
    }
}

// grid: (chunks, Pb).  With Q_j the prefix sum of the weights along the sorted column, P_j = j / S,
// d_j the gap to the next sorted value, delta = Q - P and x0 the column's middle order statistic,
// part[jb][w][chunk][.] holds the chunk's sums of
//   0: P d    1: Q d    2: d (-P log1p(delta / 2P) + delta / 2) / ln 2
//   3: d (-Q log1p(-delta / 2Q) - delta / 2) / ln 2   (Q = 0: d P / (2 ln 2))
//   4: w (x - x0)    5: w (x - x0)^2
// each in position order in the thread, a butterfly over the wave, the four waves in order.
__global__ __launch_bounds__(SENS_BLOCK) void sens_cjs_kernel(
    const uint64_t* __restrict__ keys, const uint32_t* __restrict__ idx, int64_t S, int64_t S_pad, int32_t W,
    const double* __restrict__ Wt, int64_t chunks, const double* __restrict__ offs, double* __restrict__ part) {
    __shared__ double wtot[SENS_WG][SENS_BLOCK / 64];
    __shared__ double red[SENS_PART * SENS_WG][SENS_BLOCK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t chunk = blockIdx.x, jb = blockIdx.y;
    const uint64_t* k = keys + jb * S_pad;
    const int64_t p0 = chunk * SENS_CHUNK + (int64_t)threadIdx.x * SENS_ITEMS;
    const int64_t left = S - p0;
    const int n_mine = left >= SENS_ITEMS ? SENS_ITEMS : (left > 0 ? (int)left : 0);
    uint32_t d[SENS_ITEMS];
    double x[SENS_ITEMS + 1];
#pragma unroll
    for (int i = 0; i < SENS_ITEMS; ++i) d[i] = i < n_mine ? idx[jb * S_pad + p0 + i] : 0u;
#pragma unroll
    for (int i = 0; i <= SENS_ITEMS; ++i) {
        const int64_t p = p0 + i < S ? p0 + i : S - 1;   // (past the end: the last value, a gap of 0)
        x[i] = rank_unkey(k[p]);
    }
    const double x0 = rank_unkey(k[S / 2]);
    const double dS = (double)S;
    for (int32_t w0 = 0; w0 < W; w0 += SENS_WG) {
        double wv[SENS_ITEMS][SENS_WG];
        load_weights(Wt, d, n_mine, W, w0, wv);
        // the sum of the weights before this thread's draws, in the chunk
        double before[SENS_WG];
#pragma unroll
        for (int g = 0; g < SENS_WG; ++g) {
            double s = 0.0;
#pragma unroll
            for (int i = 0; i < SENS_ITEMS; ++i) s += wv[i][g];
            double inc = s;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const double v = __shfl_up(inc, o);
                if (lane >= o) inc += v;
            }
            if (lane == 63) wtot[g][wave] = inc;
            before[g] = inc - s;
        }
        __syncthreads();
        double acc[SENS_WG][SENS_PART];
#pragma unroll
        for (int g = 0; g < SENS_WG; ++g) {
            double base = w0 + g < W ? offs[(jb * W + w0 + g) * chunks + chunk] : 0.0;
            for (int v = 0; v < wave; ++v) base += wtot[g][v];
            double Q = base + before[g];
#pragma unroll
            for (int f = 0; f < SENS_PART; ++f) acc[g][f] = 0.0;
#pragma unroll
            for (int i = 0; i < SENS_ITEMS; ++i) {
                if (i < n_mine) {
                    const double wi = wv[i][g];
                    Q += wi;
                    const double P = (double)(p0 + i + 1) / dS;
                    const double gap = x[i + 1] - x[i];
                    const double delta = Q - P;
                    acc[g][0] += P * gap;
                    acc[g][1] += Q * gap;
                    acc[g][2] += gap * ((-P * log1p(delta / (2.0 * P)) + delta / 2.0) / LN2);
                    const double tq = Q == 0.0 ? P / 2.0 : -Q * log1p(-delta / (2.0 * Q)) - delta / 2.0;
                    acc[g][3] += gap * (tq / LN2);
                    const double xc = x[i] - x0;
                    acc[g][4] += wi * xc;
                    acc[g][5] += wi * xc * xc;
                }
            }
        }
#pragma unroll
        for (int g = 0; g < SENS_WG; ++g)
#pragma unroll
            for (int f = 0; f < SENS_PART; ++f) {
                const double s = lane_sum_ordered<64>(acc[g][f], lane);
                if (lane == 0) red[g * SENS_PART + f][wave] = s;
            }
        __syncthreads();
        if (threadIdx.x < SENS_WG * SENS_PART) {
            const int g = threadIdx.x / SENS_PART, f = threadIdx.x - g * SENS_PART;
            if (w0 + g < W) {
                const double* r = red[threadIdx.x];
                part[((jb * W + w0 + g) * chunks + chunk) * SENS_PART + f] = ((r[0] + r[1]) + r[2]) + r[3];
            }
        }
        __syncthreads();
    }
}

// one thread per (column, vector): the chunks' partial sums in chunk order -> cjs, mean, sd
__global__ void sens_finish_kernel(int64_t n_rows, int64_t chunks, int64_t S, int64_t S_pad, int32_t W,
                                   const uint64_t* __restrict__ keys, const double* __restrict__ part,
                                   double* __restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    double t[SENS_PART] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t c = 0; c < chunks; ++c)
#pragma unroll
        for (int f = 0; f < SENS_PART; ++f) t[f] += part[(r * chunks + c) * SENS_PART + f];
    const double a = t[2] < 0.0 ? 0.0 : t[2], b = t[3] < 0.0 ? 0.0 : t[3];   // (a NaN stays one)
    const double den = t[0] + t[1];
    const double x0 = rank_unkey(keys[(r / W) * S_pad + S / 2]);
    const double var = t[5] - t[4] * t[4];
    out[r * 3] = den == 0.0 ? 0.0 : sqrt((a + b) / den);
    out[r * 3 + 1] = x0 + t[4];
    out[r * 3 + 2] = sqrt(var < 0.0 ? 0.0 : var);
}

inline unsigned capped_blocks(int64_t elements) {
    int64_t blocks = (elements + 255) / 256;
    return (unsigned)(blocks > 8192 ? 8192 : (blocks < 1 ? 1 : blocks));
}

}  // namespace

hipError_t launch_sens_logdens(const SensLogdensArgs& a, hipStream_t s) {
    const int64_t S64 = (a.S + SENS_TILE - 1) / SENS_TILE * SENS_TILE;
    const NuPerDraw& v = a.per_draw;
    if (a.S < 1 || a.k < 1 || a.k > SENS_MAX_K || a.ldt < (int64_t)a.k + 1 || a.k_pad < a.k || a.k_pad % SC_KT ||
        a.n_pad < 1 || a.n_pad % SENS_TILE || a.q_pad < a.k || a.q_pad % SENS_TILE || a.S_pad != S64 ||
        S64 / SENS_TILE > 0x7fffffffll || a.components == 0 ||
        a.components >= (1u << (v.n_nu > 0 ? SENS_T_COMPONENTS : SENS_COMPONENTS)) ||
        !v.valid(0.0, SENS_MAX_NU_VALUES, true) || (v.n_nu > 0 && !a.tc))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(sens_pad_draws_kernel, dim3(capped_blocks(S64 * a.k_pad)), dim3(256), 0, s, a.theta, a.S,
                       a.ldt, a.k, S64, a.k_pad, a.Tp);
    const dim3 grid((unsigned)(S64 / SENS_TILE)), per_draw((unsigned)((a.S + 255) / 256));
    if (v.n_nu > 0) {
        hipLaunchKernelGGL(sens_consts_t_kernel, per_draw, dim3(256), 0, s, a.theta, a.S, a.ldt, a.k, v.tab,
                           v.n_nu, v.index, v.flag, a.tc);
        hipLaunchKernelGGL(sens_tsum_tile_kernel, grid, dim3(256), 0, s, (const double*)a.Tp, a.Ap, a.yo, a.n_pad,
                           a.k, a.k_pad, a.n_pad / SENS_TILE, a.S, (const double*)a.tc, a.rss);
    } else {
        hipLaunchKernelGGL(sens_rss_tile_kernel, grid, dim3(256), 0, s, (const double*)a.Tp, a.Ap, a.yo, a.n_pad,
                           a.k, a.k_pad, a.n_pad / SENS_TILE, a.S, a.rss);
    }
    hipLaunchKernelGGL(sens_rss_tile_kernel, grid, dim3(256), 0, s, (const double*)a.Tp, a.Lp, a.Ly, a.q_pad,
                       a.k, a.k_pad, a.q_pad / SENS_TILE, a.S, a.rss + a.S);
    if (v.n_nu > 0)
        hipLaunchKernelGGL(sens_logdens_t_kernel, per_draw, dim3(256), 0, s, a.theta, a.S, a.ldt, a.k,
                           (const double*)a.rss, (const double*)(a.rss + a.S), (const double*)a.tc, (double)a.n,
                           a.nu0, a.sigma20, a.components, a.lp, a.comps);
    else
        hipLaunchKernelGGL(sens_logdens_kernel, per_draw, dim3(256), 0, s, a.theta, a.S, a.ldt, a.k,
                           (const double*)a.rss, (const double*)(a.rss + a.S), (double)a.n, a.nu0, a.sigma20,
                           a.components, a.lp, a.comps);
    if (a.n_models > 0) {
        const int64_t total = a.S * a.n_models;
        if ((total + 255) / 256 > 0x7fffffffll) return hipErrorInvalidValue;
        hipLaunchKernelGGL(sens_omega_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a.theta,
                           a.S, a.ldt, a.k, a.Vt, a.n_models, a.omega);
    }
    return hipGetLastError();
}

hipError_t launch_sens_gather(const SensSource& src, int64_t S, int32_t col0, int32_t Pb, uint64_t* keys,
                              uint32_t* idx, uint64_t* or_and, uint32_t* flags, hipStream_t s) {
    if (S < 1 || S > SENS_MAX_S || Pb < 1 || col0 < 0) return hipErrorInvalidValue;
    const hipError_t e = launch_key_gather(src, S, sens_padded(S), col0, Pb, keys, idx, or_and, flags, s);
    if (e != hipSuccess) return e;   // (more workgroups than a grid holds)
    hipLaunchKernelGGL(sens_pad_key_kernel, dim3((Pb + 255) / 256), dim3(256), 0, s, Pb, S, sens_padded(S),
                       (const uint64_t*)or_and, keys, idx);
    return hipGetLastError();
}

hipError_t launch_sens_psis(const uint64_t* keys, const uint32_t* idx, int64_t S, int32_t n_components,
                            int32_t n_alphas, const double* d_alphas, double* xs, double* Wt, double* khat,
                            hipStream_t s) {
    const int64_t M = psis_tail_length(S);
    if (S < 2 || S > SENS_MAX_S || n_components < 1 || n_components > SENS_T_COMPONENTS || n_alphas < 1 ||
        n_alphas > SENS_MAX_ALPHAS || (M >= PSIS_MIN_TAIL && psis_grid_points(M) > SENS_MAX_GRID))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(sens_psis_kernel, dim3((unsigned)(n_components * n_alphas)), dim3(256), 0, s, keys, idx,
                       S, sens_padded(S), (int32_t)M, M >= PSIS_MIN_TAIL ? psis_grid_points(M) : 0, n_alphas,
                       d_alphas, xs, Wt, khat);
    return hipGetLastError();
}

hipError_t launch_sens_cjs(const uint64_t* keys, const uint32_t* idx, int64_t S, int32_t Pb, int32_t W,
                           const double* Wt, double* offs, double* part, double* out, hipStream_t s) {
    const int64_t chunks = sens_chunks(S), rows = (int64_t)Pb * W;
    if (S < 1 || S > SENS_MAX_S || Pb < 1 || Pb > 65535 || W < 1 || chunks > 0x7fffffffll)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)chunks, (unsigned)Pb);
    const int64_t S_pad = sens_padded(S);
    hipLaunchKernelGGL(sens_chunk_sum_kernel, grid, dim3(SENS_BLOCK), 0, s, idx, S, S_pad, W, Wt, chunks, offs);
    hipLaunchKernelGGL(sens_chunk_scan_kernel, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, s, rows, chunks,
                       offs);
    hipLaunchKernelGGL(sens_cjs_kernel, grid, dim3(SENS_BLOCK), 0, s, keys, idx, S, S_pad, W, Wt, chunks,
                       (const double*)offs, part);
    hipLaunchKernelGGL(sens_finish_kernel, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, s, rows, chunks, S,
                       S_pad, W, keys, (const double*)part, out);
    return hipGetLastError();
}

}  // namespace bmc
