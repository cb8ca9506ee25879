// Pointwise log predictive density of a sampled fit: for design
// rows A (n x k), targets y and draws theta = (beta_s, sigma_s),
//   ll[i][s] = -1/2 log(2 pi) - log sigma_s - (y_i - a_i . beta_s)^2 / (2 sigma_s^2)
// and per point i, over the S draws: logsumexp_s ll - log S, var_s ll (ddof 1), mean_s ll.
//
//   pad_points     A (either layout, any lda) and y -> whole 64-point tiles and 16-column slabs,
//                  zero in the padding; with an offset row for kernels_ppc.hip (launch_pad_points:
//                  the one staging kernel of launch_score, launch_ppc and the sensitivity)
//   score_consts   per draw: c_s = -1/2 log(2 pi) - log sigma_s,  h_s = 1 / (2 sigma_s^2)
//                  (score_consts_t: the constants of the Student-t density, ScoreArgs::nu > 0;
//                  score_consts_tv: the same at a nu per draw, ScoreArgs::per_draw)
//   score_tile     workgroup = 64 points x the draw tiles of one split.  a_i . beta_s on
//                  v_mfma_f64_16x16x4_f64 (the tile loop of bmc_score_tile.h, shared with
//                  kernels_loo.hip); the tile is reduced in the epilogue
//                  and never stored: per lane and point an online log-sum-exp (running max, one
//                  rescale per tile) and a mean / centred-M2 pair merged tile by tile (Chan et
//                  al.); the 16 lanes that share a point merge at the end of the split
//   score_merge    per point: the splits' partials (max, sumexp, count, mean, M2) merged in split
//                  order, then lppd = max + log(sumexp) - log S, p_waic = M2 / (S - 1), mean
//
// No atomics: every sum has one fixed order (lane, tile, lane tree, split), so two calls return
// the same bits.  Non-finite inputs propagate by the arithmetic alone: a NaN in a_i or y_i
// reaches every ll[i][.], a NaN in theta or a sigma_s <= 0 reaches ll[.][s] of every point (the
// running max ignores a NaN, the sums do not).
#include "bmc_dev.h"
#include "bmc_launch.h"
#include "bmc_plan.h"
#include "bmc_score_tile.h"

namespace bmc {

namespace {

// (max, sum of exp(ll - max), count, mean, centred sum of squares) of a set of draws
struct LlState {
    double m, L, cnt, mean, M2;
};

// The union of two disjoint sets, a's draws before b's.  An empty side (a lane or a split that
// saw no draw: m = -inf, L = 0) returns the other one untouched.
__device__ __forceinline__ LlState ll_merge(const LlState& a, const LlState& b) {
    LlState r;
    r.m = fmax(a.m, b.m);
    r.L = a.L * exp(a.m - r.m) + b.L * exp(b.m - r.m);
    r.cnt = a.cnt + b.cnt;
    const double d = b.mean - a.mean;
    r.mean = fma(d, b.cnt / r.cnt, a.mean);
    r.M2 = (a.M2 + b.M2) + d * d * (a.cnt * b.cnt / r.cnt);
    if (b.cnt == 0.0) return a;
    if (a.cnt == 0.0) return b;
    return r;
}

// OFFSET_ROW: yo has a second row, the offsets (zeros without one)
template <bool OFFSET_ROW>
__global__ __launch_bounds__(256) void pad_points_kernel(
    const double* __restrict__ A, const double* __restrict__ y, const double* __restrict__ offset,
    int64_t n, int32_t k, int64_t lda, int32_t col_major, int64_t n_pad, int32_t k_pad,
    double* __restrict__ Ap, double* __restrict__ yo) {
    const int64_t total = n_pad * k_pad;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const int64_t i = e / k_pad;
        const int32_t j = (int32_t)(e - i * k_pad);
        double v = 0.0;
        if (i < n && j < k) v = col_major ? A[(int64_t)j * lda + i] : A[i * lda + j];
        Ap[e] = v;
        if (j == 0) {
            yo[i] = i < n ? y[i] : 0.0;
            if constexpr (OFFSET_ROW) yo[n_pad + i] = (i < n && offset != nullptr) ? offset[i] : 0.0;
        }
    }
}

__global__ __launch_bounds__(256) void score_consts_kernel(const double* __restrict__ theta,
                                                           int64_t S, int64_t ldt, int32_t k,
                                                           double* __restrict__ ch) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const double sg = theta[s * ldt + k];
    ch[s] = -HALF_LOG_2PI - log(sg);
    ch[S + s] = 1.0 / (2.0 * sg * sg);
}

// the Student-t constants of TileDrawsT: cnu = lgamma((nu + 1)/2) - lgamma(nu/2) - 1/2 log(nu pi)
__global__ __launch_bounds__(256) void score_consts_t_kernel(const double* __restrict__ theta,
                                                             int64_t S, int64_t ldt, int32_t k,
                                                             double cnu, double nu,
                                                             double* __restrict__ ch) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const double sg = theta[s * ldt + k];
    ch[s] = cnu - log(sg);
    ch[S + s] = 1.0 / (nu * sg * sg);
}

// the constants of TileDrawsTV: those of score_consts_t_kernel at the draw's own nu, gathered from the
// table of distinct values; an index out of range is clamped and reported through flag
__global__ __launch_bounds__(256) void score_consts_tv_kernel(const double* __restrict__ theta,
                                                              int64_t S, int64_t ldt, int32_t k,
                                                              const double* __restrict__ tab,
                                                              int32_t n_nu,
                                                              const int32_t* __restrict__ index,
                                                              int32_t* __restrict__ flag,
                                                              double* __restrict__ ch) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const int32_t iv = nu_index_clamped(index[s], n_nu, flag);
    const double cnu = tab[iv], nu = tab[n_nu + iv];
    const double sg = theta[s * ldt + k];
    ch[s] = cnu - log(sg);
    ch[S + s] = 1.0 / (nu * sg * sg);
    ch[2 * S + s] = 0.5 * (nu + 1.0);
}

// The running state of one point in one lane; the count is the lane's (the same for its 4 points).
struct LlRun {
    double m, L, mean, M2;
};

// One 64-draw tile into the lane's running state of ONE point: x[t] = ll of draw cl + 16 t, nb of
// them exist (ok[t]); w1 = nb / (cnt + nb) and w2 = cnt w1 are Chan's weights for joining nb
// draws to cnt.  FULL: all four exist.
template <bool FULL>
__device__ __forceinline__ void score_fold(LlRun& st, const double (&x)[4], const bool (&ok)[4],
                                           double nb, double w1, double w2) {
    double mt = -__builtin_inf(), sum = 0.0;
#pragma unroll
    for (int t = 0; t < 4; ++t)
        if (FULL || ok[t]) {
            mt = fmax(mt, x[t]);
            sum += x[t];
        }
    const double mn = fmax(st.m, mt);
    double se = 0.0;
#pragma unroll
    for (int t = 0; t < 4; ++t)
        if (FULL || ok[t]) se += exp(x[t] - mn);
    st.L = fma(st.L, exp(st.m - mn), se);   // (first tile: L = 0, exp(-inf) = 0)
    st.m = mn;
    const double mb = FULL ? sum * 0.25 : sum / nb;
    double m2b = 0.0;
#pragma unroll
    for (int t = 0; t < 4; ++t)
        if (FULL || ok[t]) {
            const double e = x[t] - mb;
            m2b = fma(e, e, m2b);
        }
    const double d = mb - st.mean;
    st.mean = fma(d, w1, st.mean);
    st.M2 = (st.M2 + m2b) + d * d * w2;
}

// grid: splits * point_tiles, point tile fastest: the workgroups that run together walk the SAME
// draws (one split) over different points, so each XCD's L2 fetches a slab of theta once for
// all of them; the A tiles (64 x k_pad each) stay in L2 for the whole launch.
// <D, L...>: the draws type and its scalars lik (bmc_score_tile.h).
template <class D, class... L>
__global__ __launch_bounds__(256) void score_tile_kernel(
    const double* __restrict__ Ap, const double* __restrict__ yp, const double* __restrict__ theta,
    const double* __restrict__ ch, int64_t S, int64_t ldt, int32_t k, int32_t k_pad,
    uint32_t point_tiles, int64_t tiles_per_split, int64_t draw_tiles, int64_t n_pad,
    double* __restrict__ part, L... lik) {
    __shared__ double As[SC_LDS_DOUBLES];
    __shared__ double Bs[SC_LDS_DOUBLES];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t pt = blockIdx.x % point_tiles;
    const int64_t split = blockIdx.x / point_tiles;
    const int64_t p0 = (int64_t)pt * SC_TM;
    const int64_t dt0 = split * tiles_per_split;
    const int64_t dt1 = dt0 + tiles_per_split < draw_tiles ? dt0 + tiles_per_split : draw_tiles;
    const int cl = lane & 15, kq = lane >> 4;

    // this lane's four points: rows 16 wave + kq + 4 r of the tile (MFMA D: row = kq + 4 reg)
    double yv[4];
    LlRun st[4];
    double cnt = 0.0;   // draws this lane has folded
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        yv[r] = yp[p0 + 16 * wave + kq + 4 * r];
        st[r] = LlRun{-__builtin_inf(), 0.0, 0.0, 0.0};
    }

    // epilogue: ll (D::ll) for the lane's 4 points x 4 draws, folded into the running state of
    // each point
    score_tile_loop(Ap, theta, S, ldt, k, k_pad, p0, dt0, dt1, As, Bs,
                    [&](int64_t s0, const f64x4(&acc)[4]) {
        const D d(ch, S, s0, cl, lik...);
        const bool full = s0 + SC_TM <= S;   // wave-uniform
        const double nb = (double)((int)d.ok[0] + (int)d.ok[1] + (int)d.ok[2] + (int)d.ok[3]);
        if (nb > 0.0) {   // (not a lane whose draws of the last tile are all past S)
            const double w1 = nb / (cnt + nb), w2 = cnt * w1;
            cnt += nb;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double x[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) x[t] = d.ll(yv[r], acc[t][r], t);
                if (full) score_fold<true>(st[r], x, d.ok, nb, w1, w2);
                else score_fold<false>(st[r], x, d.ok, nb, w1, w2);
            }
        }
    });

    // the 16 lanes (cl) that hold draws of the same four points: a tree over cl, the lower lane's
    // draws first, so every lane ends with the same bits; lane cl = 0 writes them
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        LlState me{st[r].m, st[r].L, cnt, st[r].mean, st[r].M2};
#pragma unroll
        for (int bit = 1; bit < 16; bit <<= 1) {
            LlState o;
            o.m = __shfl_xor(me.m, bit);
            o.L = __shfl_xor(me.L, bit);
            o.cnt = __shfl_xor(me.cnt, bit);
            o.mean = __shfl_xor(me.mean, bit);
            o.M2 = __shfl_xor(me.M2, bit);
            me = (cl & bit) ? ll_merge(o, me) : ll_merge(me, o);
        }
        if (cl == 0) {
            double* o = part + ((int64_t)split * n_pad + p0 + 16 * wave + kq + 4 * r) * 5;
            o[0] = me.m;
            o[1] = me.L;
            o[2] = me.cnt;
            o[3] = me.mean;
            o[4] = me.M2;
        }
    }
}

__global__ __launch_bounds__(256) void score_merge_kernel(const double* __restrict__ part,
                                                          int64_t n, int64_t n_pad, int64_t splits,
                                                          int64_t S, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    auto load = [&](int64_t sp) {
        const double* p = part + (sp * n_pad + i) * 5;
        return LlState{p[0], p[1], p[2], p[3], p[4]};
    };
    LlState st = load(0);
    for (int64_t sp = 1; sp < splits; ++sp) st = ll_merge(st, load(sp));
    out[i] = st.m + (log(st.L) - log((double)S));
    out[n + i] = st.M2 / (double)(S - 1);
    out[2 * n + i] = st.mean;
}

}  // namespace

ScoreBuffers score_buffers(const ScorePlan& p, int64_t n_draws) {
    const size_t n_pad = (size_t)p.point_tiles * SC_TM;
    ScoreBuffers b;
    b.Ap = n_pad * (size_t)p.k_pad * 8;
    b.yp = n_pad * 8;
    b.ch = (size_t)n_draws * 3 * 8;   // (the third row: TileDrawsTV only)
    b.part = (size_t)p.splits * n_pad * 5 * 8;
    return b;
}

hipError_t launch_pad_points(const double* A, const double* y, const double* offset, bool offset_row,
                             int64_t n, int32_t k, int64_t lda, int32_t col_major, int64_t n_pad,
                             int32_t k_pad, double* Ap, double* yo, hipStream_t s) {
    if (n < 1 || k < 1 || n_pad < n || n_pad % SC_TM || k_pad < k || k_pad % SC_KT)
        return hipErrorInvalidValue;
    int64_t blocks = (n_pad * k_pad + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    if (offset_row)
        hipLaunchKernelGGL(pad_points_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, A, y, offset, n,
                           k, lda, col_major, n_pad, k_pad, Ap, yo);
    else
        hipLaunchKernelGGL(pad_points_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, A, y, offset, n,
                           k, lda, col_major, n_pad, k_pad, Ap, yo);
    return hipGetLastError();
}

hipError_t launch_score(const ScoreArgs& a, const ScorePlan& p, hipStream_t s) {
    if (a.n < 1 || a.S < 2 || a.k < 1 || a.k > SCORE_MAX_K || a.ldt < a.k + 1 ||
        a.lda < (a.col_major ? a.n : (int64_t)a.k) || !(a.nu >= 0.0 && a.nu < __builtin_inf()) ||
        !a.per_draw.valid(a.nu, INT32_MAX) || p.k_pad < a.k || p.k_pad % SC_KT != 0 ||
        p.point_tiles != (a.n + SC_TM - 1) / SC_TM || p.draw_tiles != (a.S + SC_TM - 1) / SC_TM ||
        p.splits < 1 || p.tiles_per_split < 1 || p.splits * p.tiles_per_split < p.draw_tiles ||
        (p.splits - 1) * p.tiles_per_split >= p.draw_tiles)
        return hipErrorInvalidValue;
    const uint64_t groups = (uint64_t)p.splits * (uint64_t)p.point_tiles;
    if (groups > 0x7fffffffull || p.point_tiles > 0x7fffffffll) return hipErrorInvalidValue;
    const int64_t n_pad = p.point_tiles * SC_TM;
    const hipError_t e = launch_pad_points(a.A, a.y, nullptr, false, a.n, a.k, a.lda, a.col_major, n_pad,
                                           p.k_pad, a.Ap, a.yp, s);
    if (e != hipSuccess) return e;
    {
        const int64_t blocks = (a.S + 255) / 256;
        if (blocks > 0x7fffffffll) return hipErrorInvalidValue;
        if (a.per_draw.n_nu > 0) {
            const NuPerDraw& v = a.per_draw;
            hipLaunchKernelGGL(score_consts_tv_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a.theta,
                               a.S, a.ldt, a.k, v.tab, v.n_nu, v.index, v.flag, a.ch);
        } else if (a.nu > 0.0) {
            hipLaunchKernelGGL(score_consts_t_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a.theta,
                               a.S, a.ldt, a.k, student_t_cnu(a.nu), a.nu, a.ch);
        } else {
            hipLaunchKernelGGL(score_consts_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a.theta,
                               a.S, a.ldt, a.k, a.ch);
        }
    }
    if (a.per_draw.n_nu > 0)
        hipLaunchKernelGGL(score_tile_kernel<TileDrawsTV>, dim3((unsigned)groups), dim3(256), 0, s,
                           (const double*)a.Ap, (const double*)a.yp, a.theta, (const double*)a.ch, a.S,
                           a.ldt, a.k, p.k_pad, (uint32_t)p.point_tiles, p.tiles_per_split,
                           p.draw_tiles, n_pad, a.part);
    else if (a.nu > 0.0)
        hipLaunchKernelGGL((score_tile_kernel<TileDrawsT, double>), dim3((unsigned)groups), dim3(256), 0,
                           s, (const double*)a.Ap, (const double*)a.yp, a.theta, (const double*)a.ch,
                           a.S, a.ldt, a.k, p.k_pad, (uint32_t)p.point_tiles, p.tiles_per_split,
                           p.draw_tiles, n_pad, a.part, 0.5 * (a.nu + 1.0));
    else
        hipLaunchKernelGGL(score_tile_kernel<TileDraws>, dim3((unsigned)groups), dim3(256), 0, s,
                           (const double*)a.Ap, (const double*)a.yp, a.theta, (const double*)a.ch, a.S,
                           a.ldt, a.k, p.k_pad, (uint32_t)p.point_tiles, p.tiles_per_split,
                           p.draw_tiles, n_pad, a.part);
    hipLaunchKernelGGL(score_merge_kernel, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, s,
                       (const double*)a.part, a.n, n_pad, p.splits, a.S, a.out);
    return hipGetLastError();
}

}  // namespace bmc
