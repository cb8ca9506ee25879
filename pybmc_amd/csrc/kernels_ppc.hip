// Posterior predictive check of a sampled fit: for design rows
// A (n x k), targets y, offsets and draws theta = (beta_s, sigma_s), replicated data
//   y_rep[i][s] = a_i . beta_s + sigma_s z[i][s] + offset_i,   z the STREAM_PPC variates (below)
// and per draw s, over the n points: min, max, mean, sd, skew, kurt of y_rep[.][s], sum_i z^2,
// max_i |z|, and of the observed data sum_i e^2 and max_i |e|, e = (y_i - a_i . beta_s) / sigma_s.
//
//   ppc_pad_points  A (either layout, any lda), y, offset -> whole 64-point tiles and 16-column
//                   slabs, zero in the padding
//   ppc_pad_draws   theta (any ldt) -> the coefficients in whole 64-draw tiles and 16-column slabs,
//                   sigma_s and 1 / sigma_s per draw (1 in the padding)
//   ppc_tile        workgroup = 64 draws x ALL point tiles: the tile loop of bmc_score_tile.h with
//                   the operands swapped (the draws are the owner rows, the padded design is
//                   walked).  A wave owns 16 draws, a lane 4 draws x 4 points of every tile; the
//                   ten running values of each draw stay in the lane's registers over the whole
//                   walk and meet once, at the end, in a tree over the 16 lanes that share the
//                   draws.  The lane that ends the tree turns the power sums into the moments and
//                   writes the draw's row.
//
// The variate of (point i, draw s): Philox4x32-10 keyed by the seed, counter (s lo, s hi,
// STREAM_PPC, pair(i)), pair(i) = (i >> 6) 32 + (i & 31); its Box-Muller pair (bmc_math.h) gives
// the cosine half to the point with (i >> 5) & 1 == 0 and the sine half to point i + 32: both are
// points of one lane (MFMA columns cl + 16 t, t and t + 2), so a Philox call serves two elements.
// z[i][s] depends on (seed, i, s) alone.
//
// No atomics and no split over the points: every sum has one fixed order (tile by tile in the
// lane, then the lane tree), whatever the CU count.  Padded points add nothing (their z, e and
// centred value are replaced by 0, their y_rep by +-inf for min / max); padded draws are computed
// and dropped.  Non-finite input propagates through the sums; min / max ignore a NaN.
#include "bmc_dev.h"
#include "bmc_launch.h"
#include "bmc_plan.h"
#include "bmc_score_tile.h"

namespace bmc {

namespace {

__global__ __launch_bounds__(256) void ppc_pad_points_kernel(
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
            yo[n_pad + i] = (i < n && offset != nullptr) ? offset[i] : 0.0;
        }
    }
}

__global__ __launch_bounds__(256) void ppc_pad_draws_kernel(const double* __restrict__ theta,
                                                            int64_t S, int64_t ldt, int32_t k,
                                                            int64_t S_pad, int32_t k_pad,
                                                            double* __restrict__ Tp,
                                                            double* __restrict__ sg) {
    const int64_t total = S_pad * k_pad;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const int64_t s = e / k_pad;
        const int32_t j = (int32_t)(e - s * k_pad);
        Tp[e] = (s < S && j < k) ? theta[s * ldt + j] : 0.0;
        if (j == 0) {
            const double sigma = s < S ? theta[s * ldt + k] : 1.0;
            sg[s] = sigma;
            sg[S_pad + s] = 1.0 / sigma;
        }
    }
}

// What a lane keeps of ONE of its draws over the walk
struct PpcRun {
    double mn, mx, p1, p2, p3, p4, zz, mz, ee, me;
};

// One element into its draw's running values: dot = a_i . beta_s, z its variate.  FULL: the point
// exists (every tile but a partly filled last one).
template <bool FULL>
__device__ __forceinline__ void ppc_fold(PpcRun& st, double dot, double z, double yv, double ov,
                                         double sigma, double center, bool ok) {
    double e = yv - dot;   // (un-scaled: 1 / sigma_s meets the sum and the maximum at the end)
    const double yr = fma(z, sigma, dot) + ov;
    double x = yr - center;
    double lo = yr, hi = yr;
    if (!FULL && !ok) {
        z = 0.0, e = 0.0, x = 0.0;
        lo = __builtin_inf(), hi = -__builtin_inf();
    }
    st.mn = fmin(st.mn, lo);
    st.mx = fmax(st.mx, hi);
    const double x2 = x * x;
    st.p1 += x;
    st.p2 += x2;
    st.p3 = fma(x2, x, st.p3);
    st.p4 = fma(x2, x2, st.p4);
    st.zz = fma(z, z, st.zz);
    st.mz = fmax(st.mz, fabs(z));
    st.ee = fma(e, e, st.ee);
    st.me = fmax(st.me, fabs(e));
}

// grid: one workgroup per draw tile.  The workgroups that run together walk the same point tiles
// at about the same time, so a tile of the design is fetched into each XCD's L2 once for all.
__global__ __launch_bounds__(256, 2) void ppc_tile_kernel(
    const double* __restrict__ Tp, const double* __restrict__ sg, const double* __restrict__ Ap,
    const double* __restrict__ yo, int64_t n, int64_t n_pad, int64_t S, int64_t S_pad, int32_t k,
    int32_t k_pad, int64_t point_tiles, uint64_t seed, double center, double* __restrict__ t_rep,
    double* __restrict__ t_obs2) {
    __shared__ double As[SC_LDS_DOUBLES];
    __shared__ double Bs[SC_LDS_DOUBLES];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cl = lane & 15, kq = lane >> 4;
    const int64_t d0 = (int64_t)blockIdx.x * SC_TM;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);

    // this lane's four draws: rows 16 wave + kq + 4 r of the tile (MFMA D: row = kq + 4 reg)
    // (a tile starts at a multiple of 64: the high word of the draw index is the workgroup's)
    const uint32_t dlo = (uint32_t)d0 + (uint32_t)(16 * wave + kq);
    const uint32_t dhi = (uint32_t)((uint64_t)d0 >> 32);
    double sigma[4];
    PpcRun st[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        sigma[r] = sg[d0 + 16 * wave + kq + 4 * r];
        st[r] = PpcRun{__builtin_inf(), -__builtin_inf(), 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    }

    // epilogue: the lane's points are i0 + cl + 16 t; points t and t + 2 (32 apart) share a
    // counter, the cosine half to t
    score_tile_loop(Tp, Ap, n_pad, (int64_t)k_pad, k, k_pad, d0, 0, point_tiles, As, Bs,
                    [&](int64_t i0, const f64x4(&acc)[4]) {
        const bool full = i0 + SC_TM <= n;   // wave-uniform
        double yv[4], ov[4];
        bool ok[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int64_t i = i0 + cl + 16 * t;
            yv[t] = yo[i];
            ov[t] = yo[n_pad + i];
            ok[t] = i < n;
        }
        const uint32_t pr = (uint32_t)(i0 >> 6) * 32u + (uint32_t)cl;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const u32x4 w = philox4x32_10(u32x4{dlo + 4u * r, dhi, STREAM_PPC, pr + 16u * h}, k0, k1);
                double z0, z1;
                box_muller_pair(u53_open0(w.x, w.y), u53_open0(w.z, w.w), z0, z1);
                if (full) {
                    ppc_fold<true>(st[r], acc[h][r], z0, yv[h], ov[h], sigma[r], center, true);
                    ppc_fold<true>(st[r], acc[h + 2][r], z1, yv[h + 2], ov[h + 2], sigma[r],
                                   center, true);
                } else {
                    ppc_fold<false>(st[r], acc[h][r], z0, yv[h], ov[h], sigma[r], center, ok[h]);
                    ppc_fold<false>(st[r], acc[h + 2][r], z1, yv[h + 2], ov[h + 2], sigma[r],
                                    center, ok[h + 2]);
                }
                // one pair at a time: left to itself the scheduler interleaves the eight
                // Philox / Box-Muller chains of a tile and their temporaries no longer fit beside
                // the 80 registers of running values
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    });

    // the 16 lanes (cl) that hold points of the same four draws: a tree over cl.  Both sides of a
    // step add (or compare) the same two numbers, so every lane ends with the same bits; lane
    // cl = 0 writes them.
    const double nn = (double)n;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        PpcRun me = st[r];
#pragma unroll
        for (int bit = 1; bit < 16; bit <<= 1) {
            me.mn = fmin(me.mn, __shfl_xor(me.mn, bit));
            me.mx = fmax(me.mx, __shfl_xor(me.mx, bit));
            me.p1 += __shfl_xor(me.p1, bit);
            me.p2 += __shfl_xor(me.p2, bit);
            me.p3 += __shfl_xor(me.p3, bit);
            me.p4 += __shfl_xor(me.p4, bit);
            me.zz += __shfl_xor(me.zz, bit);
            me.mz = fmax(me.mz, __shfl_xor(me.mz, bit));
            me.ee += __shfl_xor(me.ee, bit);
            me.me = fmax(me.me, __shfl_xor(me.me, bit));
        }
        const int64_t d = d0 + 16 * wave + kq + 4 * r;
        if (cl == 0 && d < S) {
            // central moments (ddof 0) from the power sums about `center`
            const double a1 = me.p1 / nn, a2 = me.p2 / nn, a3 = me.p3 / nn, a4 = me.p4 / nn;
            const double a1s = a1 * a1;
            const double m2 = a2 - a1s;
            const double m3 = fma(2.0 * a1s, a1, fma(-3.0 * a1, a2, a3));
            const double m4 = fma(-3.0 * a1s, a1s, fma(6.0 * a1s, a2, fma(-4.0 * a1, a3, a4)));
            const double sd = sqrt(m2);
            double* o = t_rep + d * PPC_STATS;
            o[0] = me.mn;
            o[1] = me.mx;
            o[2] = center + a1;
            o[3] = sd;
            o[4] = m3 / (m2 * sd);
            o[5] = m4 / (m2 * m2) - 3.0;
            o[6] = me.zz;
            o[7] = me.mz;
            const double inv_sigma = sg[S_pad + d];
            t_obs2[d * PPC_OBS] = me.ee * inv_sigma * inv_sigma;
            t_obs2[d * PPC_OBS + 1] = me.me * inv_sigma;
        }
    }
}

}  // namespace

hipError_t launch_ppc(const PpcArgs& a, const PpcPlan& p, hipStream_t s) {
    const PpcPlan want = plan_ppc(a.n, a.S, a.k, 1);
    if (!p.ok || !want.ok || a.ldt < (int64_t)a.k + 1 || a.lda < (a.col_major ? a.n : (int64_t)a.k) ||
        p.point_tiles != want.point_tiles || p.draw_tiles != want.draw_tiles || p.n_pad != want.n_pad ||
        p.S_pad != want.S_pad || p.k_pad != want.k_pad || p.grid != want.grid || p.grid > 0x7fffffffll)
        return hipErrorInvalidValue;
    {
        int64_t blocks = (p.n_pad * p.k_pad + 255) / 256;
        if (blocks > 8192) blocks = 8192;
        hipLaunchKernelGGL(ppc_pad_points_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a.A, a.y,
                           a.offset, a.n, a.k, a.lda, a.col_major, p.n_pad, p.k_pad, a.Ap, a.yo);
    }
    {
        int64_t blocks = (p.S_pad * p.k_pad + 255) / 256;
        if (blocks > 8192) blocks = 8192;
        hipLaunchKernelGGL(ppc_pad_draws_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a.theta, a.S,
                           a.ldt, a.k, p.S_pad, p.k_pad, a.Tp, a.sg);
    }
    hipLaunchKernelGGL(ppc_tile_kernel, dim3((unsigned)p.grid), dim3(256), 0, s, (const double*)a.Tp,
                       (const double*)a.sg, (const double*)a.Ap, (const double*)a.yo, a.n, p.n_pad, a.S,
                       p.S_pad, a.k, p.k_pad, p.point_tiles, a.seed, a.center, a.t_rep, a.t_obs2);
    return hipGetLastError();
}

}  // namespace bmc
