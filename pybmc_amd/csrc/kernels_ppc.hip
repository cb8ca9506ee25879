// Posterior predictive check of a sampled fit: for design rows
// A (n x k), targets y, offsets and draws theta = (beta_s, sigma_s), replicated data
//   y_rep[i][s] = a_i . beta_s + sigma_s z[i][s] + offset_i,   z the STREAM_PPC variates (below)
// and per draw s, over the n points: min, max, mean, sd, skew, kurt of y_rep[.][s], sum_i z^2,
// max_i |z|, and of the observed data sum_i e^2 and max_i |e|, e = (y_i - a_i . beta_s) / sigma_s.
//
//   pad_points      A (either layout, any lda), y, offset -> whole 64-point tiles and 16-column
//                   slabs, zero in the padding (launch_pad_points of kernels_waic.hip, with the
//                   offset row)
//   ppc_col_mean    the column means a_bar of the padded design and the mean offset, each summed in
//                   one fixed order (a workgroup per 16-column slab, one for the offset)
//   ppc_pad_draws   theta (any ldt) -> the coefficients in whole 64-draw tiles and 16-column slabs
//                   (pad_rows of bmc_score_tile.h),
//                   sigma_s and 1 / sigma_s per draw (1 in the padding; 1 / sigma_s is NaN for a
//                   bad draw: a non-finite coefficient, or no finite sigma_s > 0), and the draw's
//                   centre c_s = a_bar . beta_s + mean(offset) (0 where that is not finite)
//   ppc_tile        workgroup = 64 draws x ALL point tiles: the tile loop of bmc_score_tile.h with
//                   the operands swapped (the draws are the owner rows, the padded design is
//                   walked).  A wave owns 16 draws, a lane 4 draws x 4 points of every tile; the
//                   ten running values of each draw stay in the lane's registers over the whole
//                   walk and meet once, at the end, in a tree over the 16 lanes that share the
//                   draws.  The lane that ends the tree turns the power sums into the moments and
//                   writes the draw's row.  The power sums are of y_rep - c_s, the draw's OWN
//                   centre: about a point all draws share, a fit whose predictions are biased by
//                   D loses (D / sd)^4 u of kurt to m4 = a4 - 4 a1 a3 + ..., and such a fit is
//                   what the check exists to flag.  sigma_s and c_s of the workgroup's 64 draws
//                   wait in LDS (the lane's registers are full of running values).
//
// The variate of (point i, draw s): Philox4x32-10 keyed by the seed, counter (s lo, s hi,
// STREAM_PPC, pair(i)), pair(i) = (i >> 6) 32 + (i & 31); its Box-Muller pair (bmc_math.h) gives
// the cosine half to the point with (i >> 5) & 1 == 0 and the sine half to point i + 32: both are
// points of one lane (MFMA columns cl + 16 t, t and t + 2), so a Philox call serves two elements.
// z[i][s] depends on (seed, i, s) alone.
//
// For a Student-t fit z is a t variate instead (PpcNoise below): one nu for all draws,
// or nu_s per draw, staged by ppc_pad_draws beside sigma_s.  Everything after z is the same text.
//
// No atomics and no split over the points: every sum has one fixed order (tile by tile in the
// lane, then the lane tree), whatever the CU count.  Padded points add nothing (their z, e and
// centred value are replaced by 0, their y_rep by +-inf for min / max); padded draws are computed
// and dropped.
//
// Non-finite input is data (every index comes from the shapes).  A value is NaN exactly where the
// definitions above give NaN: a NaN among y_rep[.][s] makes min, max, mean, sd, skew and kurt NaN,
// a NaN among e the two observed values, and nothing else (the sums propagate it; fmin / fmax would
// drop it, so the epilogue after the walk reads it off p4 and ee, which are sums of squares and
// NaN only if a term is).  All ten values of a bad draw are NaN.  A draw's row depends on that draw
// alone, and a bad point on nothing but what it enters.
#include "bmc_dev.h"
#include "bmc_launch.h"
#include "bmc_plan.h"
#include "bmc_score_tile.h"

namespace bmc {

namespace {

// grid: k_pad / 16 workgroups of 1024 threads, one per slab of 16 columns of the padded design, and
// one more for the offset.  Thread t of a slab's workgroup sums column t & 15 over the rows
// (t >> 4) + 64 m, m in order, into four partial sums by m & 3 (the padded rows are zeros and add
// nothing); the four meet as (s0 + s1) + (s2 + s3) and the 64 row groups of a column in a fixed
// tree in LDS.  The offset is summed the same way by the threads of column 0.  cm [k_pad + 1]: the
// column means (0 in the padded columns), then the mean offset.
__global__ __launch_bounds__(1024) void ppc_col_mean_kernel(const double* __restrict__ Ap,
                                                            const double* __restrict__ yo, int64_t n,
                                                            int64_t n_pad, int32_t k_pad,
                                                            double* __restrict__ cm) {
    __shared__ double part[1024];
    const int tid = threadIdx.x, c = tid & 15, g = tid >> 4;
    const int slab = blockIdx.x;
    const bool is_offset = slab == k_pad / 16;   // workgroup-uniform
    const double* col = is_offset ? yo + n_pad : Ap + 16 * slab + c;
    const int64_t step = is_offset ? 1 : k_pad;
    const int64_t tiles = n_pad / SC_TM;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    if (!is_offset || c == 0) {
        int64_t m = 0;
        for (; m + 4 <= tiles; m += 4) {
            s0 += col[(m * SC_TM + g) * step];
            s1 += col[((m + 1) * SC_TM + g) * step];
            s2 += col[((m + 2) * SC_TM + g) * step];
            s3 += col[((m + 3) * SC_TM + g) * step];
        }
        if (m < tiles) s0 += col[(m * SC_TM + g) * step];
        if (m + 1 < tiles) s1 += col[((m + 1) * SC_TM + g) * step];
        if (m + 2 < tiles) s2 += col[((m + 2) * SC_TM + g) * step];
    }
    part[tid] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    for (int h = 512; h >= 16; h >>= 1) {
        if (tid < h) part[tid] += part[tid + h];
        __syncthreads();
    }
    if (is_offset) {
        if (tid == 0) cm[k_pad] = part[0] / (double)n;
    } else if (tid < 16) {
        cm[16 * slab + tid] = part[tid] / (double)n;
    }
}

// Nu... is empty (the Gaussian check and the one-nu t check) or the staging of a nu per draw (PpcNuStage,
// the t check with nu_index): the draw's nu_s and 2 / nu_s to nus [2][S_pad], 4 and 1/2 in the padding.
struct PpcNuStage {
    const double* tab;      // [2][n_nu]: the distinct values, then 2 / value (formed on the host)
    const int32_t* index;   // [S] into them; out of range: clamped, and *flag = 1
    int32_t* flag;
    double* nus;
    int32_t n_nu;
};

template <typename... Nu>
__global__ __launch_bounds__(256) void ppc_pad_draws_kernel(const double* __restrict__ theta,
                                                            int64_t S, int64_t ldt, int32_t k,
                                                            int64_t S_pad, int32_t k_pad,
                                                            const double* __restrict__ cm,
                                                            double* __restrict__ Tp,
                                                            double* __restrict__ sg, Nu... nu) {
    pad_rows(theta, S, ldt, k, S_pad, k_pad, Tp);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    // then a thread per draw (all lanes of a wave at work, not one in k_pad): sigma_s, whether the
    // draw is good, and its centre c_s = a_bar . beta_s + mean(offset), the columns in order
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < S_pad; s += stride) {
        const double sigma = s < S ? theta[s * ldt + k] : 1.0;
        bool good = sigma > 0.0 && sigma < __builtin_inf();
        double c = 0.0;
        if (s < S) {
            for (int32_t jj = 0; jj < k; ++jj) {
                const double b = theta[s * ldt + jj];
                good = good && is_finite(b);
                c += cm[jj] * b;
            }
        }
        c += cm[k_pad];
        sg[s] = sigma;
        sg[S_pad + s] = good ? 1.0 / sigma : __builtin_nan("");
        sg[2 * S_pad + s] = is_finite(c) ? c : 0.0;
        if constexpr (sizeof...(Nu) > 0) {
            const PpcNuStage st{nu...};
            double v = 4.0, tv = 0.5;
            if (s < S) {
                const int32_t iv = nu_index_clamped(st.index[s], st.n_nu, st.flag);
                v = st.tab[iv];
                tv = st.tab[st.n_nu + iv];
            }
            st.nus[s] = v;
            st.nus[S_pad + s] = tv;
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

// The noise of the replicated data.  PPC_GAUSS: the standard normals of the header, no further
// argument.  PPC_T and PPC_TV: Student-t with one nu for all draws or a nu per draw, Lik as TNoise
// (bmc_dev.h) names it; the pairs of PPC_TV wait in LDS beside sigma_s and c_s.  The t variate of (point i, draw s) is student_t_variate (bmc_math.h)
// of the two uniforms of counter (s lo, s hi, STREAM_PPC_T, i): the point index itself, one Philox
// call per element.  Only the cosine half of Bailey's polar pair is taken: the sine half shares
// its radius, and handing it to point i + 32 as the Gaussian walk does would replicate data whose
// errors depend on each other in pairs.  z[i][s] depends on (seed, i, s, nu_s) alone.
enum PpcNoise { PPC_GAUSS = 0, PPC_T = 1, PPC_TV = 2 };

// grid: one workgroup per draw tile.  The workgroups that run together walk the same point tiles
// at about the same time, so a tile of the design is fetched into each XCD's L2 once for all.
// The t instantiations build for one workgroup per CU: the temporaries of the t variate do not fit
// beside the running values in the 256 registers that two workgroups leave each (45 to 51 spilled);
// with one, the overflow lives in AGPRs and nothing goes to scratch.
template <PpcNoise NOISE, typename... Lik>
__global__ __launch_bounds__(256, NOISE == PPC_GAUSS ? 2 : 1) void ppc_tile_kernel(
    const double* __restrict__ Tp, const double* __restrict__ sg, const double* __restrict__ Ap,
    const double* __restrict__ yo, int64_t n, int64_t n_pad, int64_t S, int64_t S_pad, int32_t k,
    int32_t k_pad, int64_t point_tiles, uint64_t seed, double* __restrict__ t_rep,
    double* __restrict__ t_obs2, Lik... lik) {
    // doubles per draw in LDS: (sigma_s, c_s), and (nu_s, 2 / nu_s) behind them for PPC_TV
    constexpr int SCW = NOISE == PPC_TV ? 4 : 2;
    __shared__ double As[SC_LDS_DOUBLES];
    __shared__ double Bs[SC_LDS_DOUBLES];
    __shared__ double sc[SCW * SC_TM];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cl = lane & 15, kq = lane >> 4;
    const int64_t d0 = (int64_t)blockIdx.x * SC_TM;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);

    // this lane's four draws: rows 16 wave + kq + 4 r of the tile (MFMA D: row = kq + 4 reg)
    // (a tile starts at a multiple of 64: the high word of the draw index is the workgroup's)
    const uint32_t dlo = (uint32_t)d0 + (uint32_t)(16 * wave + kq);
    const uint32_t dhi = (uint32_t)((uint64_t)d0 >> 32);
    PpcRun st[4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
        st[r] = PpcRun{__builtin_inf(), -__builtin_inf(), 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const TNoise<Lik...> lk{lik...};
    if (tid < SC_TM) {
        sc[SCW * tid] = sg[d0 + tid];
        sc[SCW * tid + 1] = sg[2 * S_pad + d0 + tid];
        if constexpr (NOISE == PPC_TV) {
            sc[SCW * tid + 2] = lk.nus[d0 + tid];
            sc[SCW * tid + 3] = lk.nus[S_pad + d0 + tid];
        }
    }
    __syncthreads();
    // draw r of the lane: sc_r[4 SCW r], sc_r[4 SCW r + 1], ..
    const double* sc_r = sc + SCW * (16 * wave + kq);
    // where the walk finds (nu, 2 / nu): the pairs of PPC_TV in LDS, behind (sigma_s, c_s)
    const auto noise = [&] {
        if constexpr (NOISE == PPC_TV) return TNoise<const double*>{sc_r + 2};
        else return lk;
    }();

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
        if constexpr (NOISE == PPC_GAUSS) {
            // the lane's points are i0 + cl + 16 t; points t and t + 2 (32 apart) share a counter,
            // the cosine half to t
            const uint32_t pr = (uint32_t)(i0 >> 6) * 32u + (uint32_t)cl;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double sigma = sc_r[4 * SCW * r], center = sc_r[4 * SCW * r + 1];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const u32x4 w =
                        philox4x32_10(u32x4{dlo + 4u * r, dhi, STREAM_PPC, pr + 16u * h}, k0, k1);
                    double z0, z1;
                    box_muller_pair(u53_open0(w.x, w.y), u53_open0(w.z, w.w), z0, z1);
                    if (full) {
                        ppc_fold<true>(st[r], acc[h][r], z0, yv[h], ov[h], sigma, center, true);
                        ppc_fold<true>(st[r], acc[h + 2][r], z1, yv[h + 2], ov[h + 2], sigma, center,
                                       true);
                    } else {
                        ppc_fold<false>(st[r], acc[h][r], z0, yv[h], ov[h], sigma, center, ok[h]);
                        ppc_fold<false>(st[r], acc[h + 2][r], z1, yv[h + 2], ov[h + 2], sigma, center,
                                        ok[h + 2]);
                    }
                    // one pair at a time: left to itself the scheduler interleaves the eight
                    // Philox / Box-Muller chains of a tile and their temporaries no longer fit
                    // beside the 80 registers of running values
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        } else {
            // the lane's points are i0 + cl + 16 t, each with a counter of its own (the padded
            // index fits the word: plan_ppc refuses more than 2^31 points)
            const uint32_t pt = (uint32_t)i0 + (uint32_t)cl;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double sigma = sc_r[4 * SCW * r], center = sc_r[4 * SCW * r + 1];
                const NuPair nt = noise.pair(4 * SCW * r, 1);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const double z =
                        student_t_at(u32x4{dlo + 4u * r, dhi, STREAM_PPC_T, pt + 16u * t}, k0, k1, nt);
                    if (full) ppc_fold<true>(st[r], acc[t][r], z, yv[t], ov[t], sigma, center, true);
                    else ppc_fold<false>(st[r], acc[t][r], z, yv[t], ov[t], sigma, center, ok[t]);
                    // one variate at a time, as above
                    __builtin_amdgcn_sched_barrier(0);
                }
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
            // central moments (ddof 0) from the power sums about the draw's centre
            const double center = sc_r[4 * SCW * r + 1];
            const double a1 = me.p1 / nn, a2 = me.p2 / nn, a3 = me.p3 / nn, a4 = me.p4 / nn;
            const double a1s = a1 * a1;
            const double m2 = a2 - a1s;
            const double m3 = fma(2.0 * a1s, a1, fma(-3.0 * a1, a2, a3));
            const double m4 = fma(-3.0 * a1s, a1s, fma(6.0 * a1s, a2, fma(-4.0 * a1, a3, a4)));
            const double sd = sqrt(m2);
            // fmin / fmax dropped a NaN that the definitions keep: p4 and ee are sums of squares,
            // NaN only if a y_rep (an e) of the draw is.  A bad draw (1 / sigma_s is NaN) is NaN in
            // all ten values.
            const double nan = __builtin_nan("");
            const double inv_sigma = sg[S_pad + d];
            const bool bad = inv_sigma != inv_sigma;
            const bool rep_nan = bad || me.p4 != me.p4, obs_nan = bad || me.ee != me.ee;
            double* o = t_rep + d * PPC_STATS;
            o[0] = rep_nan ? nan : me.mn;
            o[1] = rep_nan ? nan : me.mx;
            o[2] = rep_nan ? nan : center + a1;
            o[3] = rep_nan ? nan : sd;
            o[4] = rep_nan ? nan : m3 / (m2 * sd);
            o[5] = rep_nan ? nan : m4 / (m2 * m2) - 3.0;
            o[6] = bad ? nan : me.zz;
            o[7] = bad ? nan : me.mz;
            t_obs2[d * PPC_OBS] = obs_nan ? nan : me.ee * inv_sigma * inv_sigma;
            t_obs2[d * PPC_OBS + 1] = obs_nan ? nan : me.me * inv_sigma;
        }
    }
}

}  // namespace

hipError_t launch_ppc(const PpcArgs& a, const PpcPlan& p, hipStream_t s) {
    const PpcPlan want = plan_ppc(a.n, a.S, a.k, 1);
    const NuPerDraw& v = a.per_draw;
    if (!p.ok || !want.ok || a.ldt < (int64_t)a.k + 1 || a.lda < (a.col_major ? a.n : (int64_t)a.k) ||
        p.point_tiles != want.point_tiles || p.draw_tiles != want.draw_tiles || p.n_pad != want.n_pad ||
        p.S_pad != want.S_pad || p.k_pad != want.k_pad || p.grid != want.grid || p.grid > 0x7fffffffll ||
        !(a.nu >= 0.0 && a.nu < __builtin_inf()) || !v.valid(a.nu, PPC_MAX_NU_VALUES) || (v.n_nu > 0 && !a.nus))
        return hipErrorInvalidValue;
    const hipError_t e = launch_pad_points(a.A, a.y, a.offset, true, a.n, a.k, a.lda, a.col_major, p.n_pad,
                                           p.k_pad, a.Ap, a.yo, s);
    if (e != hipSuccess) return e;
    double* cm = a.sg + 3 * p.S_pad;   // the column means and the mean offset, behind the three rows
    hipLaunchKernelGGL(ppc_col_mean_kernel, dim3((unsigned)(p.k_pad / 16 + 1)), dim3(1024), 0, s,
                       (const double*)a.Ap, (const double*)a.yo, a.n, p.n_pad, p.k_pad, cm);
    int64_t blocks = (p.S_pad * p.k_pad + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    if (v.n_nu > 0)
        hipLaunchKernelGGL(ppc_pad_draws_kernel<PpcNuStage>, dim3((unsigned)blocks), dim3(256), 0, s,
                           a.theta, a.S, a.ldt, a.k, p.S_pad, p.k_pad, (const double*)cm, a.Tp, a.sg,
                           PpcNuStage{v.tab, v.index, v.flag, a.nus, v.n_nu});
    else
        hipLaunchKernelGGL(ppc_pad_draws_kernel<>, dim3((unsigned)blocks), dim3(256), 0, s, a.theta, a.S,
                           a.ldt, a.k, p.S_pad, p.k_pad, (const double*)cm, a.Tp, a.sg);
    if (v.n_nu > 0)
        hipLaunchKernelGGL((ppc_tile_kernel<PPC_TV, const double*>), dim3((unsigned)p.grid), dim3(256), 0,
                           s, (const double*)a.Tp, (const double*)a.sg, (const double*)a.Ap,
                           (const double*)a.yo, a.n, p.n_pad, a.S, p.S_pad, a.k, p.k_pad, p.point_tiles,
                           a.seed, a.t_rep, a.t_obs2, (const double*)a.nus);
    else if (a.nu > 0.0)
        hipLaunchKernelGGL((ppc_tile_kernel<PPC_T, double, double>), dim3((unsigned)p.grid), dim3(256), 0,
                           s, (const double*)a.Tp, (const double*)a.sg, (const double*)a.Ap,
                           (const double*)a.yo, a.n, p.n_pad, a.S, p.S_pad, a.k, p.k_pad, p.point_tiles,
                           a.seed, a.t_rep, a.t_obs2, a.nu, 2.0 / a.nu);
    else
        hipLaunchKernelGGL(ppc_tile_kernel<PPC_GAUSS>, dim3((unsigned)p.grid), dim3(256), 0, s,
                           (const double*)a.Tp, (const double*)a.sg, (const double*)a.Ap,
                           (const double*)a.yo, a.n, p.n_pad, a.S, p.S_pad, a.k, p.k_pad, p.point_tiles,
                           a.seed, a.t_rep, a.t_obs2);
    return hipGetLastError();
}

}  // namespace bmc
