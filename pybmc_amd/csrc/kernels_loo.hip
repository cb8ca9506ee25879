// PSIS-LOO: Pareto-smoothed importance-sampling leave-one-out cross-validation of a sampled fit
// (Vehtari, Gelman & Gabry 2017; Vehtari et al. 2024; the
// generalised Pareto fit of Zhang & Stephens 2009).  With ll[i][s] as in kernels_waic.hip and
// lw = -ll, each point needs the M largest lw (the M smallest ll) and the next one, of a matrix
// that is never stored.  The passes (plan_loo in bmc_plan.h says what bounds each):
//
//   launch_score   lppd_i, and the padded A, y and per-draw constants every later pass reads
//   loo_range      per point the smallest and largest KEY of ll: the IEEE bits mapped to an
//                  unsigned integer of the same order; and whether any ll is not finite
//   loo_init       the point's select state: the bits kmin and kmax share are fixed
//   loo_select     one radix digit: keys that match the fixed bits are counted by their next
//                  LOO_DIGIT_BITS bits, in LDS per 64-point tile, then added to the point's
//                  global counts (integer atomics: any order, the same result)
//   loo_scan       per point: the digit whose bucket holds rank M + 1 joins the fixed bits;
//                  settled when bucket + everything below fits the candidate slots, or when all
//                  64 bits are fixed (the bucket is then one value, repeated)
//   loo_append     keys below the bucket, and the bucket if it fits, to the point's slots (in
//                  any order: they are sorted next); exp(lw) of every key above it summed per
//                  lane, tile, lane tree and split, one fixed order
//   loo_fit        one workgroup per point: bitonic sort of the candidates in LDS, tail and
//                  cutoff, the Pareto fit (psis_fit of bmc_psis.h, shared with sens_psis_kernel; its
//                  grid size is the plan's), the smoothed tail, elpd_loo_i
//
// The leave-one-out predictive moments (launch_loo_predict) run the same passes with
// the PREDICT variants of the last two: the append also records each candidate's draw index and
// sums w r, w (sigma^2 + r^2), w Phi(r / sigma) and w^2 of everything above the bucket, one more
// pass (loo_bucket) sums the payload of a bucket that is one repeated value, and the fit sorts
// (value, draw) pairs, shares the weights of equal values and adds the payload up.
//
// Two calls return the same bits: the only atomics are integer counts and slot numbers of values
// that are sorted before use.  A point with a non-finite ll (a NaN or infinity in a_i, y_i or any
// draw, a sigma_s <= 0) is flagged by loo_range and gets NaN; its keys are never used as an index
// (digits are masked, slots are bounded by the cap).
//
// The likelihood enters through the draws type alone (bmc_score_tile.h): the passes that compute ll
// (range, select, the non-PREDICT append) are templates <D, L...> on it, TileDraws for the Gaussian
// density, TileDrawsT with its scalar for the Student-t one (ScoreArgs::nu > 0) and TileDrawsTV for
// the Student-t one with a nu per draw (ScoreArgs::per_draw); init, scan and
// fit see values of ll only.  The PREDICT passes of the Student-t likelihood are kernels of their own
// (loo_append_t_kernel in two phases, loo_bucket_t_kernel, loo_fit_kernel<true, TFit>): the t
// density and distribution function do not fit the registers of one append.
#include "bmc_dev.h"
#include "bmc_launch.h"
#include "bmc_plan.h"
#include "bmc_psis.h"
#include "bmc_score_tile.h"

namespace bmc {

namespace {

constexpr uint32_t LF_DONE = 1, LF_APPEND_EQ = 2, LF_NOTAIL = 4, LF_BAD = 8;
constexpr int LOO_BINS = 1 << LOO_DIGIT_BITS;
constexpr int LOO_MAX_GRID = 128;   // grid points of the fit held on chip (120 at LOO_MAX_CAP)
constexpr uint64_t SIGN = 0x8000000000000000ull;
constexpr size_t LOO_SELECT_LDS = 2 * SC_LDS_DOUBLES * 8 + (size_t)SC_TM * LOO_BINS * 4;

// a < b as doubles  <=>  ord_key(a) < ord_key(b) as unsigned (for all non-NaN a, b; -0 < +0)
__device__ __forceinline__ uint64_t ord_key(double x) {
    const uint64_t u = (uint64_t)__double_as_longlong(x);
    return (u & SIGN) ? ~u : (u | SIGN);
}
__device__ __forceinline__ double key_value(uint64_t key) {
    return __longlong_as_double((long long)((key & SIGN) ? (key ^ SIGN) : ~key));
}
// the r highest bits of a key
__device__ __forceinline__ uint64_t key_top(uint64_t key, uint32_t r) {
    return r == 0 ? 0ull : key >> (64 - r);
}

// The split and point tile of a workgroup (grid of score_tile_kernel: point tile fastest)
struct TilePos {
    int64_t p0, split, dt0, dt1;
    __device__ __forceinline__ TilePos(uint32_t point_tiles, int64_t tiles_per_split,
                                       int64_t draw_tiles) {
        const uint32_t pt = blockIdx.x % point_tiles;
        split = blockIdx.x / point_tiles;
        p0 = (int64_t)pt * SC_TM;
        dt0 = split * tiles_per_split;
        dt1 = dt0 + tiles_per_split < draw_tiles ? dt0 + tiles_per_split : draw_tiles;
    }
};

// Arguments every pass over the matrix shares
struct PassArgs {
    const double *Ap, *yp, *theta, *ch;
    int64_t S, ldt, tiles_per_split, draw_tiles, n_pad;
    int32_t k, k_pad;
    uint32_t point_tiles;
};

template <class D, class... L>
__global__ __launch_bounds__(256) void loo_range_kernel(PassArgs a, uint64_t* __restrict__ range,
                                                        L... lik) {
    __shared__ double As[SC_LDS_DOUBLES];
    __shared__ double Bs[SC_LDS_DOUBLES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, cl = lane & 15, kq = lane >> 4;
    const TilePos pos(a.point_tiles, a.tiles_per_split, a.draw_tiles);
    double yv[4];
    uint64_t kmin[4], kmax[4], bad[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        yv[r] = a.yp[pos.p0 + 16 * wave + kq + 4 * r];
        kmin[r] = ~0ull;
        kmax[r] = 0ull;
        bad[r] = 0ull;
    }
    score_tile_loop(a.Ap, a.theta, a.S, a.ldt, a.k, a.k_pad, pos.p0, pos.dt0, pos.dt1, As, Bs,
                    [&](int64_t s0, const f64x4(&acc)[4]) {
        const D d(a.ch, a.S, s0, cl, lik...);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (d.ok[t]) {
                    const double x = d.ll(yv[r], acc[t][r], t);
                    const uint64_t key = ord_key(x);
                    kmin[r] = key < kmin[r] ? key : kmin[r];
                    kmax[r] = key > kmax[r] ? key : kmax[r];
                    bad[r] |= is_finite(x) ? 0ull : 1ull;
                }
    });
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int bit = 1; bit < 16; bit <<= 1) {
            const uint64_t lo = __shfl_xor((unsigned long long)kmin[r], bit);
            const uint64_t hi = __shfl_xor((unsigned long long)kmax[r], bit);
            const uint64_t b = __shfl_xor((unsigned long long)bad[r], bit);
            kmin[r] = lo < kmin[r] ? lo : kmin[r];
            kmax[r] = hi > kmax[r] ? hi : kmax[r];
            bad[r] |= b;
        }
        if (cl == 0) {
            uint64_t* o = range + ((int64_t)pos.split * a.n_pad + pos.p0 + 16 * wave + kq + 4 * r) * 3;
            o[0] = kmin[r];
            o[1] = kmax[r];
            o[2] = bad[r];
        }
    }
}

// meta: x = bits fixed, y = keys below the bucket, z = keys in the bucket, w = flags
__global__ __launch_bounds__(256) void loo_init_kernel(const uint64_t* __restrict__ range,
                                                       int64_t n_pad, int64_t splits, int64_t S,
                                                       int32_t M, int32_t cap,
                                                       uint64_t* __restrict__ prefix,
                                                       uint64_t* __restrict__ kmin_out,
                                                       uint4* __restrict__ meta) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pad) return;
    uint64_t lo = ~0ull, hi = 0ull, bad = 0ull;
    for (int64_t sp = 0; sp < splits; ++sp) {
        const uint64_t* p = range + (sp * n_pad + i) * 3;
        lo = p[0] < lo ? p[0] : lo;
        hi = p[1] > hi ? p[1] : hi;
        bad |= p[2];
    }
    uint4 m{0u, 0u, (uint32_t)S, 0u};
    uint64_t pre = 0ull;
    if (bad) {
        m.w = LF_BAD | LF_DONE;
    } else if (M == 0) {
        m.w = LF_NOTAIL | LF_DONE;
    } else if (S <= (int64_t)cap) {
        m.w = LF_DONE | LF_APPEND_EQ;   // no bit fixed: every key is in the bucket
    } else if (lo == hi) {
        m.x = 64u;
        pre = lo;
        m.w = LF_DONE;
    } else {
        m.x = (uint32_t)__builtin_clzll(lo ^ hi);
        pre = key_top(lo, m.x);
    }
    prefix[i] = pre;
    kmin_out[i] = lo;
    meta[i] = m;
}

template <class D, class... L>
__global__ __launch_bounds__(256) void loo_select_kernel(PassArgs a,
                                                         const uint64_t* __restrict__ prefix,
                                                         const uint4* __restrict__ meta,
                                                         uint32_t* __restrict__ hist, L... lik) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double* As = (double*)smem_raw;
    double* Bs = As + SC_LDS_DOUBLES;
    uint32_t* h = (uint32_t*)(Bs + SC_LDS_DOUBLES);   // [64][LOO_BINS]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, cl = lane & 15, kq = lane >> 4;
    const TilePos pos(a.point_tiles, a.tiles_per_split, a.draw_tiles);
    double yv[4];
    uint64_t pre[4];
    uint32_t fixed[4], low[4], mask[4];
    bool live[4];
    int any = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t pi = pos.p0 + 16 * wave + kq + 4 * r;
        const uint4 m = meta[pi];
        yv[r] = a.yp[pi];
        pre[r] = prefix[pi];
        live[r] = !(m.w & LF_DONE);
        fixed[r] = live[r] ? m.x : 0u;   // (a settled point may have all 64 bits fixed)
        const uint32_t nb = 64u - fixed[r] < (uint32_t)LOO_DIGIT_BITS ? 64u - fixed[r]
                                                                       : (uint32_t)LOO_DIGIT_BITS;
        low[r] = 64u - fixed[r] - nb;
        mask[r] = (1u << nb) - 1u;
        any |= live[r];
    }
    if (!__syncthreads_or(any)) return;   // all 64 points settled
    for (int e = tid; e < SC_TM * LOO_BINS; e += 256) h[e] = 0u;
    __syncthreads();
    score_tile_loop(a.Ap, a.theta, a.S, a.ldt, a.k, a.k_pad, pos.p0, pos.dt0, pos.dt1, As, Bs,
                    [&](int64_t s0, const f64x4(&acc)[4]) {
        const D d(a.ch, a.S, s0, cl, lik...);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (!live[r]) continue;
            uint32_t* hr = h + (16 * wave + kq + 4 * r) * LOO_BINS;
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (d.ok[t]) {
                    const uint64_t key = ord_key(d.ll(yv[r], acc[t][r], t));
                    if (key_top(key, fixed[r]) == pre[r])
                        atomicAdd(hr + ((uint32_t)(key >> low[r]) & mask[r]), 1u);
                }
        }
    });
    __syncthreads();
    for (int e = tid; e < SC_TM * LOO_BINS; e += 256) {
        const uint32_t v = h[e];
        if (v) atomicAdd(hist + pos.p0 * LOO_BINS + e, v);
    }
}

__global__ __launch_bounds__(256) void loo_scan_kernel(int64_t n_pad, int32_t M, int32_t cap,
                                                       uint64_t* __restrict__ prefix,
                                                       uint4* __restrict__ meta,
                                                       uint32_t* __restrict__ hist) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pad) return;
    uint4 m = meta[i];
    if (m.w & LF_DONE) return;
    const uint32_t nb = 64u - m.x < (uint32_t)LOO_DIGIT_BITS ? 64u - m.x : (uint32_t)LOO_DIGIT_BITS;
    const uint32_t want = (uint32_t)M + 1u - m.y;   // rank of the threshold inside the bucket, >= 1
    uint4* hp = (uint4*)(hist + i * LOO_BINS);
    uint32_t cum = 0, below = 0, in = 0;
    int digit = -1;
    for (int q = 0; q < LOO_BINS / 4; ++q) {
        const uint4 c4 = hp[q];
        const uint32_t c[4] = {c4.x, c4.y, c4.z, c4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (digit < 0 && cum + c[e] >= want) {
                digit = 4 * q + e;
                below = cum;
                in = c[e];
            }
            cum += c[e];
        }
        hp[q] = uint4{0u, 0u, 0u, 0u};
    }
    if (digit < 0 || cum != m.z) {   // the counts do not add up: cannot happen; a value, not a hang
        m.w = LF_BAD | LF_DONE;
        meta[i] = m;
        return;
    }
    prefix[i] = (prefix[i] << nb) | (uint64_t)digit;
    m.x += nb;
    m.y += below;
    m.z = in;
    if ((uint64_t)m.y + m.z <= (uint64_t)cap) m.w = LF_DONE | LF_APPEND_EQ;
    else if (m.x == 64u) m.w = LF_DONE;
    meta[i] = m;
}

// sigma_s^2 and Phi(r / sigma_s) of a draw with h_s = 1 / (2 sigma_s^2): r / (sigma sqrt 2) = r sqrt(h)
__device__ __forceinline__ double draw_phi(double res, double sqrt_h) {
    return 0.5 * erfc(-(res * sqrt_h));
}

// PREDICT: besides sum w (body), pay[split][point][4] = sum w r, sum w (sigma^2 + r^2),
// sum w Phi(r / sigma), sum w^2 over the keys above the bucket, each in the order of `body`; and
// the draw index of every candidate next to its value (TileDraws only: it reads h_s).
template <bool PREDICT, class D, class... L>
__global__ __launch_bounds__(256) void loo_append_kernel(PassArgs a,
                                                         const uint64_t* __restrict__ prefix,
                                                         const uint64_t* __restrict__ kmin,
                                                         const uint4* __restrict__ meta,
                                                         uint32_t cap, uint32_t* __restrict__ count,
                                                         double* __restrict__ cand,
                                                         double* __restrict__ body,
                                                         uint32_t* __restrict__ candidx,
                                                         double* __restrict__ pay, L... lik) {
    __shared__ double As[SC_LDS_DOUBLES];
    __shared__ double Bs[SC_LDS_DOUBLES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, cl = lane & 15, kq = lane >> 4;
    const TilePos pos(a.point_tiles, a.tiles_per_split, a.draw_tiles);
    double yv[4], llmin[4], sum[4];
    double psum[PREDICT ? 4 : 1][4];
    uint64_t pre[4];
    uint32_t fixed[4], flags[4];
    int64_t pi[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        pi[r] = pos.p0 + 16 * wave + kq + 4 * r;
        const uint4 m = meta[pi[r]];
        yv[r] = a.yp[pi[r]];
        pre[r] = prefix[pi[r]];
        llmin[r] = key_value(kmin[pi[r]]);
        fixed[r] = m.x;
        flags[r] = m.w;
        sum[r] = 0.0;
        if constexpr (PREDICT)
#pragma unroll
            for (int f = 0; f < 4; ++f) psum[f][r] = 0.0;
    }
    score_tile_loop(a.Ap, a.theta, a.S, a.ldt, a.k, a.k_pad, pos.p0, pos.dt0, pos.dt1, As, Bs,
                    [&](int64_t s0, const f64x4(&acc)[4]) {
        const D d(a.ch, a.S, s0, cl, lik...);
        double s2[4], sq[4];
        if constexpr (PREDICT)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                s2[t] = 1.0 / (2.0 * d.hs[t]);
                sq[t] = sqrt(d.hs[t]);
            }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (flags[r] & LF_BAD) continue;
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (d.ok[t]) {
                    const double x = d.ll(yv[r], acc[t][r], t);
                    const uint64_t top = key_top(ord_key(x), fixed[r]);
                    if ((flags[r] & LF_NOTAIL) || top > pre[r]) {
                        const double w = exp(llmin[r] - x);
                        sum[r] += w;
                        if constexpr (PREDICT) {
                            const double res = yv[r] - acc[t][r];
                            psum[0][r] += w * res;
                            psum[1][r] += w * (s2[t] + res * res);
                            psum[2][r] += w * draw_phi(res, sq[t]);
                            psum[3][r] += w * w;
                        }
                    } else if (top < pre[r] || (flags[r] & LF_APPEND_EQ)) {
                        const uint32_t slot = atomicAdd(count + pi[r], 1u);
                        if (slot < cap) {
                            cand[pi[r] * (int64_t)cap + slot] = x;
                            if constexpr (PREDICT)
                                candidx[pi[r] * (int64_t)cap + slot] = (uint32_t)(s0 + cl + 16 * t);
                        }
                    }
                }
        }
    });
    // the 16 lanes that hold draws of the same point: a tree over cl, every lane the same bits
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const double v = lane_sum_ordered<16>(sum[r], cl);
        if (cl == 0) body[(int64_t)pos.split * a.n_pad + pi[r]] = v;
        if constexpr (PREDICT)
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                const double u = lane_sum_ordered<16>(psum[f][r], cl);
                if (cl == 0) pay[((int64_t)pos.split * a.n_pad + pi[r]) * 4 + f] = u;
            }
    }
}

// A point whose bucket is ONE value, repeated (settled with all 64 bits fixed): its draws are not
// candidates, and they share one weight.  bucket[split][point][3] = sum r, sum (sigma^2 + r^2),
// sum Phi(r / sigma) over them, in the order of `body`.  A workgroup without such a point (every
// one, for ordinary input) returns at once.
__global__ __launch_bounds__(256) void loo_bucket_kernel(PassArgs a,
                                                         const uint64_t* __restrict__ prefix,
                                                         const uint4* __restrict__ meta,
                                                         double* __restrict__ bucket) {
    __shared__ double As[SC_LDS_DOUBLES];
    __shared__ double Bs[SC_LDS_DOUBLES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, cl = lane & 15, kq = lane >> 4;
    const TilePos pos(a.point_tiles, a.tiles_per_split, a.draw_tiles);
    double yv[4], sum[3][4];
    uint64_t pre[4];
    bool live[4];
    int64_t pi[4];
    int any = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        pi[r] = pos.p0 + 16 * wave + kq + 4 * r;
        yv[r] = a.yp[pi[r]];
        pre[r] = prefix[pi[r]];
        live[r] = (meta[pi[r]].w & (LF_DONE | LF_APPEND_EQ | LF_NOTAIL | LF_BAD)) == LF_DONE;
        any |= live[r];
#pragma unroll
        for (int f = 0; f < 3; ++f) sum[f][r] = 0.0;
    }
    if (!__syncthreads_or(any)) return;
    score_tile_loop(a.Ap, a.theta, a.S, a.ldt, a.k, a.k_pad, pos.p0, pos.dt0, pos.dt1, As, Bs,
                    [&](int64_t s0, const f64x4(&acc)[4]) {
        const TileDraws d(a.ch, a.S, s0, cl);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (!live[r]) continue;
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (d.ok[t] && ord_key(d.ll(yv[r], acc[t][r], t)) == pre[r]) {
                    const double res = yv[r] - acc[t][r];
                    sum[0][r] += res;
                    sum[1][r] += 1.0 / (2.0 * d.hs[t]) + res * res;
                    sum[2][r] += draw_phi(res, sqrt(d.hs[t]));
                }
        }
    });
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int f = 0; f < 3; ++f) {
            const double u = lane_sum_ordered<16>(sum[f][r], cl);
            if (cl == 0 && live[r]) bucket[((int64_t)pos.split * a.n_pad + pi[r]) * 3 + f] = u;
        }
}

// ---- the PREDICT passes under the Student-t likelihood ----------------------------
// tc = [2][S]: v_s = sigma_s^2 nu_s / (nu_s - 2), the variance of draw s's predictive (0 for every
// draw of a call whose loo_sd is +inf: some nu_s <= 2), and nu_s; staged by loo_t_consts_kernel.
// F_nu(z) of a pair comes from what the pass has anyway: u = g_s r^2 is the argument of ll's log1p
// and |z| f_nu(z) = |r| exp(ll) (student_t_cdf_from, bmc_math.h).
__global__ __launch_bounds__(256) void loo_t_consts_kernel(const double* __restrict__ theta, int64_t S,
                                                           int64_t ldt, int32_t k, double nu_all,
                                                           const double* __restrict__ tab, int32_t n_nu,
                                                           const int32_t* __restrict__ index,
                                                           int32_t* __restrict__ flag, int32_t sd_inf,
                                                           double* __restrict__ tc) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const double nu = n_nu > 0 ? tab[n_nu + nu_index_clamped(index[s], n_nu, flag)] : nu_all;
    const double sg = theta[s * ldt + k];
    tc[s] = sd_inf ? 0.0 : (sg * sg) * (nu / (nu - 2.0));
    tc[S + s] = nu;
}

// row `row` of tc for the lane's 4 draws (a draw past S reads draw S - 1, as TileDraws does)
__device__ __forceinline__ void tile_row(const double* __restrict__ tc, int row, int64_t S, int64_t s0,
                                         int cl, double (&v)[4]) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int64_t sd = s0 + cl + 16 * t;
        v[t] = tc[row * S + (sd < S ? sd : S - 1)];
    }
}

// loo_append_kernel<true> in two phases, D = TileDrawsT or TileDrawsTV.  PHASE 0: the candidates
// with their draw indices, body = sum w, and pay[.][0] = sum w r, pay[.][1] = sum w (v_s + r^2),
// pay[.][3] = sum w^2 over the keys above the bucket.  PHASE 1: x and w recomputed the same way,
// pay[.][2] = sum w F_nu(r / sigma) alone.  Every sum in the order of `body`.
template <int PHASE, class D, class... L>
__global__ __launch_bounds__(256) void loo_append_t_kernel(PassArgs a,
                                                           const uint64_t* __restrict__ prefix,
                                                           const uint64_t* __restrict__ kmin,
                                                           const uint4* __restrict__ meta,
                                                           uint32_t cap, uint32_t* __restrict__ count,
                                                           double* __restrict__ cand,
                                                           double* __restrict__ body,
                                                           uint32_t* __restrict__ candidx,
                                                           double* __restrict__ pay,
                                                           const double* __restrict__ tc, L... lik) {
    __shared__ double As[SC_LDS_DOUBLES];
    __shared__ double Bs[SC_LDS_DOUBLES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, cl = lane & 15, kq = lane >> 4;
    const TilePos pos(a.point_tiles, a.tiles_per_split, a.draw_tiles);
    constexpr int N_SUMS = PHASE == 0 ? 4 : 1;   // PHASE 0: w, w r, w (v + r^2), w^2; PHASE 1: w F
    double yv[4], llmin[4], psum[N_SUMS][4];
    uint64_t pre[4];
    uint32_t fixed[4], flags[4];
    int64_t pi[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        pi[r] = pos.p0 + 16 * wave + kq + 4 * r;
        const uint4 m = meta[pi[r]];
        yv[r] = a.yp[pi[r]];
        pre[r] = prefix[pi[r]];
        llmin[r] = key_value(kmin[pi[r]]);
        fixed[r] = m.x;
        flags[r] = m.w;
#pragma unroll
        for (int f = 0; f < N_SUMS; ++f) psum[f][r] = 0.0;
    }
    score_tile_loop(a.Ap, a.theta, a.S, a.ldt, a.k, a.k_pad, pos.p0, pos.dt0, pos.dt1, As, Bs,
                    [&](int64_t s0, const f64x4(&acc)[4]) {
        const D d(a.ch, a.S, s0, cl, lik...);
        double row[4];   // PHASE 0: v_s; PHASE 1: nu_s
        tile_row(tc, PHASE, a.S, s0, cl, row);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (flags[r] & LF_BAD) continue;
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (d.ok[t]) {
                    const double x = d.ll(yv[r], acc[t][r], t);
                    const uint64_t top = key_top(ord_key(x), fixed[r]);
                    if ((flags[r] & LF_NOTAIL) || top > pre[r]) {
                        const double w = exp(llmin[r] - x);
                        const double res = yv[r] - acc[t][r];
                        if constexpr (PHASE == 0) {
                            psum[0][r] += w;
                            psum[1][r] += w * res;
                            psum[2][r] += w * (row[t] + res * res);
                            psum[3][r] += w * w;
                        } else {
                            psum[0][r] += w * student_t_cdf_from(res < 0.0, (res * res) * d.hs[t], row[t],
                                                                 fabs(res) * exp(x));
                        }
                    } else if (PHASE == 0 && (top < pre[r] || (flags[r] & LF_APPEND_EQ))) {
                        const uint32_t slot = atomicAdd(count + pi[r], 1u);
                        if (slot < cap) {
                            cand[pi[r] * (int64_t)cap + slot] = x;
                            candidx[pi[r] * (int64_t)cap + slot] = (uint32_t)(s0 + cl + 16 * t);
                        }
                    }
                }
        }
    });
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t o = (int64_t)pos.split * a.n_pad + pi[r];
#pragma unroll
        for (int f = 0; f < N_SUMS; ++f) {
            const double u = lane_sum_ordered<16>(psum[f][r], cl);
            if (cl != 0) continue;
            if (PHASE == 1) pay[o * 4 + 2] = u;
            else if (f == 0) body[o] = u;
            else pay[o * 4 + (f == 3 ? 3 : f - 1)] = u;
        }
    }
}

// loo_bucket_kernel under the t likelihood: bucket[split][point][3] = sum r, sum (v_s + r^2),
// sum F_nu(r / sigma) over the draws of a one-value bucket
template <class D, class... L>
__global__ __launch_bounds__(256) void loo_bucket_t_kernel(PassArgs a,
                                                           const uint64_t* __restrict__ prefix,
                                                           const uint4* __restrict__ meta,
                                                           double* __restrict__ bucket,
                                                           const double* __restrict__ tc, L... lik) {
    __shared__ double As[SC_LDS_DOUBLES];
    __shared__ double Bs[SC_LDS_DOUBLES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, cl = lane & 15, kq = lane >> 4;
    const TilePos pos(a.point_tiles, a.tiles_per_split, a.draw_tiles);
    double yv[4], sum[3][4];
    uint64_t pre[4];
    bool live[4];
    int64_t pi[4];
    int any = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        pi[r] = pos.p0 + 16 * wave + kq + 4 * r;
        yv[r] = a.yp[pi[r]];
        pre[r] = prefix[pi[r]];
        live[r] = (meta[pi[r]].w & (LF_DONE | LF_APPEND_EQ | LF_NOTAIL | LF_BAD)) == LF_DONE;
        any |= live[r];
#pragma unroll
        for (int f = 0; f < 3; ++f) sum[f][r] = 0.0;
    }
    if (!__syncthreads_or(any)) return;
    score_tile_loop(a.Ap, a.theta, a.S, a.ldt, a.k, a.k_pad, pos.p0, pos.dt0, pos.dt1, As, Bs,
                    [&](int64_t s0, const f64x4(&acc)[4]) {
        const D d(a.ch, a.S, s0, cl, lik...);
        double vs[4], nus[4];
        tile_row(tc, 0, a.S, s0, cl, vs);
        tile_row(tc, 1, a.S, s0, cl, nus);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (!live[r]) continue;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (!d.ok[t]) continue;
                const double x = d.ll(yv[r], acc[t][r], t);
                if (ord_key(x) == pre[r]) {
                    const double res = yv[r] - acc[t][r];
                    sum[0][r] += res;
                    sum[1][r] += vs[t] + res * res;
                    sum[2][r] += student_t_cdf_from(res < 0.0, (res * res) * d.hs[t], nus[t],
                                                    fabs(res) * exp(x));
                }
            }
        }
    });
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int f = 0; f < 3; ++f) {
            const double u = lane_sum_ordered<16>(sum[f][r], cl);
            if (cl == 0 && live[r]) bucket[((int64_t)pos.split * a.n_pad + pi[r]) * 3 + f] = u;
        }
}

// What the PREDICT fit reads besides the select state: the padded operands and per-draw constants
// of the score kernels (a candidate's r and sigma are recomputed from its draw index), the
// candidates' draw indices and the payload sums of loo_append_kernel<true> and loo_bucket_kernel.
struct FitPayload {
    const double *Ap, *yp, *theta, *ch, *pay, *bucket;
    const uint32_t* candidx;
    int64_t ldt;
    int32_t k, k_pad;
};

// out[2 .. 5][i] from the point's sums over all draws: W = sum w, then sum w r, sum w (sigma^2 + r^2),
// sum w Phi, sum w^2
__device__ __forceinline__ void predict_store(double* __restrict__ out, int64_t n, int64_t i,
                                              double y, double W, const double (&t)[4]) {
    const double mr = t[0] / W;
    out[2 * n + i] = y - mr;
    out[3 * n + i] = sqrt(t[1] / W - mr * mr);
    out[4 * n + i] = t[2] / W;
    out[5 * n + i] = W * (W / t[3]);
}

// What the fit under the t likelihood takes besides: tc of loo_t_consts_kernel and the call's sd_inf
struct TFit {
    const double* tc;
    int32_t sd_inf;
};
__device__ __forceinline__ const double* fit_tc() { return nullptr; }
__device__ __forceinline__ const double* fit_tc(const TFit& t) { return t.tc; }
__device__ __forceinline__ bool fit_sd_inf() { return false; }
__device__ __forceinline__ bool fit_sd_inf(const TFit& t) { return t.sd_inf != 0; }

// One workgroup per point.  buf: `cap` doubles of LDS, cap >= 2 (M + 1): the sorted candidates in
// buf[0 .. M] and, behind them, M doubles for the tail's x_j and then its smoothed lw.  mg: the
// grid points of the fit (LooPlan::grid_points).
// PREDICT: 16 bytes of LDS per slot: every sorted candidate stays in buf[0 .. cap), the tail's M
// doubles are buf[cap .. cap + cap / 2), then the candidates' draw indices, sorted along as the
// second key; out is [6][n]: elpd_loo_i, pareto_k, loo_mean, loo_sd, loo_pit, ess.
// T...: nothing, or one TFit: the fit under the Student-t likelihood (STUDENT; with PREDICT), the
// payload of a candidate from v_s and nu_s of tc and F_nu from the candidate's own ll.  Without it
// the kernel has the arguments and the code of the untemplated one.
template <bool PREDICT, class... T>
__global__ __launch_bounds__(256) void loo_fit_kernel(const uint64_t* __restrict__ prefix,
                                                      const uint64_t* __restrict__ kmin,
                                                      const uint4* __restrict__ meta,
                                                      const uint32_t* __restrict__ count,
                                                      const double* __restrict__ cand,
                                                      const double* __restrict__ body, int64_t n,
                                                      int64_t n_pad, int64_t splits, int64_t S,
                                                      int32_t M, int32_t mg, int32_t cap,
                                                      double* __restrict__ out, FitPayload pa,
                                                      T... tfit) {
    constexpr bool STUDENT = sizeof...(T) > 0;
    const double* tc = fit_tc(tfit...);
    const bool sd_inf = fit_sd_inf(tfit...);

    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double* buf = (double*)smem_raw;
    __shared__ double red[256];
    __shared__ double g_theta[LOO_MAX_GRID], g_l[LOO_MAX_GRID], g_w[LOO_MAX_GRID];
    const int tid = threadIdx.x;
    const int64_t i = blockIdx.x;
    const uint4 m = meta[i];
    const double inf = __builtin_inf();
    constexpr int N_OUT = PREDICT ? 6 : 2;
    if (m.w & LF_BAD) {
        if (tid == 0)
            for (int f = 0; f < N_OUT; ++f) out[f * n + i] = __builtin_nan("");
        return;
    }
    const double llmin = key_value(kmin[i]);   // -c_i
    double B = 0.0;
    for (int64_t sp = 0; sp < splits; ++sp) B += body[sp * n_pad + i];
    double tot[4] = {0.0, 0.0, 0.0, 0.0};   // PREDICT: the payload sums over all draws
    if constexpr (PREDICT)
        for (int64_t sp = 0; sp < splits; ++sp)
            for (int f = 0; f < 4; ++f) tot[f] += pa.pay[(sp * n_pad + i) * 4 + f];
    if (m.w & LF_NOTAIL) {
        // raw importance sampling: every ll + lw is -c
        if (tid == 0) {
            out[i] = (log((double)S) + llmin) - log(B);
            out[n + i] = inf;
            if constexpr (PREDICT) predict_store(out, n, i, pa.yp[i], B, tot);
            if constexpr (STUDENT)
                if (sd_inf) out[3 * n + i] = inf;
        }
        return;
    }

    // ---- sort ------------------------------------------------------------------------------
    const uint32_t cnt_raw = count[i];
    const int c_n = (int)(cnt_raw < (uint32_t)cap ? cnt_raw : (uint32_t)cap);
    if ((m.w & LF_APPEND_EQ) ? c_n <= M : c_n != (int)m.y) {
        // the slots do not hold what the select counted: cannot happen; a value, not a wild read
        if (tid == 0)
            for (int f = 0; f < N_OUT; ++f) out[f * n + i] = __builtin_nan("");
        return;
    }
    int P2 = 2;
    while (P2 < c_n) P2 <<= 1;
    uint32_t* ids = (uint32_t*)(buf + cap + cap / 2);   // (PREDICT)
    for (int j = tid; j < P2; j += 256) {
        buf[j] = j < c_n ? cand[i * (int64_t)cap + j] : inf;
        if constexpr (PREDICT) ids[j] = j < c_n ? pa.candidx[i * (int64_t)cap + j] : ~0u;
    }
    __syncthreads();
    for (int ks = 2; ks <= P2; ks <<= 1)
        for (int j = ks >> 1; j > 0; j >>= 1) {
            for (int e = tid; e < P2; e += 256) {
                const int o = e ^ j;
                if (o > e) {
                    const double x = buf[e], y = buf[o];
                    if constexpr (PREDICT) {
                        // by value, then by draw: one layout whatever the slot order was
                        const uint32_t ix = ids[e], iy = ids[o];
                        const bool gt = x > y || (x == y && ix > iy), lt = x < y || (x == y && ix < iy);
                        if ((e & ks) == 0 ? gt : lt) {
                            buf[e] = y;
                            buf[o] = x;
                            ids[e] = iy;
                            ids[o] = ix;
                        }
                    } else if ((e & ks) == 0 ? x > y : x < y) {
                        buf[e] = y;
                        buf[o] = x;
                    }
                }
            }
            __syncthreads();
        }

    // ---- the body's share of the bucket -------------------------------------------------------
    double extra;
    if (m.w & LF_APPEND_EQ) {
        // candidates M .. c_n - 1 (the cutoff and what else of the bucket is not in the tail)
        double part = 0.0;
        for (int j = M + tid; j < c_n; j += 256) part += exp(llmin - buf[j]);
        extra = block_sum(part, red);
    } else {
        // the bucket is one value v, repeated m.z times; the slots hold the m.y keys below it
        const double v = key_value(prefix[i]);
        __syncthreads();
        for (int j = c_n + tid; j <= M; j += 256) buf[j] = v;
        __syncthreads();
        extra = (double)((int64_t)m.y + (int64_t)m.z - (int64_t)M) * exp(llmin - v);
    }
    const double Btot = B + extra;
    const double cut = llmin - buf[M];   // cutoff, as lw
    const double ecut = exp(cut);
    bool smooth = buf[0] != buf[M - 1];
    PsisFit fit{inf, 0.0, false};
    double* xs = PREDICT ? buf + cap : buf + M + 1;
    __syncthreads();   // (buf[M + 1 ..] has been read above)

    // ---- generalised Pareto fit (bmc_psis.h) on the exceedances over the cutoff, ascending ------
    if (smooth) {
        for (int j = tid; j < M; j += 256) xs[j] = exp(llmin - buf[M - 1 - j]) - ecut;
        __syncthreads();
        fit = psis_fit(xs, M, mg, red, g_theta, g_l, g_w);
        if (!fit.finite) {
            fit.khat = inf;
            smooth = false;
        }
    }

    // ---- the tail's weights, smoothed or raw, truncated at 0; then elpd_loo_i -----------------
    double dpart = 0.0, mpart = -inf;
    for (int j = tid; j < M; j += 256) {
        const double llj = buf[M - 1 - j];
        double lw = smooth ? psis_smoothed_lw(j, M, fit, ecut) : llmin - llj;
        lw = lw > 0.0 ? 0.0 : lw;
        xs[j] = lw;
        dpart += exp(lw);
        mpart = fmax(mpart, llj + lw);
    }
    const double wsum = Btot + block_sum(dpart, red);
    const double den = log(wsum);
    const double mx = fmax(block_max(mpart, red), llmin);
    double npart = 0.0;
    for (int j = tid; j < M; j += 256) npart += exp((buf[M - 1 - j] + xs[j]) - mx);
    const double num = mx + log((double)(S - M) * exp(llmin - mx) + block_sum(npart, red));
    if (tid == 0) {
        out[i] = num - den;
        out[n + i] = fit.khat;
    }

    if constexpr (PREDICT) {
        // ---- ties share: every draw of a run of equal ll gets the mean W of the run's ranks ------
        // xs[j] becomes W of rank M - 1 - j; the one run that may cross rank M (its other ranks
        // carry the raw weight) is remembered: ranks M .. cross_end - 1 have weight cross_w.  A
        // one-value bucket is such a run, of ranks m.y .. m.y + m.z - 1 (buf[m.y .. M] stand for it).
        // A run is found with == on doubles while the select works on keys, for which -0 < +0: a
        // point whose ll take BOTH zeros (ll exactly 0 under two draws, one of each sign) could have
        // that run cut at the bucket's edge and its two parts not share.  The fma of TileDraws::ll
        // gives -0 only for c_s = -0 and a zero residual, so this is not reachable in practice.
        // One thread sums and rewrites its run in rank order (at most M ranks of it are in the
        // tail): the time of this step grows with the longest run of ties in a point's tail.
        __shared__ long long cross_end;
        __shared__ double cross_w;
        const bool eq = (m.w & LF_APPEND_EQ) != 0;
        const int n_valid = eq ? c_n : M + 1;
        const long long n_ranks = eq ? (long long)c_n : (long long)m.y + (long long)m.z;
        if (tid == 0) {
            cross_end = M;
            cross_w = 0.0;
        }
        for (int j = tid; j < M; j += 256) xs[j] = exp(xs[j]);
        __syncthreads();
        for (int q = tid; q < M; q += 256) {
            const double v = buf[q];
            if (q > 0 && buf[q - 1] == v) continue;   // (the run's first rank does the work)
            int lo = q + 1, hi = n_valid;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (buf[mid] == v) lo = mid + 1;
                else hi = mid;
            }
            const long long end = (!eq && lo == n_valid) ? n_ranks : (long long)lo;
            if (end - q < 2) continue;
            const int t_end = end < (long long)M ? (int)end : M;
            double sw = 0.0;
            for (int p = q; p < t_end; ++p) sw += xs[M - 1 - p];
            if (end > (long long)M) sw += (double)(end - M) * exp(llmin - v);
            const double wbar = sw / (double)(end - q);
            for (int p = q; p < t_end; ++p) xs[M - 1 - p] = wbar;
            if (end > (long long)M) {
                cross_end = end;
                cross_w = wbar;
            }
        }
        __syncthreads();

        // ---- the candidates' payload, then the bucket's and the body's ------------------------------
        const double* arow = pa.Ap + i * (int64_t)pa.k_pad;
        const double yi = pa.yp[i];
        double part[4] = {0.0, 0.0, 0.0, 0.0};
        for (int q = tid; q < c_n; q += 256) {
            const double w = q < M ? xs[M - 1 - q]
                                   : ((long long)q < cross_end ? cross_w : exp(llmin - buf[q]));
            const int64_t sd = (int64_t)ids[q] < S ? (int64_t)ids[q] : S - 1;
            const double* th = pa.theta + sd * pa.ldt;
            double dot = 0.0;
            for (int j = 0; j < pa.k; ++j) dot = fma(arow[j], th[j], dot);
            const double res = yi - dot, h = pa.ch[S + sd];   // (STUDENT: h is g_s)
            part[0] += w * res;
            if constexpr (STUDENT) {
                part[1] += w * (tc[sd] + res * res);
                part[2] += w * student_t_cdf_from(res < 0.0, (res * res) * h, tc[S + sd],
                                                  fabs(res) * exp(buf[q]));
            } else {
                part[1] += w * (1.0 / (2.0 * h) + res * res);
                part[2] += w * draw_phi(res, sqrt(h));
            }
            part[3] += w * w;
        }
        for (int f = 0; f < 4; ++f) tot[f] += block_sum(part[f], red);
        if (!eq) {
            const double wb = (int)m.y < M ? cross_w : exp(llmin - key_value(prefix[i]));
            double bs[3] = {0.0, 0.0, 0.0};
            for (int64_t sp = 0; sp < splits; ++sp)
                for (int f = 0; f < 3; ++f) bs[f] += pa.bucket[(sp * n_pad + i) * 3 + f];
            for (int f = 0; f < 3; ++f) tot[f] += wb * bs[f];
            tot[3] += (double)m.z * (wb * wb);
        }
        if (tid == 0) predict_store(out, n, i, yi, wsum, tot);
        if constexpr (STUDENT)   // (some nu_s <= 2: the predictive variance is infinite)
            if (tid == 0 && sd_inf) out[3 * n + i] = inf;
    }
}

struct Work {
    uint64_t *range, *prefix, *kmin;
    uint4* meta;
    uint32_t *hist, *count;
    double *cand, *body, *out;
    char* end;
    Work(void* base, const LooBuffers& b) {
        char* p = (char*)base;
        auto take = [&](size_t bytes) {
            char* q = p;
            p += bytes;
            return q;
        };
        range = (uint64_t*)take(b.range);
        prefix = (uint64_t*)take(b.prefix);
        kmin = (uint64_t*)take(b.kmin);
        meta = (uint4*)take(b.meta);
        hist = (uint32_t*)take(b.hist);
        count = (uint32_t*)take(b.count);
        cand = (double*)take(b.cand);
        body = (double*)take(b.body);
        out = (double*)take(b.out);
        end = p;
    }
};

// The PREDICT passes' own buffers, behind the ones every call has
struct PredictWork {
    uint32_t* candidx;
    double *pay, *bucket, *out, *tc;
    PredictWork(const Work& w, const LooPredictBuffers& b) {
        char* p = w.end;
        candidx = (uint32_t*)p;
        pay = (double*)(p += b.candidx);
        bucket = (double*)(p += b.pay);
        out = (double*)(p += b.bucket);
        tc = (double*)(p += b.out);
    }
};

}  // namespace

double* loo_out(const LooArgs& a, const LooPlan& p) {
    return Work(a.work, loo_buffers(p, a.score.n)).out;
}

double* loo_predict_out(const LooArgs& a, const LooPredictPlan& p) {
    const LooPredictBuffers b = loo_predict_buffers(p, a.score.n);
    return PredictWork(Work(a.work, b.loo), b).out;
}

namespace {

// Both calls: the score kernels, then range, init, select and scan; then append and fit, or their
// PREDICT variants with the bucket pass between them (pp != nullptr).
hipError_t launch_loo_passes(const LooArgs& a, const LooPlan& p, const LooPredictPlan* pp,
                             hipStream_t s) {
    const ScoreArgs& sa = a.score;
    const ScorePlan& sp = p.score;
    if (!p.ok || !a.work || sa.S - p.tail < 1 || p.cap < 2 * (p.tail + 1) || p.cap > LOO_MAX_CAP ||
        (p.cap & (p.cap - 1)) != 0 || p.tail != loo_tail(sa.S) || sa.n > 0x7fffffffll ||
        p.grid_points != (p.tail > 0 ? psis_grid_points(p.tail) : 0) || p.grid_points > LOO_MAX_GRID)
        return hipErrorInvalidValue;   // (the fit's grid is one workgroup per point)
    hipError_t e = launch_score(sa, sp, s);   // (checks the shapes and the split plan)
    if (e != hipSuccess) return e;
    const LooBuffers lb = loo_buffers(p, sa.n);
    const Work w(a.work, lb);
    const int64_t n_pad = sp.point_tiles * SC_TM;
    const unsigned groups = (unsigned)((uint64_t)sp.splits * (uint64_t)sp.point_tiles);
    const unsigned pblocks = (unsigned)((n_pad + 255) / 256);
    const int32_t M = (int32_t)p.tail, cap = (int32_t)p.cap;
    PassArgs pa;
    pa.Ap = sa.Ap;
    pa.yp = sa.yp;
    pa.theta = sa.theta;
    pa.ch = sa.ch;
    pa.S = sa.S;
    pa.ldt = sa.ldt;
    pa.tiles_per_split = sp.tiles_per_split;
    pa.draw_tiles = sp.draw_tiles;
    pa.n_pad = n_pad;
    pa.k = sa.k;
    pa.k_pad = sp.k_pad;
    pa.point_tiles = (uint32_t)sp.point_tiles;

    // a pass over the matrix under the call's likelihood (launch_score has checked sa.nu)
    const bool student = sa.nu > 0.0, per_draw = sa.per_draw.n_nu > 0;
    const double hn = 0.5 * (sa.nu + 1.0);
    auto pass = [&](auto gauss, auto student_t, auto student_tv, size_t lds, auto... args) {
        if (per_draw) hipLaunchKernelGGL(student_tv, dim3(groups), dim3(256), lds, s, pa, args...);
        else if (student) hipLaunchKernelGGL(student_t, dim3(groups), dim3(256), lds, s, pa, args..., hn);
        else hipLaunchKernelGGL(gauss, dim3(groups), dim3(256), lds, s, pa, args...);
    };

    auto pass_t = [&](auto student_t, auto student_tv, auto... args) {   // (the t-only kernels)
        if (per_draw) hipLaunchKernelGGL(student_tv, dim3(groups), dim3(256), 0, s, pa, args...);
        else hipLaunchKernelGGL(student_t, dim3(groups), dim3(256), 0, s, pa, args..., hn);
    };

    if ((e = hipMemsetAsync(w.hist, 0, lb.hist, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(w.count, 0, lb.count, s)) != hipSuccess) return e;
    pass(loo_range_kernel<TileDraws>, loo_range_kernel<TileDrawsT, double>, loo_range_kernel<TileDrawsTV>, 0,
         w.range);
    hipLaunchKernelGGL(loo_init_kernel, dim3(pblocks), dim3(256), 0, s, (const uint64_t*)w.range,
                       n_pad, sp.splits, sa.S, M, cap, w.prefix, w.kmin, w.meta);
    if (p.select_passes > 0) {
        e = hipFuncSetAttribute(per_draw  ? (const void*)loo_select_kernel<TileDrawsTV>
                                : student ? (const void*)loo_select_kernel<TileDrawsT, double>
                                          : (const void*)loo_select_kernel<TileDraws>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)LOO_SELECT_LDS);
        if (e != hipSuccess) return e;
        for (int sel = 0; sel < p.select_passes; ++sel) {
            pass(loo_select_kernel<TileDraws>, loo_select_kernel<TileDrawsT, double>,
                 loo_select_kernel<TileDrawsTV>, LOO_SELECT_LDS,
                 (const uint64_t*)w.prefix, (const uint4*)w.meta, w.hist);
            hipLaunchKernelGGL(loo_scan_kernel, dim3(pblocks), dim3(256), 0, s, n_pad, M, cap,
                               w.prefix, w.meta, w.hist);
        }
    }
    if (pp && (student || per_draw)) {
        // the PREDICT passes under the t likelihood: both phases of the append, the bucket, the fit
        const PredictWork pw(w, loo_predict_buffers(*pp, sa.n));
        const NuPerDraw& v = sa.per_draw;
        const int32_t sd_inf = a.t_sd_inf ? 1 : 0;
        hipLaunchKernelGGL(loo_t_consts_kernel, dim3((unsigned)((sa.S + 255) / 256)), dim3(256), 0, s,
                           sa.theta, sa.S, sa.ldt, sa.k, sa.nu, v.tab, v.n_nu, v.index, v.flag, sd_inf,
                           pw.tc);
        const double* tc = pw.tc;
        pass_t(loo_append_t_kernel<0, TileDrawsT, double>, loo_append_t_kernel<0, TileDrawsTV>,
             (const uint64_t*)w.prefix, (const uint64_t*)w.kmin, (const uint4*)w.meta, (uint32_t)cap,
             w.count, w.cand, w.body, pw.candidx, pw.pay, tc);
        pass_t(loo_append_t_kernel<1, TileDrawsT, double>, loo_append_t_kernel<1, TileDrawsTV>,
             (const uint64_t*)w.prefix, (const uint64_t*)w.kmin, (const uint4*)w.meta, (uint32_t)cap,
             w.count, w.cand, w.body, pw.candidx, pw.pay, tc);
        if (pp->bucket_pass)
            pass_t(loo_bucket_t_kernel<TileDrawsT, double>, loo_bucket_t_kernel<TileDrawsTV>,
                 (const uint64_t*)w.prefix, (const uint4*)w.meta, pw.bucket, tc);
        FitPayload fp;
        fp.Ap = sa.Ap;
        fp.yp = sa.yp;
        fp.theta = sa.theta;
        fp.ch = sa.ch;
        fp.pay = pw.pay;
        fp.bucket = pw.bucket;
        fp.candidx = pw.candidx;
        fp.ldt = sa.ldt;
        fp.k = sa.k;
        fp.k_pad = sp.k_pad;
        e = hipFuncSetAttribute((const void*)loo_fit_kernel<true, TFit>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)pp->fit_lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((loo_fit_kernel<true, TFit>), dim3((unsigned)sa.n), dim3(256), (size_t)pp->fit_lds, s,
                           (const uint64_t*)w.prefix, (const uint64_t*)w.kmin, (const uint4*)w.meta,
                           (const uint32_t*)w.count, (const double*)w.cand, (const double*)w.body, sa.n,
                           n_pad, sp.splits, sa.S, M, p.grid_points, cap, pw.out, fp, TFit{tc, sd_inf});
        return hipGetLastError();
    }
    if (pp) {
        const PredictWork pw(w, loo_predict_buffers(*pp, sa.n));
        hipLaunchKernelGGL((loo_append_kernel<true, TileDraws>), dim3(groups), dim3(256), 0, s, pa,
                           (const uint64_t*)w.prefix, (const uint64_t*)w.kmin,
                           (const uint4*)w.meta, (uint32_t)cap, w.count, w.cand, w.body, pw.candidx,
                           pw.pay);
        if (pp->bucket_pass)
            hipLaunchKernelGGL(loo_bucket_kernel, dim3(groups), dim3(256), 0, s, pa,
                               (const uint64_t*)w.prefix, (const uint4*)w.meta, pw.bucket);
        FitPayload fp;
        fp.Ap = sa.Ap;
        fp.yp = sa.yp;
        fp.theta = sa.theta;
        fp.ch = sa.ch;
        fp.pay = pw.pay;
        fp.bucket = pw.bucket;
        fp.candidx = pw.candidx;
        fp.ldt = sa.ldt;
        fp.k = sa.k;
        fp.k_pad = sp.k_pad;
        e = hipFuncSetAttribute((const void*)loo_fit_kernel<true>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)pp->fit_lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(loo_fit_kernel<true>, dim3((unsigned)sa.n), dim3(256),
                           (size_t)pp->fit_lds, s, (const uint64_t*)w.prefix,
                           (const uint64_t*)w.kmin, (const uint4*)w.meta, (const uint32_t*)w.count,
                           (const double*)w.cand, (const double*)w.body, sa.n, n_pad, sp.splits, sa.S,
                           M, p.grid_points, cap, pw.out, fp);
        return hipGetLastError();
    }
    pass(loo_append_kernel<false, TileDraws>, loo_append_kernel<false, TileDrawsT, double>,
         loo_append_kernel<false, TileDrawsTV>, 0,
         (const uint64_t*)w.prefix, (const uint64_t*)w.kmin, (const uint4*)w.meta, (uint32_t)cap,
         w.count, w.cand, w.body, (uint32_t*)nullptr, (double*)nullptr);
    const size_t fit_lds = (size_t)cap * 8;
    e = hipFuncSetAttribute((const void*)loo_fit_kernel<false>,
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)fit_lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(loo_fit_kernel<false>, dim3((unsigned)sa.n), dim3(256), fit_lds, s,
                       (const uint64_t*)w.prefix, (const uint64_t*)w.kmin, (const uint4*)w.meta,
                       (const uint32_t*)w.count, (const double*)w.cand, (const double*)w.body, sa.n,
                       n_pad, sp.splits, sa.S, M, p.grid_points, cap, w.out, FitPayload{});
    return hipGetLastError();
}

}  // namespace

hipError_t launch_loo(const LooArgs& a, const LooPlan& p, hipStream_t s) {
    return launch_loo_passes(a, p, nullptr, s);
}

hipError_t launch_loo_predict(const LooArgs& a, const LooPredictPlan& p, hipStream_t s) {
    const bool student = a.score.nu != 0.0 || a.score.per_draw.n_nu != 0;
    if (!p.ok || p.loo.cap > LOO_PREDICT_MAX_CAP || p.fit_lds != p.loo.cap * LOO_PREDICT_SLOT_LDS ||
        p.append_phases != (student ? LOO_PREDICT_T_PHASES : 1) ||
        p.draw_rows != (student ? (int64_t)LOO_PREDICT_T_ROWS * a.score.S : 0))
        return hipErrorInvalidValue;
    return launch_loo_passes(a, p.loo, &p, s);
}

}  // namespace bmc
