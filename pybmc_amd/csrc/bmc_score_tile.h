// The tile loop shared by the kernels that walk ll[i][s] without storing it (kernels_waic.hip,
// kernels_loo.hip): a workgroup of 256 threads owns SCORE_TILE points and walks draw tiles of
// SCORE_TILE draws; a_i . beta_s on v_mfma_f64_16x16x4_f64 (staging and LDS layout of
// predict_gemm_kernel; the draws are read from theta in place, any ldt).  Every tile is handed to
// the caller's epilogue in registers and never stored.
#pragma once
#include "bmc_dev.h"
#include "bmc_plan.h"

namespace bmc {

using f64x4 = __attribute__((ext_vector_type(4))) double;

constexpr int SC_KT = 16, SC_LD = 18, SC_TM = SCORE_TILE;
constexpr int SC_LDS_DOUBLES = 2 * SC_TM * SC_LD;   // each of As and Bs
constexpr double HALF_LOG_2PI = 0.91893853320467274178;

// Walks draw tiles dt0 .. dt1 - 1 of point tile p0 .. p0 + 63.  Ap is the padded design
// ([n_pad][k_pad], zero in the padding); As and Bs are SC_LDS_DOUBLES doubles of LDS each.  After
// each tile: epi(s0, acc), where lane (cl = lane & 15, kq = lane >> 4) of wave w holds
//   acc[t][r] = a_i . beta_s,  i = p0 + 16 w + kq + 4 r,  s = s0 + cl + 16 t
// (MFMA D: row = kq + 4 reg).  A draw past S holds draw S - 1's product: the epilogue drops it.
template <class Epi>
__device__ __forceinline__ void score_tile_loop(const double* __restrict__ Ap,
                                                const double* __restrict__ theta, int64_t S,
                                                int64_t ldt, int32_t k, int32_t k_pad, int64_t p0,
                                                int64_t dt0, int64_t dt1, double* As, double* Bs,
                                                Epi&& epi) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cl = lane & 15, kq = lane >> 4;

    // staging: element tid + 256 q of a 64 x 16 slab -> row sr + 16 q, column sc
    const int sr = tid >> 4, sc = tid & 15;
    const double* arow = Ap + (p0 + sr) * k_pad + sc;   // rows 16 k_pad apart, no bounds: padded
    const double* brow[4];
    double ra[4], rb[4];
    // theta is read in place: a draw past S reads draw S - 1 (its ll is dropped in the epilogue),
    // a column past k reads column k (in bounds) and stages 0
    auto point_rows = [&](int64_t s0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t sd = s0 + sr + 16 * q;
            brow[q] = theta + (sd < S ? sd : S - 1) * ldt;
        }
    };
    auto fetch = [&](int m0) {
        const int j = m0 + sc;
        const int jc = j < k ? j : k;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            ra[q] = arow[(int64_t)(16 * q) * k_pad + m0];
            const double v = brow[q][jc];
            rb[q] = j < k ? v : 0.0;
        }
    };
    double* as_w = As + sr * SC_LD + sc;
    double* bs_w = Bs + sr * SC_LD + sc;
    auto stash = [&](int buf) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            as_w[(buf * SC_TM + 16 * q) * SC_LD] = ra[q];
            bs_w[(buf * SC_TM + 16 * q) * SC_LD] = rb[q];
        }
    };
    const double* a_r = As + (16 * wave + cl) * SC_LD + kq;
    const double* b_r = Bs + cl * SC_LD + kq;
    const int nslab = k_pad / SC_KT;
    const int last_nk = (k - SC_KT * (nslab - 1) + 3) / 4;   // k-steps of the last slab, 1 .. 4

    point_rows(dt0 * SC_TM);
    fetch(0);
    for (int64_t dt = dt0; dt < dt1; ++dt) {
        const int64_t s0 = dt * SC_TM;
        f64x4 acc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
        stash(0);
        __syncthreads();
        for (int sl = 0; sl + 1 < nslab; ++sl) {
            const int buf = sl & 1;
            fetch((sl + 1) * SC_KT);
            const double* Ab = a_r + buf * SC_TM * SC_LD;
            const double* Bb = b_r + buf * SC_TM * SC_LD;
#pragma unroll
            for (int kk = 0; kk < SC_KT / 4; ++kk) {
                const double a = Ab[4 * kk];
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Bb[16 * t * SC_LD + 4 * kk],
                                                                  acc[t], 0, 0, 0);
            }
            stash(buf ^ 1);
            __syncthreads();
        }
        {
            const int buf = (nslab - 1) & 1;
            const double* Ab = a_r + buf * SC_TM * SC_LD;
            const double* Bb = b_r + buf * SC_TM * SC_LD;
            for (int kk = 0; kk < last_nk; ++kk) {
                const double a = Ab[4 * kk];
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Bb[16 * t * SC_LD + 4 * kk],
                                                                  acc[t], 0, 0, 0);
            }
        }
        // every wave is done with the LDS slabs before the next tile's first slab lands there;
        // its global reads are issued now and wait behind the epilogue
        __syncthreads();
        if (dt + 1 < dt1) {
            point_rows(s0 + SC_TM);
            fetch(0);
        }
        epi(s0, acc);
    }
}

// The epilogue's view of a tile: ll = c_s - h_s (y_i - a_i . beta_s)^2 for the lane's 4 draws
// (ch = [2][S]: c_s = -1/2 log(2 pi) - log sigma_s, h_s = 1 / (2 sigma_s^2)); ok[t]: draw exists.
struct TileDraws {
    double cs[4], hs[4];
    bool ok[4];
    __device__ __forceinline__ TileDraws(const double* __restrict__ ch, int64_t S, int64_t s0, int cl) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int64_t sd = s0 + cl + 16 * t;
            ok[t] = sd < S;
            const int64_t sdc = ok[t] ? sd : S - 1;
            cs[t] = ch[sdc];
            hs[t] = ch[S + sdc];
        }
    }
    __device__ __forceinline__ double ll(double y, double dot, int t) const {
        const double res = y - dot;
        return fma(-(hs[t] * res), res, cs[t]);
    }
};

// The same view under the Student-t density with nu degrees of freedom, the latent row weights
// integrated out: ll = c_s - (nu + 1)/2 log1p(g_s r^2), with ch = [2][S] holding
// c_s = lgamma((nu + 1)/2) - lgamma(nu/2) - 1/2 log(nu pi) - log sigma_s in place of the Gaussian
// constant and g_s = 1 / (nu sigma_s^2) in place of h_s (so hs[] is g_s here); hn = (nu + 1)/2 is
// the likelihood's one kernel scalar.  The kernels that walk the matrix are templates on the draws
// type <D, L...>: L... are the scalars D's constructor takes behind TileDraws' own, none for
// TileDraws (those instantiations have the arguments and the code of the untemplated kernels).
struct TileDrawsT : TileDraws {
    double hn;
    __device__ __forceinline__ TileDrawsT(const double* __restrict__ ch, int64_t S, int64_t s0, int cl,
                                          double half_nu1)
        : TileDraws(ch, S, s0, cl), hn(half_nu1) {}
    __device__ __forceinline__ double ll(double y, double dot, int t) const {
        const double res = y - dot;
        return fma(-hn, log1p_nonneg((res * res) * hs[t]), cs[t]);
    }
};

// The Student-t view with degrees of freedom of each draw's own (a fit that estimated nu): ch =
// [3][S] holds c_s and g_s = 1 / (nu_s sigma_s^2) as TileDrawsT reads them at nu = nu_s, and
// hn_s = (nu_s + 1)/2 in its third row; no kernel scalar.  With one nu for all draws the three rows
// and the arithmetic are TileDrawsT's.
struct TileDrawsTV : TileDraws {
    double hn[4];
    __device__ __forceinline__ TileDrawsTV(const double* __restrict__ ch, int64_t S, int64_t s0, int cl)
        : TileDraws(ch, S, s0, cl) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int64_t sd = s0 + cl + 16 * t;
            hn[t] = ch[2 * S + (sd < S ? sd : S - 1)];
        }
    }
    __device__ __forceinline__ double ll(double y, double dot, int t) const {
        const double res = y - dot;
        return fma(-hn[t], log1p_nonneg((res * res) * hs[t]), cs[t]);
    }
};

// The other operand of the walks that own DRAWS (kernels_ppc.hip, kernels_sens.hip): theta (any ldt)
// -> Tp [S_pad][k_pad], the k coefficients of every draw in whole tiles and slabs, zero in the
// padding.  A grid-stride loop: every thread of the launch calls it.
__device__ __forceinline__ void pad_rows(const double* __restrict__ theta, int64_t S, int64_t ldt,
                                         int32_t k, int64_t S_pad, int32_t k_pad,
                                         double* __restrict__ Tp) {
    const int64_t total = S_pad * k_pad;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const int64_t s = e / k_pad;
        const int32_t j = (int32_t)(e - s * k_pad);
        Tp[e] = (s < S && j < k) ? theta[s * ldt + j] : 0.0;
    }
}

}  // namespace bmc
