// gfx950 kernels of the Student-t (outlier-robust) Gibbs sampler (bmc_robust_run).
//
// Model: y_n | beta, sigma2, lambda_n ~ N(x_n . beta, sigma2 / lambda_n), lambda_n ~ Gamma(nu/2, rate
// nu/2) -- marginally t_nu -- under the priors of the Gaussian sampler.  X'LX changes with every
// sweep, so nothing reduces to fixed sufficient statistics: per sweep a chain needs the weighted
// Gram of its rows, a k x k Cholesky factorisation and N gamma variates.
//
//   * robust_pack_kernel    the resident panels -> Z [rows_padded][16 NT] row-major (zero-padded
//                           columns and rows) and y: the operand layout of the MFMA pass;
//   * robust_chain_kernel   ONE workgroup of 4 waves per chain, all sweeps.  A chain talks to no other
//                           workgroup: the only synchronisation is __syncthreads() and LDS.
//
// One sweep t (lambda = 1 and the OLS sigma2 before the first):
//   G  wave w walks its slab of rows (bmc_robust_plan.h) in k-steps of 4 rows: lane l loads
//      Z[row0 + (l >> 4)][16 t + (l & 15)] per column tile t, scales it by the row's lambda for the A
//      operand and issues one v_mfma_f64_16x16x4_f64 per tile pair (ti <= tj); X'Ly is summed beside
//      them, one fma per tile.  Wave partials go to LDS and are added in wave order.
//   C  Q = X'LX / sigma2 + P + 1e-6 I (lower triangle), rhs = P b0 + X'Ly / sigma2.
//   S  wave 0, lane i = row i of Q in registers: Cholesky Q = L L' (pivots through v_readlane),
//      z = L^-1 rhs, beta = L^-T (z + xi_t).  Rows k .. KC-1 are those of the identity.
//   B  r_n = y_n - x_n . beta (the fma chain of the loop kernels), S = sum lambda_n r_n^2: lane sums
//      in row order, wave_sum, waves in order.  sigma2 = max(((nu0 sigma20 + S) / 2) / G_t, 1e-6).
//   L  lambda_n = g_{t,n} / ((nu + r_n^2 / sigma2) / 2), added to the row's running sum when the
//      sweep is kept.  g_{t,n}: Marsaglia-Tsang at shape (nu + 1) / 2 on the STREAM_ROBUST counters
//      (n, t lo, STREAM_ROBUST, ((t >> 32) << 8) | attempt), or the caller's array (replay).
//   N  (robust_chain_kernel<KC, true> only: nu on a grid, bmc_robust_run_nu)  phase L also sums
//      log lambda_n - lambda_n in the order of S; after the sweep's last barrier wave 0, lane g = grid
//      value g, forms l_g = fma(nu_g / 2, T, c_g), p_g = exp(l_g - max l), the running sums P_g strictly
//      left to right (one v_readlane per grid value) and picks #{g < G - 1 : P_g < u P_{G-1}}, u from
//      Philox counter (t lo, t hi, STREAM_NU, 0) or the caller's array.  The index lives in LDS; phase L
//      of the next sweep reads nu and (nu + 1) / 2 from the grid's LDS table, three barriers later.
// Every sum's order is fixed by (N, k): a chain's bits do not depend on its index, its launch, its
// neighbours or the device.
//   * robust_chain_kernel<KC, NU_FREE, true>   the folded form (bmc_kfold_cv_t): chains
//                           of DIFFERENT problems in one launch, each workgroup finding its rows, row
//                           count, slab size, start value and nu table through a descriptor;
//   * robust_thin_kernel    every thin-th row of a chain's draws or nu indices.
#include <type_traits>

#include "bmc_dev.h"
#include "bmc_rng.h"
#include "bmc_robust.h"

namespace bmc {

namespace {

using f64x4 = __attribute__((ext_vector_type(4))) double;

__global__ __launch_bounds__(256) void robust_pack_kernel(const double* __restrict__ Xp,
                                                          const double* __restrict__ yp, int64_t n,
                                                          int32_t k, int32_t RP, int64_t n_pad,
                                                          int32_t ldz, double* __restrict__ Z,
                                                          double* __restrict__ yv) {
    const int64_t total = n_pad * ldz;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const int64_t r = e / ldz;
        const int32_t j = (int32_t)(e - r * ldz);
        Z[e] = (r < n && j < k) ? Xp[panel_offset(r, j, k, RP)] : 0.0;
        if (j == 0) yv[r] = r < n ? yp[r] : 0.0;
    }
}

// a wave-uniform double held in scalar registers
__device__ __forceinline__ double uniform_f64(double v) {
    const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v));
    const int hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
    return __hiloint2double(hi, lo);
}

// max over the 64 lanes, the same bits in every lane (a maximum has no order to fix)
__device__ __forceinline__ double wave_max(double v) {   // the data movement of wave_sum
    v = fmax(v, dpp_mov_f64<0xB1>(v));
    v = fmax(v, dpp_mov_f64<0x4E>(v));
    v = fmax(v, dpp_mov_f64<0x141>(v));
    v = fmax(v, dpp_mov_f64<0x140>(v));
    return fmax(fmax(readlane_f64(v, 0), readlane_f64(v, 16)), fmax(readlane_f64(v, 32), readlane_f64(v, 48)));
}

// NU_FREE = false: nu is a.nu in every sweep.  NU_FREE = true: nu is a value of the grid a.nu_tab,
// drawn anew at the end of every sweep (steps 5 and 6 of bmc_robust_run_nu).
// FOLDED = true (bmc_kfold_cv_t): every workgroup finds its own problem through a
// descriptor -- chain c of the launch works on the packed rows, the row count, the slab size, the
// start value and (NU_FREE) the nu table of fold a.fold_of_chain[c], and on rows a.row0[c] .. of ws and
// wsum.  Device RNG only.  Everything after these reads is the code of the unfolded form: the chain
// is the one a launch on that fold's rows alone draws.
template <int KC, bool NU_FREE, bool FOLDED>
__global__ __launch_bounds__(ROBUST_THREADS) void robust_chain_kernel(
    const typename std::conditional<FOLDED, RobustFoldedArgs, RobustArgs>::type a) {
    constexpr int NT = KC > 16 ? 2 : 1, NP = NT * (NT + 1) / 2, LDZ = 16 * NT, LDL = KC + 1;
    __shared__ double s_part[ROBUST_WAVES][NP][256];
    __shared__ double s_xty[ROBUST_WAVES][4][LDZ];
    __shared__ double s_L[KC * LDL];
    __shared__ double s_rhs[KC], s_w[KC], s_beta[KC];
    __shared__ double s_wsum[ROBUST_WAVES];
    __shared__ int s_fail;
    // NU_FREE only: the grid's four rows, the waves' partials of T_t, the grid index in force
    __shared__ double s_nu[NU_FREE ? 4 * ROBUST_MAX_NU_GRID : 1];
    __shared__ double s_tsum[NU_FREE ? ROBUST_WAVES : 1];
    __shared__ int s_idx;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kq = lane >> 4, cl = lane & 15;
    // the chain's problem: the launch's own, or (FOLDED) what its fold's descriptor names
    const RobustFold* fd = nullptr;
    if constexpr (FOLDED) fd = a.fold + a.fold_of_chain[blockIdx.x];
    int64_t N_;
    if constexpr (FOLDED) N_ = fd->n; else N_ = a.n;
    const int64_t c = blockIdx.x, N = N_, Tt = a.burn + a.iters;
    const int k = a.k;
    const double *Z_, *yv_;
    if constexpr (FOLDED) { Z_ = fd->Z; yv_ = fd->yv; } else { Z_ = a.Z; yv_ = a.yv; }
    const double* __restrict__ Z = Z_;
    const double* __restrict__ yv = yv_;
    const double* xi = a.xi + (size_t)c * Tt * k;
    const double* gam = a.gam + (size_t)c * Tt;
    const double* gl = nullptr;      // replay mode: the unfolded form only
    double *ws, *wsum;
    if constexpr (FOLDED) {
        ws = a.ws + 2 * a.row0[c];
        wsum = a.wsum + a.row0[c];
    } else {
        gl = a.gl ? a.gl + (size_t)c * Tt * N : nullptr;
        ws = a.ws + (size_t)c * N * 2;
        wsum = a.wsum + (size_t)c * N;
    }
    double* out = a.samples + (size_t)c * a.iters * (k + 1);
    uint32_t k0 = 0, k1 = 0;
    if (a.seeds) {
        const uint64_t seed = a.seeds[c];
        k0 = (uint32_t)seed;
        k1 = (uint32_t)(seed >> 32);
    }
    // this wave's slab; phases B and L give row slab0 + lane + 64 i to the lane, every sweep
    int64_t rpw;
    if constexpr (FOLDED) rpw = fd->rows_per_wave; else rpw = a.rows_per_wave;
    const int64_t slab0 = wave * rpw;
    const int64_t slab1 = slab0 + rpw < N ? slab0 + rpw : N;
    const int64_t gsteps = slab1 > slab0 ? (slab1 - slab0 + 3) / 4 * 4 : 0;   // rows of phase G

    for (int64_t row = slab0 + lane; row < slab1; row += 64) {
        ws[2 * row] = 0.0;
        ws[2 * row + 1] = 1.0;
        wsum[row] = 0.0;
    }
    if (tid == 0) s_fail = 0;
    if constexpr (NU_FREE) {
        if constexpr (FOLDED) {
            if (tid < 4 * a.n_grid) s_nu[tid] = fd->nu_tab[tid];
        } else {
            if (tid < 4 * a.n_grid) s_nu[tid] = a.nu_tab[tid];
        }
        if (tid == 0) s_idx = a.nu_init;
    }
    double sigma2;
    if constexpr (FOLDED) sigma2 = fd->sigma2_init; else sigma2 = a.sigma2_init;
    int64_t t_fail = -1;
    __syncthreads();

    for (int64_t t = 0; t < Tt; ++t) {
        // ---- G: weighted Gram of the slab ---------------------------------------------------------
        {
            f64x4 acc[NP];
            double xty[NT];
#pragma unroll
            for (int p = 0; p < NP; ++p) acc[p] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int q = 0; q < NT; ++q) xty[q] = 0.0;
            for (int64_t r = 0; r < gsteps; r += 4) {
                const int64_t row = slab0 + r + kq;       // < rows_padded: Z and yv are zero past N
                const double lam = row < N ? ws[2 * row + 1] : 0.0;
                const double yr = yv[row];
                double x[NT], ax[NT];
#pragma unroll
                for (int q = 0; q < NT; ++q) {
                    x[q] = Z[row * LDZ + 16 * q + cl];
                    ax[q] = lam * x[q];
                    xty[q] = fma(ax[q], yr, xty[q]);
                }
                int p = 0;
#pragma unroll
                for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                    for (int tj = ti; tj < NT; ++tj, ++p)
                        acc[p] = __builtin_amdgcn_mfma_f64_16x16x4f64(ax[ti], x[tj], acc[p], 0, 0, 0);
            }
#pragma unroll
            for (int p = 0; p < NP; ++p)
#pragma unroll
                for (int i = 0; i < 4; ++i) s_part[wave][p][(kq + 4 * i) * 16 + cl] = acc[p][i];
#pragma unroll
            for (int q = 0; q < NT; ++q) s_xty[wave][kq][16 * q + cl] = xty[q];
        }
        __syncthreads();
        // ---- C: Q (lower triangle) and rhs ----------------------------------------------------------
        for (int e = tid; e < KC * KC; e += ROBUST_THREADS) {
            const int i = e / KC, j = e - i * KC;
            if (j > i) continue;
            double q = i == j ? 1.0 : 0.0;
            if (i < k) {
                const int ti = j >> 4, tj = i >> 4;          // element (j, i), j <= i, of X'LX
                const int p = ti * NT - ti * (ti - 1) / 2 + (tj - ti);
                const int idx = (j & 15) * 16 + (i & 15);
                const double g = ((s_part[0][p][idx] + s_part[1][p][idx]) + s_part[2][p][idx]) +
                                 s_part[3][p][idx];
                q = g / sigma2 + a.P[i * k + j] + (i == j ? 1e-6 : 0.0);
            }
            s_L[i * LDL + j] = q;
        }
        if (tid < KC) {
            double rhs = 0.0;
            if (tid < k) {
                double s = 0.0;
#pragma unroll
                for (int w = 0; w < ROBUST_WAVES; ++w)
#pragma unroll
                    for (int q = 0; q < 4; ++q) s += s_xty[w][q][tid];
                rhs = a.Pb0[tid] + s / sigma2;
            }
            s_rhs[tid] = rhs;
        }
        __syncthreads();
        // ---- S: Cholesky, forward solve (wave 0) ----------------------------------------------------
        double row[KC];
        if (wave == 0) {
            const int li = lane < KC ? lane : KC - 1;
#pragma unroll
            for (int j = 0; j < KC; ++j) row[j] = (j <= lane && lane < KC) ? s_L[li * LDL + j] : 0.0;
            bool bad = false;
#pragma unroll
            for (int cc = 0; cc < KC; ++cc) {
                const double piv = readlane_f64(row[cc], cc);
                bad = bad || !(piv > 0.0) || !(piv < __builtin_huge_val());
                const double d = sqrt(piv);
                row[cc] = lane == cc ? d : row[cc] / d;
#pragma unroll
                for (int j = cc + 1; j < KC; ++j) {
                    const double ljc = readlane_f64(row[cc], j);
                    row[j] = fma(-row[cc], ljc, row[j]);
                }
            }
            if (bad) {
                if (lane == 0) s_fail = 1;
            } else {
                double z = lane < KC ? s_rhs[li] : 0.0;
#pragma unroll
                for (int cc = 0; cc < KC; ++cc) {
                    const double zc = readlane_f64(z, cc) / readlane_f64(row[cc], cc);
                    z = lane == cc ? zc : (lane > cc ? fma(-row[cc], zc, z) : z);
                }
                if (lane < KC) {
                    s_w[lane] = lane < k ? z + xi[(size_t)t * k + lane] : z;
#pragma unroll
                    for (int j = 0; j < KC; ++j) s_L[lane * LDL + j] = row[j];
                }
            }
        }
        __syncthreads();
        if (s_fail) {
            t_fail = t;
            break;
        }
        // ---- S: back solve L' beta = z + xi (wave 0) ------------------------------------------------
        if (wave == 0) {
            const int li = lane < KC ? lane : 0;
            double b = s_w[li];
#pragma unroll
            for (int cc = KC - 1; cc >= 0; --cc) {
                const double bc = readlane_f64(b, cc) / readlane_f64(row[cc], cc);
                const double lci = s_L[cc * LDL + li];
                b = lane == cc ? bc : (lane < cc ? fma(-lci, bc, b) : b);
            }
            if (lane < KC) s_beta[lane] = b;
        }
        __syncthreads();
        const bool keep = t >= a.burn;
        double* orow = out + (size_t)(t - a.burn) * (k + 1);
        if (keep && tid < k) orow[tid] = s_beta[tid];
        // ---- B: residuals and their weighted sum of squares -----------------------------------------
        {
            double s = 0.0;
            for (int64_t r = slab0 + lane; r < slab1; r += 64) {
                double acc = yv[r];
#pragma unroll
                for (int j = 0; j < KC; ++j)
                    if (j < k) acc = fma(-Z[r * LDZ + j], s_beta[j], acc);
                ws[2 * r] = acc;
                s = fma(ws[2 * r + 1] * acc, acc, s);
            }
            s = wave_sum(s);
            if (lane == 0) s_wsum[wave] = s;
        }
        __syncthreads();
        {
            const double S = ((s_wsum[0] + s_wsum[1]) + s_wsum[2]) + s_wsum[3];
            const double v = ((a.nu0_s20 + S) * 0.5) / gam[t];
            sigma2 = v < 1e-6 ? 1e-6 : v;
            if (keep && tid == 0) orow[k] = sqrt(sigma2);
        }
        // ---- L: the rows' weights ---------------------------------------------------------------------
        double nu_t = a.nu, shape_t = a.shape_l;
        if constexpr (NU_FREE) {
            const int gi = s_idx;                    // written after the previous sweep's last barrier
            nu_t = uniform_f64(s_nu[gi]);
            shape_t = uniform_f64(s_nu[a.n_grid + gi]);
        }
        double tl = 0.0;
        for (int64_t r = slab0 + lane; r < slab1; r += 64) {
            const double res = ws[2 * r];
            const double g = gl ? gl[(size_t)t * N + r]
                                : gamma_mt_at<STREAM_ROBUST>(shape_t, (uint32_t)r, (uint32_t)t,
                                                             (uint32_t)((uint64_t)t >> 32) << 8, k0, k1);
            const double lam = g / ((nu_t + res * res / sigma2) * 0.5);
            ws[2 * r + 1] = lam;
            if (keep) wsum[r] += lam;
            if constexpr (NU_FREE) tl += log(lam) - lam;
        }
        if constexpr (NU_FREE) {
            tl = wave_sum(tl);
            if (lane == 0) s_tsum[wave] = tl;
        }
        __syncthreads();
        // ---- N: nu | lambda, an exact draw from the grid (wave 0; the others go on to phase G) ---------
        if constexpr (NU_FREE) {
            if (wave == 0) {
                const int G = a.n_grid, cur = s_idx;
                const double T = ((s_tsum[0] + s_tsum[1]) + s_tsum[2]) + s_tsum[3];
                int pick = cur;
                if (__builtin_isfinite(T)) {
                    const bool on = lane < G;
                    const int gi = on ? lane : G - 1;
                    const double l = on ? fma(s_nu[2 * G + gi], T, s_nu[3 * G + gi]) : -__builtin_huge_val();
                    const double m = wave_max(l);
                    const double p = on ? exp(l - m) : 0.0;
                    // P_g = P_{g-1} + p_g, strictly in grid order.  Eight steps at a time, so that the
                    // readlanes run ahead of the chain of additions; lanes past G hold p = 0, which
                    // leaves the running sum as it is.
                    double run = 0.0, P = 0.0;
                    for (int g0 = 0; g0 < G; g0 += 8) {
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            run = run + readlane_f64(p, g0 + j);
                            if (lane == g0 + j) P = run;
                        }
                    }
                    double u;
                    const double* u_nu = nullptr;    // replay mode: the unfolded form only
                    if constexpr (!FOLDED) u_nu = a.u_nu;
                    if (u_nu) {
                        u = u_nu[(size_t)c * Tt + t];
                    } else {
                        const u32x4 w = philox4x32_10(
                            u32x4{(uint32_t)t, (uint32_t)((uint64_t)t >> 32), STREAM_NU, 0u}, k0, k1);
                        u = u53_open0(w.x, w.y);
                    }
                    pick = __builtin_popcountll(__ballot(lane < G - 1 && P < u * run));
                }
                if (lane == 0) {
                    if (keep) {
                        a.nu_idx[(size_t)c * a.iters + (t - a.burn)] = pick;
                        if (a.tstat) a.tstat[(size_t)c * a.iters + (t - a.burn)] = T;
                    }
                    if constexpr (FOLDED) s_idx = pick;
                    else s_idx = a.nu_path ? a.nu_path[(size_t)c * Tt + t] : pick;
                }
            }
        }
    }

    // mean weight over the kept sweeps; a stopped chain leaves NaN from the failing sweep on
    const double nan = __builtin_nan("");
    for (int64_t r = slab0 + lane; r < slab1; r += 64)
        wsum[r] = t_fail >= 0 ? nan : (a.iters > 0 ? wsum[r] / (double)a.iters : 0.0);
    if (t_fail >= 0) {
        const int64_t first = t_fail > a.burn ? t_fail - a.burn : 0;
        for (int64_t e = first * (k + 1) + tid; e < a.iters * (k + 1); e += ROBUST_THREADS) out[e] = nan;
        if (tid == 0) a.status[c] = 1;
    }
}

template <int KC, bool NU_FREE>
hipError_t launch_kc(const RobustArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((robust_chain_kernel<KC, NU_FREE, false>), dim3((unsigned)a.n_chains), dim3(ROBUST_THREADS), 0, s, a);
    return hipGetLastError();
}
template <int KC, bool NU_FREE>
hipError_t launch_kc(const RobustFoldedArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((robust_chain_kernel<KC, NU_FREE, true>), dim3((unsigned)a.n_chains), dim3(ROBUST_THREADS), 0, s, a);
    return hipGetLastError();
}
template <bool NU_FREE>
hipError_t launch_folded_kc(const RobustFoldedArgs& a, hipStream_t s) {
    switch (robust_kc(a.k)) {
        case 4: return launch_kc<4, NU_FREE>(a, s);
        case 8: return launch_kc<8, NU_FREE>(a, s);
        case 16: return launch_kc<16, NU_FREE>(a, s);
        default: return launch_kc<32, NU_FREE>(a, s);
    }
}

// out[ch][s][.] = in[ch][s * thin][.], s < kept, rows of `width` elements: every thin-th of the
// `rows_in` rows a chain holds
template <class T>
__global__ __launch_bounds__(256) void robust_thin_kernel(const T* __restrict__ in, int64_t chains,
                                                          int64_t rows_in, int64_t thin, int64_t kept,
                                                          int32_t width, T* __restrict__ out) {
    const int64_t total = chains * kept * width;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const int64_t row = e / width;
        const int32_t j = (int32_t)(e - row * width);
        const int64_t ch = row / kept, sdraw = row - ch * kept;
        out[e] = in[(ch * rows_in + sdraw * thin) * width + j];
    }
}
template <class T>
hipError_t launch_thin(const T* in, int64_t chains, int64_t rows_in, int64_t thin, int64_t kept, int32_t width,
                       T* out, hipStream_t s) {
    if (chains < 1 || kept < 1 || thin < 1 || width < 1 || (kept - 1) * thin >= rows_in) return hipErrorInvalidValue;
    int64_t blocks = (chains * kept * width + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(robust_thin_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, s, in, chains, rows_in, thin,
                       kept, width, out);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_robust_pack(const Panels& P, double* Z, double* yv, hipStream_t s) {
    const int64_t n_pad = robust_rows_padded(P.n);
    const int32_t ldz = robust_ldz(P.k);
    int64_t blocks = (n_pad * ldz + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(robust_pack_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (const double*)P.X,
                       (const double*)P.y, P.n, P.k, 64 * P.vec, n_pad, ldz, Z, yv);
    return hipGetLastError();
}

hipError_t launch_robust(const RobustArgs& a, hipStream_t s) {
    if (a.n_chains < 1 || a.n_chains > ROBUST_MAX_CHAINS_PER_LAUNCH || a.k < 1 || a.k > ROBUST_MAX_K)
        return hipErrorInvalidValue;
    switch (robust_kc(a.k)) {
        case 4: return launch_kc<4, false>(a, s);
        case 8: return launch_kc<8, false>(a, s);
        case 16: return launch_kc<16, false>(a, s);
        default: return launch_kc<32, false>(a, s);
    }
}

hipError_t launch_robust_nu(const RobustArgs& a, hipStream_t s) {
    if (a.n_chains < 1 || a.n_chains > ROBUST_MAX_CHAINS_PER_LAUNCH || a.k < 1 || a.k > ROBUST_MAX_K ||
        a.n_grid < 1 || a.n_grid > ROBUST_MAX_NU_GRID || a.nu_init < 0 || a.nu_init >= a.n_grid ||
        !a.nu_tab || !a.nu_idx)
        return hipErrorInvalidValue;
    switch (robust_kc(a.k)) {
        case 4: return launch_kc<4, true>(a, s);
        case 8: return launch_kc<8, true>(a, s);
        case 16: return launch_kc<16, true>(a, s);
        default: return launch_kc<32, true>(a, s);
    }
}

hipError_t launch_robust_folded(const RobustFoldedArgs& a, hipStream_t s) {
    if (a.n_chains < 1 || a.n_chains > ROBUST_MAX_CHAINS_PER_LAUNCH || a.k < 1 || a.k > ROBUST_MAX_K ||
        !a.fold || !a.fold_of_chain || !a.row0 || !a.seeds)
        return hipErrorInvalidValue;
    if (a.n_grid == 0) return launch_folded_kc<false>(a, s);
    if (a.n_grid < 1 || a.n_grid > ROBUST_MAX_NU_GRID || a.nu_init < 0 || a.nu_init >= a.n_grid || !a.nu_idx)
        return hipErrorInvalidValue;
    return launch_folded_kc<true>(a, s);
}

hipError_t launch_robust_thin(const double* in, int64_t chains, int64_t rows_in, int64_t thin, int64_t kept,
                              int32_t width, double* out, hipStream_t s) {
    return launch_thin(in, chains, rows_in, thin, kept, width, out, s);
}
hipError_t launch_robust_thin_idx(const int32_t* in, int64_t chains, int64_t rows_in, int64_t thin, int64_t kept,
                                  int32_t* out, hipStream_t s) {
    return launch_thin(in, chains, rows_in, thin, kept, 1, out, s);
}

}  // namespace bmc
