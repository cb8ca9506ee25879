// The generalised Pareto fit of Pareto-smoothed importance sampling (Zhang & Stephens 2009, as
// loo::gpdfit; Vehtari et al. 2024), once for every kernel that smooths a tail: loo_fit_kernel
// (kernels_loo.hip) and sens_psis_kernel (kernels_sens.hip).  The tail length and the grid size are
// the host's (bmc_psis_plan.h).  Every sum has one order, so two calls return the same bits:
// the grid points' sums lane-strided and then an ordered butterfly, the grid weights and theta in
// index order, kraw thread-strided and then block_sum.
#pragma once
#include "bmc_dev.h"

namespace bmc {

struct PsisFit {
    double khat, sigma;
    bool finite;   // khat is finite: the tail can be smoothed
};

// A workgroup of 256 threads, all of them, calls it.  xs[0 .. M): the tail's exceedances over the
// cutoff, ascending, written and visible (a barrier behind them).  mg = psis_grid_points(M) grid
// points; red[256] and the three grid arrays of mg doubles are the caller's LDS.  Every thread
// returns the same fit.
__device__ __forceinline__ PsisFit psis_fit(const double* xs, int M, int mg, double* red, double* g_theta,
                                            double* g_l, double* g_w) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double dM = (double)M;
    const double xM = xs[M - 1], xq = xs[(M + 2) / 4 - 1];
    // a wave per grid point: lane-strided sums, then a butterfly (every lane the same bits)
    for (int j = wave; j < mg; j += 4) {
        const double th = 1.0 / xM + (1.0 - sqrt((double)mg / ((double)j + 0.5))) / (3.0 * xq);
        double s = 0.0;
        for (int e = lane; e < M; e += 64) s += log1p(-th * xs[e]);
        s = lane_sum_ordered<64>(s, lane);
        const double kj = s / dM;
        if (lane == 0) {
            g_theta[j] = th;
            g_l[j] = dM * (log(-th / kj) - kj - 1.0);
        }
    }
    __syncthreads();
    for (int j = tid; j < mg; j += 256) {
        double s = 0.0;
        for (int e = 0; e < mg; ++e) s += exp(g_l[e] - g_l[j]);   // (+inf: weight 0)
        g_w[j] = 1.0 / s;
    }
    __syncthreads();
    double theta = 0.0;
    for (int e = 0; e < mg; ++e) theta += g_w[e] * g_theta[e];
    double part = 0.0;
    for (int e = tid; e < M; e += 256) part += log1p(-theta * xs[e]);
    const double kraw = block_sum(part, red) / dM;
    PsisFit f;
    f.sigma = -kraw / theta;
    f.khat = (dM * kraw + 5.0) / (dM + 10.0);
    f.finite = is_finite(f.khat);
    return f;
}

// log of the smoothed weight of tail position j < M (ascending) over the cutoff's exp(lw) = ecut:
// log(ecut + q_j), q_j the fitted quantile at (j + 1/2) / M
__device__ __forceinline__ double psis_smoothed_lw(int j, int M, const PsisFit& f, double ecut) {
    const double l1p = log1p(-((double)j + 0.5) / (double)M);
    const double q = fabs(f.khat) < 1e-30 ? -f.sigma * l1p : f.sigma * expm1(-f.khat * l1p) / f.khat;
    return log(ecut + q);
}

}  // namespace bmc
