// Device-side variate transforms shared by the fill kernels (kernels_setup.hip) and the Student-t
// sampler (kernels_robust.hip): the Box-Muller pair of one Philox block and the Marsaglia-Tsang
// gamma variate.  DESIGN.md "Variate streams" gives the counter layouts.
#pragma once
#include "bmc_dev.h"

namespace bmc {

__device__ __forceinline__ void box_muller(u32x4 r, double& z0, double& z1) {
    box_muller_pair(u53_open0(r.x, r.y), u53_open0(r.z, r.w), z0, z1);   // bmc_math.h
}

// Gamma(a, 1), Marsaglia & Tsang (2000).  Attempt m of the element named by the counter words
// (w0, w1) of stream STREAM uses Philox counters (w0, w1, STREAM, w3 | 2m) and (.., w3 | (2m+1)),
// at most 64 attempts (w3 has its low 8 bits clear).  For a < 1 the usual boost
// Gamma(a) = Gamma(a+1) * U^(1/a) is applied.
template <uint32_t STREAM>
__device__ inline double gamma_mt_at(double a, uint32_t w0, uint32_t w1, uint32_t w3, uint32_t k0,
                                     uint32_t k1) {
    const bool boost = a < 1.0;
    const double aa = boost ? a + 1.0 : a;
    const double d = aa - 1.0 / 3.0;
    const double c = 1.0 / sqrt(9.0 * d);
    double res = d;
    for (uint32_t m = 0; m < 64; ++m) {
        const u32x4 r0 = philox4x32_10(u32x4{w0, w1, STREAM, w3 | (2 * m)}, k0, k1);
        const u32x4 r1 = philox4x32_10(u32x4{w0, w1, STREAM, w3 | (2 * m + 1)}, k0, k1);
        double x, unused;
        box_muller(r0, x, unused);
        const double u = u53_open0(r1.x, r1.y);
        double v = 1.0 + c * x;
        if (v <= 0.0) continue;
        v = v * v * v;
        const double x2 = x * x;
        if (u < 1.0 - 0.0331 * x2 * x2 || log(u) < 0.5 * x2 + d * (1.0 - v + log(v))) {
            res = d * v;
            if (boost) res *= pow(u53_open0(r1.z, r1.w), 1.0 / a);
            break;
        }
    }
    return res;
}

// element t of a chain's gamma stream: counters (t_lo, t_hi, STREAM_GAMMA, 2m) and (.., 2m+1)
__device__ inline double gamma_mt(double a, uint64_t t, uint32_t k0, uint32_t k1) {
    return gamma_mt_at<STREAM_GAMMA>(a, (uint32_t)t, (uint32_t)(t >> 32), 0u, k0, k1);
}

}  // namespace bmc
