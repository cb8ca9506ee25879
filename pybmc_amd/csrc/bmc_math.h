// Elementary functions of the on-device variate generators, written out so that the Box-Muller
// transform costs a few dozen f64 operations instead of the general-purpose library calls
// (log, sincospi: special cases, denormals, huge arguments -- none of which can occur here).
// Plain C++ (no HIP headers): the CPU test suite compiles the same text with g++ and checks it
// against libm (tests/test_host_math.py).  Algorithms: the classic fdlibm kernels (Sun
// Microsystems, freely distributable) -- log by s = f / (2 + f) and an odd polynomial in s,
// sin / cos on [-pi/4, pi/4] by their minimax polynomials -- with the argument reductions that
// the restricted domains allow.  Each result is within 1-2 ulp of the correctly rounded value.
#pragma once
#include <stdint.h>
#include <string.h>
#include <math.h>

#if defined(__HIPCC__) 
#define BMC_HD __host__ __device__ inline
#else
#define BMC_HD inline
#endif

namespace bmc {

// fma(a, b, c) with c a compile-time constant of a polynomial.  On the GPU the constant is handed
// to v_fma_f64 as a scalar-register operand: left to itself hipcc copies every such constant into
// a vector register pair in front of a v_fmac (two extra vector instructions per coefficient --
// 32 per Box-Muller pair, and vector instructions are what the predictive GEMM's epilogue is
// made of).  Same operation, same bits; the CPU build is plain fma.
BMC_HD double fma_c(double a, double b, double c) {
#if defined(__HIP_DEVICE_COMPILE__)
    double d;
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "s"(c));
    return d;
#else
    return fma(a, b, c);
#endif
}

// neither an infinity nor a NaN
BMC_HD bool is_finite(double x) { return fabs(x) < __builtin_inf(); }

// natural logarithm of a NORMAL double 0 < x (the generators call it with x in [2^-53, 1])
BMC_HD double log_normal_arg(double x) {
    const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10;
    const double Lg1 = 6.666666666666735130e-01, Lg2 = 3.999999999940941908e-01,
                 Lg3 = 2.857142874366239149e-01, Lg4 = 2.222219843214978396e-01,
                 Lg5 = 1.818357216161805012e-01, Lg6 = 1.531383769920937332e-01,
                 Lg7 = 1.479819860511658591e-01;
    uint64_t ix;
    memcpy(&ix, &x, 8);
    // x = 2^k m with m in [sqrt(1/2), sqrt(2)): shift the exponent so that the high word of
    // sqrt(1/2) lands on an exponent boundary
    uint32_t hx = (uint32_t)(ix >> 32);
    hx += 0x3ff00000u - 0x3fe6a09eu;
    const int k = (int)(hx >> 20) - 0x3ff;
    hx = (hx & 0x000fffffu) + 0x3fe6a09eu;
    ix = ((uint64_t)hx << 32) | (ix & 0xffffffffull);
    double m;
    memcpy(&m, &ix, 8);
    // (the polynomials are written with explicit fma: one instruction per coefficient on the
    // GPU -- the library is compiled with -ffp-contract=off -- and the same, exactly rounded,
    // operation in the CPU build of this text, so both produce the same bits)
    const double f = m - 1.0;
    const double hfsq = (0.5 * f) * f;
    const double s = f / (2.0 + f);
    const double z = s * s;
    const double w = z * z;
    const double t1 = w * fma_c(w, fma_c(w, Lg6, Lg4), Lg2);
    const double t2 = z * fma_c(w, fma_c(w, fma_c(w, Lg7, Lg5), Lg3), Lg1);
    const double R = t2 + t1;
    const double dk = (double)k;
    const double lo = fma(s, hfsq + R, dk * ln2_lo);
    return fma(dk, ln2_hi, f - (hfsq - lo));
}

// log(1 + x) for x >= 0 (subnormals included; NaN gives NaN, +inf gives NaN): the Student-t
// density of the scoring kernels (bmc_score_tile.h), where a naive log(1 + x) loses every digit of
// a small x.  u = fl(1 + x) >= 1 is a normal double and c = x - (u - 1) the exact rounding error of
// that sum while it matters (x < 2^53), so log(1 + x) = log(u) + c / u + O((c / u)^2): the kernel
// of log_normal_arg on u = 2^k m, with c / u = c 2^-k / m added to its low part.  The one division
// stays that kernel's s = f / (2 + f): 1 / m = (1 - s) / (1 + s) = 1 - 2 s (1 - s (1 - s)) + O(s^4),
// |s| < 0.1716, and c / u is at most half an ulp of 1 against a result of about 2 s or more, so the
// truncation is below 0.01 ulp of the result.  Worst error found against log1pl: 0.82 ulp
// (tests/test_tscore_host.py).  Ten vector operations more than log_normal_arg, none a division.
BMC_HD double log1p_nonneg(double x) {
    const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10;
    const double Lg1 = 6.666666666666735130e-01, Lg2 = 3.999999999940941908e-01,
                 Lg3 = 2.857142874366239149e-01, Lg4 = 2.222219843214978396e-01,
                 Lg5 = 1.818357216161805012e-01, Lg6 = 1.531383769920937332e-01,
                 Lg7 = 1.479819860511658591e-01;
    const double u = 1.0 + x;
    const double c = x - (u - 1.0);   // (+inf: NaN, which reaches the result)
    uint64_t ix;
    memcpy(&ix, &u, 8);
    uint32_t hx = (uint32_t)(ix >> 32);
    hx += 0x3ff00000u - 0x3fe6a09eu;
    const int k = (int)(hx >> 20) - 0x3ff;   // 0 .. 1024
    hx = (hx & 0x000fffffu) + 0x3fe6a09eu;
    ix = ((uint64_t)hx << 32) | (ix & 0xffffffffull);
    double m;
    memcpy(&m, &ix, 8);
    const double f = m - 1.0;
    const double hfsq = (0.5 * f) * f;
    const double s = f / (2.0 + f);
    const double z = s * s;
    const double w = z * z;
    const double t1 = w * fma_c(w, fma_c(w, Lg6, Lg4), Lg2);
    const double t2 = z * fma_c(w, fma_c(w, fma_c(w, Lg7, Lg5), Lg3), Lg1);
    const double R = t2 + t1;
    const double dk = (double)k;
    const double rm = fma(-(s + s), fma(-s, 1.0 - s, 1.0), 1.0);
    const double cu = ldexp(c, -k) * rm;
    const double lo = fma(s, hfsq + R, fma(dk, ln2_lo, cu));
    return fma(dk, ln2_hi, f - (hfsq - lo));
}

// sin(2 pi u) and cos(2 pi u) for 0 <= u <= 1: 4u = q + r with q the nearest integer (exact),
// the kernels on (pi/2) r in [-pi/4, pi/4], then the quadrant
BMC_HD void sincos_2pi(double u, double& sn, double& cs) {
    const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03,
                 S3 = -1.98412698298579493134e-04, S4 = 2.75573137070700676789e-06,
                 S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03,
                 C3 = 2.48015872894767294178e-05, C4 = -2.75573143513906633035e-07,
                 C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    const double t = 4.0 * u;
    const double q = rint(t);
    const double r = t - q;                         // exact, |r| <= 1/2
    const double x = r * 1.57079632679489661923;    // |x| <= pi/4
    const double z = x * x;
    const double v = z * x;
    const double rs = fma_c(z, fma_c(z, fma_c(z, fma_c(z, S6, S5), S4), S3), S2);
    const double ksin = fma(v, fma_c(z, rs, S1), x);
    const double w = z * z;
    const double rc = fma(w * w, fma_c(z, fma_c(z, C6, C5), C4), z * fma_c(z, fma_c(z, C3, C2), C1));
    const double hz = 0.5 * z;
    const double w1 = 1.0 - hz;
    const double kcos = w1 + fma(z, rc, (1.0 - w1) - hz);
    const int iq = (int)q & 3;
    const double a = (iq & 1) ? kcos : ksin;        // |sin| of the quadrant
    const double b = (iq & 1) ? ksin : kcos;
    sn = (iq & 2) ? -a : a;
    cs = ((iq + 1) & 2) ? -b : b;
}

// two independent N(0,1) variates from two uniforms, u1 in (0, 1] and u2 in [0, 1]  (Box-Muller)
// (the library's log() and sincospi() in this place were the baseline these routines replaced:
// slower, and the normals then depend on the device library's version -- see the header)
BMC_HD void box_muller_pair(double u1, double u2, double& z0, double& z1) {
    const double rad = sqrt(-2.0 * log_normal_arg(u1));
    double sn, cs;
    sincos_2pi(u2, sn, cs);
    z0 = rad * cs;
    z1 = rad * sn;
}

// exp(x) - 1 for 0 <= x < 710 (x >= 710 gives +inf, as 710 itself does): the radius of the
// Student-t variate below.  fdlibm's expm1 without the cases that cannot occur: x = k ln2 + r with
// k = rint(x / ln2) in 0 .. 1024 and |r| <= ln2 / 2 (the product k ln2_hi is exact: ln2_hi ends in 32
// zero bits), c the rounding error of r; p = expm1(r) by the rational kernel in r^2 / 2, with c
// folded in as fdlibm folds it; then exp(x) - 1 = 2^k p + (2^k - 1), formed at half scale (2^1024 is
// no double) by ONE fma where fdlibm branches three ways on k, since a branch per lane is what a
// wave cannot afford.  2^(k-1) - 1/2 is exact up to k = 53 and is 2^(k-1) to well below an ulp
// after.  Worst error found against expm1l: 1.34 ulp (tests/test_ppc_t_host.py, whose bar is 2.7).
BMC_HD double expm1_nonneg(double x) {
    const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10;
    const double Q1 = -3.33333333333331316428e-02, Q2 = 1.58730158725481460165e-03,
                 Q3 = -7.93650757867487942473e-05, Q4 = 4.00821782732936239552e-06,
                 Q5 = -2.01099218183624371326e-07;
    x = fmin(x, 710.0);
    const double dk = rint(x * 1.44269504088896338700e+00);
    const int k = (int)dk;
    const double hi = fma(-dk, ln2_hi, x);
    const double lo = dk * ln2_lo;
    const double r = hi - lo;
    const double c = (hi - r) - lo;
    const double hfx = 0.5 * r;
    const double hxs = r * hfx;
    const double r1 = fma_c(hxs, fma_c(hxs, fma_c(hxs, fma_c(hxs, fma_c(hxs, Q5, Q4), Q3), Q2), Q1), 1.0);
    const double t = fma(-r1, hfx, 3.0);
    double e = hxs * ((r1 - t) / fma(-r, t, 6.0));
    e = fma(r, e - c, -c) - hxs;
    const double p = r - e;
    const uint64_t ih = (uint64_t)(k + 1022) << 52;   // 2^(k-1); not read for k = 0
    double h;
    memcpy(&h, &ih, 8);
    const double big = 2.0 * fma(h, p, h - 0.5);
    return k == 0 ? p : big;
}

// One Student-t variate with nu > 0 degrees of freedom from two uniforms, u1 in (0, 1] and u2 in
// [0, 1]: Bailey's polar form (R. W. Bailey, "Polar generation of random variates with the
// t-distribution", Math. Comp. 62, 1994),
//     t = sqrt(nu (u1^(-2/nu) - 1)) cos(2 pi u2) = sqrt(nu expm1(-(2/nu) log u1)) cos(2 pi u2),
// exact, no rejection step, a fixed number of uniforms; as nu grows the radius tends to
// Box-Muller's sqrt(-2 log u1).  The sine half is t_nu too, but it shares this radius: the two are
// NOT independent (their magnitudes correlate at 0.80 for nu = 1.5), so a caller that needs
// independent variates takes this one and draws again.  two_over_nu is 2 / nu, rounded once by the
// caller.  u1 = 1 gives 0.  Past x = 64 the radius is sqrt(nu) exp(x / 2), which differs from
// sqrt(nu expm1(x)) by exp(-64) / 2 of itself and is finite where exp(x) is not: the largest |t|,
// at u1 = 2^-53, is sqrt(nu) 2^(53/nu), finite for nu >= 0.06 and +-inf only below about 0.052.
// The logarithm, expm1 and the cosine are this file's, so the CPU build gives the device's bits.
BMC_HD double student_t_variate(double u1, double u2, double nu, double two_over_nu) {
    const double x = two_over_nu * -log_normal_arg(u1);
    const bool far = x > 64.0;
    const double em = expm1_nonneg(far ? 0.5 * x : x);
    const double root = sqrt(nu * (far ? 1.0 : em));
    const double rad = far ? root * (em + 1.0) : root;
    double sn, cs;
    sincos_2pi(u2, sn, cs);
    return rad * cs;
}

// Inverse of the standard normal CDF for 0 < p < 1 with min(p, 1 - p) a normal double: Wichura's
// AS 241, routine PPND16 (Applied Statistics 37(3), 1988; about 1e-16 relative).  Three rational
// approximations of degree 7: |p - 1/2| <= 0.425 in q^2, the tails in r = sqrt(-log(min(p, 1 - p))),
// split at r = 5.  Odd about 1/2 by construction: the two sides differ in the sign alone wherever
// 1 - p is exact.  The logarithm is log_normal_arg, so the CPU build gives the device's bits.
BMC_HD double ndtri(double p) {
    const double q = p - 0.5;
    if (fabs(q) <= 0.425) {
        const double r = 0.180625 - q * q;
        const double num = fma(fma(fma(fma(fma(fma(fma(2.5090809287301226727e3, r,
            3.3430575583588128105e4), r, 6.7265770927008700853e4), r, 4.5921953931549871457e4), r,
            1.3731693765509461125e4), r, 1.9715909503065514427e3), r, 1.3314166789178437745e2), r,
            3.3871328727963666080);
        const double den = fma(fma(fma(fma(fma(fma(fma(5.2264952788528545610e3, r,
            2.8729085735721942674e4), r, 3.9307895800092710610e4), r, 2.1213794301586595867e4), r,
            5.3941960214247511077e3), r, 6.8718700749205790830e2), r, 4.2313330701600911252e1), r,
            1.0);
        return q * num / den;
    }
    double r = q < 0 ? p : 1.0 - p;
    r = sqrt(-log_normal_arg(r));
    double val;
    if (r <= 5.0) {
        r -= 1.6;
        const double num = fma(fma(fma(fma(fma(fma(fma(7.74545014278341407640e-4, r,
            2.27238449892691845833e-2), r, 2.41780725177450611770e-1), r, 1.27045825245236838258), r,
            3.64784832476320460504), r, 5.76949722146069140550), r, 4.63033784615654529590), r,
            1.42343711074968357734);
        const double den = fma(fma(fma(fma(fma(fma(fma(1.05075007164441684324e-9, r,
            5.47593808499534494600e-4), r, 1.51986665636164571966e-2), r, 1.48103976427480074590e-1), r,
            6.89767334985100004550e-1), r, 1.67638483018380384940), r, 2.05319162663775882187), r,
            1.0);
        val = num / den;
    } else {
        r -= 5.0;
        const double num = fma(fma(fma(fma(fma(fma(fma(2.01033439929228813265e-7, r,
            2.71155556874348757815e-5), r, 1.24266094738807843860e-3), r, 2.65321895265761230930e-2), r,
            2.96560571828504891230e-1), r, 1.78482653991729133580), r, 5.46378491116411436990), r,
            6.65790464350110377720);
        const double den = fma(fma(fma(fma(fma(fma(fma(2.04426310338993978564e-15, r,
            1.42151175831644588870e-7), r, 1.84631831751005468180e-5), r, 7.86869131145613259100e-4), r,
            1.48753612908506148525e-2), r, 1.36929880922735805310e-1), r, 5.99832206555887937690e-1), r,
            1.0);
        val = num / den;
    }
    return q < 0 ? -val : val;
}

// The Student-t distribution function F_nu(z) for 0.06 <= nu <= 1000 (STUDENT_T_CDF_NU_MIN / _MAX),
// from the density f = f_nu(z) its caller already has (the leave-one-out PIT of kernels_loo.hip:
// f = sigma_s exp(ll)).  With u = z^2 / nu and x = 1 / (1 + u), the tail beyond |z| is
// 1/2 I_x(nu/2, 1/2), evaluated as such for u > 3 / (nu + 2) (x below (a + 1) / (a + b + 2)) and as
// 1/2 - 1/2 I_{u x}(1/2, nu/2) nearer the centre.  In both, the factor in front of the incomplete
// beta function's continued fraction (Numerical Recipes 6.4; DLMF 8.17.22) is |z| f: x^a (1 - x)^(1/2) /
// B(a, 1/2) = |z| f_nu(z), so no lgamma is needed and the long-double C(nu) of the density carries
// the accuracy.  The fraction 1 / (1 + d_1 / (1 + d_2 / ...)), d_n = p_n / ((a + n - 1)(a + n)), is
// brought to  a / (a + p_1 / (a + 1 + p_2 / (a + 2 + ...)))  with
//     p_(2m+1) = -(a + m)(a + b + m) x,   p_(2m) = m (b - m) x,
// and run forward, X_n = (a + n) X_(n-1) + p_n X_(n-2) on numerator and denominator, two terms a
// step, rescaled by 2^-400 past 2^400: ONE division, at the end, where Lentz's form has two a term.
// Then |z| f B_n / (2 A_n) is the tail, or what the centre branch takes from 1/2.  A lane stops on
// its own criterion, successive convergents within 2^-52 of each other (in cross-multiplied form),
// or after STUDENT_T_CDF_MAX_STEPS steps: its result depends on its own (z, nu, f) alone.  55 steps
// are the most found over the domain (at nu = 372, at the switch between the branches);
// tests/test_loo_predict_t_host.py asserts that the cap is not reached and holds the largest
// absolute error to 64 times that of scipy.special.stdtr.
// student_t_tail: P(T > |z|) if `tail`, else 1/2 - P(0 < T <= |z|), from u and zf = |z| f; steps
// receives the steps taken.  u = +inf gives 0 (|z| beyond 1.3e154 counts as infinite), NaN gives NaN.
constexpr double STUDENT_T_CDF_NU_MIN = 0.06, STUDENT_T_CDF_NU_MAX = 1000.0;
constexpr int STUDENT_T_CDF_MAX_STEPS = 80;
BMC_HD double student_t_tail(double u, double nu, double zf, int& steps) {
    steps = 0;
    if (u == __builtin_inf()) return 0.0;
    const double x = 1.0 / (1.0 + u);
    const bool centre = u <= 3.0 / (nu + 2.0);
    const double a = centre ? 0.5 : 0.5 * nu, b = centre ? 0.5 * nu : 0.5;
    const double xx = centre ? u * x : x, ab = a + b;
    double Am = 1.0, A = a, Bm = 0.0, B = 1.0, fm = 0.0;
    bool more = true;
    while (more) {
        // terms 2 m + 1 and 2 m + 2
        const double p1 = -((a + fm) * (ab + fm)) * xx, d1 = a + (2.0 * fm + 1.0);
        const double A1 = fma(d1, A, p1 * Am), B1 = fma(d1, B, p1 * Bm);
        fm += 1.0;
        const double p2 = (fm * (b - fm)) * xx, d2 = a + 2.0 * fm;
        const double A2 = fma(d2, A1, p2 * A), B2 = fma(d2, B1, p2 * B);
        Am = A1, Bm = B1, A = A2, B = B2;
        ++steps;
        if (fabs(A) > 0x1p400) {
            Am *= 0x1p-400, A *= 0x1p-400, Bm *= 0x1p-400, B *= 0x1p-400;
        }
        const double t1 = A * Bm;
        more = fabs(t1 - Am * B) > 0x1p-52 * fabs(t1) && steps < STUDENT_T_CDF_MAX_STEPS;   // (NaN: stops)
    }
    const double m = zf * B / (2.0 * A);
    return centre ? 0.5 - m : m;
}
// F from the tail: the two sides of z share one evaluation on |z|, so F(z) + F(-z) = 1 to the last bit
BMC_HD double student_t_cdf_from(bool negative, double u, double nu, double zf) {
    int steps;
    const double q = student_t_tail(u, nu, zf, steps);
    return negative ? q : 1.0 - q;
}
// F_nu(z) from z, nu and f = f_nu(z).  F(0) = 1/2, F(+-inf) = 1 and 0, NaN gives NaN.
BMC_HD double student_t_cdf(double z, double nu, double f) {
    const double az = fabs(z);
    return student_t_cdf_from(z < 0.0, (az * az) / nu, nu, az < __builtin_inf() ? az * f : 0.0);
}

// The order-preserving 64-bit image of a double (the sort key of kernels_rank.hip): a < b exactly
// when rank_key(a) < rank_key(b), and -0.0 has the key of +0.0 (equality is by value).  NaNs land
// beyond the infinities of their sign; rank_unkey inverts it (-0.0 comes back as +0.0).
BMC_HD uint64_t rank_key(double x) {
    if (x == 0.0) x = 0.0;
    uint64_t u;
    memcpy(&u, &x, 8);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
BMC_HD double rank_unkey(uint64_t k) {
    const uint64_t u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    double x;
    memcpy(&x, &u, 8);
    return x;
}

}  // namespace bmc
