// The K x K host algebra that turns X'X, X'y and a prior into a chain's set-up arrays, once, for
// bmc_set_prior (capi_core.hip) and for every fold of bmc_kfold_cv / bmc_cv_path (capi_cv.hip).
// Host only: host_linalg.hpp and the standard library, no HIP type and no bmc_ctx, so that g++
// builds it for tests/basis_check.cpp (tests/test_basis_host.py).  Nothing here formats a message:
// the callers turn a BasisStatus into their own.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

#include "host_linalg.hpp"

namespace bmc {

enum BasisStatus {
    BASIS_OK = 0,
    BASIS_C0_SINGULAR,   // inv(C0) does not exist
    BASIS_NOT_PD,        // inv(C0) + 1e-6 I has no Cholesky factor
    BASIS_A_SINGULAR,    // X'X is (numerically) rank deficient
};

// What depends on the prior alone: P = inv(C0), P b0 and the inverse Cholesky factor of
// B = sym(P) + 1e-6 I
struct PriorBasis {
    bmc_la::Mat P, Li;
    std::vector<double> Pb0;
};

// From the leading k x k block of C0 (leading dimension ldc) and the leading k entries of b0.
// After BASIS_NOT_PD pb.P is inv(C0) and the rest is unset.
inline BasisStatus prior_basis(int k, const double* C0, int ldc, const double* b0, PriorBasis& pb) {
    pb.P.resize((size_t)k * k);
    for (int i = 0; i < k; ++i)
        for (int j = 0; j < k; ++j) pb.P[(size_t)i * k + j] = C0[(size_t)i * ldc + j];
    if (!bmc_la::invert(pb.P, k)) return BASIS_C0_SINGULAR;      // (inference_utils.py:22)
    bmc_la::Mat B((size_t)k * k), L;
    for (int i = 0; i < k; ++i)
        for (int j = 0; j < k; ++j)
            B[(size_t)i * k + j] = 0.5 * (pb.P[(size_t)i * k + j] + pb.P[(size_t)j * k + i]) +
                                   (i == j ? 1e-6 : 0.0);
    if (!bmc_la::cholesky(B, k, L)) return BASIS_NOT_PD;
    bmc_la::lower_inverse(L, k, pb.Li);
    pb.Pb0.assign(k, 0.0);
    for (int i = 0; i < k; ++i) {
        long double s = 0.0L;
        for (int j = 0; j < k; ++j) s += (long double)pb.P[(size_t)i * k + j] * b0[j];
        pb.Pb0[i] = (double)s;
    }
    return BASIS_OK;
}

// The basis of one problem: B = L L', L^-1 A L^-T = Q diag(lam) Q', W = L^-T Q, c1 = W'P b0,
// c2 = W'xty; with want_gram the sufficient statistics of rss_mode 1 as well, all in extended
// precision: G = W'AW (= diag(lam) up to rounding), the least-squares point u0 in the rotated
// basis and g0 = X~'(y - X~ u0) = c2 - G u0 (else G, u0, g0 are left empty).
struct ChainBasis {
    std::vector<double> lam, W, c1, c2;   // [k], [k][k], [k], [k]
    std::vector<double> G, u0, g0;        // [k][k], [k], [k]
};

inline void chain_basis(int k, const bmc_la::Mat& A, const std::vector<double>& xty, const PriorBasis& pb,
                        bool want_gram, ChainBasis& o) {
    const bmc_la::Mat& Li = pb.Li;
    bmc_la::Mat tmp((size_t)k * k, 0.0), M((size_t)k * k, 0.0);
    for (int i = 0; i < k; ++i)          // tmp = Li * A
        for (int m = 0; m <= i; ++m) {
            const double l = Li[(size_t)i * k + m];
            if (l == 0.0) continue;
            for (int j = 0; j < k; ++j) tmp[(size_t)i * k + j] += l * A[(size_t)m * k + j];
        }
    for (int i = 0; i < k; ++i)          // M = tmp * Li'
        for (int j = 0; j < k; ++j) {
            long double s = 0.0L;
            for (int m = 0; m <= j; ++m) s += (long double)tmp[(size_t)i * k + m] * Li[(size_t)j * k + m];
            M[(size_t)i * k + j] = (double)s;
        }
    for (int i = 0; i < k; ++i)
        for (int j = i + 1; j < k; ++j) {
            const double v = 0.5 * (M[(size_t)i * k + j] + M[(size_t)j * k + i]);
            M[(size_t)i * k + j] = M[(size_t)j * k + i] = v;
        }
    bmc_la::Mat Q;
    bmc_la::sym_eigh(M, k, o.lam, Q);
    std::vector<double>& W = o.W;
    W.assign((size_t)k * k, 0.0);
    for (int i = 0; i < k; ++i)          // W = Li' Q
        for (int j = 0; j < k; ++j) {
            long double s = 0.0L;
            for (int m = i; m < k; ++m) s += (long double)Li[(size_t)m * k + i] * Q[(size_t)m * k + j];
            W[(size_t)i * k + j] = (double)s;
        }
    o.c1.assign(k, 0.0);
    o.c2.assign(k, 0.0);
    for (int j = 0; j < k; ++j) {
        long double s1 = 0.0L, s2l = 0.0L;
        for (int i = 0; i < k; ++i) {
            s1 += (long double)W[(size_t)i * k + j] * pb.Pb0[i];
            s2l += (long double)W[(size_t)i * k + j] * xty[i];
        }
        o.c1[j] = (double)s1;
        o.c2[j] = (double)s2l;
    }
    o.G.clear();
    o.u0.clear();
    o.g0.clear();
    if (!want_gram) return;
    std::vector<long double> AW((size_t)k * k, 0.0L);
    for (int i = 0; i < k; ++i)
        for (int m = 0; m < k; ++m) {
            const long double aim = A[(size_t)i * k + m];
            for (int j = 0; j < k; ++j) AW[(size_t)i * k + j] += aim * W[(size_t)m * k + j];
        }
    std::vector<long double> Gl((size_t)k * k, 0.0L);
    for (int i = 0; i < k; ++i)
        for (int j = 0; j < k; ++j) {
            long double sum = 0.0L;
            for (int m = 0; m < k; ++m) sum += (long double)W[(size_t)m * k + i] * AW[(size_t)m * k + j];
            Gl[(size_t)i * k + j] = sum;
        }
    o.G.assign((size_t)k * k, 0.0);
    for (int i = 0; i < k; ++i)
        for (int j = 0; j < k; ++j)
            o.G[(size_t)i * k + j] = (double)(0.5L * (Gl[(size_t)i * k + j] + Gl[(size_t)j * k + i]));
    double gmax = 0.0;
    for (int j = 0; j < k; ++j) gmax = std::max(gmax, o.G[(size_t)j * k + j]);
    o.u0.assign(k, 0.0);
    for (int j = 0; j < k; ++j) {
        const double gj = o.G[(size_t)j * k + j];
        o.u0[j] = gj > 1e-14 * gmax ? o.c2[j] / gj : 0.0;
    }
    o.g0.assign(k, 0.0);
    for (int i = 0; i < k; ++i) {
        long double sum = o.c2[i];
        for (int j = 0; j < k; ++j) sum -= (long double)o.G[(size_t)i * k + j] * o.u0[j];
        o.g0[i] = (double)sum;
    }
}

// The training Gram of a fold is total - own: each entry carries an absolute error of a few ulps
// of sqrt(D_i D_j), D the diagonal of the TOTAL Gram.  A pivot of D^-1/2 A D^-1/2 that is not above
// that noise says nothing: the fold's training design is numerically rank deficient.
inline bool numerically_regular(const double* A, const double* dtot, int k) {
    std::vector<double> a((size_t)k * k);
    for (int i = 0; i < k; ++i) {
        if (!(dtot[i] > 0.0)) return false;
        for (int j = 0; j < k; ++j) a[(size_t)i * k + j] = A[(size_t)i * k + j] / std::sqrt(dtot[i] * dtot[j]);
    }
    const double tol = 16.0 * k * 2.220446049250313e-16;
    for (int c = 0; c < k; ++c) {
        int p = c;
        double best = std::fabs(a[(size_t)c * k + c]);
        for (int r = c + 1; r < k; ++r) {
            const double v = std::fabs(a[(size_t)r * k + c]);
            if (v > best) { best = v; p = r; }
        }
        if (!(best > tol) || !std::isfinite(best)) return false;
        if (p != c)
            for (int j = 0; j < k; ++j) std::swap(a[(size_t)p * k + j], a[(size_t)c * k + j]);
        for (int r = c + 1; r < k; ++r) {
            const double f = a[(size_t)r * k + c] / a[(size_t)c * k + c];
            if (f == 0.0) continue;
            for (int j = c; j < k; ++j) a[(size_t)r * k + j] -= f * a[(size_t)c * k + j];
        }
    }
    return true;
}

// The per-fold quantities of the cross-validation chains, flat over the folds
struct FoldArrays {
    std::vector<double> G, WT, lam, c1, c2, u0, g0;   // [F][k][k] x 2, [F][k] x 5
    std::vector<double> beta;   // [2F][k]: the least-squares point of fold f (row f), W u0 (row F + f)
    std::vector<double> scal;   // [F][4]: rss0, sigma2_init, nu0 * sigma20, 0
    FoldArrays(int F, int k)
        : G((size_t)F * k * k), WT((size_t)F * k * k), lam((size_t)F * k), c1((size_t)F * k),
          c2((size_t)F * k), u0((size_t)F * k), g0((size_t)F * k), beta((size_t)2 * F * k),
          scal((size_t)F * 4, 0.0) {}
};

// Fold f of F from its training statistics A = X'X, xty = X'y (k <= 64): the least-squares start
// and chain_basis with the statistics of rss_mode 1, packed into o with W transposed.
// BASIS_A_SINGULAR when A is numerically rank deficient against the total diagonal dtot.
inline BasisStatus fold_setup(int k, int F, int f, const bmc_la::Mat& A, const std::vector<double>& xty,
                              const double* dtot, const PriorBasis& pb, FoldArrays& o) {
    if (!numerically_regular(A.data(), dtot, k)) return BASIS_A_SINGULAR;
    std::vector<double> bols;
    if (!bmc_la::solve(A, xty, k, bols)) return BASIS_A_SINGULAR;
    ChainBasis cb;
    chain_basis(k, A, xty, pb, true, cb);
    const size_t v = (size_t)f * k, m = v * k;
    std::copy(cb.G.begin(), cb.G.end(), o.G.begin() + m);
    std::copy(cb.lam.begin(), cb.lam.end(), o.lam.begin() + v);
    std::copy(cb.c1.begin(), cb.c1.end(), o.c1.begin() + v);
    std::copy(cb.c2.begin(), cb.c2.end(), o.c2.begin() + v);
    std::copy(cb.u0.begin(), cb.u0.end(), o.u0.begin() + v);
    std::copy(cb.g0.begin(), cb.g0.end(), o.g0.begin() + v);
    for (int i = 0; i < k; ++i) {
        o.beta[v + i] = bols[i];
        long double s = 0.0L;     // the centre of the expansion in the coefficient basis: W u0
        for (int j = 0; j < k; ++j) {
            o.WT[m + (size_t)i * k + j] = cb.W[(size_t)j * k + i];
            s += (long double)cb.W[(size_t)i * k + j] * cb.u0[j];
        }
        o.beta[((size_t)F + f) * k + i] = (double)s;
    }
    return BASIS_OK;
}

}  // namespace bmc
