// C ABI, exact K-fold / leave-group-out cross-validation (bmc_kfold_cv; kernels_cv.hip, the plan in
// bmc_cv_plan.h).  One pass over the rows gives every fold's own
// Gram; the host takes total - own, does the K x K algebra of bmc_set_prior per fold, and all
// F x C chains run from those statistics, one wave each.  The context's resident problem and prior
// are not touched; its variate, draw and score buffers are used.
// bmc_cv_path (the plan in bmc_cvpath_plan.h) does the same for every candidate
// component count at once: model k is the leading k columns, so one gather and one Gram pass at
// the widest candidate serve all of them, and the m x F x C chains share the device.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <thread>

#include "bmc_ctx.h"
#include "bmc_cv.h"
#include "host_linalg.hpp"

namespace {

// What depends on the prior alone: P = inv(C0), P b0 and the inverse Cholesky factor of
// B = P + 1e-6 I (bmc_set_prior)
struct PriorBasis {
    bmc_la::Mat P, Li;
    std::vector<double> Pb0;
};

// The per-fold quantities of the chains, flat over the folds
struct FoldArrays {
    std::vector<double> G, WT, lam, c1, c2, u0, g0;   // [F][k][k] x 2, [F][k] x 5
    std::vector<double> beta;   // [2F][k]: the least-squares point of fold f (row f), W u0 (row F + f)
    std::vector<double> scal;   // [F][4]: rss0, sigma2_init, nu0 * sigma20, 0
    FoldArrays(int F, int k)
        : G((size_t)F * k * k), WT((size_t)F * k * k), lam((size_t)F * k), c1((size_t)F * k),
          c2((size_t)F * k), u0((size_t)F * k), g0((size_t)F * k), beta((size_t)2 * F * k),
          scal((size_t)F * 4, 0.0) {}
};

// The training Gram is total - own: each entry carries an absolute error of a few ulps of
// sqrt(D_i D_j), D the diagonal of the TOTAL Gram.  A pivot of D^-1/2 A D^-1/2 that is not above
// that noise says nothing: the fold's training design is numerically rank deficient.
bool numerically_regular(const double* A, const double* dtot, int k) {
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

// The algebra of bmc_set_prior for one fold, from its training statistics A = X'X, xty = X'y with
// the same host_linalg.hpp routines in the same order: the least-squares start, the basis
// W = L^-T Q of L^-1 A L^-T = Q diag(lam) Q', c1, c2, and the sufficient statistics of rss_mode 1
// (G = W'AW, u0, g0).  false: singular.
bool fold_setup(int k, int F, int f, const bmc_la::Mat& A, const std::vector<double>& xty,
                const double* dtot, const PriorBasis& pb, FoldArrays& o) {
    if (!numerically_regular(A.data(), dtot, k)) return false;
    std::vector<double> bols;
    if (!bmc_la::solve(A, xty, k, bols)) return false;
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
    std::vector<double> lam;
    bmc_la::sym_eigh(M, k, lam, Q);
    bmc_la::Mat W((size_t)k * k, 0.0);
    for (int i = 0; i < k; ++i)          // W = Li' Q
        for (int j = 0; j < k; ++j) {
            long double s = 0.0L;
            for (int m = i; m < k; ++m) s += (long double)Li[(size_t)m * k + i] * Q[(size_t)m * k + j];
            W[(size_t)i * k + j] = (double)s;
        }
    double* c1 = &o.c1[(size_t)f * k];
    double* c2 = &o.c2[(size_t)f * k];
    for (int j = 0; j < k; ++j) {
        long double s1 = 0.0L, s2l = 0.0L;
        for (int i = 0; i < k; ++i) {
            s1 += (long double)W[(size_t)i * k + j] * pb.Pb0[i];
            s2l += (long double)W[(size_t)i * k + j] * xty[i];
        }
        c1[j] = (double)s1;
        c2[j] = (double)s2l;
    }
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
    double* G = &o.G[(size_t)f * k * k];
    for (int i = 0; i < k; ++i)
        for (int j = 0; j < k; ++j)
            G[(size_t)i * k + j] = (double)(0.5L * (Gl[(size_t)i * k + j] + Gl[(size_t)j * k + i]));
    double gmax = 0.0;
    for (int j = 0; j < k; ++j) gmax = std::max(gmax, G[(size_t)j * k + j]);
    double* u0 = &o.u0[(size_t)f * k];
    for (int j = 0; j < k; ++j) {
        const double gj = G[(size_t)j * k + j];
        u0[j] = gj > 1e-14 * gmax ? c2[j] / gj : 0.0;
    }
    double* g0 = &o.g0[(size_t)f * k];
    for (int i = 0; i < k; ++i) {
        long double sum = c2[i];
        for (int j = 0; j < k; ++j) sum -= (long double)G[(size_t)i * k + j] * u0[j];
        g0[i] = (double)sum;
    }
    for (int i = 0; i < k; ++i) {
        o.lam[(size_t)f * k + i] = lam[i];
        o.beta[(size_t)f * k + i] = bols[i];
        long double s = 0.0L;     // the centre of the expansion in the coefficient basis: W u0
        for (int j = 0; j < k; ++j) {
            o.WT[((size_t)f * k + i) * k + j] = W[(size_t)j * k + i];
            s += (long double)W[(size_t)i * k + j] * u0[j];
        }
        o.beta[((size_t)F + f) * k + i] = (double)s;
    }
    return true;
}

// The prior's part of the basis (bmc_set_prior) from the leading k x k block of C0 (leading
// dimension ldc) and the leading k entries of b0.  BMC_OK, or the status with *msg set.
int prior_basis(int k, const double* C0, int ldc, const double* b0, PriorBasis& pb, std::string* msg) {
    pb.P.resize((size_t)k * k);
    for (int i = 0; i < k; ++i)
        for (int j = 0; j < k; ++j) pb.P[(size_t)i * k + j] = C0[(size_t)i * ldc + j];
    if (!bmc_la::invert(pb.P, k)) {
        *msg = "Singular matrix (b_mean_cov)";
        return BMC_ESINGULAR;
    }
    bmc_la::Mat B((size_t)k * k), L;
    for (int i = 0; i < k; ++i)
        for (int j = 0; j < k; ++j)
            B[(size_t)i * k + j] = 0.5 * (pb.P[(size_t)i * k + j] + pb.P[(size_t)j * k + i]) +
                                   (i == j ? 1e-6 : 0.0);
    if (!bmc_la::cholesky(B, k, L)) {
        *msg = "prior precision inv(b_mean_cov) + 1e-6 I is not positive definite";
        return BMC_EINVAL;
    }
    bmc_la::lower_inverse(L, k, pb.Li);
    pb.Pb0.assign(k, 0.0);
    for (int i = 0; i < k; ++i) {
        long double s = 0.0L;
        for (int j = 0; j < k; ++j) s += (long double)pb.P[(size_t)i * k + j] * b0[j];
        pb.Pb0[i] = (double)s;
    }
    return BMC_OK;
}

// work(i) for i in 0 .. n_items - 1 on a few host threads (one when `flops` says the threads would
// cost more); work takes items from a shared counter
template <class Work>
void host_pool(int n_items, size_t flops, Work work_item) {
    std::atomic<int> next{0};
    auto work = [&] {
        for (int i = next++; i < n_items; i = next++) work_item(i);
    };
    unsigned nth = std::thread::hardware_concurrency();
    nth = std::min<unsigned>({nth ? nth : 1u, 16u, (unsigned)n_items});
    if (flops < 200000) nth = 1;
    std::vector<std::thread> th;
    for (unsigned i = 1; i < nth; ++i) th.emplace_back(work);
    work();
    for (auto& t : th) t.join();
}

void lower_min(std::atomic<int>& a, int v) {
    int cur = a.load();
    while (v < cur && !a.compare_exchange_weak(cur, v)) {}
}

// ensure + copy host -> device on the context's stream
int upload(bmc_ctx* c, DevBuf& b, const void* src, size_t bytes) {
    if (int rc = ensure(c, b, bytes)) return rc;
    HIPCHK(c, hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, c->stream));
    return BMC_OK;
}

// device bytes the call may spend on a batch's chains: what is free now, what the context's own
// run buffers already hold, less room for the score buffers and the runtime; PYBMC_AMD_CV_MAX_BYTES
// (a test hook: small values force several batches) caps it
int chain_budget(bmc_ctx* c, size_t* budget) {
    size_t free_b = 0, total_b = 0;
    HIPCHK(c, hipMemGetInfo(&free_b, &total_b));
    const size_t have = free_b + c->xi.cap + c->gam.cap + c->uout.cap + c->samples.cap;
    const size_t margin = std::max((size_t)256 << 20, have / 16);
    *budget = have > margin ? have - margin : 0;
    if (const char* e = std::getenv("PYBMC_AMD_CV_MAX_BYTES")) {
        const long long v = std::strtoll(e, nullptr, 10);
        if (v > 0 && (size_t)v < *budget) *budget = (size_t)v;
    }
    return BMC_OK;
}

}  // namespace

extern "C" {

int bmc_kfold_cv(bmc_ctx* c, const double* A, int64_t n, int32_t k, int64_t lda, int layout,
                 const double* y, const int64_t* fold, int32_t n_folds, const double* b0,
                 const double* C0, double nu0, double sigma20, int32_t n_chains, int64_t iters,
                 int64_t burn, int64_t thin, const uint64_t* seeds, double* elpd_out,
                 double* mean_out, double* draws_out) {
    if (!c) return BMC_EINVAL;
    if (!A || !y || !fold || !b0 || !C0 || !seeds || !elpd_out || !mean_out)
        return fail(c, BMC_EINVAL, "A, y, fold, b0, C0, seeds, elpd_out and mean_out must not be NULL");
    if (layout != BMC_ROW_MAJOR && layout != BMC_COL_MAJOR)
        return fail(c, BMC_EINVAL, "layout must be BMC_ROW_MAJOR or BMC_COL_MAJOR");
    const int F = n_folds, C = n_chains;
    std::vector<int64_t> count;
    const std::string bad = cv_check(n, k, F, fold, &count);
    if (!bad.empty()) return fail(c, BMC_EINVAL, bad);
    if (lda < (layout == BMC_COL_MAJOR ? n : (int64_t)k))
        return fail(c, BMC_EINVAL, "lda is smaller than the leading dimension of A");
    if (C < 1 || C > 65535) return fail(c, BMC_EINVAL, "n_chains must be between 1 and 65535");
    if (iters < 1 || iters >= 0xffffffffll) return fail(c, BMC_EINVAL, "iters must be between 1 and 2^32 - 2");
    if (burn < 0 || burn >= iters || thin < 1)
        return fail(c, BMC_EINVAL, "need 0 <= burn < iters and thin >= 1");
    const int64_t T = iters, kept = cv_kept_draws(T, burn, thin), S = (int64_t)C * kept;
    if (S < 2) return fail(c, BMC_EINVAL, "need at least 2 draws per fold after burn and thin");
    HIPCHK(c, hipSetDevice(c->device));

    // ---- the prior's part of the basis (bmc_set_prior) ----
    PriorBasis pb;
    {
        std::string msg;
        if (int prc = prior_basis(k, C0, k, b0, pb, &msg)) return fail(c, prc, msg);
    }

    // ---- rows into fold order, one Gram per fold ----
    const CvSegments seg = cv_segments(n, F, fold);
    const int ka = k + 1, ldz = cv_ldz(k), nt = cv_tiles(k), np = nt * (nt + 1) / 2;
    const size_t abytes = strided_bytes(n, k, lda, layout, 8);
    DevBuf dA, dY, dSrc, dRowFold, dZ, dYs, dGr0, dGrn, dGoff, dGpart, dGram;
    int rc;
    if ((rc = upload(c, dA, A, abytes)) || (rc = upload(c, dY, y, (size_t)n * 8)) ||
        (rc = upload(c, dSrc, seg.src.data(), (size_t)seg.n_pad * 8)) ||
        (rc = upload(c, dRowFold, seg.row_fold.data(), (size_t)seg.n_pad * 4)) ||
        (rc = upload(c, dGr0, seg.gram.row0.data(), seg.gram.row0.size() * 8)) ||
        (rc = upload(c, dGrn, seg.gram.rows.data(), seg.gram.rows.size() * 4)) ||
        (rc = upload(c, dGoff, seg.gram.fold_off.data(), seg.gram.fold_off.size() * 4)) ||
        (rc = ensure_all(c, {{dZ, (size_t)seg.n_pad * ldz * 8}, {dYs, (size_t)seg.n_pad * 8},
                             {dGpart, seg.gram.row0.size() * np * 256 * 8},
                             {dGram, (size_t)F * ka * ka * 8}})))
        return rc;
    HIPCHK(c, launch_cv_gather((const double*)dA.p, (const double*)dY.p, lda, layout == BMC_COL_MAJOR, k,
                               (const int64_t*)dSrc.p, seg.n_pad, (double*)dZ.p, (double*)dYs.p, c->stream));
    HIPCHK(c, launch_cv_fold_gram((const double*)dZ.p, k, F, (const int64_t*)dGr0.p, (const int32_t*)dGrn.p,
                                  (int32_t)seg.gram.row0.size(), (const int32_t*)dGoff.p, (double*)dGpart.p,
                                  (double*)dGram.p, c->stream));
    std::vector<double> own((size_t)F * ka * ka);
    HIPCHK(c, hipMemcpyAsync(own.data(), dGram.p, own.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));

    // ---- training statistics: total (folds added in order) minus own, in extended precision ----
    std::vector<long double> total((size_t)ka * ka, 0.0L);
    for (int f = 0; f < F; ++f)
        for (int e = 0; e < ka * ka; ++e) total[e] += (long double)own[(size_t)f * ka * ka + e];
    std::vector<double> dtot(k);
    for (int i = 0; i < k; ++i) dtot[i] = (double)total[(size_t)i * ka + i];

    // ---- the K x K algebra of every fold, a few host threads ----
    FoldArrays fa(F, k);
    std::atomic<int> first_bad{F};
    host_pool(F, (size_t)F * k * k * k, [&](int f) {
        bmc_la::Mat At((size_t)k * k);
        std::vector<double> xty(k);
        const double* o = &own[(size_t)f * ka * ka];
        for (int i = 0; i < k; ++i) {
            for (int j = 0; j < k; ++j)
                At[(size_t)i * k + j] = (double)(total[(size_t)i * ka + j] - (long double)o[(size_t)i * ka + j]);
            xty[i] = (double)(total[(size_t)i * ka + k] - (long double)o[(size_t)i * ka + k]);
        }
        if (!fold_setup(k, F, f, At, xty, dtot.data(), pb, fa)) lower_min(first_bad, f);
    });
    if (first_bad.load() < F)
        return fail(c, BMC_ESINGULAR, "fold " + std::to_string(first_bad.load()) +
                                          ": Singular matrix (X'X of its training rows)");

    // ---- rss at the least-squares point and at the centre of the expansion: block sums ----
    DevBuf dBeta, dRr0, dRrn, dRpart;
    const size_t nrc = seg.rss.row0.size();
    if ((rc = upload(c, dBeta, fa.beta.data(), fa.beta.size() * 8)) ||
        (rc = upload(c, dRr0, seg.rss.row0.data(), nrc * 8)) ||
        (rc = upload(c, dRrn, seg.rss.rows.data(), nrc * 4)) ||
        (rc = ensure(c, dRpart, nrc * 2 * F * 8)))
        return rc;
    HIPCHK(c, launch_cv_block_rss((const double*)dZ.p, k, (const double*)dBeta.p, 2 * F,
                                  (const int64_t*)dRr0.p, (const int32_t*)dRrn.p, (int32_t)nrc,
                                  (double*)dRpart.p, c->stream));
    std::vector<double> rpart(nrc * 2 * F);
    HIPCHK(c, hipMemcpyAsync(rpart.data(), dRpart.p, rpart.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int g = 0; g < F; ++g) {
        // R[b][h] over the chunks of fold h in order, then the folds h != g in order
        long double at_ols = 0.0L, at_u0 = 0.0L;
        for (int h = 0; h < F; ++h) {
            if (h == g) continue;
            long double r0 = 0.0L, r1 = 0.0L;
            for (int32_t ch = seg.rss.fold_off[h]; ch < seg.rss.fold_off[h + 1]; ++ch) {
                r0 += (long double)rpart[(size_t)ch * 2 * F + g];
                r1 += (long double)rpart[(size_t)ch * 2 * F + F + g];
            }
            at_ols += r0;
            at_u0 += r1;
        }
        double s2 = (double)at_ols / (double)(n - count[g]);
        if (!(s2 >= 1e-6)) s2 = s2 != s2 ? s2 : 1e-6;   // max(s2, 1e-6); NaN propagates
        fa.scal[(size_t)g * 4 + 0] = (double)at_u0;
        fa.scal[(size_t)g * 4 + 1] = s2;
        fa.scal[(size_t)g * 4 + 2] = nu0 * sigma20;
    }
    DevBuf dG, dWT, dLam, dC1, dC2, dU0, dG0, dScal, dBbar, dElpd, dMean;
    if ((rc = upload(c, dG, fa.G.data(), fa.G.size() * 8)) || (rc = upload(c, dWT, fa.WT.data(), fa.WT.size() * 8)) ||
        (rc = upload(c, dLam, fa.lam.data(), fa.lam.size() * 8)) ||
        (rc = upload(c, dC1, fa.c1.data(), fa.c1.size() * 8)) || (rc = upload(c, dC2, fa.c2.data(), fa.c2.size() * 8)) ||
        (rc = upload(c, dU0, fa.u0.data(), fa.u0.size() * 8)) || (rc = upload(c, dG0, fa.g0.data(), fa.g0.size() * 8)) ||
        (rc = upload(c, dScal, fa.scal.data(), fa.scal.size() * 8)) ||
        (rc = upload(c, c->seeds, seeds, (size_t)F * C * sizeof(uint64_t))) ||
        (rc = ensure_all(c, {{dBbar, (size_t)F * k * 8}, {dElpd, (size_t)seg.n_pad * 8},
                             {dMean, (size_t)seg.n_pad * 8}})))
        return rc;
    HIPCHK(c, hipMemsetAsync(dElpd.p, 0, (size_t)seg.n_pad * 8, c->stream));

    // ---- the chains, in batches of folds that fit the device ----
    size_t budget = 0;
    if ((rc = chain_budget(c, &budget))) return rc;
    std::vector<CvBatch> batches;
    if (!plan_cv_batches(F, C, cv_chain_bytes(k, T, kept), budget, batches))
        return fail(c, BMC_ENOMEM, "the " + std::to_string(C) + " chains of one fold need " +
                                       std::to_string(cv_chain_bytes(k, T, kept) * (size_t)C) +
                                       " bytes of device memory; " + std::to_string(budget) + " are free");
    const size_t K = (size_t)k, K1 = K + 1;
    for (const CvBatch& b : batches) {
        const size_t nch = (size_t)(b.f1 - b.f0) * C;
        if ((rc = ensure_all(c, {{c->xi, nch * T * K * 8}, {c->gam, nch * T * 8}, {c->uout, nch * T * K1 * 8},
                                 {c->samples, nch * kept * K1 * 8}})))
            return rc;
        // the variates of chain (f, c) under its own seed; the gamma shape is the fold's
        for (int f = b.f0; f < b.f1; ++f) {
            const size_t l0 = (size_t)(f - b.f0) * C;
            const double shape = (nu0 + (double)(n - count[f])) / 2.0;   // inference_utils.py:50
            HIPCHK(c, launch_rng_fill((const uint64_t*)c->seeds.p + (size_t)f * C, C, (int64_t)(T * K),
                                      (double*)c->xi.p + l0 * T * K, shape, T, (double*)c->gam.p + l0 * T,
                                      c->stream));
        }
        CvGramArgs ga;
        ga.k = k;
        ga.chains_per_fold = C;
        ga.G = (const double*)dG.p; ga.lam = (const double*)dLam.p;
        ga.c1 = (const double*)dC1.p; ga.c2 = (const double*)dC2.p;
        ga.u0 = (const double*)dU0.p; ga.g0 = (const double*)dG0.p;
        ga.scal = (const double*)dScal.p;
        ga.xi = (const double*)c->xi.p; ga.gam = (const double*)c->gam.p; ga.uout = (double*)c->uout.p;
        ga.iters = T;
        for (const CvLaunch& l : b.launches) {
            ga.chain0 = l.chain0;
            ga.local0 = l.chain0 - (int64_t)b.f0 * C;
            ga.n_chains = l.n_chains;
            HIPCHK(c, launch_cv_gram(ga, c->stream));
        }
        HIPCHK(c, launch_cv_unrotate((const double*)c->uout.p, (const double*)dWT.p, k, C, b.f0, (int64_t)nch,
                                     T, burn, thin, kept, (double*)c->samples.p, c->stream));
        HIPCHK(c, launch_cv_colmean((const double*)c->samples.p, k, S, b.f1 - b.f0, b.f0, (double*)dBbar.p,
                                    c->stream));
        // held-out scores: the score kernels on the fold's row segment against the fold's draws
        for (int f = b.f0; f < b.f1; ++f) {
            const int64_t nf = count[f];
            const ScorePlan plan = plan_score(nf, S, k, c->n_cu);
            const ScoreBuffers sb = score_buffers(plan, S);
            if ((rc = ensure_all(c, {{c->scAp, sb.Ap}, {c->scYp, sb.yp}, {c->scCh, sb.ch}, {c->scPart, sb.part},
                                     {c->scOut, (size_t)nf * 3 * 8}})))
                return rc;
            ScoreArgs sa;
            sa.A = (const double*)dZ.p + (size_t)seg.offset[f] * ldz;
            sa.y = (const double*)dYs.p + seg.offset[f];
            sa.theta = (const double*)c->samples.p + (size_t)(f - b.f0) * S * K1;
            sa.n = nf; sa.lda = ldz; sa.S = S; sa.ldt = (int64_t)K1; sa.k = k; sa.col_major = 0;
            sa.Ap = (double*)c->scAp.p; sa.yp = (double*)c->scYp.p; sa.ch = (double*)c->scCh.p;
            sa.part = (double*)c->scPart.p; sa.out = (double*)c->scOut.p;
            HIPCHK(c, launch_score(sa, plan, c->stream));
            HIPCHK(c, hipMemcpyAsync((double*)dElpd.p + seg.offset[f], sa.out, (size_t)nf * 8,
                                     hipMemcpyDeviceToDevice, c->stream));
        }
        if (draws_out)
            if ((rc = copy_to_host(c, draws_out + (size_t)b.f0 * C * kept * K1, c->samples.p,
                                   nch * kept * K1 * 8, nch * kept * K1 * 8, 1)))
                return rc;
    }
    HIPCHK(c, launch_cv_mean((const double*)dZ.p, ldz, k, (const int32_t*)dRowFold.p, (const double*)dBbar.p,
                             seg.n_pad, (double*)dMean.p, c->stream));
    std::vector<double> elpd_s(seg.n_pad), mean_s(seg.n_pad);
    HIPCHK(c, hipMemcpyAsync(elpd_s.data(), dElpd.p, (size_t)seg.n_pad * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(mean_s.data(), dMean.p, (size_t)seg.n_pad * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int64_t r = 0; r < seg.n_pad; ++r)
        if (seg.src[r] >= 0) {
            elpd_out[seg.src[r]] = elpd_s[r];
            mean_out[seg.src[r]] = mean_s[r];
        }
    return BMC_OK;
}

int bmc_cv_path(bmc_ctx* c, const double* A, int64_t n, int32_t k, int64_t lda, int layout,
                const double* y, const int64_t* fold, int32_t n_folds, const double* b0,
                const double* C0, double nu0, double sigma20, int32_t n_chains, int64_t iters,
                int64_t burn, int64_t thin, const uint64_t* seeds, const int32_t* comps,
                int32_t n_comps, double* elpd_out, double* mean_out, double* draws_out) {
    if (!c) return BMC_EINVAL;
    if (!A || !y || !fold || !b0 || !C0 || !seeds || !comps || !elpd_out || !mean_out)
        return fail(c, BMC_EINVAL,
                    "A, y, fold, b0, C0, seeds, comps, elpd_out and mean_out must not be NULL");
    if (layout != BMC_ROW_MAJOR && layout != BMC_COL_MAJOR)
        return fail(c, BMC_EINVAL, "layout must be BMC_ROW_MAJOR or BMC_COL_MAJOR");
    const int F = n_folds, C = n_chains, m = n_comps;
    std::vector<int64_t> count;
    std::string bad = cvpath_check(k, comps, m);
    if (!bad.empty()) return fail(c, BMC_EINVAL, bad);
    const int kx = comps[m - 1];   // the widest candidate: the columns of A the device ever reads
    bad = cv_check(n, kx, F, fold, &count);
    if (!bad.empty()) return fail(c, BMC_EINVAL, bad);
    if (lda < (layout == BMC_COL_MAJOR ? n : (int64_t)k))
        return fail(c, BMC_EINVAL, "lda is smaller than the leading dimension of A");
    if (C < 1 || C > 65535) return fail(c, BMC_EINVAL, "n_chains must be between 1 and 65535");
    if (iters < 1 || iters >= 0xffffffffll) return fail(c, BMC_EINVAL, "iters must be between 1 and 2^32 - 2");
    if (burn < 0 || burn >= iters || thin < 1)
        return fail(c, BMC_EINVAL, "need 0 <= burn < iters and thin >= 1");
    const int64_t T = iters, kept = cv_kept_draws(T, burn, thin), S = (int64_t)C * kept;
    if (S < 2) return fail(c, BMC_EINVAL, "need at least 2 draws per fold after burn and thin");
    HIPCHK(c, hipSetDevice(c->device));

    // ---- the prior's part of the basis, per candidate: inv of the LEADING block of C0 ----
    std::vector<PriorBasis> pb(m);
    for (int j = 0; j < m; ++j) {
        std::string msg;
        if (int prc = prior_basis(comps[j], C0, k, b0, pb[j], &msg))
            return fail(c, prc, std::to_string(comps[j]) + " components: " + msg);
    }

    // ---- rows into fold order and one Gram per fold, once, at the widest candidate ----
    const CvSegments seg = cv_segments(n, F, fold);
    const int ka = kx + 1, ldz = cv_ldz(kx), nt = cv_tiles(kx), np = nt * (nt + 1) / 2;
    const size_t abytes = strided_bytes(n, k, lda, layout, 8);
    DevBuf dA, dY, dSrc, dRowFold, dZ, dYs, dGr0, dGrn, dGoff, dGpart, dGram;
    int rc;
    if ((rc = upload(c, dA, A, abytes)) || (rc = upload(c, dY, y, (size_t)n * 8)) ||
        (rc = upload(c, dSrc, seg.src.data(), (size_t)seg.n_pad * 8)) ||
        (rc = upload(c, dRowFold, seg.row_fold.data(), (size_t)seg.n_pad * 4)) ||
        (rc = upload(c, dGr0, seg.gram.row0.data(), seg.gram.row0.size() * 8)) ||
        (rc = upload(c, dGrn, seg.gram.rows.data(), seg.gram.rows.size() * 4)) ||
        (rc = upload(c, dGoff, seg.gram.fold_off.data(), seg.gram.fold_off.size() * 4)) ||
        (rc = ensure_all(c, {{dZ, (size_t)seg.n_pad * ldz * 8}, {dYs, (size_t)seg.n_pad * 8},
                             {dGpart, seg.gram.row0.size() * np * 256 * 8},
                             {dGram, (size_t)F * ka * ka * 8}})))
        return rc;
    HIPCHK(c, launch_cv_gather((const double*)dA.p, (const double*)dY.p, lda, layout == BMC_COL_MAJOR, kx,
                               (const int64_t*)dSrc.p, seg.n_pad, (double*)dZ.p, (double*)dYs.p, c->stream));
    HIPCHK(c, launch_cv_fold_gram((const double*)dZ.p, kx, F, (const int64_t*)dGr0.p, (const int32_t*)dGrn.p,
                                  (int32_t)seg.gram.row0.size(), (const int32_t*)dGoff.p, (double*)dGpart.p,
                                  (double*)dGram.p, c->stream));
    std::vector<double> own((size_t)F * ka * ka);
    HIPCHK(c, hipMemcpyAsync(own.data(), dGram.p, own.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<long double> total((size_t)ka * ka, 0.0L);
    for (int f = 0; f < F; ++f)
        for (int e = 0; e < ka * ka; ++e) total[e] += (long double)own[(size_t)f * ka * ka + e];
    std::vector<double> dtot(kx);
    for (int i = 0; i < kx; ++i) dtot[i] = (double)total[(size_t)i * ka + i];

    // ---- the k x k algebra of every (candidate, fold): the leading block, y's column last ----
    std::vector<FoldArrays> fa;
    fa.reserve(m);
    size_t flops = 0;
    for (int j = 0; j < m; ++j) {
        fa.emplace_back(F, comps[j]);
        flops += (size_t)F * comps[j] * comps[j] * comps[j];
    }
    const int P = m * F;
    std::atomic<int> first_bad{P};
    host_pool(P, flops, [&](int p) {
        const int j = p / F, f = p - j * F, kj = comps[j];
        bmc_la::Mat At((size_t)kj * kj);
        std::vector<double> xty(kj);
        const double* o = &own[(size_t)f * ka * ka];
        for (int i = 0; i < kj; ++i) {
            for (int l = 0; l < kj; ++l)
                At[(size_t)i * kj + l] = (double)(total[(size_t)i * ka + l] - (long double)o[(size_t)i * ka + l]);
            xty[i] = (double)(total[(size_t)i * ka + kx] - (long double)o[(size_t)i * ka + kx]);
        }
        if (!fold_setup(kj, F, f, At, xty, dtot.data(), pb[j], fa[j])) lower_min(first_bad, p);
    });
    if (first_bad.load() < P) {
        const int j = first_bad.load() / F, f = first_bad.load() - j * F;
        return fail(c, BMC_ESINGULAR, "fold " + std::to_string(f) + ", " + std::to_string(comps[j]) +
                                          " components: Singular matrix (X'X of its training rows)");
    }

    // ---- rss of every (candidate, fold) at its two points in one launch: coefficients zero-padded
    //      to the gathered width, row b = 2 p (least squares), 2 p + 1 (centre of the expansion) ----
    const int nb = 2 * P;
    std::vector<double> beta((size_t)nb * kx, 0.0);
    for (int p = 0; p < P; ++p) {
        const int j = p / F, f = p - j * F, kj = comps[j];
        for (int i = 0; i < kj; ++i) {
            beta[(size_t)(2 * p) * kx + i] = fa[j].beta[(size_t)f * kj + i];
            beta[(size_t)(2 * p + 1) * kx + i] = fa[j].beta[((size_t)F + f) * kj + i];
        }
    }
    DevBuf dBeta, dRr0, dRrn, dRpart;
    const size_t nrc = seg.rss.row0.size();
    if ((rc = upload(c, dBeta, beta.data(), beta.size() * 8)) ||
        (rc = upload(c, dRr0, seg.rss.row0.data(), nrc * 8)) ||
        (rc = upload(c, dRrn, seg.rss.rows.data(), nrc * 4)) ||
        (rc = ensure(c, dRpart, nrc * nb * 8)))
        return rc;
    HIPCHK(c, launch_cv_block_rss((const double*)dZ.p, kx, (const double*)dBeta.p, nb,
                                  (const int64_t*)dRr0.p, (const int32_t*)dRrn.p, (int32_t)nrc,
                                  (double*)dRpart.p, c->stream));
    std::vector<double> rpart(nrc * nb);
    HIPCHK(c, hipMemcpyAsync(rpart.data(), dRpart.p, rpart.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int p = 0; p < P; ++p) {
        const int j = p / F, g = p - j * F;
        long double at_ols = 0.0L, at_u0 = 0.0L;
        for (int h = 0; h < F; ++h) {
            if (h == g) continue;
            long double r0 = 0.0L, r1 = 0.0L;
            for (int32_t ch = seg.rss.fold_off[h]; ch < seg.rss.fold_off[h + 1]; ++ch) {
                r0 += (long double)rpart[(size_t)ch * nb + 2 * p];
                r1 += (long double)rpart[(size_t)ch * nb + 2 * p + 1];
            }
            at_ols += r0;
            at_u0 += r1;
        }
        double s2 = (double)at_ols / (double)(n - count[g]);
        if (!(s2 >= 1e-6)) s2 = s2 != s2 ? s2 : 1e-6;   // max(s2, 1e-6); NaN propagates
        fa[j].scal[(size_t)g * 4 + 0] = (double)at_u0;
        fa[j].scal[(size_t)g * 4 + 1] = s2;
        fa[j].scal[(size_t)g * 4 + 2] = nu0 * sigma20;
    }

    // ---- the set-up arrays of all problems, candidate after candidate ----
    std::vector<int64_t> moff, voff;
    cvpath_setup_offsets(F, comps, m, moff, voff);
    std::vector<double> hG(moff[m]), hWT(moff[m]), hLam(voff[m]), hC1(voff[m]), hC2(voff[m]), hU0(voff[m]),
        hG0(voff[m]), hScal((size_t)P * 4);
    for (int j = 0; j < m; ++j) {
        std::copy(fa[j].G.begin(), fa[j].G.end(), hG.begin() + moff[j]);
        std::copy(fa[j].WT.begin(), fa[j].WT.end(), hWT.begin() + moff[j]);
        std::copy(fa[j].lam.begin(), fa[j].lam.end(), hLam.begin() + voff[j]);
        std::copy(fa[j].c1.begin(), fa[j].c1.end(), hC1.begin() + voff[j]);
        std::copy(fa[j].c2.begin(), fa[j].c2.end(), hC2.begin() + voff[j]);
        std::copy(fa[j].u0.begin(), fa[j].u0.end(), hU0.begin() + voff[j]);
        std::copy(fa[j].g0.begin(), fa[j].g0.end(), hG0.begin() + voff[j]);
        std::copy(fa[j].scal.begin(), fa[j].scal.end(), hScal.begin() + (size_t)j * F * 4);
    }
    DevBuf dG, dWT, dLam, dC1, dC2, dU0, dG0, dScal, dBbar, dElpd, dMean, dDesc;
    const size_t npad = (size_t)seg.n_pad;
    if ((rc = upload(c, dG, hG.data(), hG.size() * 8)) || (rc = upload(c, dWT, hWT.data(), hWT.size() * 8)) ||
        (rc = upload(c, dLam, hLam.data(), hLam.size() * 8)) || (rc = upload(c, dC1, hC1.data(), hC1.size() * 8)) ||
        (rc = upload(c, dC2, hC2.data(), hC2.size() * 8)) || (rc = upload(c, dU0, hU0.data(), hU0.size() * 8)) ||
        (rc = upload(c, dG0, hG0.data(), hG0.size() * 8)) || (rc = upload(c, dScal, hScal.data(), hScal.size() * 8)) ||
        (rc = upload(c, c->seeds, seeds, (size_t)F * C * sizeof(uint64_t))) ||
        (rc = ensure_all(c, {{dBbar, (size_t)voff[m] * 8}, {dElpd, (size_t)m * npad * 8},
                             {dMean, (size_t)m * npad * 8}})))
        return rc;
    HIPCHK(c, hipMemsetAsync(dElpd.p, 0, (size_t)m * npad * 8, c->stream));

    // ---- the chains, in batches of whole problems that fit the device ----
    size_t budget = 0;
    if ((rc = chain_budget(c, &budget))) return rc;
    std::vector<CvPathBatch> batches;
    {
        int32_t too_big = 0;
        size_t need = 0;
        if (!plan_cvpath(F, C, comps, m, T, kept, budget, batches, &too_big, &need))
            return fail(c, BMC_ENOMEM, "the " + std::to_string(C) + " chains of one fold at " +
                                           std::to_string(comps[too_big / F]) + " components need " +
                                           std::to_string(need) + " bytes of device memory; " +
                                           std::to_string(budget) + " are free");
    }
    std::vector<size_t> doff(m + 1, 0);   // candidate j's block of draws_out, in doubles
    for (int j = 0; j < m; ++j) doff[j + 1] = doff[j] + (size_t)F * C * kept * (comps[j] + 1);
    for (const CvPathBatch& b : batches) {
        const int nprob = b.p1 - b.p0;
        if ((rc = ensure_all(c, {{c->xi, (size_t)b.xi_len * 8}, {c->gam, (size_t)b.gam_len * 8},
                                 {c->uout, (size_t)b.u_len * 8}, {c->samples, (size_t)b.d_len * 8}})) ||
            (rc = upload(c, dDesc, b.desc.data(), (size_t)nprob * sizeof(CvPathDesc))))
            return rc;
        // the variates of chain (k, f, c) under seeds[f][c]: what bmc_kfold_cv draws at width k
        for (const CvPathDesc& d : b.desc) {
            const double shape = (nu0 + (double)(n - count[d.fold])) / 2.0;
            HIPCHK(c, launch_rng_fill((const uint64_t*)c->seeds.p + (size_t)d.fold * C, C, (int64_t)(T * d.k),
                                      (double*)c->xi.p + d.xi_off, shape, T, (double*)c->gam.p + d.gam_off,
                                      c->stream));
        }
        CvPathArgs pa;
        pa.desc = (const CvPathDesc*)dDesc.p;
        pa.chains_per_problem = C;
        pa.G = (const double*)dG.p; pa.lam = (const double*)dLam.p;
        pa.c1 = (const double*)dC1.p; pa.c2 = (const double*)dC2.p;
        pa.u0 = (const double*)dU0.p; pa.g0 = (const double*)dG0.p;
        pa.scal = (const double*)dScal.p;
        pa.xi = (const double*)c->xi.p; pa.gam = (const double*)c->gam.p; pa.uout = (double*)c->uout.p;
        pa.iters = T;
        for (const CvPathLaunch& l : b.launches) {
            pa.kmax = l.kmax;
            pa.chain0 = l.chain0;
            pa.n_chains = l.n_chains;
            HIPCHK(c, launch_cv_path(pa, c->stream));
        }
        // downstream, per run of one candidate's folds [q0, q1) of the batch
        for (int q0 = 0; q0 < nprob;) {
            int q1 = q0;
            while (q1 < nprob && b.desc[q1].cand == b.desc[q0].cand) ++q1;
            const CvPathDesc& d0 = b.desc[q0];
            const int j = d0.cand, kj = d0.k, f0 = d0.fold, nf_run = q1 - q0;
            const size_t K1 = (size_t)kj + 1;
            double* draws = (double*)c->samples.p + d0.d_off;
            HIPCHK(c, launch_cv_unrotate((const double*)c->uout.p + d0.u_off, (const double*)dWT.p + moff[j], kj,
                                         C, f0, (int64_t)nf_run * C, T, burn, thin, kept, draws, c->stream));
            HIPCHK(c, launch_cv_colmean(draws, kj, S, nf_run, f0, (double*)dBbar.p + voff[j], c->stream));
            for (int q = q0; q < q1; ++q) {
                const int f = b.desc[q].fold;
                const int64_t nf = count[f];
                const ScorePlan plan = plan_score(nf, S, kj, c->n_cu);
                const ScoreBuffers sb = score_buffers(plan, S);
                if ((rc = ensure_all(c, {{c->scAp, sb.Ap}, {c->scYp, sb.yp}, {c->scCh, sb.ch},
                                         {c->scPart, sb.part}, {c->scOut, (size_t)nf * 3 * 8}})))
                    return rc;
                ScoreArgs sa;
                sa.A = (const double*)dZ.p + (size_t)seg.offset[f] * ldz;
                sa.y = (const double*)dYs.p + seg.offset[f];
                sa.theta = (const double*)c->samples.p + b.desc[q].d_off;
                sa.n = nf; sa.lda = ldz; sa.S = S; sa.ldt = (int64_t)K1; sa.k = kj; sa.col_major = 0;
                sa.Ap = (double*)c->scAp.p; sa.yp = (double*)c->scYp.p; sa.ch = (double*)c->scCh.p;
                sa.part = (double*)c->scPart.p; sa.out = (double*)c->scOut.p;
                HIPCHK(c, launch_score(sa, plan, c->stream));
                HIPCHK(c, hipMemcpyAsync((double*)dElpd.p + (size_t)j * npad + seg.offset[f], sa.out,
                                         (size_t)nf * 8, hipMemcpyDeviceToDevice, c->stream));
            }
            if (draws_out) {
                const size_t bytes = (size_t)nf_run * C * kept * K1 * 8;
                if ((rc = copy_to_host(c, draws_out + doff[j] + (size_t)f0 * C * kept * K1, draws, bytes, bytes, 1)))
                    return rc;
            }
            q0 = q1;
        }
    }
    for (int j = 0; j < m; ++j)
        HIPCHK(c, launch_cv_mean((const double*)dZ.p, ldz, comps[j], (const int32_t*)dRowFold.p,
                                 (const double*)dBbar.p + voff[j], seg.n_pad, (double*)dMean.p + (size_t)j * npad,
                                 c->stream));
    std::vector<double> elpd_s((size_t)m * npad), mean_s((size_t)m * npad);
    HIPCHK(c, hipMemcpyAsync(elpd_s.data(), dElpd.p, elpd_s.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(mean_s.data(), dMean.p, mean_s.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int j = 0; j < m; ++j)
        for (int64_t r = 0; r < seg.n_pad; ++r)
            if (seg.src[r] >= 0) {
                elpd_out[(size_t)j * n + seg.src[r]] = elpd_s[(size_t)j * npad + r];
                mean_out[(size_t)j * n + seg.src[r]] = mean_s[(size_t)j * npad + r];
            }
    return BMC_OK;
}

}  // extern "C"
