// C ABI, exact K-fold / leave-group-out cross-validation (bmc_kfold_cv; kernels_cv.hip, the plan in
// bmc_cv_plan.h).  One pass over the rows gives every fold's own
// Gram; the host takes total - own, does the K x K algebra of bmc_basis.h per fold (fold_setup:
// what bmc_set_prior computes for the resident problem), and all F x C chains run from those
// statistics, one wave each.  The context's resident problem and prior are not touched; its
// variate, draw and score buffers are used.
// bmc_cv_path (the plan in bmc_cvpath_plan.h) does the same for every candidate
// component count at once: model k is the leading k columns, so one gather and one Gram pass at
// the widest candidate serve all of them, and the m x F x C chains share the device.
// bmc_kfold_cv_t / bmc_kfold_cv_tv (the plan in bmc_cvt_plan.h) are the Student-t
// form: X'LX changes every sweep, so every fold's training rows are packed for the robust sampler's
// kernel and all F x C chains run in its folded form, one workgroup each.
// All entry points are the same stages around their own chain stage (the variates, the chain
// kernel and its batching): cv_check_args, cv_front, training_stats, cv_rss, score_fold, cv_scatter.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <thread>

#include "bmc_basis.h"
#include "bmc_ctx.h"
#include "bmc_cv.h"
#include "bmc_cvt_plan.h"
#include "bmc_robust.h"
#include "host_linalg.hpp"

namespace {

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

// The argument checks both entry points share, after their NULL, layout and candidate checks.  A
// has k columns of which the device reads the leading kx.  Fills the fold sizes and the kept draws
// per chain.
int cv_check_args(bmc_ctx* c, int64_t n, int32_t k, int32_t kx, int64_t lda, int layout, const int64_t* fold,
                  int F, int C, int64_t iters, int64_t burn, int64_t thin, std::vector<int64_t>* count,
                  int64_t* kept) {
    const std::string bad = cv_check(n, kx, F, fold, count);
    if (!bad.empty()) return fail(c, BMC_EINVAL, bad);
    if (lda < (layout == BMC_COL_MAJOR ? n : (int64_t)k))
        return fail(c, BMC_EINVAL, "lda is smaller than the leading dimension of A");
    if (C < 1 || C > 65535) return fail(c, BMC_EINVAL, "n_chains must be between 1 and 65535");
    if (iters < 1 || iters >= 0xffffffffll) return fail(c, BMC_EINVAL, "iters must be between 1 and 2^32 - 2");
    if (burn < 0 || burn >= iters || thin < 1)
        return fail(c, BMC_EINVAL, "need 0 <= burn < iters and thin >= 1");
    *kept = cv_kept_draws(iters, burn, thin);
    if ((int64_t)C * *kept < 2) return fail(c, BMC_EINVAL, "need at least 2 draws per fold after burn and thin");
    return BMC_OK;
}

// What the front leaves for the later stages: the rows in fold order on the device (Z, ys) at
// width kx, every fold's own Gram of [A y] on the host, their sum and its diagonal; and the device
// blocks of the rss stage, which live as long
struct CvFront {
    CvSegments seg;
    int kx = 0, ka = 0, ldz = 0;      // gathered width, kx + 1 (y's column is index kx), cv_ldz(kx)
    DevBuf dA, dY, dSrc, dRowFold, dZ, dYs, dGr0, dGrn, dGoff, dGpart, dGram;
    DevBuf dBeta, dRr0, dRrn, dRpart;
    std::vector<double> own;          // [F][ka][ka]
    std::vector<long double> total;   // [ka][ka]: the folds added in order, in extended precision
    std::vector<double> dtot;         // [kx]
};

// rows into fold order, one Gram per fold, at width kx of A's k columns
int cv_front(bmc_ctx* c, const double* A, int64_t n, int32_t k, int64_t lda, int layout, const double* y,
             const int64_t* fold, int F, int kx, CvFront& fr) {
    fr.seg = cv_segments(n, F, fold);
    fr.kx = kx;
    fr.ka = kx + 1;
    fr.ldz = cv_ldz(kx);
    const CvSegments& seg = fr.seg;
    const int ka = fr.ka, nt = cv_tiles(kx), np = nt * (nt + 1) / 2;
    int rc;
    if ((rc = upload(c, fr.dA, A, strided_bytes(n, k, lda, layout, 8))) ||
        (rc = upload(c, fr.dY, y, (size_t)n * 8)) ||
        (rc = upload(c, fr.dSrc, seg.src.data(), (size_t)seg.n_pad * 8)) ||
        (rc = upload(c, fr.dRowFold, seg.row_fold.data(), (size_t)seg.n_pad * 4)) ||
        (rc = upload(c, fr.dGr0, seg.gram.row0.data(), seg.gram.row0.size() * 8)) ||
        (rc = upload(c, fr.dGrn, seg.gram.rows.data(), seg.gram.rows.size() * 4)) ||
        (rc = upload(c, fr.dGoff, seg.gram.fold_off.data(), seg.gram.fold_off.size() * 4)) ||
        (rc = ensure_all(c, {{fr.dZ, (size_t)seg.n_pad * fr.ldz * 8}, {fr.dYs, (size_t)seg.n_pad * 8},
                             {fr.dGpart, seg.gram.row0.size() * np * 256 * 8},
                             {fr.dGram, (size_t)F * ka * ka * 8}})))
        return rc;
    HIPCHK(c, launch_cv_gather((const double*)fr.dA.p, (const double*)fr.dY.p, lda, layout == BMC_COL_MAJOR, kx,
                               (const int64_t*)fr.dSrc.p, seg.n_pad, (double*)fr.dZ.p, (double*)fr.dYs.p,
                               c->stream));
    HIPCHK(c, launch_cv_fold_gram((const double*)fr.dZ.p, kx, F, (const int64_t*)fr.dGr0.p,
                                  (const int32_t*)fr.dGrn.p, (int32_t)seg.gram.row0.size(),
                                  (const int32_t*)fr.dGoff.p, (double*)fr.dGpart.p, (double*)fr.dGram.p,
                                  c->stream));
    fr.own.resize((size_t)F * ka * ka);
    HIPCHK(c, hipMemcpyAsync(fr.own.data(), fr.dGram.p, fr.own.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    fr.total.assign((size_t)ka * ka, 0.0L);
    for (int f = 0; f < F; ++f)
        for (int e = 0; e < ka * ka; ++e) fr.total[e] += (long double)fr.own[(size_t)f * ka * ka + e];
    fr.dtot.resize(kx);
    for (int i = 0; i < kx; ++i) fr.dtot[i] = (double)fr.total[(size_t)i * ka + i];
    return BMC_OK;
}

// The training statistics of fold f at the leading kj columns: total minus own, in extended
// precision
void training_stats(const CvFront& fr, int f, int kj, bmc_la::Mat& At, std::vector<double>& xty) {
    const int ka = fr.ka;
    const double* o = &fr.own[(size_t)f * ka * ka];
    At.resize((size_t)kj * kj);
    xty.resize(kj);
    for (int i = 0; i < kj; ++i) {
        for (int l = 0; l < kj; ++l)
            At[(size_t)i * kj + l] = (double)(fr.total[(size_t)i * ka + l] - (long double)o[(size_t)i * ka + l]);
        xty[i] = (double)(fr.total[(size_t)i * ka + fr.kx] - (long double)o[(size_t)i * ka + fr.kx]);
    }
}

// Where problem p of the rss stage finds its two block-rss columns and its [4] block of scal
struct RssSlot {
    int fold, at_ols, at_u0;
    double* scal;
};

// rss of n_prob problems at their least-squares points and at the centres of their expansions:
// block sums of (y - a . beta_b)^2 for the nb rows of beta [nb][kx] in one launch, then per problem
// the sums over the chunks of fold h in order and the folds h != its own in order; rss0,
// sigma2_init = max(rss_ols / n_train, 1e-6) and nu0 * sigma20 go into the problem's scal block
template <class Slot>
int cv_rss(bmc_ctx* c, CvFront& fr, const std::vector<double>& beta, int nb, int n_prob, int64_t n,
           const std::vector<int64_t>& count, double nu0_sigma20, Slot slot) {
    const CvSegments& seg = fr.seg;
    const int F = seg.F;
    const size_t nrc = seg.rss.row0.size();
    int rc;
    if ((rc = upload(c, fr.dBeta, beta.data(), beta.size() * 8)) ||
        (rc = upload(c, fr.dRr0, seg.rss.row0.data(), nrc * 8)) ||
        (rc = upload(c, fr.dRrn, seg.rss.rows.data(), nrc * 4)) ||
        (rc = ensure(c, fr.dRpart, nrc * nb * 8)))
        return rc;
    HIPCHK(c, launch_cv_block_rss((const double*)fr.dZ.p, fr.kx, (const double*)fr.dBeta.p, nb,
                                  (const int64_t*)fr.dRr0.p, (const int32_t*)fr.dRrn.p, (int32_t)nrc,
                                  (double*)fr.dRpart.p, c->stream));
    std::vector<double> rpart(nrc * nb);
    HIPCHK(c, hipMemcpyAsync(rpart.data(), fr.dRpart.p, rpart.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int p = 0; p < n_prob; ++p) {
        const RssSlot s = slot(p);
        long double at_ols = 0.0L, at_u0 = 0.0L;
        for (int h = 0; h < F; ++h) {
            if (h == s.fold) continue;
            long double r0 = 0.0L, r1 = 0.0L;
            for (int32_t ch = seg.rss.fold_off[h]; ch < seg.rss.fold_off[h + 1]; ++ch) {
                r0 += (long double)rpart[(size_t)ch * nb + s.at_ols];
                r1 += (long double)rpart[(size_t)ch * nb + s.at_u0];
            }
            at_ols += r0;
            at_u0 += r1;
        }
        s.scal[0] = (double)at_u0;
        s.scal[1] = sigma2_floor((double)at_ols / (double)(n - count[s.fold]));
        s.scal[2] = nu0_sigma20;
    }
    return BMC_OK;
}

// held-out scores of fold f (nf rows): the score kernels on the fold's row segment against its S
// pooled draws theta [S][kj + 1], the log predictive densities into the fold's segment of elpd_row.
// The likelihood as ScoreArgs names it: Gaussian, Student-t with one nu, or a nu per draw.
int score_fold(bmc_ctx* c, const CvFront& fr, int f, int64_t nf, int64_t S, int kj, const double* theta,
               double* elpd_row, double nu = 0.0, const NuPerDraw& per_draw = NuPerDraw()) {
    const ScorePlan plan = plan_score(nf, S, kj, c->n_cu);
    const ScoreBuffers sb = score_buffers(plan, S);
    if (int rc = ensure_all(c, {{c->scAp, sb.Ap}, {c->scYp, sb.yp}, {c->scCh, sb.ch}, {c->scPart, sb.part},
                                {c->scOut, (size_t)nf * 3 * 8}}))
        return rc;
    ScoreArgs sa;
    sa.A = (const double*)fr.dZ.p + (size_t)fr.seg.offset[f] * fr.ldz;
    sa.y = (const double*)fr.dYs.p + fr.seg.offset[f];
    sa.theta = theta;
    sa.n = nf; sa.lda = fr.ldz; sa.S = S; sa.ldt = (int64_t)kj + 1; sa.k = kj; sa.col_major = 0;
    sa.Ap = (double*)c->scAp.p; sa.yp = (double*)c->scYp.p; sa.ch = (double*)c->scCh.p;
    sa.part = (double*)c->scPart.p; sa.out = (double*)c->scOut.p;
    sa.nu = nu; sa.per_draw = per_draw;
    HIPCHK(c, launch_score(sa, plan, c->stream));
    HIPCHK(c, hipMemcpyAsync(elpd_row + fr.seg.offset[f], sa.out, (size_t)nf * 8, hipMemcpyDeviceToDevice,
                             c->stream));
    return BMC_OK;
}

// the m rows of dElpd and dMean (n_pad each, fold order) back to the host and into the caller's
// row order (m rows of n)
int cv_scatter(bmc_ctx* c, const CvFront& fr, int m, int64_t n, const DevBuf& dElpd, const DevBuf& dMean,
               double* elpd_out, double* mean_out) {
    const CvSegments& seg = fr.seg;
    const size_t npad = (size_t)seg.n_pad;
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

// the error of a prior_basis that did not return BASIS_OK; `who` names the candidate ("" for one)
int fail_prior(bmc_ctx* c, BasisStatus st, const std::string& who) {
    if (st == BASIS_C0_SINGULAR) return fail(c, BMC_ESINGULAR, who + "Singular matrix (b_mean_cov)");
    return fail(c, BMC_EINVAL, who + "prior precision inv(b_mean_cov) + 1e-6 I is not positive definite");
}

// ---- Student-t folds (bmc_kfold_cv_t, bmc_kfold_cv_tv) ------------------------------

// nu on a grid: the prior and where the kept indices go (host, [F][C][kept], or NULL)
struct CvtNu {
    const double *grid, *weight;
    int32_t n_grid, nu_init;
    int32_t* idx_out;
};

// device blocks of the per-fold set-up, reused from fold to fold
struct CvtSetup {
    DevBuf dTr, dG, dGy, dXp, dYp;
};

// The set-up of one fold's training rows tr [nt] (caller's row indices, ascending), the steps of
// bmc_set_problem, bmc_set_prior and bmc_robust_run on those rows alone: gather, panelise, the
// least-squares start of the panels (gram_to_host, ols_start: the routines of the resident problem),
// and the pack into Z / yv.  *singular: X'X of the rows has no solve.
int cvt_fold_setup(bmc_ctx* c, const CvFront& fr, int64_t lda, int layout, int k, const std::vector<int64_t>& tr,
                   CvtSetup& st, double* Z, double* yv, double* sigma2_init, bool* singular) {
    const int64_t nt = (int64_t)tr.size();
    const int ldg = cv_ldz(k);
    Panels P = make_panels(nt, k, 0, nullptr, nullptr);
    const int RP = 64 * P.vec;
    int rc;
    if ((rc = upload(c, st.dTr, tr.data(), (size_t)nt * 8)) ||
        (rc = ensure_all(c, {{st.dG, (size_t)nt * ldg * 8}, {st.dGy, (size_t)nt * 8},
                             {st.dXp, (size_t)P.npanels * k * RP * 8}, {st.dYp, (size_t)P.npanels * RP * 8}})))
        return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));   // tr may be a temporary of the caller
    P.X = st.dXp.p;
    P.y = st.dYp.p;
    HIPCHK(c, launch_cv_gather((const double*)fr.dA.p, (const double*)fr.dY.p, lda, layout == BMC_COL_MAJOR, k,
                               (const int64_t*)st.dTr.p, nt, (double*)st.dG.p, (double*)st.dGy.p, c->stream));
    HIPCHK(c, launch_panelize(st.dG.p, st.dGy.p, nt, k, ldg, 0, 0, P.vec, st.dXp.p, st.dYp.p, P.npanels, c->stream));
    std::vector<double> gram;
    OlsStart ols;
    if ((rc = gram_to_host(c, P, gram)) || (rc = ols_start(c, P, gram, ols))) return rc;
    *singular = ols.singular;
    *sigma2_init = ols.sigma2_init;
    if (!ols.singular) HIPCHK(c, launch_robust_pack(P, Z, yv, c->stream));
    return BMC_OK;
}

int kfold_cv_t(bmc_ctx* c, const std::string& name, const double* A, int64_t n, int32_t k, int64_t lda, int layout,
               const double* y, const int64_t* fold, int32_t F, const double* b0, const double* C0, double nu0,
               double sigma20, int32_t C, int64_t iters, int64_t burn, int64_t thin, const uint64_t* seeds,
               double nu, const CvtNu* ns, double* elpd_out, double* mean_out, double* draws_out,
               double* weight_out) {
    if (!A || !y || !fold || !b0 || !C0 || !seeds || !elpd_out || !mean_out)
        return fail(c, BMC_EINVAL, name + "A, y, fold, b0, C0, seeds, elpd_out and mean_out must not be NULL");
    if (layout != BMC_ROW_MAJOR && layout != BMC_COL_MAJOR)
        return fail(c, BMC_EINVAL, name + "layout must be BMC_ROW_MAJOR or BMC_COL_MAJOR");
    std::vector<int64_t> count;
    const std::string bad = cvt_check(n, k, F, fold, C, iters, burn, thin, nu, ns ? ns->grid : nullptr,
                                      ns ? ns->weight : nullptr, ns ? ns->n_grid : 0, ns ? ns->nu_init : 0, &count);
    if (!bad.empty()) return fail(c, BMC_EINVAL, name + bad);
    if (ns && (!ns->grid || !ns->weight)) return fail(c, BMC_EINVAL, name + "nu_grid and nu_weight must not be NULL");
    if (lda < (layout == BMC_COL_MAJOR ? n : (int64_t)k))
        return fail(c, BMC_EINVAL, name + "lda is smaller than the leading dimension of A");
    const int G = ns ? ns->n_grid : 0;
    if (ns) nu = ns->grid[ns->nu_init];
    const int64_t T = iters, Ta = T - burn, kept = cv_kept_draws(iters, burn, thin), S = (int64_t)C * kept;
    const size_t K = (size_t)k, K1 = K + 1;
    HIPCHK(c, hipSetDevice(c->device));
    int rc;

    PriorBasis pb;
    if (const BasisStatus st = prior_basis(k, C0, k, b0, pb)) return fail_prior(c, st, name);

    // ---- rows into fold order (the held-out segments of the score and the mean), A and y on the device ----
    CvFront fr;
    if ((rc = cv_front(c, A, n, k, lda, layout, y, fold, F, k, fr))) return rc;
    const CvSegments& seg = fr.seg;

    DevBuf dPrior, dBbar, dElpd, dMean, dZt, dWs, dWsum, dDesc, dFoldOf, dRow0, dNuTab, dIdxA, dIdxK, dScNu;
    std::vector<double> prior(K * K + K);
    std::copy(pb.P.begin(), pb.P.end(), prior.begin());
    std::copy(pb.Pb0.begin(), pb.Pb0.end(), prior.begin() + K * K);
    if ((rc = upload(c, dPrior, prior.data(), prior.size() * 8)) ||
        (rc = upload(c, c->seeds, seeds, (size_t)F * C * sizeof(uint64_t))) ||
        (rc = ensure_all(c, {{dBbar, (size_t)F * K * 8}, {dElpd, (size_t)seg.n_pad * 8},
                             {dMean, (size_t)seg.n_pad * 8}})))
        return rc;
    HIPCHK(c, hipMemsetAsync(dElpd.p, 0, (size_t)seg.n_pad * 8, c->stream));
    // the score's table of a nu per draw over the grid; every fold's index is set where it is scored
    NuPerDraw score_nu;
    if (ns && (rc = stage_nu(c, dScNu, NU_SCORE, ns->grid, G, 0, nullptr, false, score_nu))) return rc;
    if (weight_out) {
        const double nan = std::nan("");
        std::fill(weight_out, weight_out + (size_t)F * C * (size_t)n, nan);
    }

    // ---- batches of whole folds that fit the device ----
    size_t budget = 0;
    if ((rc = chain_budget(c, &budget))) return rc;
    std::vector<CvtBatch> batches;
    {
        int32_t too_big = 0;
        size_t need = 0;
        if (!plan_cvt(F, C, k, count.data(), n, T, burn, kept, G, budget, batches, &too_big, &need))
            return fail(c, BMC_ENOMEM, name + "fold " + std::to_string(too_big) + " with its " + std::to_string(C) +
                                           " chains needs " + std::to_string(need) + " bytes of device memory; " +
                                           std::to_string(budget) + " are free");
    }
    CvtSetup setup;
    std::vector<std::vector<int64_t>> tr;
    for (const CvtBatch& b : batches) {
        const int nf = b.f1 - b.f0;
        const size_t nch = (size_t)nf * C;
        if ((rc = ensure_all(c, {{dZt, (size_t)(b.z_len + b.yv_len) * 8}, {dWs, (size_t)b.rows * 16},
                                 {dWsum, (size_t)b.rows * 8}, {c->xi, nch * T * K * 8}, {c->gam, nch * T * 8},
                                 {c->uout, nch * Ta * K1 * 8}, {c->samples, nch * kept * K1 * 8},
                                 {c->status, nch * sizeof(int32_t)}, {dDesc, (size_t)nf * sizeof(RobustFold)},
                                 {dFoldOf, nch * 4}, {dRow0, nch * 8}})))
            return rc;
        if (ns && (rc = ensure_all(c, {{dNuTab, (size_t)nf * 4 * G * 8}, {dIdxA, nch * Ta * 4}, {dIdxK, nch * kept * 4}})))
            return rc;
        double* Zb = (double*)dZt.p;
        double* yvb = Zb + b.z_len;
        // ---- every fold's own rows, start value and nu table ----
        std::vector<RobustFold> desc(nf);
        std::vector<int32_t> fold_of(nch);
        std::vector<int64_t> row0(nch);
        std::vector<double> nutab(ns ? (size_t)nf * 4 * G : 0);
        tr.assign(nf, {});
        for (int q = 0; q < nf; ++q) {
            const CvtFold& d = b.folds[q];
            tr[q].reserve((size_t)d.n_train);
            for (int64_t i = 0; i < n; ++i)
                if (fold[i] != d.fold) tr[q].push_back(i);
            bool singular = false;
            double s2 = 0.0;
            if ((rc = cvt_fold_setup(c, fr, lda, layout, k, tr[q], setup, Zb + d.z_off, yvb + d.yv_off, &s2, &singular)))
                return rc;
            if (singular)
                return fail(c, BMC_ESINGULAR, name + "fold " + std::to_string(d.fold) +
                                                  ": Singular matrix (X'X of its training rows)");
            desc[q].Z = Zb + d.z_off;
            desc[q].yv = yvb + d.yv_off;
            desc[q].nu_tab = ns ? (const double*)dNuTab.p + (size_t)q * 4 * G : nullptr;
            desc[q].n = d.n_train;
            desc[q].rows_per_wave = d.rows_per_wave;
            desc[q].sigma2_init = s2;
            if (ns) robust_nu_table(ns->grid, ns->weight, G, d.n_train, &nutab[(size_t)q * 4 * G]);
            for (int cc = 0; cc < C; ++cc) {
                fold_of[(size_t)q * C + cc] = q;
                row0[(size_t)q * C + cc] = d.row0 + (int64_t)cc * d.n_train;
            }
        }
        HIPCHK(c, hipMemcpyAsync(dDesc.p, desc.data(), (size_t)nf * sizeof(RobustFold), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(dFoldOf.p, fold_of.data(), nch * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(dRow0.p, row0.data(), nch * 8, hipMemcpyHostToDevice, c->stream));
        if (ns) {
            HIPCHK(c, hipMemcpyAsync(dNuTab.p, nutab.data(), nutab.size() * 8, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemsetAsync(dIdxA.p, 0xff, nch * Ta * 4, c->stream));   // -1: never drawn
        }
        HIPCHK(c, hipMemsetAsync(c->status.p, 0, nch * sizeof(int32_t), c->stream));
        // ---- the variates of chain (f, c) under its own seed; the gamma shape is the fold's ----
        for (int q = 0; q < nf; ++q) {
            const CvtFold& d = b.folds[q];
            const size_t l0 = (size_t)q * C;
            const double shape = (nu0 + (double)d.n_train) / 2.0;
            HIPCHK(c, launch_rng_fill((const uint64_t*)c->seeds.p + (size_t)d.fold * C, C, (int64_t)(T * K),
                                      (double*)c->xi.p + l0 * T * K, shape, T, (double*)c->gam.p + l0 * T, c->stream));
        }
        // ---- all chains of the batch, one workgroup each ----
        RobustFoldedArgs a;
        a.fold = (const RobustFold*)dDesc.p;
        a.k = k;
        a.P = (const double*)dPrior.p;
        a.Pb0 = (const double*)dPrior.p + K * K;
        a.nu = nu;
        a.shape_l = (nu + 1.0) / 2.0;
        a.nu0_s20 = nu0 * sigma20;
        a.iters = Ta;
        a.burn = burn;
        a.ws = (double*)dWs.p;
        a.wsum = (double*)dWsum.p;
        a.n_grid = G;
        a.nu_init = ns ? ns->nu_init : 0;
        a.tstat = nullptr;
        for (const CvtLaunch& l : b.launches) {
            const size_t c0 = (size_t)l.chain0;
            a.n_chains = l.n_chains;
            a.fold_of_chain = (const int32_t*)dFoldOf.p + c0;
            a.row0 = (const int64_t*)dRow0.p + c0;
            a.seeds = (const uint64_t*)c->seeds.p + (size_t)b.f0 * C + c0;
            a.xi = (const double*)c->xi.p + c0 * T * K;
            a.gam = (const double*)c->gam.p + c0 * T;
            a.samples = (double*)c->uout.p + c0 * Ta * K1;
            a.status = (int32_t*)c->status.p + c0;
            a.nu_idx = ns ? (int32_t*)dIdxA.p + c0 * Ta : nullptr;
            HIPCHK(c, launch_robust_folded(a, c->stream));
        }
        std::vector<int32_t> st(nch, 0);
        HIPCHK(c, hipMemcpyAsync(st.data(), c->status.p, nch * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));   // also: desc, fold_of, row0 and nutab are locals
        if ((rc = robust_status_check(c, st, [&](size_t i, const std::string& what) {
                return name + "fold " + std::to_string(b.f0 + (int)(i / C)) + ", chain " + std::to_string(i % C) + ": " + what;
            })))
            return rc;
        // ---- every thin-th draw after burn, the fold means, the held-out scores ----
        HIPCHK(c, launch_robust_thin((const double*)c->uout.p, (int64_t)nch, Ta, thin, kept, (int32_t)K1,
                                     (double*)c->samples.p, c->stream));
        if (ns)
            HIPCHK(c, launch_robust_thin_idx((const int32_t*)dIdxA.p, (int64_t)nch, Ta, thin, kept, (int32_t*)dIdxK.p,
                                             c->stream));
        HIPCHK(c, launch_cv_colmean((const double*)c->samples.p, k, S, nf, b.f0, (double*)dBbar.p, c->stream));
        for (int q = 0; q < nf; ++q) {
            const int f = b.f0 + q;
            if (ns) score_nu.index = (const int32_t*)dIdxK.p + (size_t)q * S;
            if ((rc = score_fold(c, fr, f, count[f], S, k, (const double*)c->samples.p + (size_t)q * S * K1,
                                 (double*)dElpd.p, ns ? 0.0 : nu, score_nu)))
                return rc;
        }
        if (draws_out)
            if ((rc = copy_to_host(c, draws_out + (size_t)b.f0 * C * kept * K1, c->samples.p, nch * kept * K1 * 8,
                                   nch * kept * K1 * 8, 1)))
                return rc;
        if (ns && ns->idx_out)
            if ((rc = copy_to_host(c, ns->idx_out + (size_t)b.f0 * C * kept, dIdxK.p, nch * kept * 4, nch * kept * 4, 1)))
                return rc;
        if (weight_out) {
            std::vector<double> w((size_t)b.rows);
            if ((rc = copy_to_host(c, w.data(), dWsum.p, (size_t)b.rows * 8, (size_t)b.rows * 8, 1))) return rc;
            for (int q = 0; q < nf; ++q)
                for (int cc = 0; cc < C; ++cc) {
                    const double* src = &w[(size_t)row0[(size_t)q * C + cc]];
                    double* dst = weight_out + ((size_t)(b.f0 + q) * C + cc) * (size_t)n;
                    for (size_t r = 0; r < tr[q].size(); ++r) dst[tr[q][r]] = src[r];
                }
        }
    }
    HIPCHK(c, launch_cv_mean((const double*)fr.dZ.p, fr.ldz, k, (const int32_t*)fr.dRowFold.p, (const double*)dBbar.p,
                             seg.n_pad, (double*)dMean.p, c->stream));
    return cv_scatter(c, fr, 1, n, dElpd, dMean, elpd_out, mean_out);
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
    int64_t kept = 0;
    int rc;
    if ((rc = cv_check_args(c, n, k, k, lda, layout, fold, F, C, iters, burn, thin, &count, &kept))) return rc;
    const int64_t T = iters, S = (int64_t)C * kept;
    HIPCHK(c, hipSetDevice(c->device));

    // ---- the prior's part of the basis ----
    PriorBasis pb;
    if (const BasisStatus st = prior_basis(k, C0, k, b0, pb)) return fail_prior(c, st, "");

    // ---- rows into fold order, one Gram per fold ----
    CvFront fr;
    if ((rc = cv_front(c, A, n, k, lda, layout, y, fold, F, k, fr))) return rc;
    const CvSegments& seg = fr.seg;

    // ---- the K x K algebra of every fold, a few host threads ----
    FoldArrays fa(F, k);
    std::atomic<int> first_bad{F};
    host_pool(F, (size_t)F * k * k * k, [&](int f) {
        bmc_la::Mat At;
        std::vector<double> xty;
        training_stats(fr, f, k, At, xty);
        if (fold_setup(k, F, f, At, xty, fr.dtot.data(), pb, fa)) lower_min(first_bad, f);
    });
    if (first_bad.load() < F)
        return fail(c, BMC_ESINGULAR, "fold " + std::to_string(first_bad.load()) +
                                          ": Singular matrix (X'X of its training rows)");

    // ---- rss at the least-squares point (row g of beta) and at the centre of the expansion (F + g) ----
    if ((rc = cv_rss(c, fr, fa.beta, 2 * F, F, n, count, nu0 * sigma20,
                     [&](int g) { return RssSlot{g, g, F + g, &fa.scal[(size_t)g * 4]}; })))
        return rc;
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
        for (int f = b.f0; f < b.f1; ++f)
            if ((rc = score_fold(c, fr, f, count[f], S, k, (const double*)c->samples.p + (size_t)(f - b.f0) * S * K1,
                                 (double*)dElpd.p)))
                return rc;
        if (draws_out)
            if ((rc = copy_to_host(c, draws_out + (size_t)b.f0 * C * kept * K1, c->samples.p,
                                   nch * kept * K1 * 8, nch * kept * K1 * 8, 1)))
                return rc;
    }
    HIPCHK(c, launch_cv_mean((const double*)fr.dZ.p, fr.ldz, k, (const int32_t*)fr.dRowFold.p,
                             (const double*)dBbar.p, seg.n_pad, (double*)dMean.p, c->stream));
    return cv_scatter(c, fr, 1, n, dElpd, dMean, elpd_out, mean_out);
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
    const std::string bad = cvpath_check(k, comps, m);
    if (!bad.empty()) return fail(c, BMC_EINVAL, bad);
    const int kx = comps[m - 1];   // the widest candidate: the columns of A the device ever reads
    std::vector<int64_t> count;
    int64_t kept = 0;
    int rc;
    if ((rc = cv_check_args(c, n, k, kx, lda, layout, fold, F, C, iters, burn, thin, &count, &kept))) return rc;
    const int64_t T = iters, S = (int64_t)C * kept;
    HIPCHK(c, hipSetDevice(c->device));

    // ---- the prior's part of the basis, per candidate: inv of the LEADING block of C0 ----
    std::vector<PriorBasis> pb(m);
    for (int j = 0; j < m; ++j)
        if (const BasisStatus st = prior_basis(comps[j], C0, k, b0, pb[j]))
            return fail_prior(c, st, std::to_string(comps[j]) + " components: ");

    // ---- rows into fold order and one Gram per fold, once, at the widest candidate ----
    CvFront fr;
    if ((rc = cv_front(c, A, n, k, lda, layout, y, fold, F, kx, fr))) return rc;
    const CvSegments& seg = fr.seg;

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
        const int j = p / F, f = p - j * F;
        bmc_la::Mat At;
        std::vector<double> xty;
        training_stats(fr, f, comps[j], At, xty);
        if (fold_setup(comps[j], F, f, At, xty, fr.dtot.data(), pb[j], fa[j])) lower_min(first_bad, p);
    });
    if (first_bad.load() < P) {
        const int j = first_bad.load() / F, f = first_bad.load() - j * F;
        return fail(c, BMC_ESINGULAR, "fold " + std::to_string(f) + ", " + std::to_string(comps[j]) +
                                          " components: Singular matrix (X'X of its training rows)");
    }

    // ---- rss of every (candidate, fold) at its two points in one launch: coefficients zero-padded
    //      to the gathered width, row b = 2 p (least squares), 2 p + 1 (centre of the expansion) ----
    std::vector<double> beta((size_t)2 * P * kx, 0.0);
    for (int p = 0; p < P; ++p) {
        const int j = p / F, f = p - j * F, kj = comps[j];
        for (int i = 0; i < kj; ++i) {
            beta[(size_t)(2 * p) * kx + i] = fa[j].beta[(size_t)f * kj + i];
            beta[(size_t)(2 * p + 1) * kx + i] = fa[j].beta[((size_t)F + f) * kj + i];
        }
    }
    if ((rc = cv_rss(c, fr, beta, 2 * P, P, n, count, nu0 * sigma20, [&](int p) {
            const int j = p / F, g = p - j * F;
            return RssSlot{g, 2 * p, 2 * p + 1, &fa[j].scal[(size_t)g * 4]};
        })))
        return rc;

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
                if ((rc = score_fold(c, fr, f, count[f], S, kj, (const double*)c->samples.p + b.desc[q].d_off,
                                     (double*)dElpd.p + (size_t)j * npad)))
                    return rc;
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
        HIPCHK(c, launch_cv_mean((const double*)fr.dZ.p, fr.ldz, comps[j], (const int32_t*)fr.dRowFold.p,
                                 (const double*)dBbar.p + voff[j], seg.n_pad, (double*)dMean.p + (size_t)j * npad,
                                 c->stream));
    return cv_scatter(c, fr, m, n, dElpd, dMean, elpd_out, mean_out);
}

int bmc_kfold_cv_t(bmc_ctx* c, const double* A, int64_t n, int32_t k, int64_t lda, int layout,
                   const double* y, const int64_t* fold, int32_t n_folds, const double* b0,
                   const double* C0, double nu0, double sigma20, int32_t n_chains, int64_t iters,
                   int64_t burn, int64_t thin, const uint64_t* seeds, double nu, double* elpd_out,
                   double* mean_out, double* draws_out, double* weight_out) {
    if (!c) return BMC_EINVAL;
    return kfold_cv_t(c, "bmc_kfold_cv_t: ", A, n, k, lda, layout, y, fold, n_folds, b0, C0, nu0, sigma20,
                      n_chains, iters, burn, thin, seeds, nu, nullptr, elpd_out, mean_out, draws_out, weight_out);
}

int bmc_kfold_cv_tv(bmc_ctx* c, const double* A, int64_t n, int32_t k, int64_t lda, int layout,
                    const double* y, const int64_t* fold, int32_t n_folds, const double* b0,
                    const double* C0, double nu0, double sigma20, int32_t n_chains, int64_t iters,
                    int64_t burn, int64_t thin, const uint64_t* seeds, const double* nu_grid,
                    const double* nu_weight, int32_t n_grid, int32_t nu_init, double* elpd_out,
                    double* mean_out, double* draws_out, double* weight_out, int32_t* nu_idx_out) {
    if (!c) return BMC_EINVAL;
    if (n_grid < 1) return fail(c, BMC_EINVAL, "bmc_kfold_cv_tv: " + robust_nu_check(nu_grid, nu_weight, n_grid, nu_init));
    const CvtNu ns{nu_grid, nu_weight, n_grid, nu_init, nu_idx_out};
    return kfold_cv_t(c, "bmc_kfold_cv_tv: ", A, n, k, lda, layout, y, fold, n_folds, b0, C0, nu0, sigma20,
                      n_chains, iters, burn, thin, seeds, 0.0, &ns, elpd_out, mean_out, draws_out, weight_out);
}

}  // extern "C"
