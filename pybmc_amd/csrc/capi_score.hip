// C ABI, scoring a fit: the pointwise log predictive density (kernels_waic.hip),
// PSIS-LOO and its predictive moments (kernels_loo.hip).  The three families
// differ in their plan, their launcher and where their results lie; score_entry is the rest.
// Also the posterior predictive check (kernels_ppc.hip): the same operands and
// checks, results per draw instead of per point (ppc_entry).
#include "bmc_ctx.h"
#include "bmc_math.h"

namespace {

// What every scoring entry point is given: the design rows, the targets and the draws
struct ScoreIn {
    const void *A, *y, *theta;   // host or device
    int64_t n, lda, S, ldt;
    int32_t k, layout;
    double nu = 0.0;   // the likelihood: 0 Gaussian, else Student-t with nu degrees of freedom
    // the _tv entry points (Student-t, a nu per draw; nu stays 0): the distinct values (host) and
    // every draw's index into them (int32; host or device, as A)
    int32_t n_nu = 0;
    const double* nu_values = nullptr;
    const void* nu_index = nullptr;
    NuPerDraw staged;   // what score_nu has made of the three
};

int check_score_args(bmc_ctx* c, const void* A, int64_t n, int32_t k, int64_t lda, int layout,
                     const void* y, const void* theta, int64_t S, int64_t ldt, double nu = 0.0) {
    if (!c) return BMC_EINVAL;
    if (!(nu >= 0.0 && nu < INFINITY))   // (the _t entry points have turned a nu of 0 into NaN)
        return fail(c, BMC_EINVAL, "nu must be positive and finite");
    if (!A || !y || !theta) return fail(c, BMC_EINVAL, "A, y and theta must not be NULL");
    if (n < 1) return fail(c, BMC_EINVAL, "n_points must be >= 1");
    if (k < 1 || k > SCORE_MAX_K)
        return fail(c, BMC_EINVAL, "k must be between 1 and " + std::to_string(SCORE_MAX_K));
    if (layout != BMC_ROW_MAJOR && layout != BMC_COL_MAJOR)
        return fail(c, BMC_EINVAL, "layout must be BMC_ROW_MAJOR or BMC_COL_MAJOR");
    if (lda < (layout == BMC_COL_MAJOR ? n : (int64_t)k))
        return fail(c, BMC_EINVAL, "lda is smaller than the leading dimension of A");
    if (S < 2) return fail(c, BMC_EINVAL, "n_draws must be >= 2 (the variance has ddof 1)");
    if (ldt < (int64_t)k + 1) return fail(c, BMC_EINVAL, "ldt must be >= k + 1");
    return BMC_OK;
}

// The score kernels' arguments in the context's buffers
int score_args(bmc_ctx* c, const ScorePlan& plan, const ScoreIn& in, ScoreArgs& a) {
    const ScoreBuffers sb = score_buffers(plan, in.S);
    if (int rc = ensure_all(c, {{c->scAp, sb.Ap}, {c->scYp, sb.yp}, {c->scCh, sb.ch}, {c->scPart, sb.part},
                                {c->scOut, (size_t)in.n * 3 * 8}}))
        return rc;
    a.A = (const double*)in.A;
    a.y = (const double*)in.y;
    a.theta = (const double*)in.theta;
    a.n = in.n;
    a.lda = in.lda;
    a.S = in.S;
    a.ldt = in.ldt;
    a.k = in.k;
    a.col_major = in.layout == BMC_COL_MAJOR;
    a.nu = in.nu;
    a.per_draw = in.staged;
    a.Ap = (double*)c->scAp.p;
    a.yp = (double*)c->scYp.p;
    a.ch = (double*)c->scCh.p;
    a.part = (double*)c->scPart.p;
    a.out = (double*)c->scOut.p;
    return BMC_OK;
}

// Host A, y and theta into the context's staging buffers (on its stream); `in` then names those
int score_stage(bmc_ctx* c, ScoreIn& in) {
    const size_t abytes = strided_bytes(in.n, in.k, in.lda, in.layout, 8);
    const size_t tbytes = strided_bytes(in.S, in.k + 1, in.ldt, BMC_ROW_MAJOR, 8);
    if (int rc = ensure_all(c, {{c->scA, abytes}, {c->scY, (size_t)in.n * 8}, {c->scTheta, tbytes}}))
        return rc;
    HIPCHK(c, hipMemcpyAsync(c->scA.p, in.A, abytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->scY.p, in.y, (size_t)in.n * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->scTheta.p, in.theta, tbytes, hipMemcpyHostToDevice, c->stream));
    in.A = c->scA.p, in.y = c->scY.p, in.theta = c->scTheta.p;
    return BMC_OK;
}

// The _tv calls: the table of distinct nu (of `shape`), a host index and the zeroed flag word go to
// scNu (stage_nu), and in.staged names them.  BMC_EINVAL for a table entry that is not positive and
// finite, n_values < 1, a NULL pointer or a host index out of range.
int score_nu(bmc_ctx* c, ScoreIn& in, bool on_host, NuTable shape) {
    if (in.n_nu < 1) return fail(c, BMC_EINVAL, "n_values must be >= 1");
    if (!in.nu_values || !in.nu_index) return fail(c, BMC_EINVAL, "nu_values and nu_index must not be NULL");
    for (int32_t v = 0; v < in.n_nu; ++v)
        if (!(in.nu_values[v] > 0.0 && in.nu_values[v] < INFINITY))
            return fail(c, BMC_EINVAL, "nu_values must be positive and finite");
    if (on_host)
        if (int rc = check_nu_index(c, in.nu_index, in.S, in.n_nu)) return rc;
    return stage_nu(c, c->scNu, shape, in.nu_values, in.n_nu, in.S, in.nu_index, on_host, in.staged);
}

// A family plans and launches on device operands and says where result f lies: src[f], [n] each
using ScoreFamily = int (*)(bmc_ctx* c, const ScoreIn& in, const double** src);

// lppd, p_waic, mean_ll
int pointwise_family(bmc_ctx* c, const ScoreIn& in, const double** src) {
    const ScorePlan plan = plan_score(in.n, in.S, in.k, c->n_cu);
    ScoreArgs a;
    if (int rc = score_args(c, plan, in, a)) return rc;
    HIPCHK(c, launch_score(a, plan, c->stream));
    for (int f = 0; f < 3; ++f) src[f] = a.out + (size_t)f * in.n;
    return BMC_OK;
}

// elpd_loo, pareto_k, lppd
int loo_family(bmc_ctx* c, const ScoreIn& in, const double** src) {
    const LooPlan plan = plan_loo(in.n, in.S, in.k, c->n_cu);
    if (!plan.ok)
        return fail(c, BMC_EINVAL, "n_draws is too large for the per-point sort (tail of " +
                                       std::to_string(plan.tail) + " draws)");
    LooArgs a;
    int rc;
    if ((rc = score_args(c, plan.score, in, a.score)) ||
        (rc = ensure(c, c->looWork, loo_buffers(plan, in.n).total())))
        return rc;
    a.work = c->looWork.p;
    HIPCHK(c, launch_loo(a, plan, c->stream));
    const double* lo = loo_out(a, plan);
    src[0] = lo, src[1] = lo + in.n, src[2] = a.score.out;
    return BMC_OK;
}

// elpd_loo, pareto_k, lppd, loo_mean, loo_sd, loo_pit, ess.  Under the t likelihood every nu in the
// call (the scalar, or each entry of the table) must lie in the range of student_t_cdf, and one at
// or below 2 makes loo_sd +inf wherever it is not NaN.
int loo_predict_family(bmc_ctx* c, const ScoreIn& in, const double** src) {
    const bool student = in.nu > 0.0 || in.n_nu > 0;
    bool sd_inf = false;
    for (int32_t v = 0; student && v < (in.n_nu > 0 ? in.n_nu : 1); ++v) {
        const double nu = in.n_nu > 0 ? in.nu_values[v] : in.nu;
        if (!(nu >= STUDENT_T_CDF_NU_MIN && nu <= STUDENT_T_CDF_NU_MAX))
            return fail(c, BMC_EINVAL, "nu must be between 0.06 and 1000 for the leave-one-out predictive "
                                       "distribution (the range of its t distribution function)");
        sd_inf = sd_inf || nu <= 2.0;
    }
    const LooPredictPlan plan = plan_loo_predict(in.n, in.S, in.k, c->n_cu, student);
    if (!plan.ok)
        return fail(c, BMC_EINVAL, "n_draws is too large for the per-point sort of the predictive "
                                   "moments (at most " + std::to_string(LOO_PREDICT_MAX_DRAWS) +
                                       " draws; tail of " + std::to_string(plan.loo.tail) + ")");
    LooArgs a;
    int rc;
    if ((rc = score_args(c, plan.loo.score, in, a.score)) ||
        (rc = ensure(c, c->looWork, loo_predict_buffers(plan, in.n).total())))
        return rc;
    a.work = c->looWork.p;
    a.t_sd_inf = sd_inf;
    HIPCHK(c, launch_loo_predict(a, plan, c->stream));
    const double* lo = loo_predict_out(a, plan);
    src[0] = lo, src[1] = lo + in.n, src[2] = a.score.out;
    for (int f = 3; f < 7; ++f) src[f] = lo + (size_t)(f - 1) * in.n;
    return BMC_OK;
}

// One scoring call: host operands are staged first, the family runs, result f goes to dst[f]
// (host, any may be NULL), then one sync.  Everything on the context's stream, in buffers of its
// own: the resident problem, the prior and the predictive draws are not touched.
int score_entry(bmc_ctx* c, ScoreIn in, bool on_host, ScoreFamily family,
                std::initializer_list<double*> dst) {
    int rc = check_score_args(c, in.A, in.n, in.k, in.lda, in.layout, in.y, in.theta, in.S, in.ldt,
                              in.nu);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (on_host && (rc = score_stage(c, in))) return rc;
    const bool per_draw = in.nu_values || in.nu_index || in.n_nu != 0;
    if (per_draw && (rc = score_nu(c, in, on_host, NU_SCORE))) return rc;
    const double* src[7] = {};
    if ((rc = family(c, in, src))) return rc;
    NuFlagRead flag;
    if ((rc = flag.fetch(c, in.staged))) return rc;
    int f = 0;
    for (double* out : dst) {
        if (out)
            HIPCHK(c, hipMemcpyAsync(out, src[f], (size_t)in.n * 8, hipMemcpyDeviceToHost, c->stream));
        ++f;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return flag.result(c);
}

// One posterior predictive check: host operands are staged first (offset may be NULL: zeros),
// then the plan, the launch, the two result blocks to the host and one sync.  The noise is in.nu
// and in.n_nu as the scoring calls carry the likelihood (a nu per draw: score_nu's table in scNu).
int ppc_entry(bmc_ctx* c, ScoreIn in, const void* offset, bool on_host, uint64_t seed, double center,
              double* t_rep_out, double* t_obs2_out) {
    int rc = check_score_args(c, in.A, in.n, in.k, in.lda, in.layout, in.y, in.theta, in.S, in.ldt,
                              in.nu);
    if (rc) return rc;
    const bool per_draw = in.nu_values || in.nu_index || in.n_nu != 0;
    if (per_draw && in.n_nu > PPC_MAX_NU_VALUES)
        return fail(c, BMC_EINVAL, "n_values must be at most " + std::to_string(PPC_MAX_NU_VALUES));
    const PpcPlan plan = plan_ppc(in.n, in.S, in.k, c->n_cu);
    if (!plan.ok)
        return fail(c, BMC_EINVAL, "n_points must be between " + std::to_string(PPC_MIN_POINTS) + " and " +
                                       std::to_string(PPC_MAX_POINTS) + " for a posterior predictive check");
    HIPCHK(c, hipSetDevice(c->device));
    if (on_host) {
        if ((rc = score_stage(c, in))) return rc;
        if (offset) {
            if ((rc = ensure(c, c->ppcOff, (size_t)in.n * 8))) return rc;
            HIPCHK(c, hipMemcpyAsync(c->ppcOff.p, offset, (size_t)in.n * 8, hipMemcpyHostToDevice, c->stream));
            offset = c->ppcOff.p;
        }
    }
    if (per_draw && (rc = score_nu(c, in, on_host, NU_PPC))) return rc;
    const PpcBuffers pb = ppc_buffers(plan, in.S);
    if ((rc = ensure(c, c->ppcWork, pb.total() + (per_draw ? ppc_nu_bytes(plan) : 0)))) return rc;
    char* w = (char*)c->ppcWork.p;
    PpcArgs a;
    a.A = (const double*)in.A;
    a.y = (const double*)in.y;
    a.offset = (const double*)offset;
    a.theta = (const double*)in.theta;
    a.n = in.n;
    a.lda = in.lda;
    a.S = in.S;
    a.ldt = in.ldt;
    a.k = in.k;
    a.col_major = in.layout == BMC_COL_MAJOR;
    a.seed = seed;
    a.center = center;
    a.Ap = (double*)w;
    a.yo = (double*)(w += pb.Ap);
    a.Tp = (double*)(w += pb.yo);
    a.sg = (double*)(w += pb.Tp);
    a.t_rep = (double*)(w += pb.sg);
    a.t_obs2 = a.t_rep + (size_t)in.S * PPC_STATS;
    a.nu = in.nu;
    a.per_draw = in.staged;
    if (per_draw) a.nus = (double*)(w + pb.out);
    HIPCHK(c, launch_ppc(a, plan, c->stream));
    NuFlagRead flag;
    if ((rc = flag.fetch(c, in.staged))) return rc;
    if (t_rep_out)
        HIPCHK(c, hipMemcpyAsync(t_rep_out, a.t_rep, (size_t)in.S * PPC_STATS * 8, hipMemcpyDeviceToHost,
                                 c->stream));
    if (t_obs2_out)
        HIPCHK(c, hipMemcpyAsync(t_obs2_out, a.t_obs2, (size_t)in.S * PPC_OBS * 8, hipMemcpyDeviceToHost,
                                 c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return flag.result(c);
}

// nu of a _t entry point as ScoreIn carries it: what is not positive (0 would mean Gaussian there)
// becomes NaN, which check_score_args refuses
double t_nu(double nu) { return nu > 0.0 ? nu : NAN; }

// n_values of a bmc_ppc_tv entry point as ScoreIn carries it: 0 there would mean "no nu per draw"
// when both pointers are NULL too, so what is not positive becomes -1, which score_nu refuses
int32_t tv_count(int32_t n_values) { return n_values > 0 ? n_values : -1; }

}  // namespace

extern "C" {

int bmc_pointwise_loglik(bmc_ctx* c, const double* A, int64_t n_points, int32_t k, int64_t lda,
                         int layout, const double* y, const double* theta, int64_t n_draws,
                         int64_t ldt, double* lppd_out, double* pwaic_out, double* mean_ll_out) {
    return score_entry(c, {A, y, theta, n_points, lda, n_draws, ldt, k, layout}, true, pointwise_family,
                       {lppd_out, pwaic_out, mean_ll_out});
}

int bmc_pointwise_loglik_device(bmc_ctx* c, const void* dA, int64_t n_points, int32_t k, int64_t lda,
                                int layout, const void* dy, const void* dtheta, int64_t n_draws,
                                int64_t ldt, double* lppd_out, double* pwaic_out,
                                double* mean_ll_out) {
    return score_entry(c, {dA, dy, dtheta, n_points, lda, n_draws, ldt, k, layout}, false,
                       pointwise_family, {lppd_out, pwaic_out, mean_ll_out});
}

int bmc_psis_loo(bmc_ctx* c, const double* A, int64_t n_points, int32_t k, int64_t lda, int layout,
                 const double* y, const double* theta, int64_t n_draws, int64_t ldt,
                 double* elpd_loo_out, double* pareto_k_out, double* lppd_out) {
    return score_entry(c, {A, y, theta, n_points, lda, n_draws, ldt, k, layout}, true, loo_family,
                       {elpd_loo_out, pareto_k_out, lppd_out});
}

int bmc_psis_loo_device(bmc_ctx* c, const void* dA, int64_t n_points, int32_t k, int64_t lda,
                        int layout, const void* dy, const void* dtheta, int64_t n_draws, int64_t ldt,
                        double* elpd_loo_out, double* pareto_k_out, double* lppd_out) {
    return score_entry(c, {dA, dy, dtheta, n_points, lda, n_draws, ldt, k, layout}, false, loo_family,
                       {elpd_loo_out, pareto_k_out, lppd_out});
}

int bmc_pointwise_loglik_t(bmc_ctx* c, const double* A, int64_t n_points, int32_t k, int64_t lda,
                           int layout, const double* y, const double* theta, int64_t n_draws,
                           int64_t ldt, double nu, double* lppd_out, double* pwaic_out,
                           double* mean_ll_out) {
    return score_entry(c, {A, y, theta, n_points, lda, n_draws, ldt, k, layout, t_nu(nu)}, true,
                       pointwise_family, {lppd_out, pwaic_out, mean_ll_out});
}

int bmc_pointwise_loglik_t_device(bmc_ctx* c, const void* dA, int64_t n_points, int32_t k, int64_t lda,
                                  int layout, const void* dy, const void* dtheta, int64_t n_draws,
                                  int64_t ldt, double nu, double* lppd_out, double* pwaic_out,
                                  double* mean_ll_out) {
    return score_entry(c, {dA, dy, dtheta, n_points, lda, n_draws, ldt, k, layout, t_nu(nu)}, false,
                       pointwise_family, {lppd_out, pwaic_out, mean_ll_out});
}

int bmc_psis_loo_t(bmc_ctx* c, const double* A, int64_t n_points, int32_t k, int64_t lda, int layout,
                   const double* y, const double* theta, int64_t n_draws, int64_t ldt, double nu,
                   double* elpd_loo_out, double* pareto_k_out, double* lppd_out) {
    return score_entry(c, {A, y, theta, n_points, lda, n_draws, ldt, k, layout, t_nu(nu)}, true,
                       loo_family, {elpd_loo_out, pareto_k_out, lppd_out});
}

int bmc_psis_loo_t_device(bmc_ctx* c, const void* dA, int64_t n_points, int32_t k, int64_t lda,
                          int layout, const void* dy, const void* dtheta, int64_t n_draws, int64_t ldt,
                          double nu, double* elpd_loo_out, double* pareto_k_out, double* lppd_out) {
    return score_entry(c, {dA, dy, dtheta, n_points, lda, n_draws, ldt, k, layout, t_nu(nu)}, false,
                       loo_family, {elpd_loo_out, pareto_k_out, lppd_out});
}

int bmc_pointwise_loglik_tv(bmc_ctx* c, const double* A, int64_t n_points, int32_t k, int64_t lda,
                            int layout, const double* y, const double* theta, int64_t n_draws,
                            int64_t ldt, const double* nu_values, int32_t n_values,
                            const int32_t* nu_index, double* lppd_out, double* pwaic_out,
                            double* mean_ll_out) {
    return score_entry(c, {A, y, theta, n_points, lda, n_draws, ldt, k, layout, 0.0, n_values, nu_values,
                           nu_index}, true, pointwise_family, {lppd_out, pwaic_out, mean_ll_out});
}

int bmc_pointwise_loglik_tv_device(bmc_ctx* c, const void* dA, int64_t n_points, int32_t k, int64_t lda,
                                   int layout, const void* dy, const void* dtheta, int64_t n_draws,
                                   int64_t ldt, const double* nu_values, int32_t n_values,
                                   const void* d_nu_index, double* lppd_out, double* pwaic_out,
                                   double* mean_ll_out) {
    return score_entry(c, {dA, dy, dtheta, n_points, lda, n_draws, ldt, k, layout, 0.0, n_values,
                           nu_values, d_nu_index}, false, pointwise_family,
                       {lppd_out, pwaic_out, mean_ll_out});
}

int bmc_psis_loo_tv(bmc_ctx* c, const double* A, int64_t n_points, int32_t k, int64_t lda, int layout,
                    const double* y, const double* theta, int64_t n_draws, int64_t ldt,
                    const double* nu_values, int32_t n_values, const int32_t* nu_index,
                    double* elpd_loo_out, double* pareto_k_out, double* lppd_out) {
    return score_entry(c, {A, y, theta, n_points, lda, n_draws, ldt, k, layout, 0.0, n_values, nu_values,
                           nu_index}, true, loo_family, {elpd_loo_out, pareto_k_out, lppd_out});
}

int bmc_psis_loo_tv_device(bmc_ctx* c, const void* dA, int64_t n_points, int32_t k, int64_t lda,
                           int layout, const void* dy, const void* dtheta, int64_t n_draws, int64_t ldt,
                           const double* nu_values, int32_t n_values, const void* d_nu_index,
                           double* elpd_loo_out, double* pareto_k_out, double* lppd_out) {
    return score_entry(c, {dA, dy, dtheta, n_points, lda, n_draws, ldt, k, layout, 0.0, n_values,
                           nu_values, d_nu_index}, false, loo_family,
                       {elpd_loo_out, pareto_k_out, lppd_out});
}

int bmc_psis_loo_predict(bmc_ctx* c, const double* A, int64_t n_points, int32_t k, int64_t lda,
                         int layout, const double* y, const double* theta, int64_t n_draws,
                         int64_t ldt, double* elpd_loo_out, double* pareto_k_out, double* lppd_out,
                         double* loo_mean_out, double* loo_sd_out, double* loo_pit_out,
                         double* ess_out) {
    return score_entry(c, {A, y, theta, n_points, lda, n_draws, ldt, k, layout}, true, loo_predict_family,
                       {elpd_loo_out, pareto_k_out, lppd_out, loo_mean_out, loo_sd_out, loo_pit_out,
                        ess_out});
}

int bmc_psis_loo_predict_device(bmc_ctx* c, const void* dA, int64_t n_points, int32_t k, int64_t lda,
                                int layout, const void* dy, const void* dtheta, int64_t n_draws,
                                int64_t ldt, double* elpd_loo_out, double* pareto_k_out,
                                double* lppd_out, double* loo_mean_out, double* loo_sd_out,
                                double* loo_pit_out, double* ess_out) {
    return score_entry(c, {dA, dy, dtheta, n_points, lda, n_draws, ldt, k, layout}, false,
                       loo_predict_family, {elpd_loo_out, pareto_k_out, lppd_out, loo_mean_out,
                                            loo_sd_out, loo_pit_out, ess_out});
}

int bmc_psis_loo_predict_t(bmc_ctx* c, const double* A, int64_t n_points, int32_t k, int64_t lda,
                           int layout, const double* y, const double* theta, int64_t n_draws,
                           int64_t ldt, double nu, double* elpd_loo_out, double* pareto_k_out,
                           double* lppd_out, double* loo_mean_out, double* loo_sd_out,
                           double* loo_pit_out, double* ess_out) {
    return score_entry(c, {A, y, theta, n_points, lda, n_draws, ldt, k, layout, t_nu(nu)}, true,
                       loo_predict_family, {elpd_loo_out, pareto_k_out, lppd_out, loo_mean_out,
                                            loo_sd_out, loo_pit_out, ess_out});
}

int bmc_psis_loo_predict_t_device(bmc_ctx* c, const void* dA, int64_t n_points, int32_t k, int64_t lda,
                                  int layout, const void* dy, const void* dtheta, int64_t n_draws,
                                  int64_t ldt, double nu, double* elpd_loo_out, double* pareto_k_out,
                                  double* lppd_out, double* loo_mean_out, double* loo_sd_out,
                                  double* loo_pit_out, double* ess_out) {
    return score_entry(c, {dA, dy, dtheta, n_points, lda, n_draws, ldt, k, layout, t_nu(nu)}, false,
                       loo_predict_family, {elpd_loo_out, pareto_k_out, lppd_out, loo_mean_out,
                                            loo_sd_out, loo_pit_out, ess_out});
}

int bmc_psis_loo_predict_tv(bmc_ctx* c, const double* A, int64_t n_points, int32_t k, int64_t lda,
                            int layout, const double* y, const double* theta, int64_t n_draws,
                            int64_t ldt, const double* nu_values, int32_t n_values,
                            const int32_t* nu_index, double* elpd_loo_out, double* pareto_k_out,
                            double* lppd_out, double* loo_mean_out, double* loo_sd_out,
                            double* loo_pit_out, double* ess_out) {
    return score_entry(c, {A, y, theta, n_points, lda, n_draws, ldt, k, layout, 0.0, tv_count(n_values),
                           nu_values, nu_index}, true, loo_predict_family,
                       {elpd_loo_out, pareto_k_out, lppd_out, loo_mean_out, loo_sd_out, loo_pit_out,
                        ess_out});
}

int bmc_psis_loo_predict_tv_device(bmc_ctx* c, const void* dA, int64_t n_points, int32_t k, int64_t lda,
                                   int layout, const void* dy, const void* dtheta, int64_t n_draws,
                                   int64_t ldt, const double* nu_values, int32_t n_values,
                                   const void* d_nu_index, double* elpd_loo_out, double* pareto_k_out,
                                   double* lppd_out, double* loo_mean_out, double* loo_sd_out,
                                   double* loo_pit_out, double* ess_out) {
    return score_entry(c, {dA, dy, dtheta, n_points, lda, n_draws, ldt, k, layout, 0.0,
                           tv_count(n_values), nu_values, d_nu_index}, false, loo_predict_family,
                       {elpd_loo_out, pareto_k_out, lppd_out, loo_mean_out, loo_sd_out, loo_pit_out,
                        ess_out});
}

int bmc_ppc(bmc_ctx* c, const double* A, int64_t n_points, int32_t k, int64_t lda, int layout,
            const double* y, const double* offset, const double* theta, int64_t n_draws, int64_t ldt,
            uint64_t seed, double center, double* t_rep_out, double* t_obs2_out) {
    return ppc_entry(c, {A, y, theta, n_points, lda, n_draws, ldt, k, layout}, offset, true, seed, center,
                     t_rep_out, t_obs2_out);
}

int bmc_ppc_device(bmc_ctx* c, const void* dA, int64_t n_points, int32_t k, int64_t lda, int layout,
                   const void* dy, const void* doffset, const void* dtheta, int64_t n_draws, int64_t ldt,
                   uint64_t seed, double center, double* t_rep_out, double* t_obs2_out) {
    return ppc_entry(c, {dA, dy, dtheta, n_points, lda, n_draws, ldt, k, layout}, doffset, false, seed,
                     center, t_rep_out, t_obs2_out);
}

int bmc_ppc_t(bmc_ctx* c, const double* A, int64_t n_points, int32_t k, int64_t lda, int layout,
              const double* y, const double* offset, const double* theta, int64_t n_draws, int64_t ldt,
              uint64_t seed, double nu, double* t_rep_out, double* t_obs2_out) {
    return ppc_entry(c, {A, y, theta, n_points, lda, n_draws, ldt, k, layout, t_nu(nu)}, offset, true, seed,
                     0.0, t_rep_out, t_obs2_out);
}

int bmc_ppc_t_device(bmc_ctx* c, const void* dA, int64_t n_points, int32_t k, int64_t lda, int layout,
                     const void* dy, const void* doffset, const void* dtheta, int64_t n_draws,
                     int64_t ldt, uint64_t seed, double nu, double* t_rep_out, double* t_obs2_out) {
    return ppc_entry(c, {dA, dy, dtheta, n_points, lda, n_draws, ldt, k, layout, t_nu(nu)}, doffset, false,
                     seed, 0.0, t_rep_out, t_obs2_out);
}

int bmc_ppc_tv(bmc_ctx* c, const double* A, int64_t n_points, int32_t k, int64_t lda, int layout,
               const double* y, const double* offset, const double* theta, int64_t n_draws, int64_t ldt,
               uint64_t seed, const double* nu_values, int32_t n_values, const int32_t* nu_index,
               double* t_rep_out, double* t_obs2_out) {
    return ppc_entry(c, {A, y, theta, n_points, lda, n_draws, ldt, k, layout, 0.0, tv_count(n_values),
                         nu_values, nu_index}, offset, true, seed, 0.0, t_rep_out, t_obs2_out);
}

int bmc_ppc_tv_device(bmc_ctx* c, const void* dA, int64_t n_points, int32_t k, int64_t lda, int layout,
                      const void* dy, const void* doffset, const void* dtheta, int64_t n_draws,
                      int64_t ldt, uint64_t seed, const double* nu_values, int32_t n_values,
                      const void* d_nu_index, double* t_rep_out, double* t_obs2_out) {
    return ppc_entry(c, {dA, dy, dtheta, n_points, lda, n_draws, ldt, k, layout, 0.0,
                         tv_count(n_values), nu_values, d_nu_index}, doffset, false, seed, 0.0, t_rep_out,
                     t_obs2_out);
}

}  // extern "C"
