// C ABI, power-scaling sensitivity of a sampled fit to its prior and its likelihood (Kallioinen,
// Paananen, Buerkner & Vehtari 2023).  The log densities, the
// Pareto-smoothed weights and the distances are made on the device (kernels_sens.hip); every
// vector is sorted once, by the passes of the rank diagnostics (kernels_rank.hip).  The Student-t
// forms (_t, _tv) are the same driver with the likelihood as data in SensIn.
#include <algorithm>
#include <cmath>

#include "bmc_ctx.h"
#include "host_linalg.hpp"

namespace {

struct SensEvents {
    hipEvent_t e[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    ~SensEvents() {
        for (auto& x : e)
            if (x) (void)hipEventDestroy(x);
    }
};

struct SensIn {
    const void *A, *y, *theta;   // host or device
    int64_t n, lda, S, ldt;
    int32_t k, layout;
    const double *b0, *C0, *Vt, *alphas;   // host
    double nu0, sigma20;
    int32_t n_models, n_alphas, cols_per_batch;
    uint32_t components;
    // the likelihood as data: Gaussian, or (student) Student-t with nu_values[nu_index[s]] degrees of
    // freedom for draw s; per_draw false: nu_values[0] for every draw and no index (the _t entry
    // points).  nu_values and nu_log_prior (NULL: no prior of nu) are host, nu_index int32 where A is
    bool student = false, per_draw = false;
    int32_t n_nu = 0;
    const double* nu_values = nullptr;
    const void* nu_index = nullptr;
    const double* nu_log_prior = nullptr;
};

struct SensOut {
    double *logdens, *pareto_k, *mean, *sd, *cjs, *weights;
    uint32_t* flags;
};

// the sort buffers of a batch of Pb segments, in the rank diagnostics' buffers
struct SensBatch {
    RankShape sh;
    uint64_t* key[2];
    uint32_t* idx[2];
    uint32_t* hist;
    uint64_t* or_and;
    uint32_t* flags;
};

int sens_buffers(bmc_ctx* c, SensPlan p, int32_t Pb, SensBatch& b) {
    sens_scratch(p, Pb);
    int rc = ensure_all(c, {{c->rkKey[0], p.bytes_keys}, {c->rkKey[1], p.bytes_keys},
                            {c->rkIdx[0], p.bytes_idx}, {c->rkIdx[1], p.bytes_idx},
                            {c->rkHist, p.bytes_hist}, {c->rkSmall, p.bytes_small},
                            {c->snPart, p.bytes_part + p.bytes_offs}});
    if (rc) return rc;
    b.sh = RankShape{};
    b.sh.x = nullptr;
    b.sh.iters = p.S_pad;
    b.sh.ld = 1;
    b.sh.burn = 0;
    b.sh.n = p.S_pad / 2;
    b.sh.half_off = p.S_pad / 2;
    b.sh.S = p.S_pad;
    b.sh.tiles = p.tiles;
    b.sh.C = 1;
    b.sh.col0 = 0;
    b.sh.Pb = Pb;
    for (int i = 0; i < 2; ++i) {
        b.key[i] = (uint64_t*)c->rkKey[i].p;
        b.idx[i] = (uint32_t*)c->rkIdx[i].p;
    }
    b.hist = (uint32_t*)c->rkHist.p;
    b.or_and = (uint64_t*)c->rkSmall.p;
    b.flags = (uint32_t*)(b.or_and + (size_t)Pb * 2);
    return BMC_OK;
}

// gather Pb columns of src from col0 and sort them; `cur` is the buffer that holds the sorted
// pairs, flags[jb] != 0: the column holds a non-finite value
int sens_sort(bmc_ctx* c, const SensSource& src, int64_t S, int32_t col0, const SensBatch& b, int& cur,
              std::vector<uint32_t>& flags) {
    const int32_t Pb = b.sh.Pb;
    cur = 0;
    HIPCHK(c, launch_sens_gather(src, S, col0, Pb, b.key[0], b.idx[0], b.or_and, b.flags, c->stream));
    std::vector<uint64_t> oa((size_t)Pb * 2);
    flags.resize(Pb);
    HIPCHK(c, hipMemcpyAsync(oa.data(), b.or_and, oa.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(flags.data(), b.flags, flags.size() * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint32_t live = rank_live_passes(oa.data(), Pb);
    for (int d = 0; d < RANK_PASSES; ++d) {
        if (!((live >> d) & 1)) continue;
        HIPCHK(c, launch_rank_sort_pass(b.sh, d, b.key[cur], b.idx[cur], b.key[cur ^ 1], b.idx[cur ^ 1],
                                        b.hist, c->stream));
        cur ^= 1;
    }
    return BMC_OK;
}

inline size_t up256(size_t bytes) { return (bytes + 255) / 256 * 256; }

int sens_run(bmc_ctx* c, const SensIn& in, const SensOut& out) {
    const int32_t k = in.k, Mm = in.n_models, nA = in.n_alphas;
    const int64_t S = in.S;
    const bool student = in.student;
    const int32_t n_comp = student ? sens_t_count_components(in.components) : sens_count_components(in.components);
    const int32_t W = n_comp * nA, Qn = k + 1 + Mm + (in.per_draw ? 1 : 0);
    const int32_t lp_rows = student ? SENS_T_LOGDENS : SENS_LOGDENS;
    const double nan = std::nan("");

    // C0 = L L' on the host; the quadratic form is |L^-1 beta - L^-1 b0|^2
    bmc_la::Mat C0((size_t)k * k), L, Li;
    for (size_t i = 0; i < C0.size(); ++i) {
        C0[i] = in.C0[i];
        if (!std::isfinite(C0[i])) return fail(c, BMC_ESINGULAR, "Singular matrix (b_mean_cov)");
    }
    if (!bmc_la::cholesky(C0, k, L)) return fail(c, BMC_ESINGULAR, "Singular matrix (b_mean_cov)");
    bmc_la::lower_inverse(L, k, Li);
    for (double v : Li)
        if (!std::isfinite(v)) return fail(c, BMC_ESINGULAR, "Singular matrix (b_mean_cov)");

    const int64_t n_pad = (in.n + SENS_TILE - 1) / SENS_TILE * SENS_TILE;
    const int64_t q_pad = ((int64_t)k + SENS_TILE - 1) / SENS_TILE * SENS_TILE;
    const int64_t S64 = (S + SENS_TILE - 1) / SENS_TILE * SENS_TILE;
    const int32_t k_pad = (k + 15) / 16 * 16;
    const int64_t M = psis_tail_length(S);

    // small host operands in one block: Lp [q_pad][k_pad], Ly [q_pad], Vt [k][Mm], alphas [nA] and, for
    // the Student-t likelihood, the table of nu [3][V]: C(nu), nu, its log prior (zeros without one)
    const size_t n_lp = (size_t)q_pad * k_pad, n_vt = (size_t)k * Mm, V = (size_t)in.n_nu;
    const size_t h_tab = n_lp + q_pad + n_vt + nA;
    std::vector<double> host(h_tab + 3 * V, 0.0);
    nu_table(NU_SENS, in.nu_values, in.nu_log_prior, V, host.data() + h_tab);
    for (int32_t i = 0; i < k; ++i) {
        long double s = 0.0L;
        for (int32_t j = 0; j <= i; ++j) {
            host[(size_t)i * k_pad + j] = Li[(size_t)i * k + j];
            s += (long double)Li[(size_t)i * k + j] * in.b0[j];
        }
        host[n_lp + i] = (double)s;
    }
    for (size_t i = 0; i < n_vt; ++i) host[n_lp + q_pad + i] = in.Vt[i];
    for (int32_t i = 0; i < nA; ++i) host[n_lp + q_pad + n_vt + i] = in.alphas[i];

    // the work block
    size_t at = 0;
    auto take = [&](size_t doubles) {
        const size_t o = at;
        at += up256(doubles * 8);
        return o;
    };
    const size_t o_host = take(host.size()), o_Ap = take((size_t)n_pad * k_pad), o_yo = take(n_pad),
                 o_Tp = take((size_t)S64 * k_pad), o_rss = take(2 * (size_t)S), o_lp = take(lp_rows * (size_t)S),
                 o_comps = take((size_t)n_comp * S), o_omega = take((size_t)S * Mm),
                 o_Wt = take((size_t)S * W), o_xs = take((size_t)W * (M > 0 ? M : 1)), o_khat = take(W),
                 o_tc = take(student ? SENS_T_STAGED * (size_t)S : 0),
                 o_flag = take(student ? 1 : 0);   // one int32 word: an index was out of range
    const size_t fixed = at;

    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return fail(c, BMC_EHIP, "hipMemGetInfo failed");
    const size_t held = c->rkKey[0].cap + c->rkKey[1].cap + c->rkIdx[0].cap + c->rkIdx[1].cap + c->rkHist.cap +
                        c->rkSmall.cap + c->snPart.cap + c->snWork.cap;
    const size_t avail = (size_t)((double)(free_b + held) * 0.8);
    if (avail <= fixed)
        return fail(c, BMC_ENOMEM, "the log densities and weights need " + std::to_string(fixed) +
                                       " bytes of device memory; " + std::to_string(avail) + " are free");
    const SensPlan p = student ? plan_sens_t(S, Qn, W, in.cols_per_batch, avail - fixed)
                               : plan_sens(S, Qn, W, in.cols_per_batch, avail - fixed);
    if (!p.ok) return fail(c, p.S == 0 ? BMC_EINVAL : BMC_ENOMEM, p.why);
    const int32_t Pb_max = std::max(p.cols_per_batch, n_comp);
    const size_t o_out = take((size_t)Pb_max * W * 3);
    int rc;
    if ((rc = ensure(c, c->snWork, at))) return rc;
    char* w = (char*)c->snWork.p;
    auto dptr = [&](size_t o) { return (double*)(w + o); };

    SensEvents ev;
    for (auto& e : ev.e) HIPCHK(c, hipEventCreate(&e));
    for (double& m : c->sens_ms) m = 0;
    float ms = 0;

    // ---- log densities ------------------------------------------------------------------------
    HIPCHK(c, hipEventRecord(ev.e[0], c->stream));
    HIPCHK(c, hipMemcpyAsync(dptr(o_host), host.data(), host.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_pad_points((const double*)in.A, (const double*)in.y, nullptr, false, in.n, k, in.lda,
                                in.layout == BMC_COL_MAJOR, n_pad, k_pad, dptr(o_Ap), dptr(o_yo), c->stream));
    SensLogdensArgs la;
    la.theta = (const double*)in.theta;
    la.Ap = dptr(o_Ap);
    la.yo = dptr(o_yo);
    la.Lp = dptr(o_host);
    la.Ly = dptr(o_host) + n_lp;
    la.Vt = dptr(o_host) + n_lp + q_pad;
    la.S = S;
    la.S_pad = S64;
    la.ldt = in.ldt;
    la.n = in.n;
    la.n_pad = n_pad;
    la.q_pad = q_pad;
    la.k = k;
    la.k_pad = k_pad;
    la.n_models = Mm;
    la.components = in.components;
    la.nu0 = in.nu0;
    la.sigma20 = in.sigma20;
    la.Tp = dptr(o_Tp);
    la.rss = dptr(o_rss);
    la.lp = dptr(o_lp);
    la.comps = dptr(o_comps);
    la.omega = dptr(o_omega);
    if (student) {   // the NuPerDraw in this call's own work block
        la.per_draw.n_nu = in.n_nu;
        la.per_draw.tab = dptr(o_host) + h_tab;
        la.per_draw.index = in.per_draw ? (const int32_t*)in.nu_index : nullptr;
        la.per_draw.flag = (int32_t*)dptr(o_flag);
        HIPCHK(c, hipMemsetAsync(la.per_draw.flag, 0, 4, c->stream));
        la.tc = dptr(o_tc);
    }
    HIPCHK(c, launch_sens_logdens(la, c->stream));
    HIPCHK(c, hipEventRecord(ev.e[1], c->stream));

    // ---- one sort per component vector, then the weights of every (component, alpha) -------------
    SensBatch b;
    std::vector<uint32_t> comp_flags, col_flags;
    int cur = 0;
    if ((rc = sens_buffers(c, p, n_comp, b))) return rc;
    const SensSource comp_src{nullptr, dptr(o_comps), 0, 1, S, 0};
    if ((rc = sens_sort(c, comp_src, S, 0, b, cur, comp_flags))) return rc;
    HIPCHK(c, hipEventRecord(ev.e[2], c->stream));
    const double* d_alphas = dptr(o_host) + n_lp + q_pad + n_vt;
    HIPCHK(c, launch_sens_psis(b.key[cur], b.idx[cur], S, n_comp, nA, d_alphas, dptr(o_xs), dptr(o_Wt),
                               dptr(o_khat), c->stream));
    HIPCHK(c, hipEventRecord(ev.e[3], c->stream));
    std::vector<double> khat(W);
    HIPCHK(c, hipMemcpyAsync(khat.data(), dptr(o_khat), (size_t)W * 8, hipMemcpyDeviceToHost, c->stream));
    NuFlagRead flag;
    if ((rc = flag.fetch(c, la.per_draw))) return rc;
    if (out.logdens)
        HIPCHK(c, hipMemcpyAsync(out.logdens, dptr(o_lp), (size_t)lp_rows * S * 8, hipMemcpyDeviceToHost,
                                 c->stream));
    if (out.weights)
        HIPCHK(c, hipMemcpyAsync(out.weights, dptr(o_Wt), (size_t)S * W * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if ((rc = flag.result(c))) return rc;
    const int span0[3] = {0, 1, 2};
    for (int i = 0; i < 3; ++i) {
        HIPCHK(c, hipEventElapsedTime(&ms, ev.e[i], ev.e[i + 1]));
        c->sens_ms[span0[i]] += ms;
    }
    for (int32_t ci = 0; ci < n_comp; ++ci) {
        const bool bad = comp_flags[ci] != 0;
        if (out.flags) out.flags[ci] = bad ? 1u : 0u;
        for (int32_t a = 0; a < nA; ++a) {
            if (out.pareto_k) out.pareto_k[ci * nA + a] = bad ? nan : khat[ci * nA + a];
            if (bad && out.weights)
                for (int64_t s = 0; s < S; ++s) out.weights[(size_t)s * W + ci * nA + a] = nan;
        }
    }

    // ---- the quantity columns, batch by batch -------------------------------------------------------
    SensSource col_src{(const double*)in.theta, dptr(o_omega), in.ldt, (int64_t)Mm, 1, k + 1};
    if (in.per_draw) {   // the nu of every draw, staged for the pass: the last column
        col_src.p2 = dptr(o_tc) + 3 * (size_t)S;
        col_src.n1 = k + 1 + Mm;
    }
    std::vector<double> res;
    for (int32_t bi = 0; bi < p.n_batches; ++bi) {
        int32_t col0, Pb;
        sens_batch(p, Qn, bi, &col0, &Pb);
        if ((rc = sens_buffers(c, p, Pb, b))) return rc;
        HIPCHK(c, hipEventRecord(ev.e[4], c->stream));
        if ((rc = sens_sort(c, col_src, S, col0, b, cur, col_flags))) return rc;
        HIPCHK(c, hipEventRecord(ev.e[5], c->stream));
        double* offs = (double*)c->snPart.p;
        double* part = offs + (size_t)Pb * W * p.chunks;
        HIPCHK(c, launch_sens_cjs(b.key[cur], b.idx[cur], S, Pb, W, dptr(o_Wt), offs, part, dptr(o_out),
                                  c->stream));
        HIPCHK(c, hipEventRecord(ev.e[6], c->stream));
        res.resize((size_t)Pb * W * 3);
        HIPCHK(c, hipMemcpyAsync(res.data(), dptr(o_out), res.size() * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipEventElapsedTime(&ms, ev.e[4], ev.e[5]));
        c->sens_ms[1] += ms;
        HIPCHK(c, hipEventElapsedTime(&ms, ev.e[5], ev.e[6]));
        c->sens_ms[3] += ms;
        for (int32_t jb = 0; jb < Pb; ++jb) {
            const int32_t j = col0 + jb;
            if (out.flags) out.flags[n_comp + j] = col_flags[jb] ? 1u : 0u;
            for (int32_t wi = 0; wi < W; ++wi) {
                const bool bad = col_flags[jb] != 0 || comp_flags[wi / nA] != 0;
                const double* r = res.data() + ((size_t)jb * W + wi) * 3;
                if (out.cjs) out.cjs[(size_t)wi * Qn + j] = bad ? nan : r[0];
                if (out.mean) out.mean[(size_t)wi * Qn + j] = bad ? nan : r[1];
                if (out.sd) out.sd[(size_t)wi * Qn + j] = bad ? nan : r[2];
            }
        }
    }
    return BMC_OK;
}

int sens_entry(bmc_ctx* c, SensIn in, bool on_host, const SensOut& out) {
    if (!c) return BMC_EINVAL;
    if (!in.A || !in.y || !in.theta) return fail(c, BMC_EINVAL, "A, y and theta must not be NULL");
    if (!in.b0 || !in.C0) return fail(c, BMC_EINVAL, "b0 and C0 must not be NULL");
    if (in.n_models > 0 && !in.Vt) return fail(c, BMC_EINVAL, "Vt must not be NULL when n_models > 0");
    const std::string why =
        in.student ? sens_t_check(in.n, in.k, in.S, in.n_models, in.alphas, in.n_alphas, in.components,
                                  in.per_draw, in.nu_values, in.n_nu, in.nu_log_prior)
                   : sens_check(in.n, in.k, in.S, in.n_models, in.alphas, in.n_alphas, in.components);
    if (!why.empty()) return fail(c, BMC_EINVAL, why);
    if (in.per_draw && !in.nu_index) return fail(c, BMC_EINVAL, "nu_values and nu_index must not be NULL");
    if (in.per_draw && on_host)   // a host index is checked before any launch
        if (int rc = check_nu_index(c, in.nu_index, in.S, in.n_nu)) return rc;
    if (in.layout != BMC_ROW_MAJOR && in.layout != BMC_COL_MAJOR)
        return fail(c, BMC_EINVAL, "layout must be BMC_ROW_MAJOR or BMC_COL_MAJOR");
    if (in.lda < (in.layout == BMC_COL_MAJOR ? in.n : (int64_t)in.k))
        return fail(c, BMC_EINVAL, "lda is smaller than the leading dimension of A");
    if (in.ldt < (int64_t)in.k + 1) return fail(c, BMC_EINVAL, "ldt must be >= k + 1");
    if (in.cols_per_batch < 0) return fail(c, BMC_EINVAL, "cols_per_batch must be >= 0");
    if (!(in.nu0 >= 0.0) || !(in.sigma20 >= 0.0) || !std::isfinite(in.nu0) || !std::isfinite(in.sigma20))
        return fail(c, BMC_EINVAL, "nu0 and sigma20 must be finite and >= 0");
    HIPCHK(c, hipSetDevice(c->device));
    if (on_host) {
        const size_t abytes = up256(strided_bytes(in.n, in.k, in.lda, in.layout, 8));
        const size_t ybytes = up256((size_t)in.n * 8);
        const size_t tbytes = strided_bytes(in.S, in.k + 1, in.ldt, BMC_ROW_MAJOR, 8);
        const size_t ibytes = in.per_draw ? (size_t)in.S * 4 : 0;
        if (int rc = ensure(c, c->snStage, abytes + ybytes + up256(tbytes) + ibytes)) return rc;
        char* s = (char*)c->snStage.p;
        if (in.per_draw) {
            char* si = s + abytes + ybytes + up256(tbytes);
            HIPCHK(c, hipMemcpyAsync(si, in.nu_index, ibytes, hipMemcpyHostToDevice, c->stream));
            in.nu_index = si;
        }
        HIPCHK(c, hipMemcpyAsync(s, in.A, strided_bytes(in.n, in.k, in.lda, in.layout, 8), hipMemcpyHostToDevice,
                                 c->stream));
        HIPCHK(c, hipMemcpyAsync(s + abytes, in.y, (size_t)in.n * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(s + abytes + ybytes, in.theta, tbytes, hipMemcpyHostToDevice, c->stream));
        in.A = s, in.y = s + abytes, in.theta = s + abytes + ybytes;
    }
    return sens_run(c, in, out);
}

}  // namespace

extern "C" {

int bmc_power_sensitivity(bmc_ctx* c, const double* A, int64_t n_points, int32_t k, int64_t lda, int layout,
                          const double* y, const double* theta, int64_t n_draws, int64_t ldt,
                          const double* b0, const double* C0, double nu0, double sigma20, const double* Vt,
                          int32_t n_models, const double* alphas, int32_t n_alphas, uint32_t components,
                          int32_t cols_per_batch, double* logdens_out, double* pareto_k_out,
                          double* mean_out, double* sd_out, double* cjs_out, double* weights_out,
                          uint32_t* flags_out) {
    return sens_entry(c, {A, y, theta, n_points, lda, n_draws, ldt, k, layout, b0, C0, Vt, alphas, nu0,
                          sigma20, n_models, n_alphas, cols_per_batch, components},
                      true, {logdens_out, pareto_k_out, mean_out, sd_out, cjs_out, weights_out, flags_out});
}

int bmc_power_sensitivity_device(bmc_ctx* c, const void* dA, int64_t n_points, int32_t k, int64_t lda,
                                 int layout, const void* dy, const void* dtheta, int64_t n_draws,
                                 int64_t ldt, const double* b0, const double* C0, double nu0,
                                 double sigma20, const double* Vt, int32_t n_models, const double* alphas,
                                 int32_t n_alphas, uint32_t components, int32_t cols_per_batch,
                                 double* logdens_out, double* pareto_k_out, double* mean_out,
                                 double* sd_out, double* cjs_out, double* weights_out,
                                 uint32_t* flags_out) {
    return sens_entry(c, {dA, dy, dtheta, n_points, lda, n_draws, ldt, k, layout, b0, C0, Vt, alphas, nu0,
                          sigma20, n_models, n_alphas, cols_per_batch, components},
                      false, {logdens_out, pareto_k_out, mean_out, sd_out, cjs_out, weights_out, flags_out});
}

// The Student-t forms: the Gaussian call's SensIn with the likelihood filled in.  A fixed nu is a
// table of one value without an index; what is not positive and finite is refused by sens_t_check.
#define SENS_T_IN(A, y, theta)                                                                        \
    SensIn in{A, y, theta, n_points, lda, n_draws, ldt, k, layout, b0, C0, Vt, alphas, nu0, sigma20,  \
              n_models, n_alphas, cols_per_batch, components};                                        \
    in.student = true

int bmc_power_sensitivity_t(bmc_ctx* c, const double* A, int64_t n_points, int32_t k, int64_t lda, int layout,
                            const double* y, const double* theta, int64_t n_draws, int64_t ldt,
                            const double* b0, const double* C0, double nu0, double sigma20, const double* Vt,
                            int32_t n_models, const double* alphas, int32_t n_alphas, uint32_t components,
                            int32_t cols_per_batch, double nu, double* logdens_out, double* pareto_k_out,
                            double* mean_out, double* sd_out, double* cjs_out, double* weights_out,
                            uint32_t* flags_out) {
    SENS_T_IN(A, y, theta);
    in.nu_values = &nu, in.n_nu = 1;
    return sens_entry(c, in, true, {logdens_out, pareto_k_out, mean_out, sd_out, cjs_out, weights_out, flags_out});
}

int bmc_power_sensitivity_t_device(bmc_ctx* c, const void* dA, int64_t n_points, int32_t k, int64_t lda,
                                   int layout, const void* dy, const void* dtheta, int64_t n_draws,
                                   int64_t ldt, const double* b0, const double* C0, double nu0,
                                   double sigma20, const double* Vt, int32_t n_models, const double* alphas,
                                   int32_t n_alphas, uint32_t components, int32_t cols_per_batch, double nu,
                                   double* logdens_out, double* pareto_k_out, double* mean_out,
                                   double* sd_out, double* cjs_out, double* weights_out,
                                   uint32_t* flags_out) {
    SENS_T_IN(dA, dy, dtheta);
    in.nu_values = &nu, in.n_nu = 1;
    return sens_entry(c, in, false, {logdens_out, pareto_k_out, mean_out, sd_out, cjs_out, weights_out, flags_out});
}

int bmc_power_sensitivity_tv(bmc_ctx* c, const double* A, int64_t n_points, int32_t k, int64_t lda, int layout,
                             const double* y, const double* theta, int64_t n_draws, int64_t ldt,
                             const double* b0, const double* C0, double nu0, double sigma20, const double* Vt,
                             int32_t n_models, const double* alphas, int32_t n_alphas, uint32_t components,
                             int32_t cols_per_batch, const double* nu_values, int32_t n_values,
                             const int32_t* nu_index, const double* nu_log_prior, double* logdens_out,
                             double* pareto_k_out, double* mean_out, double* sd_out, double* cjs_out,
                             double* weights_out, uint32_t* flags_out) {
    SENS_T_IN(A, y, theta);
    in.per_draw = true;
    in.nu_values = nu_values, in.n_nu = n_values, in.nu_index = nu_index, in.nu_log_prior = nu_log_prior;
    return sens_entry(c, in, true, {logdens_out, pareto_k_out, mean_out, sd_out, cjs_out, weights_out, flags_out});
}

int bmc_power_sensitivity_tv_device(bmc_ctx* c, const void* dA, int64_t n_points, int32_t k, int64_t lda,
                                    int layout, const void* dy, const void* dtheta, int64_t n_draws,
                                    int64_t ldt, const double* b0, const double* C0, double nu0,
                                    double sigma20, const double* Vt, int32_t n_models, const double* alphas,
                                    int32_t n_alphas, uint32_t components, int32_t cols_per_batch,
                                    const double* nu_values, int32_t n_values, const void* d_nu_index,
                                    const double* nu_log_prior, double* logdens_out, double* pareto_k_out,
                                    double* mean_out, double* sd_out, double* cjs_out, double* weights_out,
                                    uint32_t* flags_out) {
    SENS_T_IN(dA, dy, dtheta);
    in.per_draw = true;
    in.nu_values = nu_values, in.n_nu = n_values, in.nu_index = d_nu_index, in.nu_log_prior = nu_log_prior;
    return sens_entry(c, in, false, {logdens_out, pareto_k_out, mean_out, sd_out, cjs_out, weights_out, flags_out});
}
#undef SENS_T_IN

int bmc_sens_last_timing(bmc_ctx* c, double ms_out[4]) {
    if (!c || !ms_out) return BMC_EINVAL;
    for (int i = 0; i < 4; ++i) ms_out[i] = c->sens_ms[i];
    return BMC_OK;
}

}  // extern "C"
