// C ABI, chain diagnostics: split R-hat and ESS (Vehtari et al. 2021)
#include <algorithm>
#include <cmath>

#include "bmc_ctx.h"

namespace {

int check_diag_args(bmc_ctx* c, const void* x, int32_t n_chains, int64_t iters, int32_t n_cols,
                    int64_t ld, int64_t burn) {
    if (!c) return BMC_EINVAL;
    if (!x) return fail(c, BMC_EINVAL, "samples must not be NULL");
    if (n_chains < 1 || n_chains > 65536)
        return fail(c, BMC_EINVAL, "n_chains must be between 1 and 65536");
    if (n_cols < 1 || n_cols > 65536)
        return fail(c, BMC_EINVAL, "n_cols must be between 1 and 65536");
    if (ld < n_cols) return fail(c, BMC_EINVAL, "ld must be >= n_cols");
    if (burn < 0) return fail(c, BMC_EINVAL, "burn must be >= 0");
    if (iters - burn < 8)
        return fail(c, BMC_EINVAL, "need n = (iters - burn) / 2 >= 4 draws per split half-chain (iters = " +
                                       std::to_string(iters) + ", burn = " + std::to_string(burn) + ")");
    return BMC_OK;
}

// Steps 1-5 of the ESS definition on a(t) = acov[0 .. have).  Returns false when the scan needs a
// lag >= have (the caller computes the next block); otherwise sets ess and max_lag.
bool ess_scan(const double* a, int64_t have, int64_t n, double W, double var_plus, double Mn,
              std::vector<double>& rho, double* ess, int64_t* max_lag) {
    auto rho_of = [&](int64_t t) { return 1.0 - (W - a[t]) / var_plus; };
    if (have < 2) return false;
    rho.assign((size_t)n, 0.0);
    rho[0] = 1.0;
    double re = 1.0, ro = rho_of(1);
    rho[1] = ro;
    int64_t t = 1;
    while (t < n - 3 && re + ro > 0) {
        if (t + 2 >= have) return false;
        re = rho_of(t + 1);
        ro = rho_of(t + 2);
        if (re + ro >= 0) {
            rho[t + 1] = re;
            rho[t + 2] = ro;
        }
        t += 2;
    }
    const int64_t max_t = t - 2;
    if (re > 0) rho[max_t + 1] = re;
    for (int64_t u = 1; u <= max_t - 2; u += 2)
        if (rho[u + 1] + rho[u + 2] > rho[u - 1] + rho[u]) {
            rho[u + 1] = (rho[u - 1] + rho[u]) / 2.0;
            rho[u + 2] = rho[u + 1];
        }
    double sum = 0;
    for (int64_t u = 0; u <= max_t; ++u) sum += rho[u];
    double tau = -1.0 + 2.0 * sum + rho[max_t + 1];
    tau = std::max(tau, 1.0 / std::log10(Mn));
    *ess = Mn / tau;
    *max_lag = t;
    return true;
}

// the split of DESIGN.md 4.4: n = T'/2 draws per half, the middle draws of an odd T' as sequences
// of their own
DiagShape diag_shape(const double* dx, int32_t C, int64_t iters, int32_t P, int64_t ld, int64_t burn) {
    const int64_t Tp = iters - burn, n = Tp / 2;
    DiagShape d;
    d.x = dx;
    d.iters = iters;
    d.ld = ld;
    d.burn = burn;
    d.n = n;
    d.half_off = Tp - n;
    d.C = C;
    d.P = P;
    d.n_seq = 2 * C + (Tp & 1 ? C : 0);
    return d;
}

// bmc_chain_autocov*: the moments and ONE block of lags [t0, t0 + n_lags) for the columns cols
// (host; NULL: all), straight from launch_diag_moments and launch_diag_acov
constexpr int32_t AUTOCOV_MAX_ACTIVE = 65536;
constexpr int64_t AUTOCOV_MAX_LAGS = (int64_t)1 << 20, AUTOCOV_MAX_T0 = (int64_t)1 << 40;

int check_autocov_args(bmc_ctx* c, int32_t n_cols, const int32_t* cols, int32_t n_active, int64_t t0,
                       int64_t n_lags) {
    if (n_active < 1 || n_active > AUTOCOV_MAX_ACTIVE)
        return fail(c, BMC_EINVAL, "n_active must be between 1 and 65536");
    if (!cols && n_active != n_cols)
        return fail(c, BMC_EINVAL, "n_active must be n_cols when cols is NULL (all columns)");
    for (int32_t a = 0; cols && a < n_active; ++a)
        if (cols[a] < 0 || cols[a] >= n_cols)
            return fail(c, BMC_EINVAL, "cols[" + std::to_string(a) + "] = " + std::to_string(cols[a]) +
                                           " is outside [0, n_cols)");
    if (t0 < 0 || t0 > AUTOCOV_MAX_T0) return fail(c, BMC_EINVAL, "first_lag must be between 0 and 2^40");
    if (n_lags < 1 || n_lags > AUTOCOV_MAX_LAGS)
        return fail(c, BMC_EINVAL, "n_lags must be between 1 and 2^20");
    return BMC_OK;
}

int autocov_run(bmc_ctx* c, const double* dx, int32_t C, int64_t iters, int32_t P, int64_t ld,
                int64_t burn, const int32_t* cols, int32_t n_active, int64_t t0, int64_t n_lags,
                double* seq_mean_out, double* seq_m2_out, double* shift_out, double* acov_out) {
    const DiagShape d = diag_shape(dx, C, iters, P, ld, burn);
    const size_t ms = (size_t)d.n_seq * P;
    int rc;
    if ((rc = ensure_all(c, {{c->dgPart, diag_moments_scratch(d)}, {c->dgMean, (ms + P) * 8}, {c->dgM2, ms * 8}})))
        return rc;
    HIPCHK(c, launch_diag_moments(d, (double*)c->dgPart.p, (double*)c->dgMean.p, (double*)c->dgM2.p,
                                  c->stream));
    if (acov_out) {
        std::vector<int32_t> all;
        if (!cols) {
            all.resize((size_t)P);
            for (int32_t j = 0; j < P; ++j) all[j] = j;
            cols = all.data();
        }
        const size_t stride = (size_t)((n_lags + 63) / 64 * 64);
        if ((rc = ensure_all(c, {{c->dgCols, (size_t)n_active * 4},
                                 {c->dgAcovPart, diag_acov_scratch(d, n_active, n_lags)},
                                 {c->dgAcov, (size_t)n_active * stride * 8}})))
            return rc;
        HIPCHK(c, hipMemcpyAsync(c->dgCols.p, cols, (size_t)n_active * 4, hipMemcpyHostToDevice, c->stream));
        // (a pageable source: the copy has left `all` when the call returns)
        HIPCHK(c, launch_diag_acov(d, (const double*)c->dgMean.p, (const int32_t*)c->dgCols.p, n_active, t0,
                                   n_lags, (double*)c->dgAcovPart.p, (double*)c->dgAcov.p, c->stream));
        if ((rc = copy_to_host(c, acov_out, c->dgAcov.p, (size_t)n_lags * 8, stride * 8, (size_t)n_active)))
            return rc;
    }
    if (seq_mean_out && (rc = copy_to_host(c, seq_mean_out, c->dgMean.p, ms * 8, ms * 8, 1))) return rc;
    if (shift_out && (rc = copy_to_host(c, shift_out, (const double*)c->dgMean.p + ms, (size_t)P * 8, (size_t)P * 8, 1)))
        return rc;
    if (seq_m2_out && (rc = copy_to_host(c, seq_m2_out, c->dgM2.p, ms * 8, ms * 8, 1))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BMC_OK;
}

}  // namespace

// (declared in bmc_ctx.h: bmc_rank_diagnostics* runs it on its derived series as well.  With no
// ess, mcse or max_lag wanted the autocovariance blocks are not launched.)
int diag_run(bmc_ctx* c, const double* dx, int32_t C, int64_t iters, int32_t P, int64_t ld,
             int64_t burn, double* mean_out, double* sd_out, double* rhat_out, double* ess_out,
             double* mcse_out, int64_t* max_lag_out) {
    const DiagShape d = diag_shape(dx, C, iters, P, ld, burn);
    const int64_t n = d.n;
    const int32_t M = 2 * C;
    const size_t ms = (size_t)d.n_seq * P;
    int rc;
    if ((rc = ensure(c, c->dgPart, diag_moments_scratch(d)))) return rc;
    if ((rc = ensure(c, c->dgMean, (ms + P) * 8))) return rc;   // (+ the shift row)
    if ((rc = ensure(c, c->dgM2, ms * 8))) return rc;
    HIPCHK(c, launch_diag_moments(d, (double*)c->dgPart.p, (double*)c->dgMean.p, (double*)c->dgM2.p,
                                  c->stream));
    // mean: per sequence, of x - shift (the kernels' shift row last)
    std::vector<double> mean(ms + P), m2(ms);
    HIPCHK(c, hipMemcpyAsync(mean.data(), c->dgMean.p, (ms + P) * 8, hipMemcpyDeviceToHost,
                             c->stream));
    HIPCHK(c, hipMemcpyAsync(m2.data(), c->dgM2.p, ms * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));

    const double nan = std::nan("");
    const double Mn = (double)M * (double)n;
    std::vector<double> W(P), var_plus(P), sdv(P), ess(P, nan);
    std::vector<int64_t> lag(P, 0);
    std::vector<int32_t> active;
    for (int32_t j = 0; j < P; ++j) {
        // pooled mean and sd over every kept draw: the sequences merged in order (Chan et al.)
        double na = 0, mu = 0, M2 = 0;
        bool finite = true;
        for (int32_t m = 0; m < d.n_seq; ++m) {
            const double nb = m < M ? (double)n : 1.0, mb = mean[(size_t)m * P + j];
            const double M2b = m2[(size_t)m * P + j];
            finite = finite && std::isfinite(mb) && std::isfinite(M2b);
            if (na == 0) {
                na = nb, mu = mb, M2 = M2b;
                continue;
            }
            const double nt = na + nb, delta = mb - mu;
            mu += delta * (nb / nt);
            M2 += M2b + delta * delta * (na * nb / nt);
            na = nt;
        }
        if (mean_out) mean_out[j] = mean[ms + j] + mu;
        sdv[j] = std::sqrt(M2 / (na - 1));
        if (sd_out) sd_out[j] = sdv[j];
        // split R-hat from the 2C halves
        double w = 0, mbar = 0;
        for (int32_t m = 0; m < M; ++m) {
            w += m2[(size_t)m * P + j] / (double)(n - 1);
            mbar += mean[(size_t)m * P + j];
        }
        w /= M;
        mbar /= M;
        double bn = 0;
        for (int32_t m = 0; m < M; ++m) {
            const double e = mean[(size_t)m * P + j] - mbar;
            bn += e * e;
        }
        bn /= (M - 1);
        W[j] = w;
        var_plus[j] = (double)(n - 1) / (double)n * w + bn;
        const bool ok = finite && std::isfinite(w) && w != 0.0;
        if (rhat_out) rhat_out[j] = ok ? std::sqrt(var_plus[j] / w) : nan;
        if (ok) active.push_back(j);
    }
    if (!ess_out && !mcse_out && !max_lag_out) active.clear();

    // a(t) in blocks of lags: 64 first, then doubling, for the columns whose scan ran off the end
    std::vector<std::vector<double>> acov(P);
    std::vector<double> rho, block;
    int64_t t0 = 0, L = 64;
    while (!active.empty() && t0 < n) {
        const int64_t nl = std::min(L, n - t0);
        const int32_t na = (int32_t)active.size();
        const int64_t stride = (nl + 63) / 64 * 64;
        if ((rc = ensure(c, c->dgCols, (size_t)na * 4))) return rc;
        if ((rc = ensure(c, c->dgAcovPart, diag_acov_scratch(d, na, nl)))) return rc;
        if ((rc = ensure(c, c->dgAcov, (size_t)na * stride * 8))) return rc;
        HIPCHK(c, hipMemcpyAsync(c->dgCols.p, active.data(), (size_t)na * 4, hipMemcpyHostToDevice,
                                 c->stream));
        HIPCHK(c, launch_diag_acov(d, (const double*)c->dgMean.p, (const int32_t*)c->dgCols.p, na,
                                   t0, nl, (double*)c->dgAcovPart.p, (double*)c->dgAcov.p, c->stream));
        block.resize((size_t)na * stride);
        HIPCHK(c, hipMemcpyAsync(block.data(), c->dgAcov.p, block.size() * 8, hipMemcpyDeviceToHost,
                                 c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        t0 += nl;
        L *= 2;
        std::vector<int32_t> next;
        for (int32_t a = 0; a < na; ++a) {
            const int32_t j = active[a];
            acov[j].insert(acov[j].end(), block.begin() + (size_t)a * stride,
                           block.begin() + (size_t)a * stride + nl);
            if (!ess_scan(acov[j].data(), t0, n, W[j], var_plus[j], Mn, rho, &ess[j], &lag[j]))
                next.push_back(j);
        }
        active.swap(next);
    }
    for (int32_t j = 0; j < P; ++j) {
        if (ess_out) ess_out[j] = ess[j];
        if (max_lag_out) max_lag_out[j] = lag[j];
        if (mcse_out) mcse_out[j] = sdv[j] / std::sqrt(ess[j]);
    }
    return BMC_OK;
}

extern "C" {

int bmc_chain_diagnostics(bmc_ctx* c, const double* samples, int32_t n_chains, int64_t iters,
                          int32_t n_cols, int64_t ld, int64_t burn, double* mean_out, double* sd_out,
                          double* rhat_out, double* ess_out, double* mcse_out, int64_t* max_lag_out) {
    int rc = check_diag_args(c, samples, n_chains, iters, n_cols, ld, burn);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    // (the last row of a strided host array may be shorter than ld)
    const size_t bytes = ((size_t)((int64_t)n_chains * iters - 1) * ld + n_cols) * 8;
    if ((rc = ensure(c, c->dgIn, bytes))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->dgIn.p, samples, bytes, hipMemcpyHostToDevice, c->stream));
    return diag_run(c, (const double*)c->dgIn.p, n_chains, iters, n_cols, ld, burn, mean_out, sd_out,
                    rhat_out, ess_out, mcse_out, max_lag_out);
}

int bmc_chain_diagnostics_device(bmc_ctx* c, const void* d_samples, int32_t n_chains, int64_t iters,
                                 int32_t n_cols, int64_t ld, int64_t burn, double* mean_out,
                                 double* sd_out, double* rhat_out, double* ess_out, double* mcse_out,
                                 int64_t* max_lag_out) {
    int rc = check_diag_args(c, d_samples, n_chains, iters, n_cols, ld, burn);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    return diag_run(c, (const double*)d_samples, n_chains, iters, n_cols, ld, burn, mean_out, sd_out,
                    rhat_out, ess_out, mcse_out, max_lag_out);
}

int bmc_chain_autocov(bmc_ctx* c, const double* samples, int32_t n_chains, int64_t iters, int32_t n_cols,
                      int64_t ld, int64_t burn, const int32_t* cols, int32_t n_active, int64_t t0,
                      int64_t n_lags, double* seq_mean_out, double* seq_m2_out, double* shift_out,
                      double* acov_out) {
    int rc = check_diag_args(c, samples, n_chains, iters, n_cols, ld, burn);
    if (rc) return rc;
    if ((rc = check_autocov_args(c, n_cols, cols, n_active, t0, n_lags))) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t bytes = ((size_t)((int64_t)n_chains * iters - 1) * ld + n_cols) * 8;
    if ((rc = ensure(c, c->dgIn, bytes))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->dgIn.p, samples, bytes, hipMemcpyHostToDevice, c->stream));
    return autocov_run(c, (const double*)c->dgIn.p, n_chains, iters, n_cols, ld, burn, cols, n_active, t0,
                       n_lags, seq_mean_out, seq_m2_out, shift_out, acov_out);
}

int bmc_chain_autocov_device(bmc_ctx* c, const void* d_samples, int32_t n_chains, int64_t iters,
                             int32_t n_cols, int64_t ld, int64_t burn, const int32_t* cols,
                             int32_t n_active, int64_t t0, int64_t n_lags, double* seq_mean_out,
                             double* seq_m2_out, double* shift_out, double* acov_out) {
    int rc = check_diag_args(c, d_samples, n_chains, iters, n_cols, ld, burn);
    if (rc) return rc;
    if ((rc = check_autocov_args(c, n_cols, cols, n_active, t0, n_lags))) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    return autocov_run(c, (const double*)d_samples, n_chains, iters, n_cols, ld, burn, cols, n_active, t0,
                       n_lags, seq_mean_out, seq_m2_out, shift_out, acov_out);
}

}  // extern "C"
