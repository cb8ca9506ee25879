// The Student-t (outlier-robust) Gibbs sampler behind the C ABI: bmc_robust_run*.
#include <cstring>

#include "bmc_ctx.h"
#include "bmc_robust.h"

namespace {

// nu on a grid (bmc_robust_run_nu*): the prior, the replay inputs and the outputs.  Exactly one of
// idx_host / idx_dev is set; tstat_host / tstat_dev may both be NULL.
struct NuSpec {
    const double* grid;
    const double* weight;
    int32_t n_grid, nu_init;
    const double* u_nu;        // replay: [n_chains][burn + iters]
    const int32_t* nu_path;    // replay: [n_chains][burn + iters]
    int32_t* idx_host;
    void* idx_dev;
    double* tstat_host;
    void* tstat_dev;
};

int robust_common(bmc_ctx* c, double nu, const NuSpec* ns, int32_t n_chains, int64_t iters, int64_t burn, int rng_mode,
                  const uint64_t* seeds, const double* xi, const double* g, const double* gl,
                  double* samples_host, void* samples_dev, double* weight_host, void* weight_dev,
                  bmc_stats* stats) {
    if (!c->have_problem || !c->have_prior)
        return fail(c, BMC_ESTATE, "bmc_set_problem and bmc_set_prior must be called first");
    const std::string name = ns ? "bmc_robust_run_nu: " : "bmc_robust_run: ";
    std::string why = ns ? robust_nu_check(ns->grid, ns->weight, ns->n_grid, ns->nu_init) : "";
    if (!why.empty()) return fail(c, BMC_EINVAL, name + why);
    if (ns) nu = ns->grid[ns->nu_init];
    why = robust_check(c->n, c->k, c->f32, nu, n_chains, iters, burn);
    if (!why.empty()) return fail(c, BMC_EINVAL, name + why);
    if (rng_mode == BMC_RNG_DEVICE) {
        if (!seeds) return fail(c, BMC_EINVAL, "seeds required in device RNG mode");
        if (xi || g || gl) return fail(c, BMC_EINVAL, "xi/g/gl must be NULL in device RNG mode");
        if (ns && (ns->u_nu || ns->nu_path))
            return fail(c, BMC_EINVAL, "u_nu/nu_path must be NULL in device RNG mode");
    } else if (rng_mode == BMC_RNG_REPLAY) {
        if (!xi || !g || !gl) return fail(c, BMC_EINVAL, "xi, g and gl required in replay mode");
        if (ns) {
            if (!ns->u_nu || !ns->nu_path)
                return fail(c, BMC_EINVAL, "u_nu and nu_path required in replay mode");
            const size_t cells = (size_t)n_chains * (size_t)(burn + iters);
            for (size_t i = 0; i < cells; ++i)
                if (ns->nu_path[i] < 0 || ns->nu_path[i] >= ns->n_grid)
                    return fail(c, BMC_EINVAL, name + "nu_path must index the nu grid");
        }
    } else {
        return fail(c, BMC_EINVAL, "rng_mode must be 0 or 1");
    }
    const int K = c->k;
    const int64_t N = c->n;
    const size_t C = (size_t)n_chains, Tt = (size_t)(burn + iters), T = (size_t)iters;
    int rc;
    if (rng_mode == BMC_RNG_REPLAY && Tt > 0) {
        size_t free_b = 0, total_b = 0;
        HIPCHK(c, hipMemGetInfo(&free_b, &total_b));
        const size_t need = robust_gl_bytes(N, n_chains, (int64_t)Tt);
        if (need > c->rbGl.cap && need - c->rbGl.cap > free_b)
            return fail(c, BMC_ENOMEM, "bmc_robust_run: the replayed weight variates gl (" +
                                           std::to_string(need) + " bytes) do not fit the device");
        if ((rc = ensure(c, c->rbGl, need))) return rc;
    }
    const size_t n_pad = (size_t)robust_rows_padded(N);
    if ((rc = ensure_all(c, {{c->xi, C * Tt * K * 8}, {c->gam, C * Tt * 8},
                             {c->rbZ, robust_packed_bytes(N, K)},
                             {c->rbPrior, (size_t)(K * K + K) * 8},
                             {c->rbWs, robust_workspace_bytes(N, n_chains)},
                             {c->rbWsum, C * (size_t)N * 8},
                             {c->status, C * sizeof(int32_t)}, {c->seeds, C * sizeof(uint64_t)}})))
        return rc;
    double* d_samples = (double*)samples_dev;
    if (!d_samples) {
        if ((rc = ensure(c, c->samples, C * T * (K + 1) * 8))) return rc;
        d_samples = (double*)c->samples.p;
    }
    double* d_weight = weight_dev ? (double*)weight_dev : (double*)c->rbWsum.p;
    // nu on a grid: [table 4 G f64][tstat C T f64][u C Tt f64][idx C T i32][path C Tt i32]
    const bool replay_nu = ns && rng_mode == BMC_RNG_REPLAY;
    double *d_tab = nullptr, *d_tstat = nullptr, *d_unu = nullptr;
    int32_t *d_idx = nullptr, *d_path = nullptr;
    if (ns) {
        const size_t G = (size_t)ns->n_grid;
        if ((rc = ensure(c, c->rbNu, (4 * G + C * T + C * Tt) * 8 + (C * T + C * Tt) * 4))) return rc;
        d_tab = (double*)c->rbNu.p;
        double* own_tstat = d_tab + 4 * G;
        d_unu = own_tstat + C * T;
        int32_t* own_idx = (int32_t*)(d_unu + C * Tt);
        d_path = own_idx + C * T;
        d_idx = ns->idx_dev ? (int32_t*)ns->idx_dev : own_idx;
        d_tstat = ns->tstat_dev ? (double*)ns->tstat_dev : (ns->tstat_host ? own_tstat : nullptr);
        std::vector<double> tab(4 * G);
        robust_nu_table(ns->grid, ns->weight, ns->n_grid, c->n, tab.data());
        // pageable source: the copy is staged before hipMemcpyAsync returns
        HIPCHK(c, hipMemcpyAsync(d_tab, tab.data(), 4 * G * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (T > 0) HIPCHK(c, hipMemsetAsync(d_idx, 0xff, C * T * 4, c->stream));   // -1: never drawn
        if (T > 0 && d_tstat) HIPCHK(c, hipMemsetAsync(d_tstat, 0xff, C * T * 8, c->stream));   // NaN: likewise
        if (replay_nu && Tt > 0) {
            HIPCHK(c, hipMemcpyAsync(d_unu, ns->u_nu, C * Tt * 8, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(d_path, ns->nu_path, C * Tt * 4, hipMemcpyHostToDevice, c->stream));
        }
    }
    double* dP = (double*)c->rbPrior.p;
    HIPCHK(c, hipMemsetAsync(c->status.p, 0, C * sizeof(int32_t), c->stream));
    HIPCHK(c, hipMemcpyAsync(dP, c->Pprec.data(), (size_t)K * K * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dP + (size_t)K * K, c->Pb0.data(), (size_t)K * 8, hipMemcpyHostToDevice,
                             c->stream));
    double* Z = (double*)c->rbZ.p;
    double* yv = Z + n_pad * (size_t)robust_ldz(K);
    HIPCHK(c, launch_robust_pack(panels_of(c, c->Xraw.p), Z, yv, c->stream));
    HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
    if (Tt > 0) {
        if (rng_mode == BMC_RNG_DEVICE) {
            HIPCHK(c, hipMemcpyAsync(c->seeds.p, seeds, C * sizeof(uint64_t), hipMemcpyHostToDevice,
                                     c->stream));
            HIPCHK(c, launch_rng_fill((const uint64_t*)c->seeds.p, n_chains, (int64_t)Tt * K,
                                      (double*)c->xi.p, (c->nu0 + (double)N) / 2.0, (int64_t)Tt,
                                      (double*)c->gam.p, c->stream));
        } else {
            HIPCHK(c, hipMemcpyAsync(c->xi.p, xi, C * Tt * K * 8, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(c->gam.p, g, C * Tt * 8, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(c->rbGl.p, gl, C * Tt * (size_t)N * 8, hipMemcpyHostToDevice,
                                     c->stream));
        }
    }
    HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
    RobustArgs a;
    a.Z = Z;
    a.yv = yv;
    a.n = N;
    a.k = K;
    a.rows_per_wave = robust_rows_per_wave(N);
    a.P = dP;
    a.Pb0 = dP + (size_t)K * K;
    a.nu = nu;
    a.shape_l = (nu + 1.0) / 2.0;
    a.nu_tab = d_tab;
    a.n_grid = ns ? ns->n_grid : 0;
    a.nu_init = ns ? ns->nu_init : 0;
    a.nu0_s20 = c->nu0 * c->s20;
    a.sigma2_init = c->sigma2_init;
    a.iters = iters;
    a.burn = burn;
    const std::vector<RobustLaunch> plan = robust_launches(n_chains);
    for (const RobustLaunch& l : plan) {
        const size_t c0 = (size_t)l.c0;
        a.n_chains = l.n_chains;
        a.seeds = rng_mode == BMC_RNG_DEVICE ? (const uint64_t*)c->seeds.p + c0 : nullptr;
        a.xi = (const double*)c->xi.p + c0 * Tt * K;
        a.gam = (const double*)c->gam.p + c0 * Tt;
        a.gl = rng_mode == BMC_RNG_REPLAY ? (const double*)c->rbGl.p + c0 * Tt * (size_t)N : nullptr;
        a.ws = (double*)c->rbWs.p + c0 * (size_t)N * 2;
        a.samples = d_samples + c0 * T * (K + 1);
        a.wsum = d_weight + c0 * (size_t)N;
        a.status = (int32_t*)c->status.p + c0;
        a.u_nu = replay_nu ? d_unu + c0 * Tt : nullptr;
        a.nu_path = replay_nu ? d_path + c0 * Tt : nullptr;
        a.nu_idx = ns ? d_idx + c0 * T : nullptr;
        a.tstat = d_tstat ? d_tstat + c0 * T : nullptr;
        HIPCHK(c, ns ? launch_robust_nu(a, c->stream) : launch_robust(a, c->stream));
    }
    HIPCHK(c, hipEventRecord(c->ev[2], c->stream));
    std::vector<int32_t> st(C, 0);
    HIPCHK(c, hipMemcpyAsync(st.data(), c->status.p, C * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (samples_host && iters > 0)
        if ((rc = copy_to_host(c, samples_host, d_samples, C * T * (K + 1) * 8, C * T * (K + 1) * 8, 1)))
            return rc;
    if (weight_host)
        if ((rc = copy_to_host(c, weight_host, d_weight, C * (size_t)N * 8, C * (size_t)N * 8, 1))) return rc;
    if (ns && iters > 0) {
        if (ns->idx_host && (rc = copy_to_host(c, ns->idx_host, d_idx, C * T * 4, C * T * 4, 1))) return rc;
        if (ns->tstat_host && (rc = copy_to_host(c, ns->tstat_host, d_tstat, C * T * 8, C * T * 8, 1)))
            return rc;
    }
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        if ((rc = event_ms(c, 0, 1, &stats->rng_ms)) || (rc = event_ms(c, 1, 2, &stats->loop_ms)) ||
            (rc = event_ms(c, 0, 2, &stats->total_ms)))
            return rc;
        stats->iterations = burn + iters;
        stats->n_chains = n_chains;
        stats->launches = (int32_t)plan.size();
        stats->groups_per_chain = 1;
        stats->waves_per_group = ROBUST_WAVES;
        stats->chains_per_pass = 1;
        stats->residency = 3;
        stats->bytes_per_pass = (N * K + N) * 8;
        stats->passes = 2 * (burn + iters) * (int64_t)n_chains;
    }
    return robust_status_check(c, st, [](size_t i, const std::string& what) {
        return "bmc_robust_run: " + what + " (chain " + std::to_string(i) + ")";
    });
}

}  // namespace

extern "C" {

int bmc_robust_run(bmc_ctx* c, double nu, int32_t n_chains, int64_t iters, int64_t burn, int rng_mode,
                   const uint64_t* seeds, const double* xi, const double* g, const double* gl,
                   double* samples_out, double* row_weight_out, bmc_stats* stats) {
    if (!c) return BMC_EINVAL;
    if (!samples_out && iters > 0) return fail(c, BMC_EINVAL, "samples_out must not be NULL");
    HIPCHK(c, hipSetDevice(c->device));
    return robust_common(c, nu, nullptr, n_chains, iters, burn, rng_mode, seeds, xi, g, gl, samples_out, nullptr,
                         row_weight_out, nullptr, stats);
}

int bmc_robust_run_device(bmc_ctx* c, double nu, int32_t n_chains, int64_t iters, int64_t burn,
                          const uint64_t* seeds, void* d_samples_out, void* d_row_weight_out,
                          bmc_stats* stats) {
    if (!c) return BMC_EINVAL;
    if (!d_samples_out && iters > 0) return fail(c, BMC_EINVAL, "d_samples_out must not be NULL");
    HIPCHK(c, hipSetDevice(c->device));
    return robust_common(c, nu, nullptr, n_chains, iters, burn, BMC_RNG_DEVICE, seeds, nullptr, nullptr, nullptr,
                         nullptr, d_samples_out, nullptr, d_row_weight_out, stats);
}

int bmc_robust_run_nu(bmc_ctx* c, const double* nu_grid, const double* nu_weight, int32_t n_grid,
                      int32_t nu_init, int32_t n_chains, int64_t iters, int64_t burn, int rng_mode,
                      const uint64_t* seeds, const double* xi, const double* g, const double* gl,
                      const double* u_nu, const int32_t* nu_path, double* samples_out,
                      double* row_weight_out, int32_t* nu_idx_out, double* tstat_out, bmc_stats* stats) {
    if (!c) return BMC_EINVAL;
    if ((!samples_out || !nu_idx_out) && iters > 0)
        return fail(c, BMC_EINVAL, "samples_out and nu_idx_out must not be NULL");
    HIPCHK(c, hipSetDevice(c->device));
    const NuSpec ns{nu_grid, nu_weight, n_grid, nu_init, u_nu, nu_path, nu_idx_out, nullptr, tstat_out,
                    nullptr};
    return robust_common(c, 0.0, &ns, n_chains, iters, burn, rng_mode, seeds, xi, g, gl, samples_out,
                         nullptr, row_weight_out, nullptr, stats);
}

int bmc_robust_run_nu_device(bmc_ctx* c, const double* nu_grid, const double* nu_weight, int32_t n_grid,
                             int32_t nu_init, int32_t n_chains, int64_t iters, int64_t burn,
                             const uint64_t* seeds, void* d_samples_out, void* d_row_weight_out,
                             void* d_nu_idx_out, void* d_tstat_out, bmc_stats* stats) {
    if (!c) return BMC_EINVAL;
    if ((!d_samples_out || !d_nu_idx_out) && iters > 0)
        return fail(c, BMC_EINVAL, "d_samples_out and d_nu_idx_out must not be NULL");
    HIPCHK(c, hipSetDevice(c->device));
    const NuSpec ns{nu_grid, nu_weight, n_grid, nu_init, nullptr, nullptr, nullptr, d_nu_idx_out, nullptr,
                    d_tstat_out};
    return robust_common(c, 0.0, &ns, n_chains, iters, burn, BMC_RNG_DEVICE, seeds, nullptr, nullptr,
                         nullptr, nullptr, d_samples_out, nullptr, d_row_weight_out, stats);
}

}  // extern "C"
