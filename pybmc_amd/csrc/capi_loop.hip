// The persistent loops behind the C ABI: bmc_gibbs_run* and bmc_simplex_run*, and the steps the
// two drivers share.
#include <cmath>
#include <cstring>

#include "bmc_ctx.h"

namespace {

// rss_mode 1: upload G, u0, g0 and take rss(u0) from ONE residual pass over the rotated panels
int gram_device_setup(bmc_ctx* c) {
    if (c->have_gram_dev) return BMC_OK;
    const int k = c->k;
    if (k > 64 || c->Gt.empty())
        return fail(c, BMC_EINVAL, "rss_mode 1 (sufficient statistics) supports at most 64 columns");
    int rc;
    if ((rc = ensure_all(c, {{c->dGt, (size_t)k * k * 8}, {c->dU0, (size_t)k * 8}, {c->dG0, (size_t)k * 8}})))
        return rc;
    HIPCHK(c, hipMemcpyAsync(c->dGt.p, c->Gt.data(), (size_t)k * k * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->dU0.p, c->u0.data(), (size_t)k * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->dG0.p, c->g0.data(), (size_t)k * 8, hipMemcpyHostToDevice, c->stream));
    const Panels P = panels_of(c, c->Xrot.p);
    if ((rc = ensure_rss(c, P, 8))) return rc;
    HIPCHK(c, launch_residual_rss(P, (const double*)c->dU0.p, 1, (double*)c->rssPartial.p,
                                  (unsigned*)c->ticket.p, (double*)c->rssOut.p, c->stream));
    HIPCHK(c, hipMemcpyAsync(&c->rss0, c->rssOut.p, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->have_gram_dev = true;
    return BMC_OK;
}

// Workgroups of exactly this kernel, block size and LDS footprint that one CU admits
// (hipFuncSetAttribute first: the occupancy answer depends on the dynamic LDS the kernel admits)
hipError_t groups_per_cu(const LoopKernel& k, int* per_cu) {
    const hipError_t e = hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.lds);
    return e != hipSuccess ? e : hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, k.fn, (int)k.block.x, k.lds);
}

// The workgroups of a persistent launch wait for each other inside the kernel, so all of them
// must be resident at once.  A plain launch checks nothing (an over-subscribed grid would spin
// until the bounded spins expire, 4 s): ask the runtime how many workgroups of exactly this
// kernel, block size and LDS footprint one CU admits and compare with what the launch keeps
// resident.  `resident` = workgroups that stay in the loop (unused slots leave at once).
int check_residency(bmc_ctx* c, const LoopKernel& k, int resident, const char* what) {
    int per_cu = 0;
    const hipError_t e = k.fn ? groups_per_cu(k, &per_cu) : hipErrorInvalidValue;
    if (e != hipSuccess)
        return fail(c, e == hipErrorInvalidValue ? BMC_EINVAL : BMC_EHIP,
                    std::string(what) + ": no kernel for this geometry (" + hipGetErrorString(e) + ")");
    const long cap = (long)per_cu * chip_of(c).groups_max;
    if ((long)resident > cap)
        return fail(c, BMC_EINVAL,
                    std::string(what) + ": the launch needs " + std::to_string(resident) +
                        " co-resident workgroups but the device admits " + std::to_string(cap) + " (" +
                        std::to_string(per_cu) + " per CU x " + std::to_string(chip_of(c).groups_max) +
                        " CUs); use fewer groups_per_chain / waves_per_group or another residency");
    return BMC_OK;
}

// an explicit geometry request that the (possibly limited) chip cannot hold is an error, not
// something to clamp silently
int check_tuning_fits(bmc_ctx* c) {
    const Chip chip = chip_of(c);
    if (c->tune.groups_per_chain > chip.groups_max)
        return fail(c, BMC_EINVAL,
                    "groups_per_chain = " + std::to_string(c->tune.groups_per_chain) + " exceeds the " +
                        std::to_string(chip.groups_max) +
                        " workgroups that can be resident at once (one per CU; bmc_tuning.cu_limit)");
    return BMC_OK;
}

// ---- what the Gibbs and the simplex driver share --------------------------------------------------

// xi [C][T][k] and gam [C][T] into the context's buffers: the caller's arrays, or made on the
// device under one seed per chain
int stage_variates(bmc_ctx* c, int rng_mode, const uint64_t* seeds, int32_t n_chains, size_t T,
                   double shape, const double* xi, const double* g) {
    const size_t C = (size_t)n_chains;
    const int K = c->k;
    if (rng_mode == BMC_RNG_DEVICE) {
        HIPCHK(c, hipMemcpyAsync(c->seeds.p, seeds, C * sizeof(uint64_t), hipMemcpyHostToDevice,
                                 c->stream));
        HIPCHK(c, launch_rng_fill((const uint64_t*)c->seeds.p, n_chains, (int64_t)T * K,
                                  (double*)c->xi.p, shape, (int64_t)T, (double*)c->gam.p, c->stream));
    } else {
        HIPCHK(c, hipMemcpyAsync(c->xi.p, xi, C * T * K * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->gam.p, g, C * T * 8, hipMemcpyHostToDevice, c->stream));
    }
    return BMC_OK;
}

// The fields that GibbsArgs and SimplexArgs share, from one chain's geometry
template <typename Args>
void set_geometry(bmc_ctx* c, const Geometry& geo, int gran_stride, int64_t iters, Args& a) {
    a.gran = (unsigned long long*)c->gran.p;
    a.gran_stride = gran_stride;
    a.iters = iters;
    a.G = geo.G;
    a.mode = geo.mode;
    a.reg_ppw = geo.ppw;
    a.force_agent_scope = c->tune.force_agent_scope;
    a.panels_per_group = geo.ppg;
    a.one_wave = geo.one_wave;
}

// Before every persistent launch: its nonce, its exchange words zeroed, the residency check
// (`resident` workgroups wait for each other; 0: a single-workgroup chain waits for nobody) and
// the name of the kernel `k` that the launcher is about to start.
int begin_launch(bmc_ctx* c, const LoopKernel& k, uint64_t n_tags, size_t gran_bytes, int resident,
                 const char* what, uint32_t* epoch0) {
    *epoch0 = launch_nonce(c, n_tags);
    HIPCHK(c, hipMemsetAsync(c->gran.p, 0, gran_bytes, c->stream));
    if (resident > 0)
        if (int rc = check_residency(c, k, resident, what)) return rc;
    if (k.fn) c->last_kernels.push_back(kernel_name(k.key));
    return BMC_OK;
}

// status and placement of the call's chains on their way to the host (the caller synchronises)
int read_chain_words(bmc_ctx* c, std::vector<int32_t>& st, std::vector<int32_t>& place) {
    HIPCHK(c, hipMemcpyAsync(st.data(), c->status.p, st.size() * sizeof(int32_t), hipMemcpyDeviceToHost,
                             c->stream));
    HIPCHK(c, hipMemcpyAsync(place.data(), c->placement.p, place.size() * sizeof(int32_t),
                             hipMemcpyDeviceToHost, c->stream));
    return BMC_OK;
}

// The bmc_stats fields that both loops compute alike, from ev[0] (start), ev[1] (variates staged),
// ev[2] (loops done) and ev[last] (all device work done).  passes, iterations, waves_per_group,
// chains_per_pass and residency are the caller's.
int common_stats(bmc_ctx* c, bmc_stats* stats, int last, int32_t n_chains, int launches, int G,
                 const std::vector<int32_t>& place) {
    std::memset(stats, 0, sizeof(*stats));
    int rc;
    if ((rc = event_ms(c, 0, 1, &stats->rng_ms)) || (rc = event_ms(c, 1, 2, &stats->loop_ms)) ||
        (rc = event_ms(c, 0, last, &stats->total_ms)))
        return rc;
    stats->n_chains = n_chains;
    stats->launches = launches;
    stats->groups_per_chain = G;
    for (const int32_t p : place) stats->xcd_local_chains += p ? 1 : 0;
    stats->bytes_per_pass = ((int64_t)c->n * c->k + c->n) * (c->f32 ? 4 : 8);
    return BMC_OK;
}

// ---- Gibbs ------------------------------------------------------------------------------------------

int run_common(bmc_ctx* c, int32_t n_chains, int64_t iters, const uint64_t* seeds, int rng_mode,
               const double* xi, const double* g, double* samples_host, void* samples_dev,
               bmc_stats* stats) {
    c->last_kernels.clear();
    if (!c->have_problem || !c->have_prior)
        return fail(c, BMC_ESTATE, "bmc_set_problem and bmc_set_prior must be called first");
    if (n_chains < 1 || iters < 0) return fail(c, BMC_EINVAL, "need n_chains >= 1, iters >= 0");
    if (iters >= 0xffffffffll) return fail(c, BMC_EINVAL, "iters must be < 2^32 - 1");
    if (rng_mode == BMC_RNG_DEVICE) {
        if (!seeds) return fail(c, BMC_EINVAL, "seeds required in device RNG mode");
        if (xi || g) return fail(c, BMC_EINVAL, "xi/g must be NULL in device RNG mode");
    } else if (rng_mode == BMC_RNG_REPLAY) {
        if (!xi || !g) return fail(c, BMC_EINVAL, "xi and g required in replay mode");
    } else {
        return fail(c, BMC_EINVAL, "rng_mode must be 0 or 1");
    }
    const int K = c->k;
    const size_t T = (size_t)iters, C = (size_t)n_chains;
    int rc;
    // (one row more than the chains have: the loop kernel's leader prefetches row t + 1 in every
    // iteration, the last one included, and the last chain's row T is this padding -- read, never used)
    if ((rc = ensure_all(c, {{c->xi, (C * T + 1) * K * 8}, {c->gam, (C * T + 1) * 8},
                             {c->uout, C * T * (K + 1) * 8}})))
        return rc;
    double* d_samples = (double*)samples_dev;
    if (!d_samples) {
        if ((rc = ensure(c, c->samples, C * T * (K + 1) * 8))) return rc;
        d_samples = (double*)c->samples.p;
    }
    if ((rc = check_tuning_fits(c))) return rc;
    const Chip chip = chip_of(c);
    const Geometry geo = choose_geometry(shape_of(c), c->tune, chip, n_chains, true, 8);
    bool pack_ok = false;
    GibbsLaunch lp{};
    lp.n_chains = 1; lp.chains_per_pass = 1; lp.waves = geo.waves; lp.nslot = geo.nslot; lp.pack = 1;
    if (gibbs_pack_candidate(geo, chip, c->tune, n_chains) && gibbs_kernel_key(shape_of(c), geo, lp).pack) {
        // the packed variant exists for this shape: its VGPRs (<= 128) and two groups per CU?
        GibbsArgs q{};
        q.P = panels_of(c, c->Xrot.p);
        q.G = geo.G; q.waves = geo.waves; q.mode = geo.mode; q.reg_ppw = geo.ppw;
        q.nslot = geo.nslot; q.n_chains = 1; q.chains_per_pass = 1; q.panels_per_group = geo.ppg;
        q.pack = 1;
        const LoopKernel k = gibbs_kernel(q);
        hipFuncAttributes at;
        int per_cu = 0;
        pack_ok = k.fn && hipFuncGetAttributes(&at, k.fn) == hipSuccess && at.numRegs > 0 && at.numRegs <= 128 &&
                  groups_per_cu(k, &per_cu) == hipSuccess && per_cu >= 2;
    }
    const GibbsPlan plan = plan_gibbs(geo, shape_of(c), c->tune, chip, n_chains, pack_ok);
    const int gran_stride = bmc::gran_slot_words(geo.G);
    if ((rc = ensure_all(c, {{c->gran, (size_t)plan.max_per_launch * 3 * gran_stride * 8},
                             {c->status, C * sizeof(int32_t)},
                             {c->placement, C * sizeof(int32_t)},
                             {c->seeds, C * sizeof(uint64_t)}})))
        return rc;
    HIPCHK(c, hipMemsetAsync(c->placement.p, 0, C * sizeof(int32_t), c->stream));
    HIPCHK(c, hipMemsetAsync(c->status.p, 0, C * sizeof(int32_t), c->stream));
    HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
    if (iters > 0) {
        const double shape = (c->nu0 + (double)c->n) / 2.0;  // inference_utils.py:50
        if ((rc = stage_variates(c, rng_mode, seeds, n_chains, T, shape, xi, g))) return rc;
    }
    HIPCHK(c, hipEventRecord(c->ev[1], c->stream));

    GibbsArgs a;
    a.P = panels_of(c, c->Xrot.p);
    a.lam = (const double*)c->dLam.p;
    a.c1 = (const double*)c->dC1.p;
    a.c2 = (const double*)c->dC2.p;
    a.nu0_s20 = c->nu0 * c->s20;
    a.sigma2_init = c->sigma2_init;
    set_geometry(c, geo, gran_stride, iters, a);
    if (geo.mode == 2) {
        // A matrix larger than the 256 MiB Infinity Cache, swept once per iteration, would evict
        // itself before it is read again.  Each group then reads its first panels normally, about
        // 190 MB in all, which stay cached from one iteration to the next, and the rest with
        // non-temporal loads that do not displace them (410 MB: 72 -> 62.6 us per iteration).
        const double total = (double)c->npanels * (double)(K + 1) * 64.0 * c->vec * (c->f32 ? 4 : 8);
        const double budget = 190e6;
        if (total > budget) a.P.stream_keep = (int32_t)((double)geo.ppg * budget / total);
    }
    a.dbg = nullptr;
#ifdef BMC_STAMPS
    if ((rc = ensure(c, c->dbg, 12 * sizeof(long long)))) return rc;
    HIPCHK(c, hipMemsetAsync(c->dbg.p, 0, 12 * sizeof(long long), c->stream));
    a.dbg = (long long*)c->dbg.p;
#endif
    int launches = 0;
    const bool gram_mode = c->tune.rss_mode == 1;
    const bool loop = !gram_mode && iters > 0;
    if (gram_mode && iters > 0) {
        if ((rc = gram_device_setup(c))) return rc;
        GramArgs ga;
        ga.k = K;
        ga.lam = a.lam; ga.c1 = a.c1; ga.c2 = a.c2;
        ga.Gt = (const double*)c->dGt.p; ga.u0 = (const double*)c->dU0.p; ga.g0 = (const double*)c->dG0.p;
        ga.rss0 = c->rss0;
        ga.nu0_s20 = a.nu0_s20; ga.sigma2_init = a.sigma2_init;
        ga.xi = (const double*)c->xi.p; ga.gam = (const double*)c->gam.p; ga.uout = (double*)c->uout.p;
        ga.iters = iters;
        ga.n_chains = n_chains;
        HIPCHK(c, launch_gibbs_gram(ga, c->stream));
        launches = 1;
    }
    for (size_t i = 0; loop && i < plan.launches.size(); ++i) {
        const GibbsLaunch& l = plan.launches[i];
        a.n_chains = l.n_chains;
        a.chains_per_pass = l.chains_per_pass;
        a.waves = l.waves;
        a.nslot = l.nslot;
        a.pack = l.pack;
        a.bundle_slots = l.bundle_slots;
        a.bundle_bal = l.bundle_bal;
        a.xi = (const double*)c->xi.p + (size_t)l.c0 * T * K;
        a.gam = (const double*)c->gam.p + (size_t)l.c0 * T;
        a.uout = (double*)c->uout.p + (size_t)l.c0 * T * (K + 1);
        a.status = (int32_t*)c->status.p + l.c0;
        a.placement = (int32_t*)c->placement.p + l.c0;
        if (gibbs_lds_bytes(a) > LDS_LIMIT) return fail(c, BMC_EINVAL, "LDS plan exceeds 160 KiB");
        const bool waits = a.G > 1 || l.chains_per_pass > 1;   // (a single-workgroup chain waits for nobody)
        if ((rc = begin_launch(c, gibbs_kernel(a), (uint64_t)iters, (size_t)l.n_chains * 3 * gran_stride * 8,
                               waits ? l.resident : 0, "persistent Gibbs kernel", &a.epoch0)))
            return rc;
        HIPCHK(c, launch_gibbs(a, c->stream));
        ++launches;
    }
    HIPCHK(c, hipEventRecord(c->ev[2], c->stream));
    if (iters > 0)
        HIPCHK(c, launch_unrotate((const double*)c->uout.p, (const double*)c->dWT.p, K,
                                  (int64_t)(C * T), d_samples, c->stream));
    HIPCHK(c, hipEventRecord(c->ev[3], c->stream));
    std::vector<int32_t> st(C, 0), place(C, 0);
    if ((rc = read_chain_words(c, st, place))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (samples_host && iters > 0)
        if ((rc = copy_to_host(c, samples_host, d_samples, C * T * (K + 1) * 8, C * T * (K + 1) * 8, 1)))
            return rc;
    if (stats) {
        if ((rc = common_stats(c, stats, 3, n_chains, launches, geo.G, place)) ||
            (rc = event_ms(c, 2, 3, &stats->post_ms)))
            return rc;
        stats->iterations = iters;
        stats->waves_per_group = loop ? plan.waves_per_group : geo.waves;   // widened for leader waves
        stats->chains_per_pass = loop ? plan.chains_per_pass : 1;
        stats->residency = gram_mode ? 4 : geo.mode + 1;
        // a pass that serves several chains counts once
        stats->passes = loop ? plan.passes * iters : 0;
        if (gram_mode) { stats->groups_per_chain = 1; stats->waves_per_group = 1; }
    }
    for (size_t i = 0; i < C; ++i)
        if (st[i] != 0)
            return fail(c, BMC_ETIMEOUT, "persistent Gibbs kernel: bounded spin expired (chain " +
                                             std::to_string(i) + ")");
    return BMC_OK;
}

}  // namespace

extern "C" {

int bmc_gibbs_run(bmc_ctx* c, int32_t n_chains, int64_t iters, const uint64_t* seeds, int rng_mode,
                  const double* xi, const double* g, double* samples_out, bmc_stats* stats) {
    if (!c) return BMC_EINVAL;
    if (!samples_out && iters > 0) return fail(c, BMC_EINVAL, "samples_out must not be NULL");
    HIPCHK(c, hipSetDevice(c->device));
    return run_common(c, n_chains, iters, seeds, rng_mode, xi, g, samples_out, nullptr, stats);
}

int bmc_gibbs_run_device(bmc_ctx* c, int32_t n_chains, int64_t iters, const uint64_t* seeds,
                         void* d_samples_out, bmc_stats* stats) {
    if (!c) return BMC_EINVAL;
    if (!d_samples_out && iters > 0) return fail(c, BMC_EINVAL, "d_samples_out must not be NULL");
    HIPCHK(c, hipSetDevice(c->device));
    return run_common(c, n_chains, iters, seeds, BMC_RNG_DEVICE, nullptr, nullptr, nullptr,
                      d_samples_out, stats);
}

int bmc_simplex_run_chains(bmc_ctx* c, const double* Vt_hat, int32_t Km, const double* S_hat,
                           int32_t n_chains, int64_t iters, int64_t burn, double stepsize, double nu0,
                           double sigma20, int rng_mode, const uint64_t* seeds, const double* xi,
                           const double* unif, int64_t unif_ld, const int64_t* n_unif, const double* g,
                           double* samples_out, int64_t* accepted_out, int64_t* unif_used_out,
                           bmc_stats* stats) {
    if (!c) return BMC_EINVAL;
    c->last_kernels.clear();
    if (!c->have_problem) return fail(c, BMC_ESTATE, "bmc_set_problem must be called first");
    if (!Vt_hat || !S_hat || Km < 1) return fail(c, BMC_EINVAL, "Vt_hat/S_hat/n_models invalid");
    if (n_chains < 1) return fail(c, BMC_EINVAL, "need n_chains >= 1");
    if (burn < 0) return fail(c, BMC_EINVAL, "Burn-in iterations must be non-negative.");
    if (!(stepsize > 0)) return fail(c, BMC_EINVAL, "Stepsize must be positive.");
    if (iters < 0 || burn + iters >= 0xffffffffll) return fail(c, BMC_EINVAL, "bad iteration count");
    if (iters > 0 && !samples_out) return fail(c, BMC_EINVAL, "samples_out must not be NULL");
    const size_t C = (size_t)n_chains;
    std::vector<int64_t> nu(C, 0);   // uniforms chain c may consume
    if (rng_mode == BMC_RNG_REPLAY) {
        bool bad = !xi || !g || !n_unif || unif_ld < 0;
        int64_t most = 0;
        for (size_t i = 0; !bad && i < C; ++i) {
            nu[i] = n_unif[i];
            bad = nu[i] < 0 || nu[i] > unif_ld;
            if (nu[i] > most) most = nu[i];
        }
        if (bad || (most > 0 && !unif)) return fail(c, BMC_EINVAL, "xi, g and unif required in replay mode");
    } else if (rng_mode == BMC_RNG_DEVICE) {
        if (xi || g || unif) return fail(c, BMC_EINVAL, "xi/g/unif must be NULL in device RNG mode");
        if (!seeds) return fail(c, BMC_EINVAL, "seeds required in device RNG mode");
    } else {
        return fail(c, BMC_EINVAL, "rng_mode must be 0 or 1");
    }
    HIPCHK(c, hipSetDevice(c->device));
    const int K = c->k;
    const size_t Tt = (size_t)(burn + iters);
    int rc;
    // -log_likelihood at beta = 0 (inference_utils.py:83-85) through the residual kernel: every
    // chain starts there (:82)
    std::vector<double> zero(K, 0.0);
    double rss0 = 0.0;
    if ((rc = rss_on_raw(c, zero.data(), 1, &rss0))) return rc;
    if (rng_mode == BMC_RNG_DEVICE) {
        unif_ld = (int64_t)Tt;
        for (size_t i = 0; i < C; ++i) nu[i] = (int64_t)Tt;
    }
    const size_t uld = (size_t)unif_ld;
    if ((rc = ensure_all(c, {{c->xi, C * Tt * K * 8}, {c->gam, C * Tt * 8},
                             {c->sVt, (size_t)K * Km * 8}, {c->sStep, (size_t)K * 8},
                             {c->sOut, C * (size_t)iters * (K + 1) * 8}, {c->sCnt, C * 16 + 48},
                             {c->sNUnif, C * 8}, {c->status, C * 4 + 12},
                             {c->placement, C * 4 + 12}, {c->seeds, C * 8 + 8},
                             {c->sUnif, (C * uld > 0 ? C * uld : 1) * 8}})))
        return rc;
    std::vector<double> step(K);
    for (int j = 0; j < K; ++j) step[j] = std::sqrt(S_hat[j] * S_hat[j] * stepsize * stepsize);  // :80
    if ((rc = check_tuning_fits(c))) return rc;
    // the geometry of ONE chain (a model per lane in the one-wave form) and the chains' launches
    const SimplexPlan plan = plan_simplex_launches(shape_of(c), c->tune, chip_of(c), Km, n_chains);
    const Geometry& geo = plan.geo;
    const int gran_stride = bmc::gran_slot_words(geo.G);
    const size_t gran_chain = (size_t)3 * gran_stride * 8;   // bytes of one chain's exchange words
    if ((rc = ensure(c, c->gran, (size_t)plan.max_per_launch * gran_chain))) return rc;
    HIPCHK(c, hipMemsetAsync(c->status.p, 0, C * 4 + 12, c->stream));
    HIPCHK(c, hipMemsetAsync(c->placement.p, 0, C * 4 + 12, c->stream));
    HIPCHK(c, hipMemsetAsync(c->sCnt.p, 0, C * 16 + 48, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->sVt.p, Vt_hat, (size_t)K * Km * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->sStep.p, step.data(), (size_t)K * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->sNUnif.p, nu.data(), C * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
    if (Tt > 0) {
        // chain c: the three streams of DESIGN.md 6 under its own seed, whatever its index
        const double shape = (nu0 + (double)c->n) / 2.0;                       // :115
        if ((rc = stage_variates(c, rng_mode, seeds, n_chains, Tt, shape, xi, g))) return rc;
        if (rng_mode == BMC_RNG_DEVICE)
            HIPCHK(c, launch_uniform_fill_chains((const uint64_t*)c->seeds.p, n_chains, unif_ld, unif_ld,
                                                 (double*)c->sUnif.p, c->stream));
        else if (C * uld > 0)
            HIPCHK(c, hipMemcpyAsync(c->sUnif.p, unif, C * uld * 8, hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
    SimplexArgs a;
    a.P = panels_of(c, c->Xraw.p);
    a.Vt = (const double*)c->sVt.p;
    a.Km = Km;
    a.vt_in_lds = (size_t)K * Km <= 4096;
    a.step = (const double*)c->sStep.p;
    a.nu0_s20 = nu0 * sigma20;
    a.rss_init = rss0;
    a.unif_ld = unif_ld;
    set_geometry(c, geo, gran_stride, iters, a);
    a.burn = burn;
    a.n_chains = 1;
    a.waves = geo.waves;
    a.nslot = geo.nslot;
    if (a.vt_in_lds && simplex_lds_bytes(a) > LDS_LIMIT) a.vt_in_lds = 0;
    if (simplex_lds_bytes(a) > LDS_LIMIT) return fail(c, BMC_EINVAL, "LDS plan exceeds 160 KiB");
    int launches = 0;
    for (size_t i = 0; Tt > 0 && i < plan.launches.size(); ++i) {
        const SimplexLaunch& l = plan.launches[i];
        const size_t c0 = (size_t)l.c0;
        a.n_chains = l.n_chains;
        a.nslot = l.nslot;
        a.xi = (const double*)c->xi.p + c0 * Tt * K;
        a.gam = (const double*)c->gam.p + c0 * Tt;
        a.unif = (const double*)c->sUnif.p + c0 * uld;
        a.n_unif = (const int64_t*)c->sNUnif.p + c0;
        a.out = (double*)c->sOut.p + c0 * (size_t)iters * (K + 1);
        a.status = (int32_t*)c->status.p + c0;
        a.placement = (int32_t*)c->placement.p + c0;
        a.counters = (long long*)c->sCnt.p + 2 * c0;
        if ((rc = begin_launch(c, simplex_kernel(a), (uint64_t)Tt, (size_t)l.n_chains * gran_chain,
                               a.G > 1 ? l.resident : 0,   // (a single-workgroup chain waits for nobody)
                               "persistent simplex kernel", &a.epoch0)))
            return rc;
        HIPCHK(c, launch_simplex(a, c->stream));
        ++launches;
    }
    HIPCHK(c, hipEventRecord(c->ev[2], c->stream));
    std::vector<int32_t> st(C, 0), place(C, 0);
    std::vector<long long> cnt(2 * C, 0);
    if ((rc = read_chain_words(c, st, place))) return rc;
    HIPCHK(c, hipMemcpyAsync(cnt.data(), c->sCnt.p, C * 16, hipMemcpyDeviceToHost, c->stream));
    if (iters > 0)
        HIPCHK(c, hipMemcpyAsync(samples_out, c->sOut.p, C * (size_t)iters * (K + 1) * 8,
                                 hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int64_t used_all = 0;
    for (size_t i = 0; i < C; ++i) {
        if (accepted_out) accepted_out[i] = cnt[2 * i];
        if (unif_used_out) unif_used_out[i] = cnt[2 * i + 1];
        used_all += cnt[2 * i + 1];
    }
    if (stats) {
        if ((rc = common_stats(c, stats, 2, n_chains, launches, geo.G, place))) return rc;
        stats->iterations = burn + iters;
        stats->waves_per_group = geo.waves;
        stats->chains_per_pass = 1;
        stats->residency = geo.mode + 1;
        stats->passes = used_all;
    }
    // the first failing chain is named when the call has more than one
    for (size_t i = 0; i < C; ++i) {
        const std::string which = n_chains > 1 ? " (chain " + std::to_string(i) + ")" : "";
        if (st[i] == 1) return fail(c, BMC_ETIMEOUT, "persistent simplex kernel: bounded spin expired" + which);
        if (st[i] == 2)
            return fail(c, BMC_EINVAL, "replay: fewer uniforms supplied than proposals inside the simplex" + which);
    }
    return BMC_OK;
}

// one chain: the C = 1 case of bmc_simplex_run_chains
int bmc_simplex_run(bmc_ctx* c, const double* Vt_hat, int32_t Km, const double* S_hat,
                    int64_t iters, int64_t burn, double stepsize, double nu0, double sigma20,
                    int rng_mode, uint64_t seed, const double* xi, const double* unif,
                    int64_t n_unif, const double* g, double* samples_out, int64_t* accepted_out,
                    int64_t* unif_used_out, bmc_stats* stats) {
    return bmc_simplex_run_chains(c, Vt_hat, Km, S_hat, 1, iters, burn, stepsize, nu0, sigma20, rng_mode,
                                  &seed, xi, unif, n_unif, &n_unif, g, samples_out, accepted_out,
                                  unif_used_out, stats);
}

}  // extern "C"
