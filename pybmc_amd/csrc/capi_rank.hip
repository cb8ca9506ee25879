// C ABI, rank-normalised chain diagnostics: folded split R-hat, bulk / tail ESS and quantiles
// (Vehtari et al. 2021).  The ranks and the four derived series of every
// column are made on the device (kernels_rank.hip); the classic estimator (capi_diag.hip,
// diag_run) then runs on them unchanged.
#include <algorithm>
#include <cmath>

#include "bmc_ctx.h"

namespace {

constexpr double RANK_TAIL_LO = 0.05, RANK_TAIL_HI = 0.95;

struct RankEvents {
    hipEvent_t e[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    ~RankEvents() {
        for (auto& x : e)
            if (x) (void)hipEventDestroy(x);
    }
};

struct RankBatch {
    RankShape sh;
    uint64_t* key[2];
    uint32_t* idx[2];
    uint32_t* hist;
    double* der;
    double* q;          // [Pb][RANK_Q_SLOTS]
    uint64_t* or_and;   // [Pb][2]
    uint32_t* flags;    // [Pb]
};

int rank_buffers(bmc_ctx* c, const RankPlan& p, const RankShape& sh, size_t der_bytes, RankBatch& b) {
    RankPlan pb = p;
    rank_scratch(pb, sh.Pb);
    int rc = ensure_all(c, {{c->rkKey[0], pb.bytes_keys}, {c->rkKey[1], pb.bytes_keys},
                            {c->rkIdx[0], pb.bytes_idx}, {c->rkIdx[1], pb.bytes_idx},
                            {c->rkHist, pb.bytes_hist}, {c->rkDer, der_bytes},
                            {c->rkSmall, pb.bytes_small}});
    if (rc) return rc;
    b.sh = sh;
    for (int i = 0; i < 2; ++i) {
        b.key[i] = (uint64_t*)c->rkKey[i].p;
        b.idx[i] = (uint32_t*)c->rkIdx[i].p;
    }
    b.hist = (uint32_t*)c->rkHist.p;
    b.der = (double*)c->rkDer.p;
    b.q = (double*)c->rkSmall.p;
    b.or_and = (uint64_t*)(b.q + (size_t)sh.Pb * RANK_Q_SLOTS);
    b.flags = (uint32_t*)(b.or_and + (size_t)sh.Pb * 2);
    return BMC_OK;
}

// The LSD passes of the digits that differ inside some segment, from buffer `cur` on; `cur` is
// the buffer that holds the sorted pairs afterwards.  Blocks for the masks of the pass before.
int rank_sort(bmc_ctx* c, const RankBatch& b, int& cur) {
    std::vector<uint64_t> oa((size_t)b.sh.Pb * 2);
    HIPCHK(c, hipMemcpyAsync(oa.data(), b.or_and, oa.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint32_t live = rank_live_passes(oa.data(), b.sh.Pb);
    for (int d = 0; d < RANK_PASSES; ++d) {
        if (!((live >> d) & 1)) continue;
        HIPCHK(c, launch_rank_sort_pass(b.sh, d, b.key[cur], b.idx[cur], b.key[cur ^ 1], b.idx[cur ^ 1],
                                        b.hist, c->stream));
        cur ^= 1;
    }
    return BMC_OK;
}

RankShape rank_shape(const RankPlan& p, const double* dx, int32_t C, int64_t iters, int64_t ld,
                     int64_t burn, int32_t col0, int32_t Pb) {
    RankShape sh;
    sh.x = dx;
    sh.iters = iters;
    sh.ld = ld;
    sh.burn = burn;
    sh.n = p.n;
    sh.half_off = (iters - burn) - p.n;
    sh.S = p.S;
    sh.tiles = p.tiles;
    sh.C = C;
    sh.col0 = col0;
    sh.Pb = Pb;
    return sh;
}

size_t rank_budget(bmc_ctx* c, size_t* out) {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return 1;
    // what the context already holds for this leg is reused; the classic leg's scratch and the
    // allocator's slack come out of the rest
    const size_t held = c->rkKey[0].cap + c->rkKey[1].cap + c->rkIdx[0].cap + c->rkIdx[1].cap +
                        c->rkHist.cap + c->rkDer.cap + c->rkSmall.cap;
    *out = (size_t)((double)(free_b + held) * 0.8);
    return 0;
}

int rank_run(bmc_ctx* c, const double* dx, int32_t C, int64_t iters, int32_t P, int64_t ld, int64_t burn,
             const double* probs, int32_t n_probs, int32_t cols_per_batch, double* mean_out,
             double* sd_out, double* q_out, double* rhat_out, double* bulk_out, double* tail_out,
             double* mcse_out) {
    size_t budget = 0;
    if (rank_budget(c, &budget)) return fail(c, BMC_EHIP, "hipMemGetInfo failed");
    const RankPlan p = plan_rank(C, iters, P, ld, burn, probs, n_probs, cols_per_batch, budget);
    if (!p.ok) return fail(c, p.S == 0 ? BMC_EINVAL : BMC_ENOMEM, p.why);
    RankEvents ev;
    for (auto& e : ev.e) HIPCHK(c, hipEventCreate(&e));
    for (double& m : c->rank_ms) m = 0;
    int rc;

    // mean and sd: the classic leg's moments of the samples themselves (the same bits)
    std::vector<double> sd(P);
    HIPCHK(c, hipEventRecord(ev.e[0], c->stream));
    if ((rc = diag_run(c, dx, C, iters, P, ld, burn, mean_out, sd.data(), nullptr, nullptr, nullptr,
                       nullptr)))
        return rc;
    HIPCHK(c, hipEventRecord(ev.e[1], c->stream));
    HIPCHK(c, hipEventSynchronize(ev.e[1]));
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
    c->rank_ms[3] = ms;
    if (sd_out) std::copy(sd.begin(), sd.end(), sd_out);

    RankQuantiles rq;
    rq.n = n_probs + RANK_Q_INTERNAL;
    const double tail[RANK_Q_INTERNAL] = {RANK_TAIL_LO, 0.5, RANK_TAIL_HI};
    for (int t = 0; t < rq.n; ++t)
        rank_order_stat(p.S, t < n_probs ? probs[t] : tail[t - n_probs], &rq.index[t], &rq.weight[t]);
    const int32_t s_lo = n_probs, s_med = n_probs + 1, s_hi = n_probs + 2;
    const double nan = std::nan("");

    for (int32_t bi = 0; bi < p.n_batches; ++bi) {
        int32_t col0, Pb;
        rank_batch(p, P, bi, &col0, &Pb);
        const RankShape sh = rank_shape(p, dx, C, iters, ld, burn, col0, Pb);
        // every column's four series in a buffer [C][2n][4] of its own: the classic leg then runs
        // column by column on the same shape whatever the batch, so its bits (its row splits
        // follow the column count) do not depend on cols_per_batch
        const int64_t ld_d = RANK_SERIES, seg = p.S * ld_d;
        RankBatch b;
        if ((rc = rank_buffers(c, p, sh, (size_t)seg * Pb * 8, b))) return rc;
        int cur = 0;
        HIPCHK(c, hipEventRecord(ev.e[0], c->stream));
        HIPCHK(c, launch_rank_gather(sh, b.key[0], b.idx[0], b.or_and, b.flags, c->stream));
        if ((rc = rank_sort(c, b, cur))) return rc;
        HIPCHK(c, hipEventRecord(ev.e[1], c->stream));
        HIPCHK(c, launch_rank_pick(sh, b.key[cur], rq, b.q, c->stream));
        HIPCHK(c, launch_rank_z(sh, b.key[cur], b.idx[cur], b.der, seg, ld_d, 0, c->stream));
        HIPCHK(c, hipEventRecord(ev.e[2], c->stream));
        HIPCHK(c, launch_rank_fold(sh, b.key[cur], b.q, s_med, b.or_and, c->stream));
        if ((rc = rank_sort(c, b, cur))) return rc;
        HIPCHK(c, hipEventRecord(ev.e[3], c->stream));
        HIPCHK(c, launch_rank_z(sh, b.key[cur], b.idx[cur], b.der, seg, ld_d, 1, c->stream));
        HIPCHK(c, launch_rank_indicators(sh, b.q, s_lo, s_hi, b.der, seg, ld_d, 2, 3, c->stream));
        HIPCHK(c, hipEventRecord(ev.e[4], c->stream));
        std::vector<double> rh((size_t)ld_d * Pb), es((size_t)ld_d * Pb), q((size_t)Pb * RANK_Q_SLOTS);
        std::vector<uint32_t> flags(Pb);
        for (int32_t jb = 0; jb < Pb; ++jb)
            if ((rc = diag_run(c, b.der + (size_t)jb * seg, C, 2 * p.n, (int32_t)ld_d, ld_d, 0, nullptr,
                               nullptr, rh.data() + jb * ld_d, es.data() + jb * ld_d, nullptr, nullptr)))
                return rc;
        HIPCHK(c, hipMemcpyAsync(q.data(), b.q, q.size() * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(flags.data(), b.flags, flags.size() * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipEventRecord(ev.e[5], c->stream));
        HIPCHK(c, hipEventSynchronize(ev.e[5]));
        const int span[5] = {0, 1, 0, 1, 2};    // sort, rank, sort, rank, classic
        for (int i = 0; i < 5; ++i) {
            HIPCHK(c, hipEventElapsedTime(&ms, ev.e[i], ev.e[i + 1]));
            c->rank_ms[span[i]] += ms;
        }
        for (int32_t jb = 0; jb < Pb; ++jb) {
            const int32_t j = col0 + jb;
            const bool bad = flags[jb] != 0;
            // NaN when either side is: a derived series with W = 0 takes its outputs with it
            const double r0 = rh[4 * jb], r1 = rh[4 * jb + 1], t0 = es[4 * jb + 2], t1 = es[4 * jb + 3];
            const double rhat = bad || std::isnan(r0) || std::isnan(r1) ? nan : std::max(r0, r1);
            const double bulk = bad ? nan : es[4 * jb];
            const double tl = bad || std::isnan(t0) || std::isnan(t1) ? nan : std::min(t0, t1);
            if (rhat_out) rhat_out[j] = rhat;
            if (bulk_out) bulk_out[j] = bulk;
            if (tail_out) tail_out[j] = tl;
            if (mcse_out) mcse_out[j] = sd[j] / std::sqrt(bulk);
            if (q_out)
                for (int32_t t = 0; t < n_probs; ++t)
                    q_out[(size_t)t * P + j] = bad ? nan : q[(size_t)jb * RANK_Q_SLOTS + t];
        }
    }
    return BMC_OK;
}

int rank_normalize_run(bmc_ctx* c, const double* dx, int32_t C, int64_t iters, int32_t P, int64_t ld,
                       int64_t burn, int folded, double* z_out) {
    if (!z_out) return fail(c, BMC_EINVAL, "z_out must not be NULL");
    size_t budget = 0;
    if (rank_budget(c, &budget)) return fail(c, BMC_EHIP, "hipMemGetInfo failed");
    const RankPlan p = plan_rank(C, iters, P, ld, burn, nullptr, 0, 0, budget);
    if (!p.ok) return fail(c, p.S == 0 ? BMC_EINVAL : BMC_ENOMEM, p.why);
    RankQuantiles rq;
    rq.n = 1;
    rank_order_stat(p.S, 0.5, &rq.index[0], &rq.weight[0]);
    int rc;
    for (int32_t bi = 0; bi < p.n_batches; ++bi) {
        int32_t col0, Pb;
        rank_batch(p, P, bi, &col0, &Pb);
        const RankShape sh = rank_shape(p, dx, C, iters, ld, burn, col0, Pb);
        RankBatch b;
        // (the derived buffer of the plan, four series wide, covers the one series written here)
        if ((rc = rank_buffers(c, p, sh, (size_t)p.S * Pb * 8, b))) return rc;
        int cur = 0;
        HIPCHK(c, launch_rank_gather(sh, b.key[0], b.idx[0], b.or_and, b.flags, c->stream));
        if ((rc = rank_sort(c, b, cur))) return rc;
        if (folded) {
            HIPCHK(c, launch_rank_pick(sh, b.key[cur], rq, b.q, c->stream));
            HIPCHK(c, launch_rank_fold(sh, b.key[cur], b.q, 0, b.or_and, c->stream));
            if ((rc = rank_sort(c, b, cur))) return rc;
        }
        HIPCHK(c, launch_rank_z(sh, b.key[cur], b.idx[cur], b.der, 1, Pb, 0, c->stream));
        std::vector<uint32_t> flags(Pb);
        HIPCHK(c, hipMemcpyAsync(flags.data(), b.flags, flags.size() * 4, hipMemcpyDeviceToHost, c->stream));
        // rows of Pb values into columns col0 .. of the [S][P] result
        HIPCHK(c, hipMemcpy2DAsync(z_out + col0, (size_t)P * 8, b.der, (size_t)Pb * 8, (size_t)Pb * 8,
                                   (size_t)p.S, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (int32_t jb = 0; jb < Pb; ++jb)
            if (flags[jb])
                for (int64_t e = 0; e < p.S; ++e) z_out[(size_t)e * P + col0 + jb] = std::nan("");
    }
    return BMC_OK;
}

int stage_samples(bmc_ctx* c, const double* samples, int32_t n_chains, int64_t iters, int32_t n_cols,
                  int64_t ld) {
    // (the last row of a strided host array may be shorter than ld)
    const size_t bytes = ((size_t)((int64_t)n_chains * iters - 1) * ld + n_cols) * 8;
    int rc = ensure(c, c->dgIn, bytes);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->dgIn.p, samples, bytes, hipMemcpyHostToDevice, c->stream));
    return BMC_OK;
}

int check_rank_args(bmc_ctx* c, const void* x, int32_t n_chains, int64_t iters, int32_t n_cols, int64_t ld,
                    int64_t burn, const double* probs, int32_t n_probs, bool want_probs) {
    if (!c) return BMC_EINVAL;
    if (!x) return fail(c, BMC_EINVAL, "samples must not be NULL");
    if (want_probs && n_probs < 1) return fail(c, BMC_EINVAL, "need between 1 and 16 probabilities");
    const std::string why = rank_check(n_chains, iters, n_cols, ld, burn, probs, n_probs);
    if (!why.empty()) return fail(c, BMC_EINVAL, why);
    return BMC_OK;
}

}  // namespace

extern "C" {

int bmc_rank_diagnostics(bmc_ctx* c, const double* samples, int32_t n_chains, int64_t iters,
                         int32_t n_cols, int64_t ld, int64_t burn, const double* probs, int32_t n_probs,
                         int32_t cols_per_batch, double* mean_out, double* sd_out, double* quantiles_out,
                         double* rhat_out, double* ess_bulk_out, double* ess_tail_out, double* mcse_out) {
    int rc = check_rank_args(c, samples, n_chains, iters, n_cols, ld, burn, probs, n_probs, true);
    if (rc) return rc;
    if (cols_per_batch < 0) return fail(c, BMC_EINVAL, "cols_per_batch must be >= 0");
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = stage_samples(c, samples, n_chains, iters, n_cols, ld))) return rc;
    return rank_run(c, (const double*)c->dgIn.p, n_chains, iters, n_cols, ld, burn, probs, n_probs,
                    cols_per_batch, mean_out, sd_out, quantiles_out, rhat_out, ess_bulk_out, ess_tail_out,
                    mcse_out);
}

int bmc_rank_diagnostics_device(bmc_ctx* c, const void* d_samples, int32_t n_chains, int64_t iters,
                                int32_t n_cols, int64_t ld, int64_t burn, const double* probs,
                                int32_t n_probs, int32_t cols_per_batch, double* mean_out, double* sd_out,
                                double* quantiles_out, double* rhat_out, double* ess_bulk_out,
                                double* ess_tail_out, double* mcse_out) {
    int rc = check_rank_args(c, d_samples, n_chains, iters, n_cols, ld, burn, probs, n_probs, true);
    if (rc) return rc;
    if (cols_per_batch < 0) return fail(c, BMC_EINVAL, "cols_per_batch must be >= 0");
    HIPCHK(c, hipSetDevice(c->device));
    return rank_run(c, (const double*)d_samples, n_chains, iters, n_cols, ld, burn, probs, n_probs,
                    cols_per_batch, mean_out, sd_out, quantiles_out, rhat_out, ess_bulk_out, ess_tail_out,
                    mcse_out);
}

int bmc_rank_normalize(bmc_ctx* c, const double* samples, int32_t n_chains, int64_t iters, int32_t n_cols,
                       int64_t ld, int64_t burn, int folded, double* z_out) {
    int rc = check_rank_args(c, samples, n_chains, iters, n_cols, ld, burn, nullptr, 0, false);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = stage_samples(c, samples, n_chains, iters, n_cols, ld))) return rc;
    return rank_normalize_run(c, (const double*)c->dgIn.p, n_chains, iters, n_cols, ld, burn, folded, z_out);
}

int bmc_rank_normalize_device(bmc_ctx* c, const void* d_samples, int32_t n_chains, int64_t iters,
                              int32_t n_cols, int64_t ld, int64_t burn, int folded, double* z_out) {
    int rc = check_rank_args(c, d_samples, n_chains, iters, n_cols, ld, burn, nullptr, 0, false);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    return rank_normalize_run(c, (const double*)d_samples, n_chains, iters, n_cols, ld, burn, folded, z_out);
}

int bmc_rank_last_timing(bmc_ctx* c, double ms_out[4]) {
    if (!c || !ms_out) return BMC_EINVAL;
    for (int i = 0; i < 4; ++i) ms_out[i] = c->rank_ms[i];
    return BMC_OK;
}

}  // extern "C"
