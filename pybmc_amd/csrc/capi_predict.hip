// C ABI, posterior predictive: bmc_predict, its draws and its timing (kernels_predict.hip)
#include "bmc_ctx.h"

#include <cmath>
#include <vector>

namespace {

// which noise a predictive call asks for: bmc_predict (normals: generated or replayed),
// bmc_predict_t (one nu), bmc_predict_tv (a nu per draw)
enum PredictNoise { NOISE_NORMAL, NOISE_T, NOISE_TV };

// below 0.06 the largest |t| = sqrt(nu) 2^(53/nu) nears the end of the doubles (+-inf below about
// 0.052) and the order statistics would interpolate inf - inf
bool nu_ok(double nu) { return std::isfinite(nu) && nu >= 0.06; }

// the one driver of bmc_predict, bmc_predict_t and bmc_predict_tv
int predict_run(bmc_ctx* c, const double* preds, int64_t M, int32_t Km, const double* theta,
                int32_t S, int32_t k, const double* Vt_hat, int rng_mode, uint64_t seed,
                const double* noise, PredictNoise kind, double nu, const double* nu_draws,
                const int32_t* q_index, const double* q_gamma, int32_t n_q,
                const double* truth, const int32_t* cov_lo, const int32_t* cov_hi, int32_t n_cov,
                double* rndm_m_out, double* bands_out, int64_t* cov_hits_out) {
    if (!c) return BMC_EINVAL;
    if (!preds || !theta || !Vt_hat) return fail(c, BMC_EINVAL, "preds/theta/Vt_hat must not be NULL");
    if (M < 1 || Km < 1 || k < 1 || S < 1) return fail(c, BMC_EINVAL, "empty predictive problem");
    // (the limits of plan_predict_orderstat, bmc_plan.h)
    if (S > PREDICT_MAX_DRAWS) return fail(c, BMC_EINVAL, "n_draws > 16384 is not supported");
    if (n_q < 0 || n_q > PREDICT_MAX_Q || n_cov < 0 || n_cov > PREDICT_MAX_COV)
        return fail(c, BMC_EINVAL, "n_q and n_cov must be in 0..64");
    if (n_q > 0 && (!q_index || !q_gamma || !bands_out))
        return fail(c, BMC_EINVAL, "order statistics requested without index/gamma/output");
    if (n_cov > 0 && (!truth || !cov_lo || !cov_hi || !cov_hits_out))
        return fail(c, BMC_EINVAL, "coverage requested without truth/bounds/output");
    if (rng_mode == BMC_RNG_REPLAY ? !noise : noise != nullptr)
        return fail(c, BMC_EINVAL, "noise must be given exactly in replay mode");
    if (rng_mode != BMC_RNG_REPLAY && rng_mode != BMC_RNG_DEVICE)
        return fail(c, BMC_EINVAL, "rng_mode must be 0 or 1");
    if (kind == NOISE_T && !nu_ok(nu))
        return fail(c, BMC_EINVAL, "nu must be finite and at least 0.06");
    if (kind == NOISE_TV) {
        if (!nu_draws) return fail(c, BMC_EINVAL, "nu_draws must not be NULL");
        for (int32_t s = 0; s < S; ++s)
            if (!nu_ok(nu_draws[s]))
                return fail(c, BMC_EINVAL, "every nu_draws[s] must be finite and at least 0.06");
    }
    for (int i = 0; i < n_q; ++i)
        if (q_index[i] < 0 || q_index[i] >= S) return fail(c, BMC_EINVAL, "q_index out of range");
    for (int i = 0; i < n_cov; ++i)
        if (cov_lo[i] < 0 || cov_lo[i] >= S || cov_hi[i] < 0 || cov_hi[i] >= S)
            return fail(c, BMC_EINVAL, "coverage index out of range");
    HIPCHK(c, hipSetDevice(c->device));
    c->pM = 0;   // (no draws to fetch until this call has produced them)
    PredictArgs a;
    a.M = M; a.Km = Km; a.k = k; a.S = S;
    a.S_pad = (S + 63) / 64 * 64;
    a.Km_pad = (Km + 3) / 4 * 4;
    a.M_pad = (M + 63) / 64 * 64;
    a.seed = seed;
    a.n_q = n_q; a.n_cov = n_cov;
    const size_t szP = (size_t)M * Km * 8, szT = (size_t)S * (k + 1) * 8, szV = (size_t)k * Km * 8;
    int rc;
    if ((rc = ensure_all(c, {{c->pPreds, szP}, {c->pTheta, szT}, {c->pVt, szV},
                             {c->pWt, ((size_t)a.S_pad * a.Km_pad + 16) * 8},
                             {c->pPad, ((size_t)a.M_pad * a.Km_pad + 16) * 8},
                             {c->pSig, (size_t)3 * a.S_pad * 8},   // sig | nu_s | 2 / nu_s
                             {c->pR, (size_t)a.M_pad * a.S_pad * 8},
                             {c->pBands, (size_t)(n_q > 0 ? n_q : 1) * M * 8}})))
        return rc;
    // aux block: q_index[64] i32 | cov_lo[64] | cov_hi[64] | q_gamma[64] f64 | hits[64] u64 |
    //            fail_count (16 B) | truth[M] f64 | fail_points[M] i32
    const size_t offQ = 0, offLo = 256, offHi = 512, offG = 768, offH = 768 + 512, offFC = offH + 512;
    const size_t offT = offFC + 16, offFP = offT + (size_t)M * 8;
    if ((rc = ensure(c, c->pAux, offFP + (size_t)M * 4))) return rc;
    char* aux = (char*)c->pAux.p;
    HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
    HIPCHK(c, hipMemsetAsync(aux, 0, offT, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->pPreds.p, preds, szP, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->pTheta.p, theta, szT, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->pVt.p, Vt_hat, szV, hipMemcpyHostToDevice, c->stream));
    if (n_q) {
        HIPCHK(c, hipMemcpyAsync(aux + offQ, q_index, n_q * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(aux + offG, q_gamma, n_q * 8, hipMemcpyHostToDevice, c->stream));
    }
    if (n_cov) {
        HIPCHK(c, hipMemcpyAsync(aux + offLo, cov_lo, n_cov * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(aux + offHi, cov_hi, n_cov * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(aux + offT, truth, (size_t)M * 8, hipMemcpyHostToDevice, c->stream));
    }
    a.noise_replay = nullptr;
    if (noise) {
        if ((rc = ensure(c, c->pNoise, (size_t)S * M * 8))) return rc;
        HIPCHK(c, hipMemcpyAsync(c->pNoise.p, noise, (size_t)S * M * 8, hipMemcpyHostToDevice, c->stream));
        a.noise_replay = (const double*)c->pNoise.p;
    }
    // nu_s and 2 / nu_s behind sig, 2 / nu_s rounded here, once per value (one value per draw
    // then gives the bits of the one-nu call); the padded draws: 4 and 1/2
    std::vector<double> nus;   // (lives until the stream is synchronised)
    if (kind == NOISE_T) a.nu = nu;
    if (kind == NOISE_TV) {
        nus.resize((size_t)2 * a.S_pad);
        for (int32_t s = 0; s < a.S_pad; ++s) {
            nus[s] = s < S ? nu_draws[s] : 4.0;
            nus[(size_t)a.S_pad + s] = 2.0 / nus[s];
        }
        double* d_nus = (double*)c->pSig.p + a.S_pad;
        HIPCHK(c, hipMemcpyAsync(d_nus, nus.data(), nus.size() * 8, hipMemcpyHostToDevice, c->stream));
        a.nus = d_nus;
    }
    a.preds = (const double*)c->pPreds.p;
    a.theta = (const double*)c->pTheta.p;
    a.Vt = (const double*)c->pVt.p;
    a.Wt = (double*)c->pWt.p;
    a.P = (double*)c->pPad.p;
    a.sig = (double*)c->pSig.p;
    a.R = (double*)c->pR.p;
    a.q_index = (const int32_t*)(aux + offQ);
    a.q_gamma = (const double*)(aux + offG);
    a.truth = n_cov ? (const double*)(aux + offT) : nullptr;
    a.cov_lo = (const int32_t*)(aux + offLo);
    a.cov_hi = (const int32_t*)(aux + offHi);
    a.bands = (double*)c->pBands.p;
    a.hits = (unsigned long long*)(aux + offH);
    a.fail_count = (int32_t*)(aux + offFC);
    a.fail_points = (int32_t*)(aux + offFP);
    a.ev_mid = c->ev[2];
    HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
    HIPCHK(c, launch_predict(a, c->stream));
    HIPCHK(c, hipEventRecord(c->ev[3], c->stream));
    if (n_q)
        HIPCHK(c, hipMemcpyAsync(bands_out, c->pBands.p, (size_t)n_q * M * 8, hipMemcpyDeviceToHost,
                                 c->stream));
    if (n_cov)
        HIPCHK(c, hipMemcpyAsync(cov_hits_out, aux + offH, (size_t)n_cov * 8, hipMemcpyDeviceToHost,
                                 c->stream));
    if (rndm_m_out)
        HIPCHK(c, hipMemcpy2DAsync(rndm_m_out, (size_t)S * 8, c->pR.p, (size_t)a.S_pad * 8,
                                   (size_t)S * 8, (size_t)M, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if ((rc = event_ms(c, 0, 1, &c->predict_ms[0])) || (rc = event_ms(c, 1, 2, &c->predict_ms[1])) ||
        (rc = event_ms(c, 2, 3, &c->predict_ms[2])) || (rc = event_ms(c, 0, 3, &c->predict_ms[3])))
        return rc;
    c->pM = M;
    c->pS = S;
    c->pS_pad = a.S_pad;
    return BMC_OK;
}

}  // namespace

extern "C" {

int bmc_predict(bmc_ctx* c, const double* preds, int64_t M, int32_t Km, const double* theta,
                int32_t S, int32_t k, const double* Vt_hat, int rng_mode, uint64_t seed,
                const double* noise, const int32_t* q_index, const double* q_gamma, int32_t n_q,
                const double* truth, const int32_t* cov_lo, const int32_t* cov_hi, int32_t n_cov,
                double* rndm_m_out, double* bands_out, int64_t* cov_hits_out) {
    return predict_run(c, preds, M, Km, theta, S, k, Vt_hat, rng_mode, seed, noise, NOISE_NORMAL, 0.0,
                       nullptr, q_index, q_gamma, n_q, truth, cov_lo, cov_hi, n_cov, rndm_m_out,
                       bands_out, cov_hits_out);
}

int bmc_predict_t(bmc_ctx* c, const double* preds, int64_t M, int32_t Km, const double* theta,
                  int32_t S, int32_t k, const double* Vt_hat, uint64_t seed, const int32_t* q_index,
                  const double* q_gamma, int32_t n_q, const double* truth, const int32_t* cov_lo,
                  const int32_t* cov_hi, int32_t n_cov, double* rndm_m_out, double* bands_out,
                  int64_t* cov_hits_out, double nu) {
    return predict_run(c, preds, M, Km, theta, S, k, Vt_hat, BMC_RNG_DEVICE, seed, nullptr, NOISE_T,
                       nu, nullptr, q_index, q_gamma, n_q, truth, cov_lo, cov_hi, n_cov, rndm_m_out,
                       bands_out, cov_hits_out);
}

int bmc_predict_tv(bmc_ctx* c, const double* preds, int64_t M, int32_t Km, const double* theta,
                   int32_t S, int32_t k, const double* Vt_hat, uint64_t seed, const int32_t* q_index,
                   const double* q_gamma, int32_t n_q, const double* truth, const int32_t* cov_lo,
                   const int32_t* cov_hi, int32_t n_cov, double* rndm_m_out, double* bands_out,
                   int64_t* cov_hits_out, const double* nu_draws) {
    return predict_run(c, preds, M, Km, theta, S, k, Vt_hat, BMC_RNG_DEVICE, seed, nullptr, NOISE_TV,
                       0.0, nu_draws, q_index, q_gamma, n_q, truth, cov_lo, cov_hi, n_cov, rndm_m_out,
                       bands_out, cov_hits_out);
}

int bmc_predict_draws(bmc_ctx* c, double* out, int layout) {
    if (!c) return BMC_EINVAL;
    if (!out) return fail(c, BMC_EINVAL, "out must not be NULL");
    if (layout != BMC_DRAWS_BY_POINT && layout != BMC_DRAWS_BY_DRAW)
        return fail(c, BMC_EINVAL, "layout must be 0 (by point) or 1 (by draw)");
    if (c->pM < 1 || !c->pR.p) return fail(c, BMC_ESTATE, "no bmc_predict has run on this context");
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t M = c->pM;
    const int32_t S = c->pS, S_pad = c->pS_pad;
    int rc;
    if (layout == BMC_DRAWS_BY_POINT)
        return copy_to_host(c, out, c->pR.p, (size_t)S * 8, (size_t)S_pad * 8, (size_t)M);
    if ((rc = ensure(c, c->pRT, (size_t)S * M * 8))) return rc;
    HIPCHK(c, launch_transpose_draws((const double*)c->pR.p, M, S, S_pad, (double*)c->pRT.p,
                                     c->stream));
    // (rows of one draw: M doubles each, dense)
    return copy_to_host(c, out, c->pRT.p, (size_t)M * 8, (size_t)M * 8, (size_t)S);
}

int bmc_predict_timing(bmc_ctx* c, double* h2d_ms, double* gemm_ms, double* orderstat_ms,
                       double* device_ms) {
    if (!c) return BMC_EINVAL;
    if (h2d_ms) *h2d_ms = c->predict_ms[0];
    if (gemm_ms) *gemm_ms = c->predict_ms[1];
    if (orderstat_ms) *orderstat_ms = c->predict_ms[2];
    if (device_ms) *device_ms = c->predict_ms[3];
    return BMC_OK;
}

}  // extern "C"
