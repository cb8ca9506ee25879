// The context behind the C ABI (include/pybmc_amd.h) and what its host files share.  Internal:
// not installed.  capi_*.hip hold the entry points, one feature family each; every function
// declared here is defined in capi_core.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>   // types only: the library itself is loaded on first use (bmc_comm_*)

#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/pybmc_amd.h"
#include "bmc_launch.h"
#include "bmc_plan.h"

using namespace bmc;

#pragma GCC visibility push(hidden)

// A device block that grows on demand (ensure) and frees itself.
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
};

// The stream, the events and the pinned staging.  A base of bmc_ctx, so that they are destroyed
// after its members: device memory goes first, as bmc_destroy has always done it.
struct CtxHandles {
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    // pinned staging for results that go back to pageable host memory (copy_to_host)
    void* hstage[2] = {nullptr, nullptr};
    hipEvent_t hev[2] = {nullptr, nullptr};
    ~CtxHandles() {
        for (auto& e : ev)
            if (e) (void)hipEventDestroy(e);
        for (int i = 0; i < 2; ++i) {
            if (hev[i]) (void)hipEventDestroy(hev[i]);
            if (hstage[i]) (void)hipHostFree(hstage[i]);
        }
        if (own_stream && stream) (void)hipStreamDestroy(stream);
    }
};

struct bmc_ctx : CtxHandles {
    int device = 0;
    std::string err;
    bmc_tuning tune{};
    int n_cu = 256;
    int env_cu_limit = 0;   // PYBMC_AMD_CU_LIMIT at bmc_create: the default of bmc_tuning.cu_limit
    uint64_t nonce_state = 0x9E3779B97F4A7C15ull;   // per-launch exchange nonces (launch_nonce)

    // problem
    bool have_problem = false, have_prior = false;
    int64_t n = 0;
    int32_t k = 0, vec = 1, npanels = 0, f32 = 0;
    DevBuf Xraw, Yp, Xrot;
    std::vector<double> gram;

    // prior / basis (host copies)
    std::vector<double> W, lam, c1, c2, b0;
    double nu0 = 0, s20 = 0, sigma2_init = 0;
    std::vector<double> Pprec, Pb0;   // inv(C0) and inv(C0) b0 (the Student-t sampler's operands)
    DevBuf dW, dWT, dLam, dC1, dC2;
    // sufficient statistics in the rotated basis (rss_mode 1; host part made by bmc_set_prior
    // when k <= 64, device part on first use)
    std::vector<double> Gt, u0, g0;
    bool have_gram_dev = false;
    double rss0 = 0;
    DevBuf dGt, dU0, dG0;

    // scratch
    DevBuf gramScratch, gramOut, rssPartial, rssOut, coef, stage, ticket;
    // run buffers
    DevBuf xi, gam, uout, samples, gran, status, seeds, dbg, placement;
    // the persistent loop kernels of the last bmc_gibbs_run* / bmc_simplex_run*, one name per
    // launch in launch order (bmc_last_kernels)
    std::vector<std::string> last_kernels;
    // predictive buffers
    DevBuf pPreds, pPad, pTheta, pVt, pWt, pSig, pR, pRT, pNoise, pAux, pBands;
    int64_t pM = 0;                        // last bmc_predict: points, draws, padded draws
    int32_t pS = 0, pS_pad = 0;
    DevBuf sVt, sStep, sUnif, sOut, sCnt, sNUnif;
    DevBuf oFc, oMu, oW, oOut;
    // chain diagnostics (bmc_chain_diagnostics*)
    DevBuf dgIn, dgPart, dgMean, dgM2, dgCols, dgAcovPart, dgAcov;
    // rank-normalised diagnostics (bmc_rank_*): the two (key, index) buffers of the sort, its
    // histograms, the derived series, and the quantiles / masks / flags of a batch
    DevBuf rkKey[2], rkIdx[2], rkHist, rkDer, rkSmall;
    double rank_ms[4] = {0, 0, 0, 0};      // last bmc_rank_diagnostics*: sort, rank, classic, moments
    // pointwise log-likelihood (bmc_pointwise_loglik*)
    DevBuf scA, scY, scTheta, scAp, scYp, scCh, scPart, scOut;
    DevBuf scNu;   // the _tv entry points: the table of distinct nu, the staged index, the flag word
    // PSIS-LOO (bmc_psis_loo*, bmc_psis_loo_predict*): the select state and candidate slots,
    // besides the score buffers
    DevBuf looWork;
    // posterior predictive check (bmc_ppc*): the staged offset, the padded operands and the results
    DevBuf ppcOff, ppcWork;
    // power-scaling sensitivity (bmc_power_sensitivity*): staged operands, log densities, weights
    // and the scan's partials (the sort reuses the rank buffers)
    DevBuf snStage, snWork, snPart;
    // Student-t sampler (bmc_robust_run*): the packed operand, the prior, per-chain row state, the
    // replayed weights' variates, the mean weights
    DevBuf rbZ, rbPrior, rbWs, rbGl, rbWsum;
    DevBuf rbNu;   // bmc_robust_run_nu*: the grid's table, T_t, the pick's uniforms, the indices, the path
    double sens_ms[4] = {0, 0, 0, 0};      // last bmc_power_sensitivity*: log densities, sorts, PSIS, CJS
    double predict_ms[4] = {0, 0, 0, 0};   // last bmc_predict: h2d, gemm, order statistics, device
    // pooling over GPUs (bmc_comm_*): RCCL communicator bound to this context's device
    ncclComm_t comm = nullptr;
    int32_t comm_world = 0, comm_rank = 0;
};

int fail(bmc_ctx* c, int code, const std::string& msg);

#define HIPCHK(ctx, expr)                                                              \
    do {                                                                               \
        hipError_t e__ = (expr);                                                       \
        if (e__ != hipSuccess)                                                         \
            return fail(ctx, e__ == hipErrorOutOfMemory ? BMC_ENOMEM : BMC_EHIP,       \
                        std::string(#expr) + ": " + hipGetErrorString(e__));           \
    } while (0)

// At least `bytes` in b (0 bytes means 16).  Grows only; the stream is synchronised before the
// old block is freed.
int ensure(bmc_ctx* c, DevBuf& b, size_t bytes);
// ensure() for each {buffer, bytes} in turn; the first error
struct Want {
    DevBuf& b;
    size_t bytes;
};
int ensure_all(bmc_ctx* c, std::initializer_list<Want> wants);
// what launch_residual_rss needs for n_out results: the partials, the results, the zeroed tickets
int ensure_rss(bmc_ctx* c, const Panels& P, size_t n_out);

// rows of `row_bytes` taken every `src_pitch` bytes on the device, written densely to `dst`
// (src_pitch == row_bytes: one contiguous block of row_bytes * rows).  Blocks until the data is
// in `dst`.
int copy_to_host(bmc_ctx* c, void* dst, const void* src_dev, size_t row_bytes, size_t src_pitch,
                 size_t rows);

// The panels of an n x k problem stored at X and y (f32: as floats): rows per lane by choose_vec
Panels make_panels(int64_t n, int32_t k, int32_t f32, const void* X, const void* y);
// those of the resident problem, with its columns at X
Panels panels_of(const bmc_ctx* c, const void* X);

// The least-squares start of a row set from its panels (the resident problem's, and every fold's
// training rows in bmc_kfold_cv_t).  gram_to_host: the Gram of [X y], (k+1) x (k+1); one sync.
// ols_start: A = X'X and xty = X'y out of it, the least-squares point (singular: A has no solve, and
// nothing further is computed), rss there by one launch_residual_rss, sigma2_init = sigma2_floor(rss / n)
int gram_to_host(bmc_ctx* c, const Panels& P, std::vector<double>& gram);
struct OlsStart {
    std::vector<double> A, xty, bols;
    bool singular = false;
    double rss = 0.0, sigma2_init = 0.0;
};
int ols_start(bmc_ctx* c, const Panels& P, const std::vector<double>& gram, OlsStart& o);
// max(s2, 1e-6); NaN propagates
inline double sigma2_floor(double s2) { return !(s2 >= 1e-6) && s2 == s2 ? 1e-6 : s2; }

// The host side of a NuPerDraw (bmc_launch.h).  stage_nu lays b out as [rows][V] f64 table of `shape`,
// [S] int32 staged index, one int32 flag word: the table up (one sync: it is a local), the flag
// zeroed, a host index copied behind the table; v names them (the index: the staged copy, else as
// given, a device pointer or NULL where the caller sets it later).
int stage_nu(bmc_ctx* c, DevBuf& b, NuTable shape, const double* values, int32_t V, int64_t S,
             const void* index, bool index_on_host, NuPerDraw& v);
// BMC_EINVAL unless every entry of a host index lies in [0, V)
int check_nu_index(bmc_ctx* c, const void* index, int64_t S, int32_t V);
// The flag word back: fetch queues the copy (nothing for an unset v); after the caller's next sync,
// result is BMC_EINVAL with the one message when an index was out of range
struct NuFlagRead {
    int32_t word = 0;
    int fetch(bmc_ctx* c, const NuPerDraw& v);
    int result(bmc_ctx* c) const;
};

// BMC_ESINGULAR for the first chain of the robust kernels whose status is not 0;
// say(i, what) is the message: how the caller names chain i around what happened
template <class Say>
int robust_status_check(bmc_ctx* c, const std::vector<int32_t>& st, Say say) {
    const std::string what = "a Cholesky pivot of X'LX / sigma2 + inv(C0) + 1e-6 I was not positive and finite";
    for (size_t i = 0; i < st.size(); ++i)
        if (st[i] != 0) return fail(c, BMC_ESINGULAR, say(i, what));
    return BMC_OK;
}

Shape shape_of(const bmc_ctx* c);
Chip chip_of(const bmc_ctx* c);
uint32_t launch_nonce(bmc_ctx* c, uint64_t n_tags);

// The classic split R-hat / ESS of device samples [C][iters][ld] (capi_diag.hip):
// what bmc_chain_diagnostics* run after their argument checks.  Every output is host [P] or NULL.
int diag_run(bmc_ctx* c, const double* dx, int32_t C, int64_t iters, int32_t P, int64_t ld,
             int64_t burn, double* mean_out, double* sd_out, double* rhat_out, double* ess_out,
             double* mcse_out, int64_t* max_lag_out);

// milliseconds from c->ev[from] to c->ev[to]
int event_ms(bmc_ctx* c, int from, int to, double* ms);

// bytes of an n x k host matrix of `es`-byte elements with leading dimension ld: the last row
// (column, when col-major) may be shorter than ld
size_t strided_bytes(int64_t n, int32_t k, int64_t ld, int layout, size_t es);

// rss of nb host coefficient vectors on the un-rotated panels -> out_host
int rss_on_raw(bmc_ctx* c, const double* coef_host, int32_t nb, double* out_host);

#pragma GCC visibility pop
