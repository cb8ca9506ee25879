/*
 * pybmc_amd.h -- C ABI of the MI355X-native Gibbs-sampling core for Bayesian
 * model combination (libpybmc_amd.so, gfx950 only).
 *
 * The reference (sudhanvalalit/pybmc) has no FFI: its boundary is three Python
 * call signatures.  Each entry point below names the reference interface it
 * replaces (file:line in the reference checkout).  INTEGRATION.md shows the
 * ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *   - plain pointers and sizes only; every HOST buffer is caller-owned, is read
 *     or written only during the call and is never retained;
 *   - every function returns a bmc_status (0 = OK); no exception, abort or
 *     longjmp crosses the ABI; bmc_last_error() gives the text;
 *   - a bmc_ctx belongs to one GPU and is driven by one host thread at a time;
 *     distinct contexts are independent (no global mutable state);
 *   - there is NO CPU fallback: without a usable gfx950 device bmc_create fails.
 */
#ifndef PYBMC_AMD_H
#define PYBMC_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PYBMC_AMD_ABI_VERSION 4

typedef struct bmc_ctx bmc_ctx;

typedef enum {
    BMC_OK = 0,
    BMC_EINVAL = 1,    /* bad argument            -> Python ValueError            */
    BMC_ESINGULAR = 2, /* singular C0 or X'X      -> numpy.linalg.LinAlgError     */
    BMC_EHIP = 3,      /* HIP runtime error       -> RuntimeError                 */
    BMC_ENOMEM = 4,    /* allocation failed       -> MemoryError                  */
    BMC_ETIMEOUT = 5,  /* bounded device spin expired (persistent kernel)         */
    BMC_ESTATE = 6     /* call order violated (e.g. run before set_prior)         */
} bmc_status;

enum { BMC_F64 = 0, BMC_F32 = 1 };           /* storage type of X and y        */
enum { BMC_ROW_MAJOR = 0, BMC_COL_MAJOR = 1 }; /* 1 = what U_hat is (F-order) */
enum { BMC_RNG_DEVICE = 0, BMC_RNG_REPLAY = 1 };

/* Launch geometry knobs (0 = let the library choose). */
typedef struct {
    int32_t groups_per_chain; /* workgroups that share one chain's rows        */
    int32_t waves_per_group;  /* 1..8 (workgroup = 64 * waves threads); 1 with no other knob set
                                 also asks for the one-wave-per-chain kernel wherever it exists
                                 (<= 1024 rows, rows/64 x columns <= 128; left to itself the
                                 library also runs such chains in 2, 4 or 8 waves, up to ~8000
                                 rows), > 1 keeps a small chain in the workgroup form */
    int32_t residency;        /* 0 auto, 1 registers, 2 LDS, 3 stream from HBM */
    int32_t panels_per_wave;  /* register residency: 1, 2 or 4 (1, asked for explicitly, also keeps
                                 bundles of 8 chains in the one-panel-per-wave layout instead of
                                 the balanced two-panel one; results are bit-identical) */
    int32_t force_agent_scope;/* 1 = never use the XCD-local (L2) exchange     */
    int32_t chains_per_pass;  /* chains served by one read of X (streamed / LDS-pinned panels) or by
                                 one set of register-resident panels (a chain over the whole chip; or,
                                 one-XCD shapes such as N = 10000 x 32 with 16 chains or more, a BUNDLE
                                 per XCD: 16 .. 64 chains per launch, each bit-identical to its solo
                                 run).  0 auto (up to 8; bundles from 4 chains per XCD on), 1 off,
                                 2/4/8 cap (2 also asks for bundles of 2)                            */
    int32_t rss_mode;         /* 0 (default): rss = sum (y - X beta)^2 by a pass over the data
                                 every iteration, as inference_utils.py:48-51 does.
                                 1 (opt-in, K <= 64): the same number from sufficient statistics,
                                 rss(u) = rss(u0) - 2 d'g0 + d'G d with d = u - u0, G = X~'X~,
                                 g0 = X~'(y - X~ u0) and u0 the least-squares point; no pass
                                 over the data inside the loop, one wave per chain          */
    int32_t cu_limit;         /* 0: the device's CU count.  > 0: plan as if only this many CUs could
                                 hold workgroups of a persistent launch (a CU-masked queue, a
                                 partition, a GPU shared with another process).  The persistent
                                 kernels need all groups of a launch resident at once; geometry and
                                 the residency check (BMC_EINVAL instead of a spin that times out)
                                 follow this number.  The environment variable
                                 PYBMC_AMD_CU_LIMIT, read by bmc_create, is the default for every
                                 context of the process (several ranks on one GPU: set each rank's
                                 share once, e.g. 128 for two)                                 */
} bmc_tuning;

/* Filled by bmc_gibbs_run*.  Times are HIP-event times on the context's stream. */
typedef struct {
    double loop_ms;           /* the persistent Gibbs kernel(s) only           */
    double rng_ms;            /* variate generation kernels (device RNG mode)  */
    double post_ms;           /* un-rotation of the draws into beta            */
    double total_ms;          /* first launch -> last kernel done              */
    int64_t iterations;       /* per chain                                     */
    int32_t n_chains;
    int32_t launches;         /* persistent-kernel launches (chain batches)    */
    int32_t groups_per_chain;
    int32_t waves_per_group;
    int32_t chains_per_pass;
    int32_t residency;        /* 1 registers, 2 LDS, 3 streamed, 4 none (rss_mode 1) */
    int32_t xcd_local_chains; /* chains whose groups were verified on one XCD  */
    int64_t bytes_per_pass;   /* algorithmic: (N*K + N) * sizeof(storage)      */
    int64_t passes;           /* X passes executed in total                    */
} bmc_stats;

/* ---- lifetime --------------------------------------------------------- */
int bmc_abi_version(void);
int bmc_create(int device_id, bmc_ctx** out);
void bmc_destroy(bmc_ctx* ctx);
const char* bmc_last_error(const bmc_ctx* ctx);     /* valid until next call  */
/* Use an existing HIP stream (e.g. torch's current stream); NULL = own stream. */
int bmc_set_stream(bmc_ctx* ctx, void* hip_stream);
int bmc_set_tuning(bmc_ctx* ctx, const bmc_tuning* t);

/* ---- problem: y (n,), X (n,k) ----------------------------------------------
 * Replaces the (y, X) arguments of gibbs_sampler, pybmc/inference_utils.py:4,
 * as passed by BayesianModelCombination.train, pybmc/bmc.py:188-193.
 * Element (i,j) of X is at X[i*ldx + j] (row-major) or X[i + j*ldx] (col-major,
 * the layout U_hat has after inference_utils.py:164).  On return the device
 * holds X, y, and the augmented Gram [X y]'[X y] (inference_utils.py:25 and the
 * loop-invariant X'y of :43), computed with f64 MFMA.
 * bmc_set_problem_device takes DEVICE pointers (same layouts). */
int bmc_set_problem(bmc_ctx* ctx, const void* X, int64_t n, int32_t k, int64_t ldx,
                    int layout, const void* y, int dtype);
int bmc_set_problem_device(bmc_ctx* ctx, const void* dX, int64_t n, int32_t k,
                           int64_t ldx, int layout, const void* dy, int dtype);

/* ---- orthogonalize on the device -----------------------------------------------------
 * Replaces the numerical part of BayesianModelCombination.orthogonalize,
 * pybmc/bmc.py:106-122, and USVt_hat_extraction, pybmc/inference_utils.py:147-168:
 *   mu = row mean of F over the models, y_c = truth - mu, Fc = F - mu          (:106-116)
 *   SVD of Fc through its Gram (f64 MFMA): Fc'Fc = V S^2 V', U_hat = Fc V_k S_k^-1   (:119,:164)
 * F is [n][n_models] with row stride ldf (host).  Outputs (any may be NULL): mean_out [n],
 * yc_out [n], U_hat_out [k][n] (= an (n,k) array in Fortran order, the layout of :164),
 * S_out [k], Vt_out [k][n_models] (rows of V'; Vt_hat of :166 is Vt_out[i] / S_out[i]).
 * Each right singular vector is signed so that its largest entry is positive (LAPACK's signs
 * are arbitrary; the model weights do not depend on them).  On return the context holds the
 * problem (y = y_c, X = U_hat) exactly as after bmc_set_problem, without a host round trip.
 * BMC_ESINGULAR when k reaches the null space of Fc (rows sum to zero: rank <= n_models-1). */
int bmc_orthogonalize(bmc_ctx* ctx, const double* F, int64_t n, int32_t n_models, int64_t ldf,
                      const double* truth, int32_t k, double* mean_out, double* yc_out,
                      double* U_hat_out, double* S_out, double* Vt_out);

/* ---- prior: prior_info = [b0 (k,), C0 (k,k row-major), nu0, sigma20] --------
 * Replaces inference_utils.py:21-37: P = inv(C0) (:22), inv(X'X) and the OLS
 * start value sigma2_0 = max(mean r^2, 1e-6) (:26-37).  Also builds the
 * per-problem basis used by the device loop (DESIGN.md "rotated draw"):
 *   B = P + 1e-6 I = L L',  L^-1 X'X L^-T = Q diag(lam) Q',  W = L^-T Q,
 * so that inv(X'X/s2 + P + 1e-6 I) = W diag(1/(lam/s2 + 1)) W'  (:41).
 * BMC_ESINGULAR when C0 or X'X is singular (numpy raises LinAlgError there). */
int bmc_set_prior(bmc_ctx* ctx, const double* b0, const double* C0, double nu0,
                  double sigma20);

/* ---- introspection used by the parity tests -------------------------------
 * gram: (k+1)x(k+1) row-major [X y]'[X y].  basis: W (k,k row-major), lam (k,),
 * sigma2_init.  moments: mean (k,), cov (k,k) of beta | sigma2 (:41-44). */
int bmc_get_gram(bmc_ctx* ctx, double* gram_out);
int bmc_get_basis(bmc_ctx* ctx, double* W_out, double* lam_out, double* sigma2_init);
int bmc_conditional_moments(bmc_ctx* ctx, double sigma2, double* mean_out,
                            double* cov_out);
/* The persistent loop kernels launched by the LAST bmc_gibbs_run* or bmc_simplex_run* on this
 * context: their demangled names (e.g. "gibbs_loop_kernel<double, 1, 0, 32, 1, false, false,
 * true>"), one per launch, in launch order, each followed by '\n', the whole NUL-terminated.
 * *n_out = launches, *needed_out = bytes including the NUL (either may be NULL); names_out may be
 * NULL to ask for the size only, BMC_EINVAL when capacity < *needed_out.  A run without a loop
 * kernel (rss_mode 1, zero iterations) or no run yet gives an empty list; the list is emptied
 * when a run is entered, so a rejected run leaves it empty and a run that fails part-way leaves
 * the launches made before the failure.  The names are built on the host from the key the
 * launcher looked its kernel up with; nothing is read from the device. */
int bmc_last_kernels(bmc_ctx* ctx, char* names_out, int64_t capacity, int32_t* n_out,
                     int64_t* needed_out);

/* ---- residual reduction: rss[b] = sum_i (y_i - sum_j X_ij beta[b][j])^2 -------
 * Replaces inference_utils.py:48-51 as a stand-alone streaming kernel over the
 * un-rotated X (nb coefficient vectors share one pass over X). */
int bmc_residual_rss(bmc_ctx* ctx, const double* beta, int32_t nb, double* rss_out);
/* Same kernel launched `reps` times back to back on data already in HBM; returns
 * the HIP-event time per launch.  Roofline measurement only. */
int bmc_residual_rss_bench(bmc_ctx* ctx, int32_t nb, int32_t reps, double* ms_per_launch);
/* The augmented Gram [X y]'[X y] of the resident problem (f64 MFMA kernel + its reduction,
 * inference_utils.py:25 and the X'y of :43) launched `reps` times back to back; HIP-event time
 * per launch pair.  Roofline measurement only. */
int bmc_gram_bench(bmc_ctx* ctx, int32_t reps, double* ms_per_launch);

/* ---- the Gibbs loop ---------------------------------------------------------
 * Replaces the loop of gibbs_sampler, pybmc/inference_utils.py:39-56, for
 * n_chains independent chains.  samples_out is [n_chains][iters][k+1] f64,
 * row t = [beta_t (k), sigma_t = sqrt(sigma2_t)]  (:54).
 * rng_mode BMC_RNG_DEVICE: seeds[n_chains]; variates from the on-device Philox
 *   generator (xi, g must be NULL).
 * rng_mode BMC_RNG_REPLAY: xi [n_chains][iters][k] standard-normal innovations
 *   in the basis of bmc_get_basis, g [n_chains][iters] Gamma((nu0+n)/2, 1)
 *   variates (seeds may be NULL).  Used to replay the reference's chain.
 * bmc_gibbs_run_device is the device-RNG form writing to a caller-owned DEVICE
 * buffer (no device->host copy of the samples); it returns after the stream has
 * drained so that the status words and the event times in `stats` are final. */
int bmc_gibbs_run(bmc_ctx* ctx, int32_t n_chains, int64_t iters, const uint64_t* seeds,
                  int rng_mode, const double* xi, const double* g, double* samples_out,
                  bmc_stats* stats);
int bmc_gibbs_run_device(bmc_ctx* ctx, int32_t n_chains, int64_t iters,
                         const uint64_t* seeds, void* d_samples_out, bmc_stats* stats);

/* ---- simplex-constrained sampler ---------------------------------------------------
 * Replaces gibbs_sampler_simplex, pybmc/inference_utils.py:59-144 (dispatched from
 * pybmc/bmc.py:173-186): random-walk Metropolis on beta with the model weights
 * beta Vt_hat + 1/n_models kept non-negative, Gibbs step for sigma2.  Uses the problem
 * of bmc_set_problem (no prior call needed).  samples_out is [iters][k+1] rows
 * [beta, sigma]; *accepted_out counts acceptances in the sampling phase (:135).
 * rng_mode BMC_RNG_DEVICE: variates from the Philox generator keyed by seed.
 * rng_mode BMC_RNG_REPLAY: xi [burn+iters][k] standard-normal proposal innovations
 *   (proposal = current + S_hat*stepsize*xi), unif [n_unif] uniforms consumed ONLY by
 *   proposals inside the simplex (:110,:132), g [burn+iters] Gamma((nu0+n)/2,1) variates.
 * The reference's argument checks (:91-94) are the caller's (Python) job: burn >= 0,
 * stepsize > 0 are re-checked here and give BMC_EINVAL. */
int bmc_simplex_run(bmc_ctx* ctx, const double* Vt_hat, int32_t n_models, const double* S_hat,
                    int64_t iters, int64_t burn, double stepsize, double nu0, double sigma20,
                    int rng_mode, uint64_t seed, const double* xi, const double* unif,
                    int64_t n_unif, const double* g, double* samples_out,
                    int64_t* accepted_out, int64_t* unif_used_out, bmc_stats* stats);

/* Several simplex chains in one call: chain c < n_chains is an independent run of bmc_simplex_run
 * on the same problem, Vt_hat, S_hat, step size and prior.  Every per-chain array gains a leading
 * chain axis: seeds [n_chains] (device mode), xi [n_chains][burn+iters][k], unif
 * [n_chains][unif_ld] of which chain c may consume the first n_unif[c] <= unif_ld, g
 * [n_chains][burn+iters]; samples_out [n_chains][iters][k+1], accepted_out [n_chains],
 * unif_used_out [n_chains] (either may be NULL).  The chains run side by side on the device: all
 * of them in one launch of the one-wave kernels, as many per launch as the device keeps resident
 * in the workgroup form, the rest in following launches (stats->launches; bmc_last_kernels lists
 * one name per launch).  stats->n_chains, launches and xcd_local_chains are filled, stats->passes
 * is the number of uniforms consumed by all chains, the rest is as for bmc_simplex_run.
 * CONTRACT: chain c of a device-mode call is bit for bit bmc_simplex_run(seed = seeds[c]) --
 * samples, acceptance count and uniforms used -- whatever its index, its launch or its
 * neighbours; a replay-mode chain is bit for bit the solo replay of its three streams.
 * Every chain starts at beta = 0 as the reference does (:82), and burn-in is PER CHAIN: each
 * chain runs burn + iters steps and keeps the last iters.
 * Argument checks and status codes are those of bmc_simplex_run, plus BMC_EINVAL for
 * n_chains < 1 or an n_unif[c] outside 0..unif_ld; BMC_ENOMEM when the variate and output
 * buffers, which grow with n_chains, cannot be allocated.  BMC_ETIMEOUT and "fewer uniforms
 * supplied than proposals" name the first failing chain in bmc_last_error ("(chain c)"); the
 * other chains' results are still written. */
int bmc_simplex_run_chains(bmc_ctx* ctx, const double* Vt_hat, int32_t n_models,
                           const double* S_hat, int32_t n_chains, int64_t iters, int64_t burn,
                           double stepsize, double nu0, double sigma20, int rng_mode,
                           const uint64_t* seeds, const double* xi, const double* unif,
                           int64_t unif_ld, const int64_t* n_unif, const double* g,
                           double* samples_out, int64_t* accepted_out, int64_t* unif_used_out,
                           bmc_stats* stats);

/* ---- posterior predictive -----------------------------------------------------
 * Replaces rndm_m_random_calculator, pybmc/sampling_utils.py:40-84 (callers
 * pybmc/bmc.py:227,323,367), and the interval test of coverage, :24-34.
 *   theta   [n_draws][k+1]   the posterior rows the caller selected (:57; the reference
 *                            draws 10000 of them without replacement), last column sigma
 *   weights = theta[:, :k] Vt_hat + 1/n_models                               (:60-67)
 *   rndm_m[s][p] = weights[s] . preds[p] + z[s][p] sigma_s                   (:70-77)
 * rng_mode BMC_RNG_DEVICE: z from the Philox generator keyed by seed (noise = NULL);
 * BMC_RNG_REPLAY: noise is [n_draws][n_points] row-major standard normals.
 * Order statistics: for each of n_q requests, numpy's linear interpolation between
 * sorted[q_index] and sorted[q_index+1] with weight q_gamma (:80-82); bands_out is
 * [n_q][n_points].  Coverage (optional, truth != NULL): hits[c] counts the points with
 * sorted[cov_lo[c]] <= truth <= sorted[cov_hi[c]]; n_q, n_cov <= 64; n_draws <= 16384.
 * rndm_m_out (optional) is [n_points][n_draws]: the reference's (n_draws, n_points)
 * array in Fortran order (bmc_predict_draws returns it C-ordered). */
int bmc_predict(bmc_ctx* ctx, const double* preds, int64_t n_points, int32_t n_models,
                const double* theta, int32_t n_draws, int32_t k, const double* Vt_hat,
                int rng_mode, uint64_t seed, const double* noise,
                const int32_t* q_index, const double* q_gamma, int32_t n_q,
                const double* truth, const int32_t* cov_lo, const int32_t* cov_hi,
                int32_t n_cov, double* rndm_m_out, double* bands_out, int64_t* cov_hits_out);

/* bmc_predict with Student-t noise made on the device (after a Student-t fit): rndm_m[s][p] =
 * preds[p] . w_s + sigma_s t[p][s], t with nu (bmc_predict_t) or nu_draws[s] (bmc_predict_tv,
 * [n_draws]) degrees of freedom.  Device generator only: t[p][s] is Bailey's polar variate of the
 * two uniforms of Philox counter (e lo, e hi, "PRET", 0), e = p * n_draws + s, under key = seed;
 * it depends on (seed, p, s, nu_s) alone.  Every other argument, the outputs and the refusals
 * are bmc_predict's; bmc_predict_draws and bmc_predict_timing follow as after bmc_predict.
 * BMC_EINVAL for nu_draws == NULL and for a nu that is not finite or below 0.06: the largest
 * |t| = sqrt(nu) 2^(53/nu) leaves the doubles below about 0.052 (replay host-made noise through
 * bmc_predict for such nu). */
int bmc_predict_t(bmc_ctx* ctx, const double* preds, int64_t n_points, int32_t n_models,
                  const double* theta, int32_t n_draws, int32_t k, const double* Vt_hat,
                  uint64_t seed, const int32_t* q_index, const double* q_gamma, int32_t n_q,
                  const double* truth, const int32_t* cov_lo, const int32_t* cov_hi,
                  int32_t n_cov, double* rndm_m_out, double* bands_out, int64_t* cov_hits_out,
                  double nu);
int bmc_predict_tv(bmc_ctx* ctx, const double* preds, int64_t n_points, int32_t n_models,
                   const double* theta, int32_t n_draws, int32_t k, const double* Vt_hat,
                   uint64_t seed, const int32_t* q_index, const double* q_gamma, int32_t n_q,
                   const double* truth, const int32_t* cov_lo, const int32_t* cov_hi,
                   int32_t n_cov, double* rndm_m_out, double* bands_out, int64_t* cov_hits_out,
                   const double* nu_draws);

/* The draws of the LAST bmc_predict on this context, in the layout the caller wants (they stay
 * on the device until the next bmc_predict or bmc_destroy, so a caller that asked bmc_predict for
 * bands / coverage only can still fetch them afterwards):
 *   BMC_DRAWS_BY_POINT  out[n_points][n_draws]   the device layout
 *   BMC_DRAWS_BY_DRAW   out[n_draws][n_points]   a C-ordered (n_draws, n_points) array: exactly
 *                       what rndm_m_random_calculator returns, pybmc/sampling_utils.py:77
 *                       (transposed on the device, one contiguous copy back).
 * BMC_ESTATE when no bmc_predict has run on this context. */
enum { BMC_DRAWS_BY_POINT = 0, BMC_DRAWS_BY_DRAW = 1 };
int bmc_predict_draws(bmc_ctx* ctx, double* out, int layout);

/* HIP-event times of the LAST bmc_predict on this context (any pointer may be NULL):
 * h2d_ms the host->device copies of its inputs, gemm_ms the weight + MFMA GEMM(+noise)
 * kernels, orderstat_ms the selection / sort kernels, device_ms first copy -> last kernel. */
int bmc_predict_timing(bmc_ctx* ctx, double* h2d_ms, double* gemm_ms, double* orderstat_ms,
                       double* device_ms);

/* ---- pooling the chains of several GPUs (a capability the reference lacks) ----
 * One process per GPU; rank r samples its block of chains with no communication, then ONE
 * all-gather over RCCL (xGMI) pools the per-rank blocks.  RCCL (librccl.so.1) is loaded on
 * first use, so a single-GPU caller needs no RCCL at all.
 *   bmc_comm_unique_id   rank 0 creates the 128-byte RCCL id; the caller hands it to the other
 *                        ranks by whatever transport it has (file, socket, MPI, env)
 *   bmc_comm_init        collective over all ranks; binds the communicator to ctx's device
 *   bmc_allgather        d_recv[r * count .. (r+1) * count) = rank r's d_send[0 .. count), f64;
 *                        DEVICE pointers; d_send may alias its own slot of d_recv (in place).
 *                        Runs on the context's stream, after every sampler launch queued there,
 *                        and returns when the pooled block is complete.
 *   bmc_comm_destroy     also done by bmc_destroy */
#define BMC_COMM_ID_BYTES 128
int bmc_comm_unique_id(char id_out[BMC_COMM_ID_BYTES]);
int bmc_comm_init(bmc_ctx* ctx, int32_t world, int32_t rank, const char id[BMC_COMM_ID_BYTES]);
int bmc_allgather(bmc_ctx* ctx, const void* d_send, void* d_recv, int64_t count_per_rank);
int bmc_comm_destroy(bmc_ctx* ctx);

/* ---- convergence diagnostics of sampled chains (a capability the reference lacks) ------------
 * Classic split R-hat and "mean" ESS of Vehtari, Gelman, Simpson, Carpenter & Buerkner (2021),
 * as Stan and ArviZ (method="split" / "mean") define them; the estimator is written out in
 * INTEGRATION.md section 6.  samples is [n_chains][iters][ld] f64 (the layout bmc_gibbs_run*
 * write), column j < n_cols.  The first `burn` draws of each chain are dropped and the
 * T' = iters - burn kept ones split into two halves of n = T'/2 draws (2 n_chains sequences).
 * Per column (every output is [n_cols]; any may be NULL):
 *   mean_out, sd_out   over all kept draws (sd with ddof 1; the middle draw of an odd T' counts)
 *   rhat_out           split R-hat;   ess_out  effective sample size;   mcse_out  sd / sqrt(ess)
 *   max_lag_out        the largest autocovariance lag the ESS scan read
 * A column with W = 0 (constant within every half) or any non-finite value gets NaN r-hat, ess
 * and mcse (max_lag 0): a value, not an error.  BMC_EINVAL when n < 4, ld < n_cols,
 * n_chains < 1, burn < 0, or n_chains / n_cols > 65536.  Results are deterministic (no atomics).
 * bmc_chain_diagnostics stages the host array on the device itself; the _device form reads
 * caller-owned DEVICE memory on the context's stream (the caller orders its producer before). */
int bmc_chain_diagnostics(bmc_ctx* ctx, const double* samples, int32_t n_chains, int64_t iters,
                          int32_t n_cols, int64_t ld, int64_t burn, double* mean_out,
                          double* sd_out, double* rhat_out, double* ess_out, double* mcse_out,
                          int64_t* max_lag_out);
int bmc_chain_diagnostics_device(bmc_ctx* ctx, const void* d_samples, int32_t n_chains,
                                 int64_t iters, int32_t n_cols, int64_t ld, int64_t burn,
                                 double* mean_out, double* sd_out, double* rhat_out,
                                 double* ess_out, double* mcse_out, int64_t* max_lag_out);

/* The raw quantities the diagnostics are built from, e.g. for autocorrelation plots: the
 * per-sequence moments and ONE block of autocovariance lags, straight from the kernels.  samples,
 * n_chains, iters, n_cols, ld and burn are those of bmc_chain_diagnostics.  Sequence 2c + h is
 * half h of chain c; when T' is odd, sequences 2 n_chains + c are the chains' middle draws, so
 * n_seq = 2 n_chains + (T' odd ? n_chains : 0).  Outputs (HOST; any may be NULL):
 *   seq_mean_out [n_seq][n_cols]   mean of x - shift over the sequence
 *   seq_m2_out   [n_seq][n_cols]   sum of (x - mean)^2 over the sequence (0 for a middle draw)
 *   shift_out    [n_cols]          the column's first kept draw of chain 0
 *   acov_out     [n_active][n_lags]  a(t) = mean over the 2 n_chains halves of
 *                (1/n) sum_{i < n - t} (x_i - mean)(x_{i+t} - mean), t = t0 .. t0 + n_lags - 1, for
 *                column cols[a]; a lag t >= n is 0, so t0 + n_lags may exceed n
 * cols is HOST [n_active], each in [0, n_cols) (repeats allowed); NULL means all columns, and
 * n_active must then be n_cols.  A non-finite value makes the column's affected outputs
 * non-finite and touches no other column.  BMC_EINVAL wherever bmc_chain_diagnostics returns it,
 * for a column index out of range, n_active < 1 or > 65536, t0 < 0 or > 2^40, n_lags < 1 or
 * > 2^20.  Results are deterministic and do not depend on the order of cols. */
int bmc_chain_autocov(bmc_ctx* ctx, const double* samples, int32_t n_chains, int64_t iters,
                      int32_t n_cols, int64_t ld, int64_t burn, const int32_t* cols,
                      int32_t n_active, int64_t t0, int64_t n_lags, double* seq_mean_out,
                      double* seq_m2_out, double* shift_out, double* acov_out);
int bmc_chain_autocov_device(bmc_ctx* ctx, const void* d_samples, int32_t n_chains, int64_t iters,
                             int32_t n_cols, int64_t ld, int64_t burn, const int32_t* cols,
                             int32_t n_active, int64_t t0, int64_t n_lags, double* seq_mean_out,
                             double* seq_m2_out, double* shift_out, double* acov_out);

/* ---- rank-normalised diagnostics and quantiles (a capability the reference lacks) -------------
 * The rank-normalised, folded split R-hat, the bulk and tail ESS of the same paper (Stan's and
 * ArviZ's defaults) and interpolated quantiles; the estimator is written out in INTEGRATION.md
 * section 13.  samples, n_chains, iters, n_cols, ld and burn are those of bmc_chain_diagnostics;
 * the S = 2 n_chains n split draws of a column (n = (iters - burn) / 2; the middle draw of an
 * odd iters - burn takes no part) are ranked exactly on the device, ties sharing their mean
 * rank and -0 tying with +0, and z = ndtri((rank - 3/8) / (S + 1/4)).  Per column (every
 * output but quantiles_out is [n_cols]; any may be NULL):
 *   mean_out, sd_out   bit-equal to bmc_chain_diagnostics's
 *   quantiles_out      [n_probs][n_cols]: numpy's method="linear" quantile of the S split draws
 *                      at probs[t] (1 <= n_probs <= 16, each in [0, 1])
 *   rhat_out           max of the split R-hat of z(x) and of z(|x - median|)
 *   ess_bulk_out       ESS of z(x);   mcse_out  sd / sqrt(ess_bulk)
 *   ess_tail_out       min of the ESS of 1[x <= q05] and of 1[x <= q95]
 * A column with any non-finite value gets NaN in every rank-based output and quantile; a derived
 * series that is constant within every half (W = 0: an all-equal column) gives NaN for the
 * outputs built on it: values, not errors.  cols_per_batch: columns ranked together (0: as many
 * as the free device memory holds); the results do not depend on it.  BMC_EINVAL outside the
 * limits above, when 2 n_chains n > 2^31 - 1, and wherever bmc_chain_diagnostics returns it;
 * BMC_ENOMEM when one column does not fit.  Results are deterministic: the only atomics are
 * integer counters and masks.  The _device form reads caller-owned DEVICE memory on the
 * context's stream.
 *   bmc_rank_normalize*   z alone: z_out is HOST [2 n_chains][n][n_cols], sequence 2c + h the
 *                         h-th half of chain c; folded != 0 ranks |x - median| instead of x.
 *                         A column with a non-finite value is all NaN.
 *   bmc_rank_last_timing  device milliseconds of the last bmc_rank_diagnostics* on ctx: the
 *                         sorts (gather and fold included), the rank / quantile / indicator
 *                         kernels, the classic leg on the derived series, the mean / sd pass */
int bmc_rank_diagnostics(bmc_ctx* ctx, const double* samples, int32_t n_chains, int64_t iters,
                         int32_t n_cols, int64_t ld, int64_t burn, const double* probs,
                         int32_t n_probs, int32_t cols_per_batch, double* mean_out, double* sd_out,
                         double* quantiles_out, double* rhat_out, double* ess_bulk_out,
                         double* ess_tail_out, double* mcse_out);
int bmc_rank_diagnostics_device(bmc_ctx* ctx, const void* d_samples, int32_t n_chains,
                                int64_t iters, int32_t n_cols, int64_t ld, int64_t burn,
                                const double* probs, int32_t n_probs, int32_t cols_per_batch,
                                double* mean_out, double* sd_out, double* quantiles_out,
                                double* rhat_out, double* ess_bulk_out, double* ess_tail_out,
                                double* mcse_out);
int bmc_rank_normalize(bmc_ctx* ctx, const double* samples, int32_t n_chains, int64_t iters,
                       int32_t n_cols, int64_t ld, int64_t burn, int folded, double* z_out);
int bmc_rank_normalize_device(bmc_ctx* ctx, const void* d_samples, int32_t n_chains, int64_t iters,
                              int32_t n_cols, int64_t ld, int64_t burn, int folded, double* z_out);
int bmc_rank_last_timing(bmc_ctx* ctx, double ms_out[4]);

/* ---- pointwise log predictive density of a sampled fit (WAIC; not in the reference) ----------
 * The model the samplers draw from: y_i ~ N(a_i . beta, sigma^2).  A is n_points x k (lda / layout
 * as in bmc_set_problem: BMC_COL_MAJOR is what U_hat is), y [n_points], theta holds n_draws rows
 * ldt >= k + 1 doubles apart: k coefficients, then sigma, the layout bmc_gibbs_run* and
 * bmc_simplex_run write (a larger ldt reads a column subset or every thin-th draw in place).
 * With  ll[i][s] = -1/2 log(2 pi) - log sigma_s - (y_i - a_i . beta_s)^2 / (2 sigma_s^2),
 * per point i over the n_draws draws (each output [n_points]; any may be NULL):
 *   lppd_out     log-mean-exp_s ll[i][s] = logsumexp_s - log n_draws
 *   pwaic_out    var_s ll[i][s], ddof 1   (p_waic 2 of Gelman, Hwang & Vehtari 2014, eq. 12)
 *   mean_ll_out  mean_s ll[i][s]
 * The n_points x n_draws matrix is never stored: the draws are streamed, n_draws is bounded by
 * the memory of theta alone; device memory used is O(n_points (k + splits) + n_draws).  Results
 * are deterministic (no atomics).  Non-finite input gives NaN, not an error, by the arithmetic
 * alone: a NaN or infinity in row i of A or in y_i makes point i's outputs NaN; a NaN in theta or
 * a sigma_s <= 0 makes every point's outputs NaN.  BMC_EINVAL when n_points < 1, k outside
 * 1..256, n_draws < 2, lda or ldt too small.  Runs on the context's stream and leaves the
 * context's problem, prior and predictive draws alone.  bmc_pointwise_loglik stages host arrays
 * itself; the _device form reads caller-owned DEVICE memory (the caller orders its producer
 * before the call); outputs are host pointers in both.  The estimators built on these
 * (elpd_waic, se, ...) are written out in INTEGRATION.md section 8. */
int bmc_pointwise_loglik(bmc_ctx* ctx, const double* A, int64_t n_points, int32_t k, int64_t lda,
                         int layout, const double* y, const double* theta, int64_t n_draws,
                         int64_t ldt, double* lppd_out, double* pwaic_out, double* mean_ll_out);
int bmc_pointwise_loglik_device(bmc_ctx* ctx, const void* dA, int64_t n_points, int32_t k,
                                int64_t lda, int layout, const void* dy, const void* dtheta,
                                int64_t n_draws, int64_t ldt, double* lppd_out,
                                double* pwaic_out, double* mean_ll_out);

/* ---- PSIS-LOO: Pareto-smoothed importance-sampling leave-one-out (not in the reference) ------
 * Same model, arguments and ll[i][s] as bmc_pointwise_loglik.  Per point i, over the n_draws
 * draws, with lw_s = -ll[i][s] shifted so that its largest is 0 and r_eff taken as 1 (as
 * loo::psis does when none is given): the M = min(floor(n_draws / 5), ceil(3 sqrt(n_draws)))
 * largest lw are replaced, in rank order, by quantiles of a generalised Pareto distribution fitted
 * to them above the next largest (Zhang & Stephens 2009 with the weak prior of loo::gpdfit), all
 * lw truncated at 0 (each output [n_points]; any may be NULL):
 *   elpd_loo_out  logsumexp_s(ll + lw) - logsumexp_s(lw)
 *   pareto_k_out  the fitted shape k-hat; +inf where nothing was smoothed (n_draws < 25, a tail of
 *                 equal values, a non-finite fit): elpd_loo is then the raw importance-sampling one
 *   lppd_out      as bmc_pointwise_loglik (p_loo_i = lppd_i - elpd_loo_i)
 * Ties are by value: the result does not depend on the order of the draws.  The matrix is never
 * stored: it is recomputed for a bounded number of passes (an exact radix select of the tail,
 * at most 11 passes for any input); device memory used is O(n_points (M + splits) + n_draws).
 * Results are deterministic.  Non-finite input as bmc_pointwise_loglik: NaN in every output of the
 * point (a NaN or infinity in row i of A or y_i) or of all points (a NaN in theta, a sigma_s <= 0).
 * BMC_EINVAL as bmc_pointwise_loglik, and when n_draws exceeds about 7.4 million (M > 8191: the
 * per-point sort is done in on-chip memory).  The summaries (elpd_loo, p_loo, looic, se,
 * n_high_k) are written out in INTEGRATION.md section 9. */
int bmc_psis_loo(bmc_ctx* ctx, const double* A, int64_t n_points, int32_t k, int64_t lda,
                 int layout, const double* y, const double* theta, int64_t n_draws, int64_t ldt,
                 double* elpd_loo_out, double* pareto_k_out, double* lppd_out);
int bmc_psis_loo_device(bmc_ctx* ctx, const void* dA, int64_t n_points, int32_t k, int64_t lda,
                        int layout, const void* dy, const void* dtheta, int64_t n_draws,
                        int64_t ldt, double* elpd_loo_out, double* pareto_k_out,
                        double* lppd_out);

/* ---- the same scores under a Student-t likelihood (not in the reference) -----------------------
 * For a fit of bmc_robust_run*: y_i ~ a_i . beta + sigma t_nu with nu fixed, the latent row weights
 * integrated out.  Everything as bmc_pointwise_loglik / bmc_psis_loo (arguments, outputs, the
 * estimators, determinism, non-finite input, BMC_EINVAL) with
 *   ll[i][s] = lgamma((nu + 1)/2) - lgamma(nu/2) - 1/2 log(nu pi) - log sigma_s
 *              - (nu + 1)/2 log1p((y_i - a_i . beta_s)^2 / (nu sigma_s^2))
 * (an infinity in row i of A or in y_i makes point i's outputs non-finite: NaN, where the Gaussian
 * density gives -inf).  BMC_EINVAL also when nu is not positive and finite; the context stays
 * usable.  INTEGRATION.md section 16. */
int bmc_pointwise_loglik_t(bmc_ctx* ctx, const double* A, int64_t n_points, int32_t k, int64_t lda,
                           int layout, const double* y, const double* theta, int64_t n_draws,
                           int64_t ldt, double nu, double* lppd_out, double* pwaic_out,
                           double* mean_ll_out);
int bmc_pointwise_loglik_t_device(bmc_ctx* ctx, const void* dA, int64_t n_points, int32_t k,
                                  int64_t lda, int layout, const void* dy, const void* dtheta,
                                  int64_t n_draws, int64_t ldt, double nu, double* lppd_out,
                                  double* pwaic_out, double* mean_ll_out);
int bmc_psis_loo_t(bmc_ctx* ctx, const double* A, int64_t n_points, int32_t k, int64_t lda,
                   int layout, const double* y, const double* theta, int64_t n_draws, int64_t ldt,
                   double nu, double* elpd_loo_out, double* pareto_k_out, double* lppd_out);
int bmc_psis_loo_t_device(bmc_ctx* ctx, const void* dA, int64_t n_points, int32_t k, int64_t lda,
                          int layout, const void* dy, const void* dtheta, int64_t n_draws,
                          int64_t ldt, double nu, double* elpd_loo_out, double* pareto_k_out,
                          double* lppd_out);

/* ---- the same with degrees of freedom of each draw's own (not in the reference) -----------------
 * For a fit of bmc_robust_run_nu*: draw s is (beta_s, sigma_s, nu_s).  Everything as the _t entry
 * points with nu_s in place of nu in ll[i][s].  The caller gives the distinct values nu_values
 * [n_values] (HOST in all four forms) and nu_index [n_draws] (int32; host, or DEVICE in the _device
 * forms): nu_s = nu_values[nu_index[s]].  The constant lgamma((nu + 1)/2) - lgamma(nu/2) -
 * 1/2 log(nu pi) is computed once per table entry with the expression of the _t entry points, so a
 * table of one value returns their bits.  BMC_EINVAL for n_values < 1, a table entry that is not
 * positive and finite, or an index outside 0 .. n_values - 1: a host index is checked before any
 * launch; a device index is clamped into range where it is read (nothing is read out of bounds)
 * and reported after the run, whose outputs are then not valid.  The context stays usable. */
int bmc_pointwise_loglik_tv(bmc_ctx* ctx, const double* A, int64_t n_points, int32_t k, int64_t lda,
                            int layout, const double* y, const double* theta, int64_t n_draws,
                            int64_t ldt, const double* nu_values, int32_t n_values,
                            const int32_t* nu_index, double* lppd_out, double* pwaic_out,
                            double* mean_ll_out);
int bmc_pointwise_loglik_tv_device(bmc_ctx* ctx, const void* dA, int64_t n_points, int32_t k,
                                   int64_t lda, int layout, const void* dy, const void* dtheta,
                                   int64_t n_draws, int64_t ldt, const double* nu_values,
                                   int32_t n_values, const void* d_nu_index, double* lppd_out,
                                   double* pwaic_out, double* mean_ll_out);
int bmc_psis_loo_tv(bmc_ctx* ctx, const double* A, int64_t n_points, int32_t k, int64_t lda,
                    int layout, const double* y, const double* theta, int64_t n_draws, int64_t ldt,
                    const double* nu_values, int32_t n_values, const int32_t* nu_index,
                    double* elpd_loo_out, double* pareto_k_out, double* lppd_out);
int bmc_psis_loo_tv_device(bmc_ctx* ctx, const void* dA, int64_t n_points, int32_t k, int64_t lda,
                           int layout, const void* dy, const void* dtheta, int64_t n_draws,
                           int64_t ldt, const double* nu_values, int32_t n_values,
                           const void* d_nu_index, double* elpd_loo_out, double* pareto_k_out,
                           double* lppd_out);

/* ---- PSIS-LOO predictive moments: what the fit would have predicted for y_i without it -------
 * Arguments, weights, elpd_loo_out, pareto_k_out and lppd_out as bmc_psis_loo.  With W_s the
 * truncated (smoothed or raw) weight of draw s for point i, every draw of a run of equal ll[i][s]
 * given the mean W of the ranks the run occupies (ties are by value), w_s = W_s / sum_t W_t and
 * r_s = y_i - a_i . beta_s (each output [n_points]; any may be NULL):
 *   loo_mean_out  y_i - sum_s w_s r_s                  (the leave-one-out predictive mean)
 *   loo_sd_out    sqrt(sum_s w_s (sigma_s^2 + r_s^2) - (sum_s w_s r_s)^2)
 *   loo_pit_out   sum_s w_s Phi(r_s / sigma_s)         (Phi the standard normal distribution function)
 *   ess_out       1 / sum_s w_s^2                      (between 1 and n_draws)
 * One more pass over the matrix than bmc_psis_loo at most; deterministic; NaN as bmc_psis_loo.
 * BMC_EINVAL as bmc_pointwise_loglik, and when n_draws exceeds 1 863 225 (M > 4095: the per-point
 * sort keeps the draw index of every candidate in on-chip memory).  INTEGRATION.md section 10. */
int bmc_psis_loo_predict(bmc_ctx* ctx, const double* A, int64_t n_points, int32_t k, int64_t lda,
                         int layout, const double* y, const double* theta, int64_t n_draws,
                         int64_t ldt, double* elpd_loo_out, double* pareto_k_out, double* lppd_out,
                         double* loo_mean_out, double* loo_sd_out, double* loo_pit_out,
                         double* ess_out);
int bmc_psis_loo_predict_device(bmc_ctx* ctx, const void* dA, int64_t n_points, int32_t k,
                                int64_t lda, int layout, const void* dy, const void* dtheta,
                                int64_t n_draws, int64_t ldt, double* elpd_loo_out,
                                double* pareto_k_out, double* lppd_out, double* loo_mean_out,
                                double* loo_sd_out, double* loo_pit_out, double* ess_out);

/* ---- the same under a Student-t likelihood (not in the reference) ------------------------------
 * The _t forms take the arguments of bmc_psis_loo_t, the _tv forms those of bmc_psis_loo_tv, each
 * followed by the four further outputs of bmc_psis_loo_predict.  Weights, tie sharing, ess, NaN
 * rules and the draw limit as bmc_psis_loo_predict; ll[i][s], elpd_loo_out, pareto_k_out and
 * lppd_out as (and bit-equal to) bmc_psis_loo_t / _tv.  With nu_s the draw's degrees of freedom (nu
 * in the _t forms) and F_nu the Student-t distribution function:
 *   loo_mean_out  y_i - sum_s w_s r_s      (the location of the predictive distribution; its mean
 *                                           where every nu_s > 1)
 *   loo_sd_out    sqrt(sum_s w_s (sigma_s^2 nu_s / (nu_s - 2) + r_s^2) - (sum_s w_s r_s)^2) when
 *                 every nu of the call (nu; every entry of nu_values) exceeds 2, else +inf at every
 *                 point that is not NaN (decided before the launch: no infinity is summed)
 *   loo_pit_out   sum_s w_s F_{nu_s}(r_s / sigma_s)
 * Two more passes over the matrix than bmc_psis_loo_t at most (the sums run in two phases).
 * BMC_EINVAL as bmc_psis_loo_t / _tv and bmc_psis_loo_predict, and when nu, or an entry of
 * nu_values, lies outside 0.06 .. 1000 (the range over which F_nu is held to its accuracy bar), or
 * n_values < 1.  INTEGRATION.md section 10. */
int bmc_psis_loo_predict_t(bmc_ctx* ctx, const double* A, int64_t n_points, int32_t k, int64_t lda,
                           int layout, const double* y, const double* theta, int64_t n_draws,
                           int64_t ldt, double nu, double* elpd_loo_out, double* pareto_k_out,
                           double* lppd_out, double* loo_mean_out, double* loo_sd_out,
                           double* loo_pit_out, double* ess_out);
int bmc_psis_loo_predict_t_device(bmc_ctx* ctx, const void* dA, int64_t n_points, int32_t k,
                                  int64_t lda, int layout, const void* dy, const void* dtheta,
                                  int64_t n_draws, int64_t ldt, double nu, double* elpd_loo_out,
                                  double* pareto_k_out, double* lppd_out, double* loo_mean_out,
                                  double* loo_sd_out, double* loo_pit_out, double* ess_out);
int bmc_psis_loo_predict_tv(bmc_ctx* ctx, const double* A, int64_t n_points, int32_t k, int64_t lda,
                            int layout, const double* y, const double* theta, int64_t n_draws,
                            int64_t ldt, const double* nu_values, int32_t n_values,
                            const int32_t* nu_index, double* elpd_loo_out, double* pareto_k_out,
                            double* lppd_out, double* loo_mean_out, double* loo_sd_out,
                            double* loo_pit_out, double* ess_out);
int bmc_psis_loo_predict_tv_device(bmc_ctx* ctx, const void* dA, int64_t n_points, int32_t k,
                                   int64_t lda, int layout, const void* dy, const void* dtheta,
                                   int64_t n_draws, int64_t ldt, const double* nu_values,
                                   int32_t n_values, const void* d_nu_index, double* elpd_loo_out,
                                   double* pareto_k_out, double* lppd_out, double* loo_mean_out,
                                   double* loo_sd_out, double* loo_pit_out, double* ess_out);

/* ---- exact K-fold / leave-group-out cross-validation, all folds in one call -------------------
 * A (n x k host f64, k <= 64, element (i, j) as in bmc_pointwise_loglik), y [n], fold [n] labels in
 * 0 .. n_folds-1 (2 <= n_folds <= 1024; no fold empty; every training set, the rows of the OTHER
 * folds, of at least k rows), the prior of bmc_set_prior.  For every fold f the posterior given
 * its training rows is sampled by n_chains chains of `iters` iterations: chain (f, c) consumes the
 * streams of seeds[f * n_chains + c] and is, up to the rounding of its residual sums, the chain
 * bmc_gibbs_run draws on those rows under that seed (same conditionals, initial sigma2, gamma
 * shape (nu0 + n_train) / 2, ridge and floors).  The first `burn` draws of a chain are dropped,
 * every `thin`-th of the rest kept (kept = ceil((iters - burn) / thin); n_chains * kept >= 2) and
 * the chains of a fold pooled: S = n_chains * kept draws.  For every row i, with f its own fold:
 *   elpd_out[i]   logsumexp_s ll[i][s] - log S over the draws of fold f   (ll: bmc_pointwise_loglik)
 *   mean_out[i]   a_i . mean_s beta_s
 *   draws_out     [n_folds][n_chains][kept][k+1], rows [beta, sigma]; may be NULL
 * The training statistics of all folds come from one pass over the rows (per-fold Gram on the
 * matrix cores, total minus own), all n_folds * n_chains chains run one wave each in launches of
 * at most 2048, in as many batches of folds as the free device memory asks for.  The resident
 * problem and prior of the context are not touched.  Deterministic.
 * BMC_EINVAL for bad arguments (the message names the offending fold), BMC_ESINGULAR when C0 or
 * the training Gram of a fold is numerically singular (the message names the fold), BMC_ENOMEM
 * when not even one fold's chains fit the device.  INTEGRATION.md section 11. */
int bmc_kfold_cv(bmc_ctx* ctx, const double* A, int64_t n, int32_t k, int64_t lda, int layout,
                 const double* y, const int64_t* fold, int32_t n_folds, const double* b0,
                 const double* C0, double nu0, double sigma20, int32_t n_chains, int64_t iters,
                 int64_t burn, int64_t thin, const uint64_t* seeds, double* elpd_out,
                 double* mean_out, double* draws_out);

/* ---- the component path: bmc_kfold_cv for every candidate component count in one call ---------
 * Arguments as bmc_kfold_cv, A with k <= 64 columns, plus comps [n_comps]: strictly increasing
 * candidate counts in 1 .. k.  Candidate k_j is the model on the LEADING k_j columns of A under the
 * prior (b0[0 .. k_j), the leading k_j x k_j block of C0 (row-major, leading dimension k), nu0,
 * sigma20): the exact marginal of the Gaussian prior.  seeds [n_folds * n_chains] serve every
 * candidate: chain (j, f, c) consumes the streams of seeds[f * n_chains + c] and is the chain
 * bmc_kfold_cv runs on those k_j columns under that seed.  Every training set must hold at least
 * comps[n_comps - 1] rows.
 *   elpd_out, mean_out   [n_comps][n] row-major: row j is bmc_kfold_cv's vector for candidate j
 *   draws_out            candidate after candidate, each [n_folds][n_chains][kept][k_j + 1]; may be NULL
 * One gather and one Gram pass at the widest candidate serve all of them (the training Gram of
 * candidate k_j is the leading block); the n_comps * n_folds * n_chains chains run one wave each,
 * in launches of one kernel width (8 / 16 / 32 / 64 columns) and at most 2048 chains, in as many
 * batches of whole (candidate, fold) problems as the free device memory asks for.  The resident
 * problem and prior of the context are not touched.  Deterministic.
 * BMC_EINVAL for bad arguments, BMC_ESINGULAR when a leading block of C0 or the training Gram of a
 * (candidate, fold) is numerically singular (the message names the fold and the component count),
 * BMC_ENOMEM when the chains of one problem do not fit the device.  INTEGRATION.md section 11.1. */
int bmc_cv_path(bmc_ctx* ctx, const double* A, int64_t n, int32_t k, int64_t lda, int layout,
                const double* y, const int64_t* fold, int32_t n_folds, const double* b0,
                const double* C0, double nu0, double sigma20, int32_t n_chains, int64_t iters,
                int64_t burn, int64_t thin, const uint64_t* seeds, const int32_t* comps,
                int32_t n_comps, double* elpd_out, double* mean_out, double* draws_out);

/* ---- exact K-fold cross-validation under the Student-t likelihood, all folds in one launch -----
 * Arguments and results as bmc_kfold_cv, with k <= 32 and these differences.
 *   The chains.  Chain (f, c) is a chain of bmc_robust_run (bmc_robust_run_nu for the _tv call) on
 *   the training rows of fold f, in the caller's row order, under seeds[f * n_chains + c]: `iters`
 *   sweeps from lambda = 1 and the OLS sigma2 of THOSE rows, the gamma shape (nu0 + n_train) / 2,
 *   the weight variates counted by the row's position within the training rows.  The kept draws
 *   (the first `burn` dropped, every `thin`-th of the rest) equal, bit for bit, rows burn, burn +
 *   thin, ... of what bmc_robust_run(nu, 1 chain, iters, burn 0) draws after bmc_set_problem and
 *   bmc_set_prior on those rows alone; likewise the nu indices of bmc_robust_run_nu.
 *   The scores.  elpd_out[i] is the lppd of bmc_pointwise_loglik_t (bmc_pointwise_loglik_tv with the
 *   draws' own nu) on the rows of fold f and its pooled kept draws.
 *   weight_out   [n_folds][n_chains][n], may be NULL: the mean of lambda_i over the sweeps after
 *                `burn` (thinning does not apply to it) at the caller's row index i, NaN at the
 *                fold's own held-out rows.
 *   nu_idx_out   (_tv) [n_folds][n_chains][kept] indices into nu_grid of the kept sweeps; may be NULL.
 * nu_grid, nu_weight, n_grid, nu_init as bmc_robust_run_nu; every fold has its own table of the
 * grid's constants, which depend on n_train.  Every fold's training rows are packed on the device
 * (n_folds copies of about n - n_f rows) and all n_folds * n_chains chains run one workgroup each,
 * in launches of at most 1024, in as many batches of whole folds as the free device memory asks
 * for.  The resident problem and prior of the context are not touched (the set-up scratch of
 * bmc_set_problem and the run buffers are used).  Deterministic.
 * BMC_EINVAL for bad arguments, BMC_ESINGULAR when C0 or X'X of a fold's training rows is singular
 * (the message names the fold) or a Cholesky pivot of a chain is not positive and finite (the
 * message names the fold and the chain), BMC_ENOMEM when not one fold fits the device.  The context
 * stays usable after an error.  INTEGRATION.md section 11.2. */
int bmc_kfold_cv_t(bmc_ctx* ctx, const double* A, int64_t n, int32_t k, int64_t lda, int layout,
                   const double* y, const int64_t* fold, int32_t n_folds, const double* b0,
                   const double* C0, double nu0, double sigma20, int32_t n_chains, int64_t iters,
                   int64_t burn, int64_t thin, const uint64_t* seeds, double nu, double* elpd_out,
                   double* mean_out, double* draws_out, double* weight_out);
int bmc_kfold_cv_tv(bmc_ctx* ctx, const double* A, int64_t n, int32_t k, int64_t lda, int layout,
                    const double* y, const int64_t* fold, int32_t n_folds, const double* b0,
                    const double* C0, double nu0, double sigma20, int32_t n_chains, int64_t iters,
                    int64_t burn, int64_t thin, const uint64_t* seeds, const double* nu_grid,
                    const double* nu_weight, int32_t n_grid, int32_t nu_init, double* elpd_out,
                    double* mean_out, double* draws_out, double* weight_out, int32_t* nu_idx_out);

/* ---- posterior predictive check: do data replicated from the fit look like the data? ----------
 * Model and arguments A, y, theta as bmc_pointwise_loglik; offset [n_points] or NULL (zeros).
 * Replicated data y_rep[i][s] = a_i . beta_s + sigma_s z[i][s] + offset_i, z[i][s] the standard
 * normal of (seed, i, s): Philox4x32-10 keyed by seed, counter (s lo, s hi, 0x50504353,
 * (i >> 6) * 32 + (i & 31)), Box-Muller, the cosine half to the point with bit 5 of i clear and
 * the sine half to point i + 32.  The n_points x n_draws matrix is never stored; it is reduced
 * over the points, per draw:
 *   t_rep_out   [n_draws][8]: min, max, mean, sd, skew, kurt of y_rep[.][s] (central moments with
 *               ddof 0: sd = sqrt(m2), skew = m3 / m2^1.5, kurt = m4 / m2^2 - 3; accumulated as
 *               power sums of y_rep - c_s about the draw's own centre c_s = mean_i(a_i) . beta_s +
 *               mean_i(offset_i), formed on the device; `center` is kept for the signature and no
 *               longer read), then sum_i z[i][s]^2 and max_i |z[i][s]|
 *   t_obs2_out  [n_draws][2]: sum_i e^2 and max_i |e|, e = (y_i - a_i . beta_s) / sigma_s: the
 *               observed counterparts of the last two (those of the first six do not depend on
 *               the draw: the same functions of y + offset, left to the caller)
 * Either output may be NULL.  The Bayesian p-value of statistic j is the share of draws with
 * t_rep[s][j] >= t_obs[s][j].  One workgroup per 64 draws walks all points and nothing is
 * combined across workgroups: the results depend on the arguments alone, not on the device.
 * Non-finite input is data: a value is NaN exactly where these definitions give NaN, and all ten
 * values of a draw with a non-finite coefficient or without a finite sigma_s > 0 are NaN.
 * BMC_EINVAL as bmc_pointwise_loglik, and when n_points < 3 or n_points > 2^31.  Runs on the
 * context's stream and leaves the problem, the prior and the predictive draws alone.
 * bmc_ppc stages host arrays itself; the _device form reads caller-owned DEVICE memory (A, y,
 * offset, theta); outputs are host pointers in both.  INTEGRATION.md section 12. */
int bmc_ppc(bmc_ctx* ctx, const double* A, int64_t n_points, int32_t k, int64_t lda, int layout,
            const double* y, const double* offset, const double* theta, int64_t n_draws,
            int64_t ldt, uint64_t seed, double center, double* t_rep_out, double* t_obs2_out);
int bmc_ppc_device(bmc_ctx* ctx, const void* dA, int64_t n_points, int32_t k, int64_t lda,
                   int layout, const void* dy, const void* doffset, const void* dtheta,
                   int64_t n_draws, int64_t ldt, uint64_t seed, double center, double* t_rep_out,
                   double* t_obs2_out);

/* The same check of a Student-t fit (bmc_robust_run): y_rep[i][s] = a_i . beta_s + sigma_s z[i][s] +
 * offset_i with z[i][s] a Student-t variate with nu (bmc_ppc_t) or nu_values[nu_index[s]]
 * (bmc_ppc_tv; the table convention of bmc_pointwise_loglik_tv, at most 4096 values) degrees of
 * freedom, made on the device: Bailey's polar form
 *   z = sqrt(nu expm1(-(2 / nu) log u1)) cos(2 pi u2),
 * u1 and u2 the two 53-bit uniforms in (0, 1] of ONE Philox4x32-10 call keyed by seed with counter
 * (s lo, s hi, 0x50504354, i): the point index itself, and only the cosine half (the sine half
 * shares the radius and is not independent of it).  z[i][s] depends on (seed, i, s, nu_s) alone,
 * is finite for nu >= 0.06 and may be +-inf only for nu below about 0.052.  The arguments are those
 * of bmc_ppc without `center`; t_rep_out and t_obs2_out, the sums, the moments and the NaN rules
 * are the same: sum_i z^2 and max_i |z| are now of the t variates, and e is still
 * (y_i - a_i . beta_s) / sigma_s.  BMC_EINVAL as bmc_ppc, and for a nu or a table entry that is not
 * positive and finite, n_values < 1 or > 4096, or an index outside the table (host index: before
 * anything runs; device index: after the run, the outputs are then not valid).  In the _device
 * forms nu_values stays a HOST pointer and d_nu_index is int32 DEVICE memory.
 * INTEGRATION.md section 12. */
int bmc_ppc_t(bmc_ctx* ctx, const double* A, int64_t n_points, int32_t k, int64_t lda, int layout,
              const double* y, const double* offset, const double* theta, int64_t n_draws,
              int64_t ldt, uint64_t seed, double nu, double* t_rep_out, double* t_obs2_out);
int bmc_ppc_t_device(bmc_ctx* ctx, const void* dA, int64_t n_points, int32_t k, int64_t lda,
                     int layout, const void* dy, const void* doffset, const void* dtheta,
                     int64_t n_draws, int64_t ldt, uint64_t seed, double nu, double* t_rep_out,
                     double* t_obs2_out);
int bmc_ppc_tv(bmc_ctx* ctx, const double* A, int64_t n_points, int32_t k, int64_t lda, int layout,
               const double* y, const double* offset, const double* theta, int64_t n_draws,
               int64_t ldt, uint64_t seed, const double* nu_values, int32_t n_values,
               const int32_t* nu_index, double* t_rep_out, double* t_obs2_out);
int bmc_ppc_tv_device(bmc_ctx* ctx, const void* dA, int64_t n_points, int32_t k, int64_t lda,
                      int layout, const void* dy, const void* doffset, const void* dtheta,
                      int64_t n_draws, int64_t ldt, uint64_t seed, const double* nu_values,
                      int32_t n_values, const void* d_nu_index, double* t_rep_out,
                      double* t_obs2_out);

/* ---- power-scaling sensitivity: does the answer depend on the prior? (not in the reference) -----
 * Model and arguments A, y, theta as bmc_pointwise_loglik (n_draws >= 2 pooled draws, row s =
 * (beta_s, sigma_s)); the prior of bmc_set_prior: b0 [k], C0 [k][k] (row-major, symmetric positive
 * definite; factored on the host), nu0, sigma20 -- HOST pointers in both forms, as are Vt
 * [k][n_models] (row-major; NULL with n_models = 0) and alphas [n_alphas] (1 .. 66 values, each
 * > 0, finite and != 1).  Per draw, additive constants dropped:
 *   lp_beta   = -1/2 (beta - b0)' C0^-1 (beta - b0)
 *   lp_sigma2 = -(nu0/2 + 1) log sigma^2 - nu0 sigma20 / (2 sigma^2)
 *   loglik    = -(n/2) log 2 pi - n log sigma - sum_i (y_i - a_i . beta)^2 / (2 sigma^2)
 * (all three NaN for a draw with a non-finite coefficient or without a finite sigma > 0).
 * `components` is a mask of bit 0 prior = lp_beta + lp_sigma2, bit 1 likelihood = loglik, bit 2
 * prior_beta, bit 3 prior_sigma2; the set bits in that order are the components c, and weight
 * vector w = c * n_alphas + a is that of (component c, alphas[a]): lw = (alpha - 1) lp_c shifted
 * to a largest of 0, Pareto-smoothed as bmc_psis_loo smooths its weights (tail of
 * M = min(floor(S / 5), ceil(3 sqrt S)) draws in ascending lw with ties in draw order, no fit when
 * M < 5 or the tail is one value), truncated at 0, normalised to sum 1.  The quantity columns are
 * q = 0 .. k-1 the coefficients, q = k sigma, q = k+1 .. k+n_models the model weights
 * beta . Vt + 1 / n_models; Q = k + 1 + n_models.  For column q and vector w, with the draws sorted
 * by (value, draw), P_j = j / S and Q_j the running sum of the weights: the cumulative
 * Jensen-Shannon distance cjs = sqrt((cjs_PQ + cjs_QP) / (I_P + I_Q)) (0 for
 * a constant column) and the weighted mean and sd.  Outputs (host; any may be NULL):
 *   logdens_out   [3][n_draws]: lp_beta, lp_sigma2, loglik
 *   pareto_k_out  [W], W = n_components * n_alphas; +inf where nothing was smoothed
 *   mean_out, sd_out, cjs_out   [W][Q]
 *   weights_out   [n_draws][W]: the normalised weights, in draw order
 *   flags_out     [n_components + Q]: 1 for a component with a non-finite log density (its
 *                 pareto_k, weights and every mean / sd / cjs are NaN) and for a column with a
 *                 non-finite value (its mean / sd / cjs are NaN), else 0
 * Every vector is sorted once, whatever n_alphas; the columns are sorted in batches of
 * cols_per_batch (0: as many as the free device memory holds).  Results are deterministic and do
 * not depend on cols_per_batch or on which other alphas are in the call.  BMC_EINVAL for bad
 * arguments (k outside 1..256, n_models > 4096, n_draws > 2^31 - 2), BMC_ESINGULAR when C0 is not
 * positive definite, BMC_ENOMEM when one column does not fit.  The _device form reads
 * caller-owned DEVICE memory (A, y, theta).  bmc_sens_last_timing: device milliseconds of the last
 * call: log densities, sorts, Pareto smoothing, distances. */
int bmc_power_sensitivity(bmc_ctx* ctx, const double* A, int64_t n_points, int32_t k, int64_t lda,
                          int layout, const double* y, const double* theta, int64_t n_draws,
                          int64_t ldt, const double* b0, const double* C0, double nu0,
                          double sigma20, const double* Vt, int32_t n_models, const double* alphas,
                          int32_t n_alphas, uint32_t components, int32_t cols_per_batch,
                          double* logdens_out, double* pareto_k_out, double* mean_out,
                          double* sd_out, double* cjs_out, double* weights_out,
                          uint32_t* flags_out);
int bmc_power_sensitivity_device(bmc_ctx* ctx, const void* dA, int64_t n_points, int32_t k,
                                 int64_t lda, int layout, const void* dy, const void* dtheta,
                                 int64_t n_draws, int64_t ldt, const double* b0, const double* C0,
                                 double nu0, double sigma20, const double* Vt, int32_t n_models,
                                 const double* alphas, int32_t n_alphas, uint32_t components,
                                 int32_t cols_per_batch, double* logdens_out, double* pareto_k_out,
                                 double* mean_out, double* sd_out, double* cjs_out,
                                 double* weights_out, uint32_t* flags_out);
int bmc_sens_last_timing(bmc_ctx* ctx, double ms_out[4]);

/* The same under the Student-t likelihood of bmc_robust_run (a fit of the robust sampler): the
 * arguments of bmc_power_sensitivity and, behind cols_per_batch, the degrees of freedom.  _t: one
 * `nu` (positive, finite) for every draw.  _tv (a fit that estimated nu): nu_values [n_values]
 * (1 .. 4096 distinct values, positive and finite; host), nu_index [n_draws] int32 into them (host;
 * DEVICE memory in the _device form) and nu_log_prior [n_values] (host; may be NULL: nu has no
 * prior), the log of the normalised prior weight of every value.  With r_is = y_i - a_i . beta_s,
 *   loglik = n (C(nu_s) - log sigma_s) - (nu_s + 1)/2 sum_i log1p(r_is^2 / (nu_s sigma_s^2)),
 *   C(nu)  = lgamma((nu + 1)/2) - lgamma(nu/2) - 1/2 log(nu pi)   (long double, once per value),
 *   lp_nu  = nu_log_prior[nu_index[s]]   (0 without a prior),
 * lp_beta and lp_sigma2 as above, bit for bit; all four NaN for a draw with a non-finite coefficient
 * or without a finite sigma > 0.  `components` has a fifth bit: bit 0 prior = lp_beta + lp_sigma2 +
 * lp_nu, bits 1 .. 3 as above, bit 4 prior_nu = lp_nu (only with nu_log_prior).  logdens_out is
 * [4][n_draws]: lp_beta, lp_sigma2, loglik, lp_nu.  The _tv forms have one more quantity column,
 * the LAST: q = k + 1 + n_models is nu_s, so Q = k + 2 + n_models; the other columns keep their
 * places.  A _tv call whose index holds one value returns the bits of the _t call.  BMC_EINVAL
 * also for a nu, a table entry or n_values outside these limits, a non-finite nu_log_prior, bit 4
 * without a prior and an index outside the table: a host index before any launch, a device index
 * clamped where it is read and reported after the run (the outputs are then not valid).  The
 * context stays usable.  bmc_sens_last_timing counts the Student-t pass under the log densities. */
int bmc_power_sensitivity_t(bmc_ctx* ctx, const double* A, int64_t n_points, int32_t k, int64_t lda,
                            int layout, const double* y, const double* theta, int64_t n_draws,
                            int64_t ldt, const double* b0, const double* C0, double nu0,
                            double sigma20, const double* Vt, int32_t n_models, const double* alphas,
                            int32_t n_alphas, uint32_t components, int32_t cols_per_batch, double nu,
                            double* logdens_out, double* pareto_k_out, double* mean_out,
                            double* sd_out, double* cjs_out, double* weights_out,
                            uint32_t* flags_out);
int bmc_power_sensitivity_t_device(bmc_ctx* ctx, const void* dA, int64_t n_points, int32_t k,
                                   int64_t lda, int layout, const void* dy, const void* dtheta,
                                   int64_t n_draws, int64_t ldt, const double* b0, const double* C0,
                                   double nu0, double sigma20, const double* Vt, int32_t n_models,
                                   const double* alphas, int32_t n_alphas, uint32_t components,
                                   int32_t cols_per_batch, double nu, double* logdens_out,
                                   double* pareto_k_out, double* mean_out, double* sd_out,
                                   double* cjs_out, double* weights_out, uint32_t* flags_out);
int bmc_power_sensitivity_tv(bmc_ctx* ctx, const double* A, int64_t n_points, int32_t k, int64_t lda,
                             int layout, const double* y, const double* theta, int64_t n_draws,
                             int64_t ldt, const double* b0, const double* C0, double nu0,
                             double sigma20, const double* Vt, int32_t n_models, const double* alphas,
                             int32_t n_alphas, uint32_t components, int32_t cols_per_batch,
                             const double* nu_values, int32_t n_values, const int32_t* nu_index,
                             const double* nu_log_prior, double* logdens_out, double* pareto_k_out,
                             double* mean_out, double* sd_out, double* cjs_out, double* weights_out,
                             uint32_t* flags_out);
int bmc_power_sensitivity_tv_device(bmc_ctx* ctx, const void* dA, int64_t n_points, int32_t k,
                                    int64_t lda, int layout, const void* dy, const void* dtheta,
                                    int64_t n_draws, int64_t ldt, const double* b0, const double* C0,
                                    double nu0, double sigma20, const double* Vt, int32_t n_models,
                                    const double* alphas, int32_t n_alphas, uint32_t components,
                                    int32_t cols_per_batch, const double* nu_values, int32_t n_values,
                                    const void* d_nu_index, const double* nu_log_prior,
                                    double* logdens_out, double* pareto_k_out, double* mean_out,
                                    double* sd_out, double* cjs_out, double* weights_out,
                                    uint32_t* flags_out);

/* ---- Student-t (outlier-robust) Gibbs sampler, many chains per launch (not in the reference) ----
 * The resident problem of bmc_set_problem (f64 storage, either layout, 1 <= k <= 32, n < 2^32) and
 * the prior of bmc_set_prior, with the likelihood y_n | beta, sigma2, lambda_n ~ N(x_n . beta,
 * sigma2 / lambda_n), lambda_n ~ Gamma(nu/2, rate nu/2): marginally t_nu(x_n . beta, sigma2); nu > 0
 * is fixed.  Start: lambda = 1, sigma2 = the OLS start of bmc_set_prior.  Sweep t = 0, 1, ..., burn-in
 * included (L = diag(lambda), P = inv(C0)):
 *   1. Q = X'LX / sigma2 + P + 1e-6 I = L_c L_c';  beta = Q^-1 (P b0 + X'Ly / sigma2) + L_c^-T xi_t
 *   2. r = y - X beta;  sigma2 = max(((nu0 sigma20 + sum lambda_n r_n^2) / 2) / G_t, 1e-6)
 *   3. lambda_n = g_{t,n} / ((nu + r_n^2 / sigma2) / 2)
 *   4. row t - burn of samples_out = [beta, sqrt(sigma2)] and lambda added to the rows' running sums
 *      (t >= burn)
 * with xi_t k standard normals, G_t ~ Gamma((nu0 + n) / 2, 1), g_{t,n} ~ Gamma((nu + 1) / 2, 1).
 * rng_mode BMC_RNG_DEVICE: seeds [n_chains]; xi and G are elements t k + j and t of the normal and
 *   gamma streams of bmc_rng_fill(seed), g_{t,n} is drawn in the kernel by Marsaglia-Tsang on the
 *   Philox counters (n, t lo, 0x524F4253, ((t >> 32) << 8) | attempt) (xi, g, gl must be NULL).
 * rng_mode BMC_RNG_REPLAY: xi [n_chains][burn+iters][k], g [n_chains][burn+iters] and
 *   gl [n_chains][burn+iters][n] are the caller's (meant for tests at small n; BMC_ENOMEM when gl
 *   does not fit the device).
 * samples_out [n_chains][iters][k+1]; row_weight_out [n_chains][n], the mean of lambda_n over the kept
 * sweeps (a per-row outlier score: far below 1 for a row the Gaussian model cannot reach), or NULL.
 * One workgroup per chain, all chains of a call side by side (launches of at most 1024); a chain
 * waits for no other workgroup.  CONTRACT: the order of every sum is fixed by (n, k) alone, so chain
 * c of any call is bit for bit the one-chain call with seeds[c] (or its replay streams), whatever
 * its index, its launch or the device, and identical calls agree bit for bit.
 * BMC_EINVAL (nothing is launched) for k > 32, a problem stored in f32, nu <= 0, n_chains < 1,
 * iters < 0, burn < 0.  A Cholesky pivot that is not positive and finite stops that chain (its later
 * rows and weights are NaN): BMC_ESINGULAR, bmc_last_error names the first such chain "(chain c)",
 * the other chains' results are still written.  stats: rng_ms, loop_ms, total_ms, iterations
 * (burn + iters), n_chains, launches.  bmc_robust_run_device is the device-RNG form writing
 * caller-owned DEVICE buffers (d_row_weight_out may be NULL); it returns after the stream has
 * drained. */
int bmc_robust_run(bmc_ctx* ctx, double nu, int32_t n_chains, int64_t iters, int64_t burn,
                   int rng_mode, const uint64_t* seeds, const double* xi, const double* g,
                   const double* gl, double* samples_out, double* row_weight_out, bmc_stats* stats);
int bmc_robust_run_device(bmc_ctx* ctx, double nu, int32_t n_chains, int64_t iters, int64_t burn,
                          const uint64_t* seeds, void* d_samples_out, void* d_row_weight_out,
                          bmc_stats* stats);

/* ---- The same sampler with the degrees of freedom estimated (not in the reference) ----
 * nu takes one of n_grid <= 64 values nu_grid[0] < ... < nu_grid[n_grid-1] (positive, finite) with
 * prior weights nu_weight[g] >= 0 (finite, at least one positive); it starts at nu_grid[nu_init], whose
 * weight must be positive.  Sweep t is steps 1-4 of bmc_robust_run with the nu in force (g_{t,n} ~
 * Gamma((nu + 1) / 2, 1) at that nu), then
 *   5. T_t = sum_n (log lambda_n - lambda_n) over the weights just drawn (the summation order of
 *      step 2's sum);
 *   6. l_g = fma(h_g, T_t, c_g), h_g = nu_g / 2, c_g = n (h_g log h_g - lgamma(h_g)) + log w_g (host,
 *      double; -inf where w_g = 0); m = max l_g; p_g = exp(l_g - m); P_0 = p_0, P_g = P_{g-1} + p_g
 *      strictly left to right; the new index is the number of g < n_grid - 1 with P_g < u_t P_{G-1}.
 *      A T_t that is not finite leaves the index where it was.
 *   7. nu_idx_out[c][t - burn] = the new index, tstat_out[c][t - burn] = T_t (t >= burn).
 * The state reported for sweep t is (beta_t, sigma_t, lambda_t, nu_t); nu_t shapes the weights of
 * sweep t + 1.
 * rng_mode BMC_RNG_DEVICE: as bmc_robust_run; u_t is the first uniform ((0, 1], 53 bits of words 0
 *   and 1) of Philox counter (t lo, t hi, 0x4E554446, 0) under the chain's key (u_nu, nu_path NULL).
 * rng_mode BMC_RNG_REPLAY: also u_nu [n_chains][burn+iters] and a FORCED path nu_path
 *   [n_chains][burn+iters] of grid indices: nu_path[t] is the index in force after sweep t, so the
 *   weights of sweep t are drawn at nu_grid[nu_path[t-1]] (nu_init for t = 0) and gl must hold gamma
 *   variates of those shapes.  The index the kernel would have picked from u_t is still computed and
 *   written to nu_idx_out; the chain continues on the forced path.
 * nu_idx_out [n_chains][iters] (rows a stopped chain never reached hold -1); tstat_out
 * [n_chains][iters] (rows a stopped chain never reached hold NaN, in d_tstat_out of the _device form
 * too) or NULL.  BMC_EINVAL (nothing is launched) for whatever bmc_robust_run refuses,
 * n_grid outside 1 .. 64, a grid that is not strictly increasing, positive and finite, weights that
 * are negative, not finite or all zero, nu_init out of range or of weight zero, a nu_path entry out of
 * range.  Everything else -- statuses, stats, launches of at most 1024 chains, chain c bit for bit its
 * one-chain call -- is as bmc_robust_run; a grid of one value gives the bits of bmc_robust_run at
 * that nu.  bmc_robust_run_nu_device writes caller-owned DEVICE buffers (d_nu_idx_out int32;
 * d_row_weight_out and d_tstat_out may be NULL). */
int bmc_robust_run_nu(bmc_ctx* ctx, const double* nu_grid, const double* nu_weight, int32_t n_grid,
                      int32_t nu_init, int32_t n_chains, int64_t iters, int64_t burn, int rng_mode,
                      const uint64_t* seeds, const double* xi, const double* g, const double* gl,
                      const double* u_nu, const int32_t* nu_path, double* samples_out,
                      double* row_weight_out, int32_t* nu_idx_out, double* tstat_out,
                      bmc_stats* stats);
int bmc_robust_run_nu_device(bmc_ctx* ctx, const double* nu_grid, const double* nu_weight,
                             int32_t n_grid, int32_t nu_init, int32_t n_chains, int64_t iters,
                             int64_t burn, const uint64_t* seeds, void* d_samples_out,
                             void* d_row_weight_out, void* d_nu_idx_out, void* d_tstat_out,
                             bmc_stats* stats);

/* ---- on-device variates (exposed so the generator itself can be tested) ----
 * normals_out [count_normal] ~ N(0,1); gammas_out [count_gamma] ~ Gamma(shape,1). */
int bmc_rng_fill(bmc_ctx* ctx, uint64_t seed, int64_t count_normal, double* normals_out,
                 double shape, int64_t count_gamma, double* gammas_out);
/* Raw Philox4x32-10 blocks: out[4*i..4*i+3] = philox(counter = (i_lo, i_hi, stream_id, 0),
 * key = seed) for i < nblocks4.  Integer output, checked bit-for-bit by the tests. */
int bmc_philox_raw(bmc_ctx* ctx, uint64_t seed, uint32_t stream_id, int64_t nblocks4,
                   uint32_t* out);

#ifdef __cplusplus
}
#endif
#endif /* PYBMC_AMD_H */
