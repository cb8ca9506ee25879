// Host-callable launchers of the gfx950 kernels (one per kernel family).  The loop kernels of
// launch_gibbs / launch_simplex are chosen on the host (bmc_plan.h, gibbs_kernel_key); gibbs_kernel /
// simplex_kernel below return the chosen instantiation for the residency and packing queries.
#pragma once
#include <cmath>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmc_plan.h"
#include "bmc_rank_plan.h"
#include "bmc_sens_plan.h"

namespace bmc {

// Storage description of the panelised problem (see bmc_dev.h "panel layout").
// u64 words between the granule pairs of consecutive groups in a (chain, parity) slot
#ifndef BMC_GRAN_PAIR_STRIDE
#define BMC_GRAN_PAIR_STRIDE 8
#endif
constexpr int GRAN_PAIR_STRIDE = BMC_GRAN_PAIR_STRIDE;
// u64 words of one (chain, parity) exchange slot: G <= 32 groups use pairs 0..G-1; larger
// chains use 8 team areas of 32 pairs, 8 team-total pairs and 8 relay pairs (bmc_loop.h,
// exchange_sum)
// (the 8 team-total pairs and the 8 relay pairs of the second level are written by one XCD each
// and polled by every group of the chain at agent scope: GRAN_L2_STRIDE words = 512 bytes
// apart.  Same-box A/B, us per iteration at 64 B / 128 B / 256 B / 512 B / 1 KiB per pair:
// N = 100 000 x 32 2.005 / 1.988 / 1.945 / 1.881 / 1.919, C4 3.291 / 3.241 / 3.156 / 3.131 / 3.164,
// N = 30 000 x 64 2.112 / 2.069 / 2.038 / 1.986 / 2.073 -- the polls of ~200 groups spread over
// the memory channels instead of landing on one or two)
#ifndef BMC_GRAN_L2_STRIDE
#define BMC_GRAN_L2_STRIDE 64
#endif
constexpr int GRAN_L2_STRIDE = BMC_GRAN_L2_STRIDE;
inline int gran_slot_words(int G) {
    return G <= 32 ? ((2 * G + 31) / 32) * 16 * GRAN_PAIR_STRIDE
                   : 256 * GRAN_PAIR_STRIDE + 16 * GRAN_L2_STRIDE;
}

struct Panels {
    const void* X;   // [NP][K][RP] of T
    const void* y;   // [NP*RP] of T
    int64_t n;       // true row count
    int32_t k;
    int32_t vec;     // rows per lane (RP = 64*vec)
    int32_t npanels;
    int32_t f32;     // 1: T = float, 0: T = double
    int32_t stream_keep;  // streaming loop: a group's first stream_keep panels are read with
                          // ordinary loads (they stay in the XCD's L2 from one iteration to
                          // the next), the others with non-temporal loads
};

// ---- set-up ----------------------------------------------------------------
// user layout (row/col-major, f32/f64, host-uploaded or device) -> panels
hipError_t launch_panelize(const void* Xsrc, const void* ysrc, int64_t n, int32_t k,
                           int64_t ldx, int col_major, int f32, int32_t vec,
                           void* Xp, void* yp, int32_t npanels, hipStream_t s);

// Augmented Gram [X y]'[X y] with v_mfma_f64_16x16x4_f64.  gram_out is
// (k+1)x(k+1) row-major f64.  scratch: >= gram_scratch_bytes().
size_t gram_scratch_bytes(const Panels& P);
hipError_t launch_gram(const Panels& P, void* scratch, double* gram_out, hipStream_t s);

// Xrot = X * W (W is P.k x ko row-major, device); output panels have ko columns, same
// rows per lane and storage type.
hipError_t launch_rotate(const Panels& P, const double* W, int32_t ko, void* Xrot, hipStream_t s);

// orthogonalize helpers: centring into panels, panels -> column-major
hipError_t launch_centre(const double* F, int64_t n, int32_t km, int64_t ldf, const double* truth,
                         int32_t vec, int32_t npanels, double* Fc, double* yc, double* mu,
                         hipStream_t s);
hipError_t launch_unpanelize(const double* Xp, int64_t n, int32_t k, int32_t vec, double* out,
                             hipStream_t s);

// rss[b] = sum_i (y_i - sum_j X_ij coef[b][j])^2, b < nb (nb <= 8), one launch.
// partial: >= rss_groups(P) * 8 doubles of scratch; ticket_word: RSS_TICKET_BYTES of zeroed u32 that
// the kernel leaves zero again.
constexpr int RSS_TICKETS = 16, RSS_TICKET_STRIDE = 128;   // u32 words: 512 bytes between ticket words
// (RSS_FLAT_TICKET_MAX, the flat / two-level threshold, and rss_groups_of(npanels): bmc_plan.h)
constexpr size_t RSS_TICKET_BYTES = (size_t)(RSS_TICKETS + 1) * RSS_TICKET_STRIDE * 4;
int32_t rss_groups(const Panels& P);
hipError_t launch_residual_rss(const Panels& P, const double* coef, int32_t nb,
                               double* partial, unsigned* ticket_word, double* rss_out,
                               hipStream_t s);

// samples[c][t][0..k) = W u[c][t][0..k);  samples[c][t][k] = u[c][t][k]
hipError_t launch_unrotate(const double* uout, const double* W, int32_t k, int64_t rows,
                           double* samples, hipStream_t s);

// ---- variates ---------------------------------------------------------------
// normals[c][e], e < per_chain_normals; gammas[c][t], t < per_chain_gammas
hipError_t launch_rng_fill(const uint64_t* seeds_dev, int32_t n_chains,
                           int64_t per_chain_normals, double* normals, double shape,
                           int64_t per_chain_gammas, double* gammas, hipStream_t s);
hipError_t launch_philox_raw(uint64_t seed, uint32_t stream, int64_t nblocks4,
                             uint32_t* out, hipStream_t s);

// ---- posterior predictive --------------------------------------------------------
struct PredictArgs {
    const double* preds;   // [M][Km]
    int64_t M;
    int32_t Km, k, S;      // models, kept components, draws
    int32_t S_pad, Km_pad; // multiples of 64 and 4
    int64_t M_pad;         // points rounded up to whole 64-point tiles
    double* P;             // [M_pad][Km_pad] + 16 doubles of slack: preds zero-padded (scratch)
    const double* theta;   // [S][k+1] selected posterior rows
    const double* Vt;      // [k][Km]
    double* Wt;            // [S_pad][Km_pad] + 16 doubles of slack, scratch
    double* sig;           // [S_pad] scratch
    uint64_t seed;
    const double* noise_replay;  // [S][M] or NULL (device generator)
    // Student-t noise, device generator only (both unset: standard normals).  nu > 0: t noise with
    // nu degrees of freedom for every draw.  nus (nu stays 0): [2][S_pad], nu_s then 2 / nu_s, the
    // padded draws holding 4 and 1/2; z[p][s] = student_t_variate (bmc_math.h) of the two uniforms
    // of counter (e lo, e hi, STREAM_PRED_T, 0), e = p S + s.
    double nu = 0.0;
    const double* nus = nullptr;
    double* R;             // [M_pad][S_pad]
    const int32_t* q_index;
    const double* q_gamma;
    int32_t n_q;
    const double* truth;   // [M] or NULL
    const int32_t* cov_lo;
    const int32_t* cov_hi;
    int32_t n_cov;
    double* bands;         // [n_q][M]
    unsigned long long* hits;  // [n_cov], zeroed
    int32_t* fail_points;  // [M] points the selection kernel hands to the sort kernel (or NULL)
    int32_t* fail_count;   // [1], zeroed
    hipEvent_t ev_mid = nullptr;  // recorded between the GEMM and the order statistics (or NULL)
};
hipError_t launch_predict(const PredictArgs& a, hipStream_t s);
// out[s][p] = R[p][s]: the draws as the reference's C-ordered (n_draws, n_points) array
hipError_t launch_transpose_draws(const double* R, int64_t M, int32_t S, int32_t S_pad, double* out,
                                  hipStream_t s);

// ---- the persistent Gibbs loop ------------------------------------------------
struct GibbsArgs {
    Panels P;               // ROTATED panels
    const double* lam;      // [k]
    const double* c1;       // [k]  W' P b0
    const double* c2;       // [k]  W' X'y
    double nu0_s20;         // nu0 * sigma20
    double sigma2_init;
    const double* xi;       // [C][T][k]
    const double* gam;      // [C][T]
    double* uout;           // [C][T][k+1]
    unsigned long long* gran;  // [C][3][gran_stride]: 2 parities of granules + XCC words, zeroed
    int32_t gran_stride;    // u64 words per (chain, parity), >= 2*G, multiple of 32
    int32_t* status;        // [C] 0 ok, 1 timeout
    int64_t iters;
    int32_t n_chains;       // chains in THIS launch
    int32_t G;              // workgroups per chain
    int32_t waves;          // waves per workgroup
    int32_t mode;           // 0 registers, 1 LDS, 2 streaming
    int32_t reg_ppw;        // panels per wave (register mode)
    int32_t nslot;          // grid = nslot x G; 8 = one slot per XCD, else = n_chains
    int32_t force_agent_scope;  // 1: never use the XCD-local exchange
    int32_t chains_per_pass;  // > 1: gibbs_multi_kernel, bundles of that many chains
    uint32_t epoch0 = 0;      // nonce of this launch: exchange tags are epoch0 + t + 1, placement
                              // words carry it in their high half (host: never lets a tag be 0)
    int32_t bundle_bal = 0;   // 1: bundles of 8 in the balanced two-panels-per-wave layout (<= 5 panels
                              // per group, 8 waves; PanelStore::partial_rss_reg_bal)
    int32_t bundle_slots = 0; // gibbs_multi_kernel: 0 = ONE bundle, grid = G (a chain over the whole
                              // chip); > 0 = grid = bundle_slots x G, bundle b = blockIdx % slots
                              // (one bundle per XCD: chains b * cpp .. b * cpp + cpp - 1), n_chains
                              // = bundles * chains_per_pass, unused slots leave at once
    int32_t* placement;     // [C] out: 1 = chain verified on one XCD (L2-local exchange)
    int32_t panels_per_group;  // max panels a group owns
    long long* dbg;         // diagnostic builds only (-DBMC_STAMPS); NULL otherwise
    // (host-only from here on: no kernel reads the fields below)
    int32_t pack;           // 1: launch the packed variant (two chains per XCD)
    int32_t one_wave = 0;   // 1: gibbs_wave_kernel, one wave per chain (gibbs_wave_capacity() > 0)
};
// rss from sufficient statistics (bmc_tuning.rss_mode = 1): one wave per chain, K <= 64
struct GramArgs {
    int32_t k;
    const double* lam;      // [k]
    const double* c1;       // [k]
    const double* c2;       // [k]
    const double* Gt;       // [k][k]  X~'X~ (symmetric)
    const double* u0;       // [k]     centre of the expansion (least-squares point)
    const double* g0;       // [k]     X~'(y - X~ u0)
    double rss0;            // rss(u0), from one residual pass
    double nu0_s20, sigma2_init;
    const double* xi;       // [C][T][k]
    const double* gam;      // [C][T]
    double* uout;           // [C][T][k+1]
    int64_t iters;
    int32_t n_chains;
};
hipError_t launch_gibbs_gram(const GramArgs& a, hipStream_t s);

// Per-chain arrays are indexed by the chain of the launch (wave form: chain = blockIdx.x;
// workgroup form: chain = blockIdx.x % nslot, group = blockIdx.x / nslot, slots >= n_chains leave at
// once).  Chains share the panels, Vt_hat and the step and nothing else: they never synchronise.
struct SimplexArgs {
    Panels P;               // UN-rotated panels (the simplex sampler proposes beta itself)
    const double* Vt;       // [k][Km]  Vt_hat
    int32_t Km;
    int32_t vt_in_lds;      // Vt_hat kept in LDS (k*Km <= 4096 doubles)
    const double* step;     // [k]  S_hat * stepsize
    double nu0_s20;
    double rss_init;        // sum y^2 (beta = 0: every chain starts there)
    const double* xi;       // [C][burn+iters][k]
    const double* unif;     // [C][unif_ld]
    int64_t unif_ld;        // doubles between the uniform streams of consecutive chains
    const int64_t* n_unif;  // [C] (device) uniforms chain c may consume
    const double* gam;      // [C][burn+iters]
    double* out;            // [C][iters][k+1]
    unsigned long long* gran;  // [C][3][gran_stride], zeroed (as in GibbsArgs)
    int32_t gran_stride;
    int32_t* status;        // [C] 0 ok, 1 timeout, 2 uniforms exhausted
    int32_t* placement;     // [C]
    long long* counters;    // [C][2] accepted (sampling phase), uniforms consumed
    int64_t iters, burn;
    int32_t n_chains;       // chains in THIS launch
    int32_t G, waves, mode, reg_ppw, nslot, force_agent_scope, panels_per_group;
    uint32_t epoch0 = 0;    // as in GibbsArgs
    int32_t one_wave = 0;   // host-only. 1: simplex_wave_kernel (gibbs_wave_capacity() > 0, Km <= 64)
};
size_t simplex_lds_bytes(const SimplexArgs& a);
// (launched: as for launch_gibbs)
hipError_t launch_simplex(const SimplexArgs& a, hipStream_t s, KernelKey* launched = nullptr);
// uniforms in (0,1]: out[i] = u53(philox(counter = (i, STREAM_UNIFORM), key = seed))
hipError_t launch_uniform_fill(uint64_t seed, int64_t n, double* out, hipStream_t s);
// the same for n_chains seeds (device): out[c * ld + i], i < n, is what launch_uniform_fill(seeds[c],
// n, out + c * ld) writes -- the counter is the index within the chain, the key the chain's seed
hipError_t launch_uniform_fill_chains(const uint64_t* seeds_dev, int32_t n_chains, int64_t n, int64_t ld,
                                      double* out, hipStream_t s);

size_t gibbs_lds_bytes(const GibbsArgs& a);
// launched (optional): the key of the instantiation the launcher looked up and launched
hipError_t launch_gibbs(const GibbsArgs& a, hipStream_t s, KernelKey* launched = nullptr);

// The kernel that launch_gibbs / launch_simplex would launch for these arguments: the
// instantiation of bmc_plan.h's gibbs_kernel_key / simplex_kernel_key, its grid, block and dynamic
// LDS bytes.  fn = nullptr when the arguments fail the launcher's checks or no such kernel is
// compiled (the launcher then returns hipErrorInvalidValue).  The host asks the runtime about fn
// itself: occupancy before a persistent launch (check_residency), registers of the packed variant.
struct LoopKernel {
    const void* fn;
    dim3 grid, block;
    size_t lds;
    KernelKey key;   // the instantiation fn is (family KF_NONE with fn = nullptr)
};
LoopKernel gibbs_kernel(const GibbsArgs& a);
LoopKernel simplex_kernel(const SimplexArgs& a);

// ---- chain diagnostics (kernels_diag.hip) -------------------------------------------
// Samples [C][iters][ld] f64, column j < P.  Each chain drops `burn` draws and splits the
// T' = iters - burn kept ones into two halves of n = T'/2 draws: sequence 2c + h starts at
// row burn + h * half_off (half_off = T' - n).  Sequences 2C .. 3C-1 exist when T' is odd: the
// middle draw of each chain, for the pooled mean and sd only.
struct DiagShape {
    const double* x;
    int64_t iters, ld, burn, n, half_off;
    int32_t C, P, n_seq;
};
// mean[m][j] = mean of (x - shift_j), m2[m][j] = sum (x - mean)^2 of sequence m < n_seq, and
// mean[n_seq][j] = shift_j, the column's first kept draw of chain 0 (device, [n_seq + 1][P] and
// [n_seq][P]); scratch >= diag_moments_scratch() bytes
size_t diag_moments_scratch(const DiagShape& d);
hipError_t launch_diag_moments(const DiagShape& d, double* scratch, double* mean, double* m2,
                               hipStream_t s);
// acov_out[a][lc*64 + l] = mean over the 2C halves of (1/n) sum_i d_i d_{i+t}, t = t0 + lc*64 + l,
// for column cols[a], a < n_active, lags t0 .. t0 + n_lags (rounded up to 64; lags >= n give 0).
// acov_out is [n_active][ceil(n_lags/64)*64]; scratch >= diag_acov_scratch() bytes.
size_t diag_acov_scratch(const DiagShape& d, int32_t n_active, int64_t n_lags);
hipError_t launch_diag_acov(const DiagShape& d, const double* mean, const int32_t* cols,
                            int32_t n_active, int64_t t0, int64_t n_lags, double* scratch,
                            double* acov_out, hipStream_t s);

// ---- rank normalisation (kernels_rank.hip; plan_rank in bmc_rank_plan.h) -----------------------------
// A batch of Pb columns col0 .. col0 + Pb - 1 of the samples of a DiagShape.  Split draw e < S = 2 C n
// of a column is draw e % n of sequence e / n (sequence 2c + h as above); e is also its row in a
// derived buffer [C][2n][ld_d].  Segment jb of a key / index buffer is [jb * S, (jb + 1) * S).
// Outputs per draw go to out[jb * seg_stride + e * ld_d + col]: seg_stride = S * ld_d gives every
// column a buffer [C][2n][ld_d] of its own, seg_stride = 1 and ld_d = Pb one [S][Pb] array.
struct RankShape {
    const double* x;
    int64_t iters, ld, burn, n, half_off, S, tiles;
    int32_t C, col0, Pb;
};
// keys[jb][e] = rank_key(x), idx[jb][e] = e; flags[jb] = 1 when the column holds a non-finite value;
// or_and[jb] = {OR, AND} of the segment's keys (integer atomics: the result is order-free)
hipError_t launch_rank_gather(const RankShape& r, uint64_t* keys, uint32_t* idx, uint64_t* or_and,
                              uint32_t* flags, hipStream_t s);
// One stable counting pass on digit `digit` (bits 8 digit .. 8 digit + 7) of every segment, from
// (kin, iin) to (kout, iout).  hist: [Pb][tiles][256] u32 of scratch.
hipError_t launch_rank_sort_pass(const RankShape& r, int digit, const uint64_t* kin, const uint32_t* iin,
                                 uint64_t* kout, uint32_t* iout, uint32_t* hist, hipStream_t s);
// From SORTED segments: the output of draw idx is ndtri((rank - 3/8) / (S + 1/4)), rank the
// 1-based average rank of the key's run of equal keys (runs may cross tiles)
hipError_t launch_rank_z(const RankShape& r, const uint64_t* keys, const uint32_t* idx, double* out,
                         int64_t seg_stride, int64_t ld_d, int32_t col, hipStream_t s);
// Order statistics of SORTED segments: q[jb][t] = lerp(x_(index[t]), x_(index[t] + 1), weight[t]),
// t < n, with the interpolation of the predictive leg; q is [Pb][RANK_Q_SLOTS]
struct RankQuantiles {
    int32_t n;
    int32_t index[RANK_Q_SLOTS];
    double weight[RANK_Q_SLOTS];
};
hipError_t launch_rank_pick(const RankShape& r, const uint64_t* keys, const RankQuantiles& rq, double* q,
                            hipStream_t s);
// In place: key -> rank_key(|x - q[jb][med_slot]|), x the value of the key; or_and as in the gather
hipError_t launch_rank_fold(const RankShape& r, uint64_t* keys, const double* q, int32_t med_slot,
                            uint64_t* or_and, hipStream_t s);
// the outputs of draw e at col_lo and col_hi: x <= q[jb][slot_lo] ? 1.0 : 0.0, and the same with slot_hi
hipError_t launch_rank_indicators(const RankShape& r, const double* q, int32_t slot_lo, int32_t slot_hi,
                                  double* out, int64_t seg_stride, int64_t ld_d, int32_t col_lo, int32_t col_hi,
                                  hipStream_t s);

// ---- pointwise log-likelihood (kernels_waic.hip; plan_score in bmc_plan.h) ---------------------
// ll[i][s] = -1/2 log(2 pi) - log sigma_s - (y_i - a_i . beta_s)^2 / (2 sigma_s^2) for design rows
// A (n x k, element (i, j) at i*lda + j, or j*lda + i when col_major), targets y [n] and draws
// theta (row s at theta + s*ldt: k coefficients, then sigma_s).  Per point, over the S draws:
// out[0][i] = logsumexp_s ll - log S, out[1][i] = var_s ll (ddof 1), out[2][i] = mean_s ll
// (out is [3][n], device).  The n x S matrix is never stored.  Work buffers (device, sized by
// score_buffers for the plan): Ap [n_pad][k_pad] and yp [n_pad], the operands padded to whole
// tiles; ch [2][S], the per-draw constants; part [splits][n_pad][5], the per-split partials.
// nu > 0 selects the Student-t density with nu degrees of freedom (bmc_score_tile.h, TileDrawsT):
// ll[i][s] = lgamma((nu + 1)/2) - lgamma(nu/2) - 1/2 log(nu pi) - log sigma_s
//            - (nu + 1)/2 log1p((y_i - a_i . beta_s)^2 / (nu sigma_s^2));  nu = 0 is the Gaussian one.
// A Student-t likelihood (or noise) with a nu of its own for every draw: n_nu > 0 distinct values and
// every draw's index into them (a scalar nu beside it stays 0).  Host-only: the kernels take the
// members as scalars and pointers.  All DEVICE pointers.  The host side of it is stage_nu (bmc_ctx.h).
enum NuTable { NU_SCORE = 0, NU_PPC = 1, NU_SENS = 2 };
struct NuPerDraw {
    int32_t n_nu = 0;
    // [rows][n_nu], a row per quantity of the distinct values (nu_table below): NU_SCORE [cnu, nu]
    // (cnu = student_t_cnu), NU_PPC [nu, 2 / nu], NU_SENS [cnu, nu, log prior of nu]
    const double* tab = nullptr;
    // [S] int32 into the values, clamped into range in the kernel (nu_index_clamped, bmc_dev.h).
    // NU_SENS only: NULL is entry 0 for every draw (a fixed nu is a table of one value)
    const int32_t* index = nullptr;
    int32_t* flag = nullptr;   // one int32 word the caller has zeroed; 1: an index was out of range
    // what every launcher asks: unset, or 1 .. max_values values with their table and flag word, an
    // index (unless NULL is allowed) and no scalar nu beside them
    bool valid(double nu, int32_t max_values, bool null_index_ok = false) const {
        return n_nu == 0 || (n_nu > 0 && n_nu <= max_values && nu == 0.0 && tab && flag && (index || null_index_ok));
    }
};

struct ScorePlan;
struct ScoreArgs {
    const double* A;
    const double* y;
    const double* theta;
    int64_t n, lda, S, ldt;
    int32_t k, col_major;
    double *Ap, *yp, *ch, *part, *out;
    double nu = 0.0;   // host-only: the likelihood (0: Gaussian; else positive and finite)
    NuPerDraw per_draw;   // host-only: set, the Student-t density with a nu per draw (TileDrawsTV; NU_SCORE)
};
// lgamma((nu + 1)/2) - lgamma(nu/2) - 1/2 log(nu pi), the constant of the t_nu density, in long
// double: the difference of the two lgamma loses digits as nu grows
inline double student_t_cnu(double nu_) {
    const long double nu = (long double)nu_;
    return (double)(lgammal(0.5L * (nu + 1.0L)) - lgammal(0.5L * nu) -
                    0.5L * logl(nu * 3.14159265358979323846264338327950288L));
}
// The table of a NuPerDraw of `shape` for V values: tab [nu_table_rows(shape)][V].  2 / nu is rounded
// here, once per value; log_prior is read for NU_SENS alone (NULL: zeros)
inline int nu_table_rows(NuTable shape) { return shape == NU_SENS ? 3 : 2; }
inline void nu_table(NuTable shape, const double* values, const double* log_prior, size_t V, double* tab) {
    for (size_t v = 0; v < V; ++v) {
        const double nu = values[v];
        tab[v] = shape == NU_PPC ? nu : student_t_cnu(nu);
        tab[V + v] = shape == NU_PPC ? 2.0 / nu : nu;
        if (shape == NU_SENS) tab[2 * V + v] = log_prior ? log_prior[v] : 0.0;
    }
}
// The staging of every scorer (kernels_waic.hip): A (n x k, either layout, any lda) -> Ap
// [n_pad][k_pad] in whole 64-point tiles and 16-column slabs, y -> yo [n_pad], zero in the padding.
// offset_row: yo has a second row, yo[n_pad + i] = offset[i] (zeros when offset is NULL).
hipError_t launch_pad_points(const double* A, const double* y, const double* offset, bool offset_row,
                             int64_t n, int32_t k, int64_t lda, int32_t col_major, int64_t n_pad,
                             int32_t k_pad, double* Ap, double* yo, hipStream_t s);
struct ScoreBuffers {
    size_t Ap, yp, ch, part;   // bytes
};
ScoreBuffers score_buffers(const ScorePlan& p, int64_t n_draws);
hipError_t launch_score(const ScoreArgs& a, const ScorePlan& p, hipStream_t s);

// ---- PSIS-LOO (kernels_loo.hip; plan_loo in bmc_plan.h) -----------------------------------------
// Pareto-smoothed importance-sampling leave-one-out of the same model and arguments as
// launch_score (whose kernels run first, into `score`'s buffers: score.out[0][i] = lppd_i).  work:
// loo_buffers(plan, n).total() bytes (device, 256-byte aligned); its `out` part, at loo_out(),
// receives elpd_loo_i [n] then pareto_k [n].  The likelihood is score.nu.
struct LooArgs {
    ScoreArgs score;
    void* work;
    // launch_loo_predict under the t likelihood: some nu in use is <= 2, so loo_sd is +inf wherever
    // it is not NaN (decided on the host: the device never sums an infinite variance)
    bool t_sd_inf = false;
};
double* loo_out(const LooArgs& a, const LooPlan& p);
hipError_t launch_loo(const LooArgs& a, const LooPlan& p, hipStream_t s);

// The leave-one-out predictive moments of every point with the same weights.
// work: loo_predict_buffers(plan, n).total() bytes; at loo_predict_out(): elpd_loo_i, pareto_k,
// loo_mean, loo_sd, loo_pit, ess, [n] each.  Under the t likelihood (score.nu > 0 or score.per_draw;
// the plan made with student = true; nu within STUDENT_T_CDF_NU_MIN .. _MAX of bmc_math.h, which the
// caller checks) loo_sd carries sigma_s^2 nu_s / (nu_s - 2) and loo_pit the t distribution function.
double* loo_predict_out(const LooArgs& a, const LooPredictPlan& p);
hipError_t launch_loo_predict(const LooArgs& a, const LooPredictPlan& p, hipStream_t s);

// ---- posterior predictive check (kernels_ppc.hip; plan_ppc in bmc_plan.h) -------------------------
// Replicated data y_rep[i][s] = a_i . beta_s + sigma_s z[i][s] + offset_i of the model and
// arguments of launch_score, z from the STREAM_PPC variates of `seed`, reduced over
// the points per draw and never stored.  t_rep [S][PPC_STATS]: min, max, mean, sd, skew, kurt of
// y_rep[.][s] (moments with ddof 0, from the power sums of y_rep - c_s, c_s = a_bar . beta_s +
// mean(offset) the draw's own centre, formed on the device), sum_i z^2, max_i |z|;
// t_obs2 [S][PPC_OBS]: sum_i ((y_i - a_i . beta_s) / sigma_s)^2 and max_i |y_i - a_i . beta_s| /
// sigma_s.  offset may be NULL (zeros).  `center` is no longer read (the C ABI keeps the argument).
// A value is NaN exactly where these definitions give NaN, and all ten of a draw with a non-finite
// coefficient or without a finite sigma > 0 are NaN.  Work buffers (device, sized by ppc_buffers
// for the plan): Ap, yo, Tp, sg.  No atomics, one workgroup per 64 draws: the bits depend on the
// arguments alone.
struct PpcArgs {
    const double* A;
    const double* y;
    const double* offset;
    const double* theta;
    int64_t n, lda, S, ldt;
    int32_t k, col_major;
    uint64_t seed;
    double center;
    double *Ap, *yo, *Tp, *sg, *t_rep, *t_obs2;
    // The noise: nu = 0 and per_draw unset, the standard normals above.  nu > 0 (finite): z is
    // Student-t with nu degrees of freedom, student_t_variate (bmc_math.h) of the two uniforms of
    // counter (s lo, s hi, STREAM_PPC_T, i).  per_draw set (NuPerDraw, NU_PPC, at most
    // PPC_MAX_NU_VALUES values): a nu per draw, and nus the work buffer of ppc_nu_bytes(plan) bytes.
    // The sums, the moments and the NaN rules do not depend on the noise.
    double nu = 0.0;
    NuPerDraw per_draw;
    double* nus = nullptr;
};
hipError_t launch_ppc(const PpcArgs& a, const PpcPlan& p, hipStream_t s);

// ---- power-scaling sensitivity (kernels_sens.hip; plan_sens in bmc_sens_plan.h) -----------------
// Per draw s of theta (row s at theta + s*ldt: k coefficients, then sigma_s):
//   lp[0][s] = -1/2 |Lp beta_s - Ly|^2   (Lp = L^-1, Ly = L^-1 b0 for C0 = L L', padded as Ap / yo)
//   lp[1][s] = -(nu0/2 + 1) log sigma_s^2 - nu0 sigma20 / (2 sigma_s^2)
//   lp[2][s] = -(n/2) log 2 pi - n log sigma_s - sum_i (y_i - a_i . beta_s)^2 / (2 sigma_s^2)
// all NaN for a draw with a non-finite coefficient or without a finite sigma_s > 0; comps [.][S]:
// the vectors of the set bits of `components` in bit order (lp0 + lp1, lp2, lp0, lp1); omega
// [S][n_models] = beta_s . Vt + 1 / n_models (Vt [k][n_models]).  Work: Tp [S_pad][k_pad], rss [2][S].
struct SensLogdensArgs {
    const double *theta, *Ap, *yo, *Lp, *Ly, *Vt;
    int64_t S, S_pad, ldt, n, n_pad, q_pad;
    int32_t k, k_pad, n_models;
    uint32_t components;
    double nu0, sigma20;
    double *Tp, *rss, *lp, *comps, *omega;
    // host-only: per_draw set (NuPerDraw, NU_SENS, at most SENS_MAX_NU_VALUES values; its index may
    // be NULL) selects the Student-t likelihood (the Gaussian kernels are not launched):
    //   lp[2][s] = n (C(nu_s) - log sigma_s) - (nu_s + 1)/2 sum_i log1p((y_i - a_i . beta_s)^2 / (nu_s sigma_s^2))
    //   lp[3][s] = the log prior of nu_s (a fourth row), comps of the bits (lp0 + lp1 + lp3, lp2, lp0, lp1, lp3)
    // tc [SENS_T_STAGED][S] work: g, hn, c, nu and lp_nu per draw (tc + 3 S is the nu column).
    NuPerDraw per_draw;
    double* tc = nullptr;
};
constexpr int SENS_T_STAGED = 5;
hipError_t launch_sens_logdens(const SensLogdensArgs& a, hipStream_t s);
// Column j of a batch is p0[e * rs0 + j] for j < n0, else p1[e * rs1 + (j - n0) * cs1], e < S; from
// column n1 on it is p2[e] (one more column behind the two sources: the nu of every draw)
struct SensSource {
    const double *p0, *p1;
    int64_t rs0, rs1, cs1;
    int32_t n0;
    const double* p2 = nullptr;
    int32_t n1 = 0x7fffffff;
};
// The gather of launch_rank_gather from a SensSource (kernels_rank.hip: the same kernel over another
// loader): segment jb of keys / idx starts at jb * seg_stride and takes the S draws of column col0 + jb
hipError_t launch_key_gather(const SensSource& src, int64_t S, int64_t seg_stride, int32_t col0, int32_t Pb,
                             uint64_t* keys, uint32_t* idx, uint64_t* or_and, uint32_t* flags, hipStream_t s);
// That gather on segments of sens_padded(S) pairs: the S draws in draw order and, when
// S is odd, one pad key that no real key exceeds (it stays last under the stable sort and adds no
// live pass); or_and and flags over the real keys
hipError_t launch_sens_gather(const SensSource& src, int64_t S, int32_t col0, int32_t Pb, uint64_t* keys,
                              uint32_t* idx, uint64_t* or_and, uint32_t* flags, hipStream_t s);
// keys / idx: the SORTED segments of the n_components component vectors.  Workgroup
// w = c * n_alphas + a: Wt[s][w] = the Pareto-smoothed normalised weight of draw s, khat[w] its
// pareto_k (+inf: nothing smoothed).  W = n_components * n_alphas; xs: [W][max(M, 1)] f64 scratch.
hipError_t launch_sens_psis(const uint64_t* keys, const uint32_t* idx, int64_t S, int32_t n_components,
                            int32_t n_alphas, const double* d_alphas, double* xs, double* Wt, double* khat,
                            hipStream_t s);
// keys / idx: the SORTED segments of Pb quantity columns.  out[jb][w][3] = cjs, weighted mean,
// weighted sd of column jb under weight vector w.  offs [Pb][W][chunks], part [Pb][W][chunks][SENS_PART].
hipError_t launch_sens_cjs(const uint64_t* keys, const uint32_t* idx, int64_t S, int32_t Pb, int32_t W,
                           const double* Wt, double* offs, double* part, double* out, hipStream_t s);

}  // namespace bmc
