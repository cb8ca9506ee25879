// C ABI of libpybmc_amd.so (see include/pybmc_amd.h).  Host orchestration only:
// every O(N) step is a gfx950 kernel; the host does the one-off K x K algebra (the prior basis:
// bmc_basis.h, shared with capi_cv.hip).
// This file: the context and what every family shares (bmc_ctx.h), problem, prior, getters,
// RSS and Gram, variates.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <thread>

#include "bmc_basis.h"
#include "bmc_ctx.h"

// Base of a persistent launch's exchange tags (GibbsArgs.epoch0): different for every launch
// (splitmix64 of a per-context counter), so that words an earlier launch left behind -- in the
// exchange buffer the launch re-zeroes, or in a cache that still holds a line of it -- can never
// be taken for this launch's.  Tags are epoch0 + 1 .. epoch0 + n_tags; none may be 0 (the
// zeroed state), so the base keeps them below 2^32 when the run is short enough to allow it.
uint32_t launch_nonce(bmc_ctx* c, uint64_t n_tags) {
    uint64_t z = (c->nonce_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    const uint64_t room = 0xffffffffull - (n_tags + 1);   // largest base with no wrap
    if (n_tags + 2 >= 0xffffffffull) return 0;
    return (uint32_t)(1 + z % room);
}

int fail(bmc_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    return code;
}

int ensure(bmc_ctx* c, DevBuf& b, size_t bytes) {
    if (bytes == 0) bytes = 16;
    if (b.cap >= bytes) return BMC_OK;
    if (b.p) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipFree(b.p));
        b.p = nullptr;
        b.cap = 0;
    }
    HIPCHK(c, hipMalloc(&b.p, bytes));
    b.cap = bytes;
    return BMC_OK;
}

int ensure_all(bmc_ctx* c, std::initializer_list<Want> wants) {
    for (const Want& w : wants)
        if (int rc = ensure(c, w.b, w.bytes)) return rc;
    return BMC_OK;
}

// Device -> caller-owned (pageable) host memory.  A plain hipMemcpy into fresh numpy memory
// pins the destination pages first, which costs far more than the transfer for the sizes that
// matter here (13.2 MB of samples at C2: 29 ms, against 0.3 ms of DMA -- bench.py extra.e2e).
// Instead: DMA into two pinned staging blocks in turn and copy out of one with the CPU while the
// next is in flight; large results are copied out by several host threads (one thread moves
// ~8 GB/s into untouched pages, the 4 GB of C5's rndm_m would take 0.5 s): 8 threads from 8 MB on.
constexpr size_t HSTAGE_BYTES = (size_t)32 << 20;
static void host_copy(char* dst, const char* src, size_t bytes) {
    const size_t MT_MIN = (size_t)8 << 20;
    // (C5's 4 GB of draws, whole bmc_predict call: 2 threads 0.184 s, 4 0.119, 8 0.097, 16 0.093)
    unsigned nt = bytes >= MT_MIN ? 8 : 1;
    const unsigned hw = std::thread::hardware_concurrency();
    if (hw && nt > hw) nt = hw;
    if (nt <= 1) {
        std::memcpy(dst, src, bytes);
        return;
    }
    std::vector<std::thread> th;
    const size_t per = ((bytes / nt) + 4095) & ~(size_t)4095;
    for (unsigned i = 0; i < nt; ++i) {
        const size_t off = (size_t)i * per;
        if (off >= bytes) break;
        const size_t n = bytes - off < per ? bytes - off : per;
        th.emplace_back([=] { std::memcpy(dst + off, src + off, n); });
    }
    for (auto& t : th) t.join();
}

// rows of `row_bytes` taken every `src_pitch` bytes on the device, written densely to `dst`
// (src_pitch == row_bytes: one contiguous block of row_bytes * rows).  Blocks until the data is
// in `dst`.
int copy_to_host(bmc_ctx* c, void* dst, const void* src_dev, size_t row_bytes, size_t src_pitch,
                 size_t rows) {
    if (row_bytes == 0 || rows == 0) return BMC_OK;
    for (int i = 0; i < 2; ++i) {
        if (!c->hstage[i] && hipHostMalloc(&c->hstage[i], HSTAGE_BYTES, hipHostMallocDefault) != hipSuccess) {
            c->hstage[i] = nullptr;
            (void)hipGetLastError();
        }
        if (!c->hev[i] && hipEventCreateWithFlags(&c->hev[i], hipEventDisableTiming) != hipSuccess)
            c->hev[i] = nullptr;
    }
    const bool dense = src_pitch == row_bytes;
    const bool staged = c->hstage[0] && c->hstage[1] && c->hev[0] && c->hev[1] &&
                        (dense || row_bytes <= HSTAGE_BYTES);
    if (!staged) {   // (no pinned memory to be had: the plain route)
        HIPCHK(c, hipMemcpy2DAsync(dst, row_bytes, src_dev, src_pitch, row_bytes, rows,
                                   hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return BMC_OK;
    }
    // pieces: dense -> byte ranges of at most one staging block; pitched -> whole rows
    const size_t total = dense ? row_bytes * rows : rows;          // bytes, or rows
    const size_t per = dense ? HSTAGE_BYTES : HSTAGE_BYTES / row_bytes;
    const size_t unit = dense ? 1 : row_bytes;                     // host bytes per unit of `total`
    char* out = (char*)dst;
    size_t issued = 0;
    size_t p_n[2] = {0, 0}, p_off[2] = {0, 0};
    bool pending[2] = {false, false};
    int next = 0;   // slot of the next transfer; the other slot holds the older pending one
    while (issued < total || pending[0] || pending[1]) {
        while (issued < total && !pending[next]) {
            const size_t n = total - issued < per ? total - issued : per;
            if (dense)
                HIPCHK(c, hipMemcpyAsync(c->hstage[next], (const char*)src_dev + issued, n,
                                         hipMemcpyDeviceToHost, c->stream));
            else
                HIPCHK(c, hipMemcpy2DAsync(c->hstage[next], row_bytes,
                                           (const char*)src_dev + issued * src_pitch, src_pitch,
                                           row_bytes, n, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipEventRecord(c->hev[next], c->stream));
            pending[next] = true;
            p_n[next] = n;
            p_off[next] = issued * unit;
            issued += n;
            next ^= 1;
        }
        // drain the older pending block (`next` if both are pending, else the one that is)
        const int o = pending[next] ? next : next ^ 1;
        HIPCHK(c, hipEventSynchronize(c->hev[o]));
        host_copy(out + p_off[o], (const char*)c->hstage[o], p_n[o] * unit);
        pending[o] = false;
        next = o;
    }
    return BMC_OK;
}

Panels make_panels(int64_t n, int32_t k, int32_t f32, const void* X, const void* y) {
    Panels P;
    P.X = X;
    P.y = y;
    P.n = n;
    P.k = k;
    P.vec = choose_vec(n, k, f32);
    P.npanels = (int32_t)((n + 64 * P.vec - 1) / (64 * P.vec));
    P.f32 = f32;
    P.stream_keep = 1 << 30;
    return P;
}

Panels panels_of(const bmc_ctx* c, const void* X) { return make_panels(c->n, c->k, c->f32, X, c->Yp.p); }

int ensure_rss(bmc_ctx* c, const Panels& P, size_t n_out) {
    if (int rc = ensure_all(c, {{c->rssPartial, (size_t)rss_groups(P) * 8 * sizeof(double)},
                                {c->rssOut, n_out * sizeof(double)}}))
        return rc;
    if (c->ticket.p) return BMC_OK;
    if (int rc = ensure(c, c->ticket, RSS_TICKET_BYTES)) return rc;
    HIPCHK(c, hipMemsetAsync(c->ticket.p, 0, RSS_TICKET_BYTES, c->stream));  // the kernel keeps it zero
    return BMC_OK;
}

// rss of nb host coefficient vectors on panels P -> out_host
static int rss_on_panels(bmc_ctx* c, const Panels& P, const double* coef_host, int32_t nb, double* out_host) {
    // all coefficient vectors up in one copy, one launch per 8 of them back to back on the
    // stream (the kernel re-zeroes its ticket), all results down in one copy, one sync
    const int32_t nb8 = (nb + 7) / 8 * 8;
    int rc;
    if ((rc = ensure_rss(c, P, nb8)) || (rc = ensure(c, c->coef, (size_t)nb8 * P.k * sizeof(double))))
        return rc;
    HIPCHK(c, hipMemcpyAsync(c->coef.p, coef_host, (size_t)nb * P.k * sizeof(double),
                             hipMemcpyHostToDevice, c->stream));
    for (int32_t b0 = 0; b0 < nb; b0 += 8) {
        const int32_t m = nb - b0 < 8 ? nb - b0 : 8;
        HIPCHK(c, launch_residual_rss(P, (const double*)c->coef.p + (size_t)b0 * P.k, m,
                                      (double*)c->rssPartial.p, (unsigned*)c->ticket.p,
                                      (double*)c->rssOut.p + b0, c->stream));
    }
    HIPCHK(c, hipMemcpyAsync(out_host, c->rssOut.p, (size_t)nb * sizeof(double), hipMemcpyDeviceToHost,
                             c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BMC_OK;
}

int rss_on_raw(bmc_ctx* c, const double* coef_host, int32_t nb, double* out_host) {
    return rss_on_panels(c, panels_of(c, c->Xraw.p), coef_host, nb, out_host);
}

int gram_to_host(bmc_ctx* c, const Panels& P, std::vector<double>& gram) {
    const size_t gsz = (size_t)(P.k + 1) * (P.k + 1);
    if (int rc = ensure_all(c, {{c->gramScratch, gram_scratch_bytes(P)}, {c->gramOut, gsz * 8}}))
        return rc;
    HIPCHK(c, launch_gram(P, c->gramScratch.p, (double*)c->gramOut.p, c->stream));
    gram.assign(gsz, 0.0);
    HIPCHK(c, hipMemcpyAsync(gram.data(), c->gramOut.p, gsz * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BMC_OK;
}

int ols_start(bmc_ctx* c, const Panels& P, const std::vector<double>& gram, OlsStart& o) {
    const int k = P.k, ka = k + 1;
    o.A.resize((size_t)k * k);   // OLS start value            (inference_utils.py:26-37)
    o.xty.resize(k);
    for (int i = 0; i < k; ++i) {
        for (int j = 0; j < k; ++j) o.A[(size_t)i * k + j] = gram[(size_t)i * ka + j];
        o.xty[i] = gram[(size_t)i * ka + k];
    }
    o.singular = !bmc_la::solve(o.A, o.xty, k, o.bols);
    if (o.singular) return BMC_OK;
    if (int rc = rss_on_panels(c, P, o.bols.data(), 1, &o.rss)) return rc;
    o.sigma2_init = sigma2_floor(o.rss / (double)P.n);
    return BMC_OK;
}

int stage_nu(bmc_ctx* c, DevBuf& b, NuTable shape, const double* values, int32_t n_values, int64_t n_draws,
             const void* index, bool index_on_host, NuPerDraw& v) {
    const size_t V = (size_t)n_values, S = (size_t)n_draws, tbytes = nu_table_rows(shape) * V * 8;
    std::vector<double> tab(tbytes / 8);
    nu_table(shape, values, nullptr, V, tab.data());
    if (int rc = ensure(c, b, tbytes + S * 4 + 4)) return rc;
    char* base = (char*)b.p;
    HIPCHK(c, hipMemcpyAsync(base, tab.data(), tbytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));   // tab is a local
    HIPCHK(c, hipMemsetAsync(base + tbytes + S * 4, 0, 4, c->stream));
    if (index_on_host) {
        HIPCHK(c, hipMemcpyAsync(base + tbytes, index, S * 4, hipMemcpyHostToDevice, c->stream));
        index = base + tbytes;
    }
    v.n_nu = n_values;
    v.tab = (const double*)base;
    v.index = (const int32_t*)index;
    v.flag = (int32_t*)(base + tbytes + S * 4);
    return BMC_OK;
}

int check_nu_index(bmc_ctx* c, const void* index, int64_t S, int32_t V) {
    const int32_t* idx = (const int32_t*)index;
    for (int64_t s = 0; s < S; ++s)
        if (idx[s] < 0 || idx[s] >= V) return fail(c, BMC_EINVAL, "nu_index must index nu_values");
    return BMC_OK;
}

int NuFlagRead::fetch(bmc_ctx* c, const NuPerDraw& v) {
    if (v.n_nu > 0) HIPCHK(c, hipMemcpyAsync(&word, v.flag, 4, hipMemcpyDeviceToHost, c->stream));
    return BMC_OK;
}
int NuFlagRead::result(bmc_ctx* c) const {
    return word ? fail(c, BMC_EINVAL, "nu_index must index nu_values (the results are not valid)") : BMC_OK;
}

Shape shape_of(const bmc_ctx* c) { return Shape{c->n, c->k, c->f32, c->vec, c->npanels}; }
Chip chip_of(const bmc_ctx* c) {
    return bmc::chip_of(c->n_cu, c->tune.cu_limit > 0 ? c->tune.cu_limit : c->env_cu_limit);
}

int event_ms(bmc_ctx* c, int from, int to, double* ms) {
    float f = 0;
    HIPCHK(c, hipEventElapsedTime(&f, c->ev[from], c->ev[to]));
    *ms = f;
    return BMC_OK;
}

size_t strided_bytes(int64_t n, int32_t k, int64_t ld, int layout, size_t es) {
    return (layout == BMC_COL_MAJOR ? (size_t)ld * (k - 1) + (size_t)n : (size_t)ld * (n - 1) + (size_t)k) * es;
}

namespace {

// Gram of the panelised problem -> host copy; marks the problem as set.
int finish_problem(bmc_ctx* c) {
    if (int rc = gram_to_host(c, panels_of(c, c->Xraw.p), c->gram)) return rc;
    c->have_problem = true;
    return BMC_OK;
}

// the context's shape fields of an n x k problem; its panels, their storage still to come
Panels set_shape(bmc_ctx* c, int64_t n, int32_t k, int32_t f32) {
    const Panels P = make_panels(n, k, f32, nullptr, nullptr);
    c->n = n;
    c->k = k;
    c->f32 = f32;
    c->vec = P.vec;
    c->npanels = P.npanels;
    return P;
}

int set_problem_common(bmc_ctx* c, const void* dX, const void* dy, int64_t n, int32_t k,
                       int64_t ldx, int layout, int dtype) {
    c->have_problem = c->have_prior = false;
    const Panels P = set_shape(c, n, k, dtype == BMC_F32);
    const size_t RP = 64 * P.vec, es = c->f32 ? 4 : 8;
    if (int rc = ensure_all(c, {{c->Xraw, (size_t)c->npanels * k * RP * es},
                                {c->Xrot, (size_t)c->npanels * k * RP * es},
                                {c->Yp, (size_t)c->npanels * RP * es}}))
        return rc;
    HIPCHK(c, launch_panelize(dX, dy, n, k, ldx, layout == BMC_COL_MAJOR, c->f32, c->vec,
                              c->Xraw.p, c->Yp.p, c->npanels, c->stream));
    return finish_problem(c);
}

int check_problem_args(bmc_ctx* c, const void* X, int64_t n, int32_t k, int64_t ldx, int layout,
                       const void* y, int dtype) {
    if (!c) return BMC_EINVAL;
    if (!X || !y) return fail(c, BMC_EINVAL, "X and y must not be NULL");
    if (n < 1 || k < 1) return fail(c, BMC_EINVAL, "need n >= 1 and k >= 1");
    if (k > 256) return fail(c, BMC_EINVAL, "k > 256 columns is not supported");
    if (dtype != BMC_F64 && dtype != BMC_F32) return fail(c, BMC_EINVAL, "dtype must be 0 or 1");
    if (layout != BMC_ROW_MAJOR && layout != BMC_COL_MAJOR)
        return fail(c, BMC_EINVAL, "layout must be 0 (row-major) or 1 (col-major)");
    if (layout == BMC_ROW_MAJOR ? ldx < k : ldx < n)
        return fail(c, BMC_EINVAL, "leading dimension too small");
    return BMC_OK;
}

// `warm` launches untimed, then the mean time of `reps` more (bmc_*_bench)
template <typename Launch>
int time_launches(bmc_ctx* c, int warm, int reps, double* ms_per_launch, Launch launch) {
    for (int i = 0; i < warm; ++i) HIPCHK(c, launch());
    HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
    for (int i = 0; i < reps; ++i) HIPCHK(c, launch());
    HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (int rc = event_ms(c, 0, 1, ms_per_launch)) return rc;
    *ms_per_launch /= reps;
    return BMC_OK;
}

}  // namespace

extern "C" {

int bmc_abi_version(void) { return PYBMC_AMD_ABI_VERSION; }

int bmc_create(int device_id, bmc_ctx** out) {
    if (!out) return BMC_EINVAL;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return BMC_EHIP;
    if (device_id < 0 || device_id >= count) return BMC_EINVAL;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) != hipSuccess) return BMC_EHIP;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return BMC_EHIP;  // MI355X only
    bmc_ctx* c = new (std::nothrow) bmc_ctx();
    if (!c) return BMC_ENOMEM;
    c->device = device_id;
    c->n_cu = prop.multiProcessorCount;
    c->nonce_state ^= (uint64_t)(uintptr_t)c * 0xD6E8FEB86659FD93ull;   // contexts differ
    // Several processes on one GPU cannot see each other's persistent launches: each is told its
    // share once, in the environment (e.g. 2 ranks per GPU: PYBMC_AMD_CU_LIMIT=128), and every
    // context it creates plans for that many CUs unless bmc_tuning.cu_limit says otherwise.
    if (const char* e = std::getenv("PYBMC_AMD_CU_LIMIT")) {
        const long v = std::strtol(e, nullptr, 10);
        if (v > 0 && v < 100000) c->env_cu_limit = (int)v;
    }
    if (hipSetDevice(device_id) != hipSuccess ||
        hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return BMC_EHIP;
    }
    c->own_stream = true;
    for (auto& e : c->ev)
        if (hipEventCreate(&e) != hipSuccess) {
            bmc_destroy(c);
            return BMC_EHIP;
        }
    *out = c;
    return BMC_OK;
}

void bmc_destroy(bmc_ctx* c) {
    if (!c) return;
    (void)bmc_comm_destroy(c);
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    delete c;   // every DevBuf frees itself, then ~CtxHandles: events, pinned staging, the owned stream
}

const char* bmc_last_error(const bmc_ctx* c) { return c ? c->err.c_str() : "null context"; }

int bmc_set_stream(bmc_ctx* c, void* hip_stream) {
    if (!c) return BMC_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    if (hip_stream) {
        c->stream = (hipStream_t)hip_stream;
        c->own_stream = false;
    } else {
        HIPCHK(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        c->own_stream = true;
    }
    return BMC_OK;
}

int bmc_set_tuning(bmc_ctx* c, const bmc_tuning* t) {
    if (!c) return BMC_EINVAL;
    if (!t) {
        c->tune = bmc_tuning{};
        return BMC_OK;
    }
    if (t->groups_per_chain < 0 || t->groups_per_chain > 256 || t->waves_per_group < 0 ||
        t->waves_per_group > 8 || t->residency < 0 || t->residency > 3 ||
        (t->panels_per_wave != 0 && t->panels_per_wave != 1 && t->panels_per_wave != 2 &&
         t->panels_per_wave != 4) ||
        (t->chains_per_pass != 0 && t->chains_per_pass != 1 && t->chains_per_pass != 2 &&
         t->chains_per_pass != 4 && t->chains_per_pass != 8) ||
        (t->rss_mode != 0 && t->rss_mode != 1) || t->cu_limit < 0)
        return fail(c, BMC_EINVAL, "tuning out of range (groups 0..256, waves 0..8, residency 0..3, "
                                   "panels_per_wave 0/1/2/4, chains_per_pass 0/1/2/4/8, rss_mode 0/1, "
                                   "cu_limit >= 0)");
    c->tune = *t;
    return BMC_OK;
}

int bmc_set_problem(bmc_ctx* c, const void* X, int64_t n, int32_t k, int64_t ldx, int layout,
                    const void* y, int dtype) {
    int rc = check_problem_args(c, X, n, k, ldx, layout, y, dtype);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t es = dtype == BMC_F32 ? 4 : 8;
    const size_t xbytes = (size_t)(layout == BMC_COL_MAJOR ? (size_t)ldx * k : (size_t)ldx * n) * es;
    const size_t ybytes = (size_t)n * es;
    const size_t yoff = (xbytes + 255) & ~(size_t)255;
    if ((rc = ensure(c, c->stage, yoff + ybytes))) return rc;
    const size_t xcopy = strided_bytes(n, k, ldx, layout, es);
    HIPCHK(c, hipMemcpyAsync(c->stage.p, X, xcopy, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync((char*)c->stage.p + yoff, y, ybytes, hipMemcpyHostToDevice, c->stream));
    return set_problem_common(c, c->stage.p, (char*)c->stage.p + yoff, n, k, ldx, layout, dtype);
}

int bmc_set_problem_device(bmc_ctx* c, const void* dX, int64_t n, int32_t k, int64_t ldx,
                           int layout, const void* dy, int dtype) {
    int rc = check_problem_args(c, dX, n, k, ldx, layout, dy, dtype);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    return set_problem_common(c, dX, dy, n, k, ldx, layout, dtype);
}

int bmc_set_prior(bmc_ctx* c, const double* b0, const double* C0, double nu0, double sigma20) {
    if (!c) return BMC_EINVAL;
    if (!c->have_problem) return fail(c, BMC_ESTATE, "bmc_set_problem must be called first");
    if (!b0 || !C0) return fail(c, BMC_EINVAL, "b0 and C0 must not be NULL");
    HIPCHK(c, hipSetDevice(c->device));
    c->have_prior = false;
    const int k = c->k;
    // P = inv(C0) and the prior's part of the basis        (inference_utils.py:22; bmc_basis.h)
    PriorBasis pb;
    const BasisStatus st = prior_basis(k, C0, k, b0, pb);
    if (st == BASIS_C0_SINGULAR) return fail(c, BMC_ESINGULAR, "Singular matrix (b_mean_cov)");
    OlsStart ols;
    int rc = ols_start(c, panels_of(c, c->Xraw.p), c->gram, ols);
    if (rc) return rc;
    if (ols.singular) return fail(c, BMC_ESINGULAR, "Singular matrix (X'X)");
    c->sigma2_init = ols.sigma2_init;
    if (st == BASIS_NOT_PD)
        return fail(c, BMC_EINVAL, "prior precision inv(b_mean_cov) + 1e-6 I is not positive definite");
    // the basis W, lam, c1, c2 and, for rss_mode 1 (k <= 64), G = W'AW, u0 and g0
    ChainBasis cb;
    chain_basis(k, ols.A, ols.xty, pb, k <= 64, cb);
    c->lam = std::move(cb.lam);
    c->W = std::move(cb.W);
    c->c1 = std::move(cb.c1);
    c->c2 = std::move(cb.c2);
    c->Gt = std::move(cb.G);
    c->u0 = std::move(cb.u0);
    c->g0 = std::move(cb.g0);
    c->have_gram_dev = false;
    c->b0.assign(b0, b0 + k);
    c->Pprec = std::move(pb.P);
    c->Pb0 = std::move(pb.Pb0);
    c->nu0 = nu0;
    c->s20 = sigma20;
    std::vector<double> WT((size_t)k * k);
    for (int i = 0; i < k; ++i)
        for (int j = 0; j < k; ++j) WT[(size_t)i * k + j] = c->W[(size_t)j * k + i];
    const size_t kk = (size_t)k * k * 8;
    if ((rc = ensure_all(c, {{c->dW, kk}, {c->dWT, kk}, {c->dLam, (size_t)k * 8}, {c->dC1, (size_t)k * 8},
                             {c->dC2, (size_t)k * 8}})))
        return rc;
    HIPCHK(c, hipMemcpyAsync(c->dW.p, c->W.data(), kk, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->dWT.p, WT.data(), kk, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->dLam.p, c->lam.data(), (size_t)k * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->dC1.p, c->c1.data(), (size_t)k * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->dC2.p, c->c2.data(), (size_t)k * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_rotate(panels_of(c, c->Xraw.p), (const double*)c->dW.p, c->k, c->Xrot.p,
                            c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // WT (stack vector) must outlive the copy
    c->have_prior = true;
    return BMC_OK;
}

int bmc_orthogonalize(bmc_ctx* c, const double* F, int64_t n, int32_t km, int64_t ldf,
                      const double* truth, int32_t k, double* mean_out, double* yc_out,
                      double* U_hat_out, double* S_out, double* Vt_out) {
    if (!c) return BMC_EINVAL;
    if (!F || !truth) return fail(c, BMC_EINVAL, "F and truth must not be NULL");
    if (n < 1 || km < 1 || k < 1 || k > km || ldf < km)
        return fail(c, BMC_EINVAL, "need n >= 1, 1 <= components_kept <= n_models, ldf >= n_models");
    if (km > 255) return fail(c, BMC_EINVAL, "more than 255 models is not supported");
    if (k > n) return fail(c, BMC_EINVAL, "components_kept exceeds the number of rows");
    HIPCHK(c, hipSetDevice(c->device));
    c->have_problem = c->have_prior = false;
    // panels of the centred matrix use the row-per-lane choice of the FINAL (n x k) problem
    Panels P = make_panels(n, k, 0, nullptr, nullptr);
    const int vec = P.vec, RP = 64 * vec;
    const int32_t npanels = P.npanels;
    int rc;
    const size_t fbytes = (size_t)((size_t)ldf * (n - 1) + km) * 8;
    const size_t toff = (fbytes + 255) & ~(size_t)255;
    if ((rc = ensure_all(c, {{c->stage, toff + (size_t)n * 8},
                             {c->oFc, (size_t)npanels * km * RP * 8},
                             {c->Yp, (size_t)npanels * RP * 8},
                             {c->oMu, (size_t)npanels * RP * 8}})))
        return rc;
    HIPCHK(c, hipMemcpyAsync(c->stage.p, F, fbytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync((char*)c->stage.p + toff, truth, (size_t)n * 8, hipMemcpyHostToDevice,
                             c->stream));
    HIPCHK(c, launch_centre((const double*)c->stage.p, n, km, ldf,
                            (const double*)((char*)c->stage.p + toff), vec, npanels,
                            (double*)c->oFc.p, (double*)c->Yp.p, (double*)c->oMu.p, c->stream));
    // Gram of the centred matrix: Fc'Fc = V S^2 V'  (the SVD of bmc.py:119 through its Gram)
    P.X = c->oFc.p, P.y = c->Yp.p, P.k = km;
    std::vector<double> ga;
    if ((rc = gram_to_host(c, P, ga))) return rc;
    bmc_la::Mat Gm((size_t)km * km), Q;
    for (int i = 0; i < km; ++i)
        for (int j = 0; j < km; ++j) Gm[(size_t)i * km + j] = ga[(size_t)i * (km + 1) + j];
    std::vector<double> ev;
    bmc_la::sym_eigh(Gm, km, ev, Q);
    std::vector<int> order(km);
    for (int i = 0; i < km; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return ev[a] > ev[b]; });
    const double s0 = std::sqrt(ev[order[0]] > 0 ? ev[order[0]] : 0.0);
    const double sk = std::sqrt(ev[order[k - 1]] > 0 ? ev[order[k - 1]] : 0.0);
    // rows of the centred matrix sum to zero -> rank <= n_models - 1 (bmc.py:114-119); the
    // Gram route also loses accuracy like (s0/sk)^2, so refuse ill-conditioned requests
    if (!(sk > s0 * 1e-6) || !(s0 > 0))
        return fail(c, BMC_ESINGULAR,
                    "components_kept reaches the (numerical) null space of the centred model matrix");
    std::vector<double> W((size_t)km * k), Vt((size_t)k * km), S(k);
    for (int q = 0; q < k; ++q) {
        const int col = order[q];
        S[q] = std::sqrt(ev[col]);
        // sign convention: the entry of largest magnitude of each right singular vector is > 0
        int big = 0;
        for (int i = 1; i < km; ++i)
            if (std::fabs(Q[(size_t)i * km + col]) > std::fabs(Q[(size_t)big * km + col])) big = i;
        const double sg = Q[(size_t)big * km + col] < 0 ? -1.0 : 1.0;
        for (int i = 0; i < km; ++i) {
            const double v = sg * Q[(size_t)i * km + col];
            Vt[(size_t)q * km + i] = v;
            W[(size_t)i * k + q] = v / S[q];          // U_hat = Fc V S^-1
        }
    }
    // the sampler's problem: X = U_hat (n x k panels), y = centred truth
    set_shape(c, n, k, 0);
    if ((rc = ensure_all(c, {{c->Xraw, (size_t)npanels * k * RP * 8},
                             {c->Xrot, (size_t)npanels * k * RP * 8},
                             {c->oW, W.size() * 8}})))
        return rc;
    HIPCHK(c, hipMemcpyAsync(c->oW.p, W.data(), W.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_rotate(P, (const double*)c->oW.p, k, c->Xraw.p, c->stream));
    if (U_hat_out) {
        if ((rc = ensure(c, c->oOut, (size_t)n * k * 8))) return rc;
        HIPCHK(c, launch_unpanelize((const double*)c->Xraw.p, n, k, vec, (double*)c->oOut.p, c->stream));
        HIPCHK(c, hipMemcpyAsync(U_hat_out, c->oOut.p, (size_t)n * k * 8, hipMemcpyDeviceToHost,
                                 c->stream));
    }
    if (mean_out)
        HIPCHK(c, hipMemcpyAsync(mean_out, c->oMu.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    if (yc_out)
        HIPCHK(c, hipMemcpyAsync(yc_out, c->Yp.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // W (host vector) must outlive its copy
    if (S_out) std::memcpy(S_out, S.data(), (size_t)k * 8);
    if (Vt_out) std::memcpy(Vt_out, Vt.data(), (size_t)k * km * 8);
    return finish_problem(c);
}

int bmc_get_gram(bmc_ctx* c, double* out) {
    if (!c || !out) return BMC_EINVAL;
    if (!c->have_problem) return fail(c, BMC_ESTATE, "no problem set");
    std::memcpy(out, c->gram.data(), c->gram.size() * sizeof(double));
    return BMC_OK;
}

int bmc_get_basis(bmc_ctx* c, double* W_out, double* lam_out, double* sigma2_init) {
    if (!c) return BMC_EINVAL;
    if (!c->have_prior) return fail(c, BMC_ESTATE, "no prior set");
    if (W_out) std::memcpy(W_out, c->W.data(), c->W.size() * sizeof(double));
    if (lam_out) std::memcpy(lam_out, c->lam.data(), c->lam.size() * sizeof(double));
    if (sigma2_init) *sigma2_init = c->sigma2_init;
    return BMC_OK;
}

int bmc_last_kernels(bmc_ctx* c, char* names_out, int64_t capacity, int32_t* n_out, int64_t* needed_out) {
    if (!c) return BMC_EINVAL;
    std::string all;
    for (const std::string& name : c->last_kernels) all += name + "\n";
    if (n_out) *n_out = (int32_t)c->last_kernels.size();
    if (needed_out) *needed_out = (int64_t)all.size() + 1;
    if (names_out) {
        if (capacity < (int64_t)all.size() + 1) return fail(c, BMC_EINVAL, "bmc_last_kernels: buffer too small");
        std::memcpy(names_out, all.c_str(), all.size() + 1);
    }
    return BMC_OK;
}

int bmc_conditional_moments(bmc_ctx* c, double sigma2, double* mean_out, double* cov_out) {
    if (!c) return BMC_EINVAL;
    if (!c->have_prior) return fail(c, BMC_ESTATE, "no prior set");
    const int k = c->k;
    std::vector<double> d(k), m(k);
    for (int j = 0; j < k; ++j) {
        d[j] = 1.0 / (c->lam[j] / sigma2 + 1.0);
        m[j] = d[j] * (c->c1[j] + c->c2[j] / sigma2);
    }
    if (mean_out)
        for (int i = 0; i < k; ++i) {
            long double s = 0.0L;
            for (int j = 0; j < k; ++j) s += (long double)c->W[(size_t)i * k + j] * m[j];
            mean_out[i] = (double)s;
        }
    if (cov_out)
        for (int i = 0; i < k; ++i)
            for (int j = 0; j < k; ++j) {
                long double s = 0.0L;
                for (int q = 0; q < k; ++q)
                    s += (long double)c->W[(size_t)i * k + q] * d[q] * c->W[(size_t)j * k + q];
                cov_out[(size_t)i * k + j] = (double)s;
            }
    return BMC_OK;
}

int bmc_residual_rss(bmc_ctx* c, const double* beta, int32_t nb, double* rss_out) {
    if (!c) return BMC_EINVAL;
    if (!c->have_problem) return fail(c, BMC_ESTATE, "no problem set");
    if (!beta || !rss_out || nb < 1) return fail(c, BMC_EINVAL, "beta/rss_out/nb invalid");
    HIPCHK(c, hipSetDevice(c->device));
    return rss_on_raw(c, beta, nb, rss_out);
}

int bmc_residual_rss_bench(bmc_ctx* c, int32_t nb, int32_t reps, double* ms_per_launch) {
    if (!c) return BMC_EINVAL;
    if (!c->have_problem) return fail(c, BMC_ESTATE, "no problem set");
    if (nb < 1 || nb > 8 || reps < 1 || !ms_per_launch) return fail(c, BMC_EINVAL, "bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    const Panels P = panels_of(c, c->Xraw.p);
    int rc;
    if ((rc = ensure_rss(c, P, 8)) || (rc = ensure(c, c->coef, (size_t)8 * c->k * sizeof(double))))
        return rc;
    std::vector<double> cf((size_t)nb * c->k);
    for (size_t i = 0; i < cf.size(); ++i) cf[i] = 0.01 * (double)((i * 2654435761u) % 97) - 0.5;
    HIPCHK(c, hipMemcpyAsync(c->coef.p, cf.data(), cf.size() * 8, hipMemcpyHostToDevice, c->stream));
    return time_launches(c, 3, reps, ms_per_launch, [&] {
        return launch_residual_rss(P, (const double*)c->coef.p, nb, (double*)c->rssPartial.p,
                                   (unsigned*)c->ticket.p, (double*)c->rssOut.p, c->stream);
    });
}

int bmc_gram_bench(bmc_ctx* c, int32_t reps, double* ms_per_launch) {
    if (!c) return BMC_EINVAL;
    if (!c->have_problem) return fail(c, BMC_ESTATE, "no problem set");
    if (reps < 1 || !ms_per_launch) return fail(c, BMC_EINVAL, "bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    const Panels P = panels_of(c, c->Xraw.p);
    if (int rc = ensure_all(c, {{c->gramScratch, gram_scratch_bytes(P)},
                                {c->gramOut, (size_t)(c->k + 1) * (c->k + 1) * 8}}))
        return rc;
    return time_launches(c, 2, reps, ms_per_launch,
                         [&] { return launch_gram(P, c->gramScratch.p, (double*)c->gramOut.p, c->stream); });
}

int bmc_rng_fill(bmc_ctx* c, uint64_t seed, int64_t count_normal, double* normals_out, double shape,
                 int64_t count_gamma, double* gammas_out) {
    if (!c) return BMC_EINVAL;
    if (count_normal < 0 || count_gamma < 0 || (count_normal > 0 && !normals_out) ||
        (count_gamma > 0 && (!gammas_out || !(shape > 0.0))))
        return fail(c, BMC_EINVAL, "bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = ensure_all(c, {{c->xi, (size_t)count_normal * 8}, {c->gam, (size_t)count_gamma * 8},
                                {c->seeds, sizeof(uint64_t)}}))
        return rc;
    HIPCHK(c, hipMemcpyAsync(c->seeds.p, &seed, sizeof(seed), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_rng_fill((const uint64_t*)c->seeds.p, 1, count_normal, (double*)c->xi.p, shape,
                              count_gamma, (double*)c->gam.p, c->stream));
    if (count_normal)
        HIPCHK(c, hipMemcpyAsync(normals_out, c->xi.p, (size_t)count_normal * 8,
                                 hipMemcpyDeviceToHost, c->stream));
    if (count_gamma)
        HIPCHK(c, hipMemcpyAsync(gammas_out, c->gam.p, (size_t)count_gamma * 8,
                                 hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BMC_OK;
}

#ifdef BMC_STAMPS
// Diagnostic build only; not part of the public ABI.
int bmc_dev_get_stamps(bmc_ctx* c, long long* out8) {
    if (!c || !out8 || !c->dbg.p) return BMC_EINVAL;
    HIPCHK(c, hipMemcpy(out8, c->dbg.p, 12 * sizeof(long long), hipMemcpyDeviceToHost));
    return BMC_OK;
}
#endif

int bmc_philox_raw(bmc_ctx* c, uint64_t seed, uint32_t stream_id, int64_t nblocks4, uint32_t* out) {
    if (!c) return BMC_EINVAL;
    if (nblocks4 < 1 || !out) return fail(c, BMC_EINVAL, "bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = ensure(c, c->xi, (size_t)nblocks4 * 16))) return rc;
    HIPCHK(c, launch_philox_raw(seed, stream_id, nblocks4, (uint32_t*)c->xi.p, c->stream));
    HIPCHK(c, hipMemcpyAsync(out, c->xi.p, (size_t)nblocks4 * 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BMC_OK;
}

}  // extern "C"
