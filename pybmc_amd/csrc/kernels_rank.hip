// Rank normalisation of sampled chains: the exact rank of
// every split draw of a column, on the raw and on the folded values, as z-scores.
//   key_gather        samples -> (key, index) pairs, one segment per column; non-finite flag.  One
//                     template over what it reads: the split draws of a RankShape (launch_rank_gather)
//                     or the two sources of a SensSource (launch_key_gather, for kernels_sens.hip)
//   rank_count        per-tile digit histogram of one LSD pass
//   rank_scan         per segment: the histograms -> the first output position of (tile, digit)
//   rank_scatter      the stable scatter of one pass (ranks inside a tile by wave ballots)
//   rank_z            sorted pairs -> runs of equal keys -> average rank -> ndtri -> z at the draw
//   rank_pick         order statistics of a sorted segment, interpolated
//   rank_fold         key -> key of |x - median|, in place
//   rank_indicators   1[x <= q05], 1[x <= q95] as 0.0 / 1.0
// Integer atomics only (LDS digit counters, the OR / AND masks and the flag in global memory):
// their results do not depend on order, so two calls return the same bits.
#include "bmc_launch.h"
#include "bmc_math.h"

namespace bmc {

namespace {

constexpr int RANK_GATHER_ITEMS = 4;
constexpr int RANK_GATHER_TILE = RANK_BLOCK * RANK_GATHER_ITEMS;   // 1024 draws per gather workgroup
constexpr int RANK_WAVES = RANK_BLOCK / 64;
constexpr int RANK_ROUNDS = RANK_ITEMS;                            // 64 keys of a wave per round
static_assert(RANK_BLOCK == RANK_DIGITS, "thread d of a sort workgroup owns digit d");

__device__ inline uint64_t wave_or(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v |= (uint64_t)__shfl_xor((unsigned long long)v, o, 64);
    return v;
}
__device__ inline uint64_t wave_and(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v &= (uint64_t)__shfl_xor((unsigned long long)v, o, 64);
    return v;
}

// OR and AND of the workgroup's keys into or_and[0], or_and[1]
__device__ inline void block_or_and(uint64_t o, uint64_t a, uint64_t* or_and) {
    __shared__ uint64_t red[2][RANK_WAVES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    o = wave_or(o);
    a = wave_and(a);
    if (lane == 0) red[0][w] = o, red[1][w] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 1; i < RANK_WAVES; ++i) o |= red[0][i], a &= red[1][i];
        atomicOr((unsigned long long*)or_and, (unsigned long long)o);
        atomicAnd((unsigned long long*)or_and + 1, (unsigned long long)a);
    }
}

__global__ void key_init_kernel(int32_t Pb, uint64_t* __restrict__ or_and, uint32_t* __restrict__ flags) {
    const int32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < Pb) {
        or_and[2 * j] = 0;
        or_and[2 * j + 1] = ~0ull;
        if (flags) flags[j] = 0;
    }
}

// the sample of split draw e of column col (RankShape comment in bmc_launch.h)
__device__ inline double rank_load(const RankShape& r, uint32_t e, int32_t col) {
    const uint32_t m = e / (uint32_t)r.n, i = e - m * (uint32_t)r.n;
    const int64_t row = (int64_t)(m >> 1) * r.iters + r.burn + (int64_t)(m & 1) * r.half_off + i;
    return r.x[row * r.ld + col];
}

// What the gather reads: element e of column col of the split draws of a RankShape, or of the two
// sources of a SensSource
struct RankLoad {
    RankShape r;
    __device__ double operator()(int64_t e, int32_t col) const { return rank_load(r, (uint32_t)e, col); }
};
struct SensLoad {
    SensSource src;
    __device__ double operator()(int64_t e, int32_t col) const {
        if (col >= src.n1) return src.p2[e];
        return col < src.n0 ? src.p0[e * src.rs0 + col] : src.p1[e * src.rs1 + (int64_t)(col - src.n0) * src.cs1];
    }
};

// grid: gblocks * Pb, column fastest (the workgroups that read the same rows run together).
// Segment jb of keys / idx starts at jb * seg_stride and takes the S draws of column col0 + jb.
template <class Load>
__global__ __launch_bounds__(RANK_BLOCK) void key_gather_kernel(
    Load load, int64_t S, int64_t seg_stride, int32_t col0, int32_t Pb, uint64_t* __restrict__ keys,
    uint32_t* __restrict__ idx, uint64_t* __restrict__ or_and, uint32_t* __restrict__ flags) {
    const int32_t jb = blockIdx.x % Pb;
    const int64_t e0 = (int64_t)(blockIdx.x / Pb) * RANK_GATHER_TILE;
    uint64_t o = 0, a = ~0ull;
    bool bad = false;
#pragma unroll
    for (int it = 0; it < RANK_GATHER_ITEMS; ++it) {
        const int64_t e = e0 + it * RANK_BLOCK + threadIdx.x;
        if (e < S) {
            const double x = load(e, col0 + jb);
            const uint64_t k = rank_key(x);
            bad = bad || !is_finite(x);
            keys[(int64_t)jb * seg_stride + e] = k;
            idx[(int64_t)jb * seg_stride + e] = (uint32_t)e;
            o |= k;
            a &= k;
        }
    }
    if (__ballot(bad) != 0 && (threadIdx.x & 63) == 0) atomicOr(flags + jb, 1u);
    block_or_and(o, a, or_and + 2 * jb);
}

// position of key `it` of thread `tid` in its tile: wave w owns keys [1024 w, 1024 w + 1024) in
// rounds of 64 consecutive keys, so (wave, round, lane) order is key order: what makes the
// scatter stable
__device__ inline int tile_pos(int it) {
    return (threadIdx.x >> 6) * (64 * RANK_ROUNDS) + it * 64 + (threadIdx.x & 63);
}

// grid: Pb * tiles, tile fastest
__global__ __launch_bounds__(RANK_BLOCK) void rank_count_kernel(
    int64_t S, int64_t tiles, int shift, const uint64_t* __restrict__ keys, uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[RANK_DIGITS];
    const int64_t seg = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    h[threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = tile * RANK_TILE;
    const uint64_t* k = keys + seg * S;
#pragma unroll
    for (int it = 0; it < RANK_ITEMS; ++it) {
        const int64_t i = base + tile_pos(it);
        if (i < S) atomicAdd(&h[(k[i] >> shift) & (RANK_DIGITS - 1)], 1u);
    }
    __syncthreads();
    hist[(int64_t)blockIdx.x * RANK_DIGITS + threadIdx.x] = h[threadIdx.x];
}

// grid: Pb; thread d owns digit d.  hist[seg][tile][d] becomes the first output position (inside
// the segment) of the keys of tile `tile` with digit d: digits in order, tiles in order in a digit.
__global__ __launch_bounds__(RANK_DIGITS) void rank_scan_kernel(int64_t tiles, uint32_t* __restrict__ hist) {
    __shared__ uint32_t tot[RANK_DIGITS];
    uint32_t* h = hist + (int64_t)blockIdx.x * tiles * RANK_DIGITS + threadIdx.x;
    uint32_t sum = 0;
#pragma unroll 8
    for (int64_t t = 0; t < tiles; ++t) sum += h[t * RANK_DIGITS];
    tot[threadIdx.x] = sum;
    __syncthreads();
    // inclusive scan over the 256 digits (Hillis-Steele)
    for (int o = 1; o < RANK_DIGITS; o <<= 1) {
        const uint32_t add = (int)threadIdx.x >= o ? tot[threadIdx.x - o] : 0;
        __syncthreads();
        tot[threadIdx.x] += add;
        __syncthreads();
    }
    uint32_t run = tot[threadIdx.x] - sum;
#pragma unroll 8
    for (int64_t t = 0; t < tiles; ++t) {
        const uint32_t c = h[t * RANK_DIGITS];
        h[t * RANK_DIGITS] = run;
        run += c;
    }
}

// grid: Pb * tiles, tile fastest
__global__ __launch_bounds__(RANK_BLOCK) void rank_scatter_kernel(
    int64_t S, int64_t tiles, int shift, const uint64_t* __restrict__ kin, const uint32_t* __restrict__ iin,
    uint64_t* __restrict__ kout, uint32_t* __restrict__ iout, const uint32_t* __restrict__ hist) {
    __shared__ uint32_t cnt[RANK_WAVES][RANK_DIGITS];
    const int64_t seg = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < RANK_WAVES; ++i) cnt[i][threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = seg * S + tile * RANK_TILE;
    const int64_t left = S - tile * RANK_TILE;       // keys from the tile's start to the segment's end
    uint64_t key[RANK_ITEMS];
#pragma unroll
    for (int it = 0; it < RANK_ITEMS; ++it) {
        const int p = tile_pos(it);
        key[it] = 0;
        if (p < left) {
            key[it] = kin[base + p];
            atomicAdd(&cnt[w][(key[it] >> shift) & (RANK_DIGITS - 1)], 1u);
        }
    }
    __syncthreads();
    {   // counts -> first output position of (wave, digit)
        uint32_t run = hist[(int64_t)blockIdx.x * RANK_DIGITS + threadIdx.x];
#pragma unroll
        for (int i = 0; i < RANK_WAVES; ++i) {
            const uint32_t c = cnt[i][threadIdx.x];
            cnt[i][threadIdx.x] = run;
            run += c;
        }
    }
    __syncthreads();
    volatile uint32_t* next = cnt[w];       // this wave's row: read and advanced round by round
    const uint64_t below = (1ull << lane) - 1;
#pragma unroll
    for (int it = 0; it < RANK_ITEMS; ++it) {
        const int p = tile_pos(it);
        const bool valid = p < left;
        const uint32_t d = (uint32_t)(key[it] >> shift) & (RANK_DIGITS - 1);
        // the lanes of this round that hold the same digit
        uint64_t same = __ballot(valid);
#pragma unroll
        for (int b = 0; b < RANK_DIGIT_BITS; ++b) {
            const bool bit = (d >> b) & 1;
            const uint64_t bal = __ballot(valid && bit);
            same &= bit ? bal : ~bal;
        }
        if (valid) {
            const uint32_t first = next[d];
            const uint32_t before = (uint32_t)__popcll(same & below);
            if (before == 0) next[d] = first + (uint32_t)__popcll(same);
            const int64_t dst = seg * S + first + before;
            kout[dst] = key[it];
            iout[dst] = iin[base + p];
        }
    }
}

// first position in k[lo, hi) whose key is >= v (hi when none)
template <typename P>
__device__ inline int64_t lower_bound(P k, int64_t lo, int64_t hi, uint64_t v) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (k[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// first position in k[lo, hi) whose key is > v (hi when none)
template <typename P>
__device__ inline int64_t upper_bound(P k, int64_t lo, int64_t hi, uint64_t v) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (k[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// grid: Pb * tiles, tile fastest.  The tile's keys in LDS; a run that reaches the tile's edge is
// completed by one binary search of the segment per edge.
__global__ __launch_bounds__(RANK_BLOCK) void rank_z_kernel(
    int64_t S, int64_t tiles, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ idx,
    double* __restrict__ out, int64_t seg_stride, int64_t ld_d, int32_t col) {
    __shared__ uint64_t sk[RANK_TILE];
    __shared__ int64_t edge[2];
    const int64_t seg = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int64_t t0 = tile * RANK_TILE;
    const int cnt = (int)(S - t0 < RANK_TILE ? S - t0 : RANK_TILE);
    const uint64_t* k = keys + seg * S;
    for (int p = threadIdx.x; p < cnt; p += RANK_BLOCK) sk[p] = k[t0 + p];
    __syncthreads();
    if (threadIdx.x == 0)        // first position of the run of the tile's first key
        edge[0] = t0 > 0 && k[t0 - 1] == sk[0] ? lower_bound(k, 0, t0 - 1, sk[0]) : t0;
    if (threadIdx.x == 64)       // last position of the run of the tile's last key
        edge[1] = t0 + cnt < S && k[t0 + cnt] == sk[cnt - 1]
                      ? upper_bound(k, t0 + cnt + 1, S, sk[cnt - 1]) - 1 : t0 + cnt - 1;
    __syncthreads();
    const double denom = (double)S + 0.25;
    for (int p = threadIdx.x; p < cnt; p += RANK_BLOCK) {
        const uint64_t v = sk[p];
        int64_t first = t0 + p, last = t0 + p;
        const bool tie_l = p > 0 ? sk[p - 1] == v : edge[0] < t0;
        const bool tie_r = p + 1 < cnt ? sk[p + 1] == v : edge[1] > t0 + cnt - 1;
        if (tie_l) {
            const int lb = (int)lower_bound(sk, 0, p, v);
            first = lb == 0 ? edge[0] : t0 + lb;
        }
        if (tie_r) {
            const int ub = (int)upper_bound(sk, p + 1, cnt, v);
            last = ub == cnt ? edge[1] : t0 + ub - 1;
        }
        const double rank = 0.5 * (double)(first + last + 2);     // exact: first + last < 2^32
        const double z = ndtri((rank - 0.375) / denom);
        out[seg * seg_stride + (int64_t)idx[seg * S + t0 + p] * ld_d + col] = z;
    }
}

// grid: Pb; thread t < rq.n takes quantile t
__global__ void rank_pick_kernel(int64_t S, const uint64_t* __restrict__ keys, RankQuantiles rq,
                                 double* __restrict__ q) {
    const int t = threadIdx.x;
    if (t >= rq.n) return;
    const uint64_t* k = keys + (int64_t)blockIdx.x * S;
    const int64_t lo = rq.index[t], hi = lo + 1 < S ? lo + 1 : S - 1;
    const double a = rank_unkey(k[lo]), b = rank_unkey(k[hi]), w = rq.weight[t];
    const double diff = b - a;
    q[(int64_t)blockIdx.x * RANK_Q_SLOTS + t] = w >= 0.5 ? b - diff * (1.0 - w) : a + diff * w;
}

// grid: Pb * gblocks, block of draws fastest
__global__ __launch_bounds__(RANK_BLOCK) void rank_fold_kernel(
    int64_t S, int64_t gblocks, uint64_t* __restrict__ keys, const double* __restrict__ q, int32_t med_slot,
    uint64_t* __restrict__ or_and) {
    const int64_t seg = blockIdx.x / gblocks;
    const int64_t e0 = (blockIdx.x % gblocks) * RANK_GATHER_TILE;
    const double med = q[seg * RANK_Q_SLOTS + med_slot];
    uint64_t o = 0, a = ~0ull;
#pragma unroll
    for (int it = 0; it < RANK_GATHER_ITEMS; ++it) {
        const int64_t e = e0 + it * RANK_BLOCK + threadIdx.x;
        if (e < S) {
            const uint64_t k = rank_key(fabs(rank_unkey(keys[seg * S + e]) - med));
            keys[seg * S + e] = k;
            o |= k;
            a &= k;
        }
    }
    block_or_and(o, a, or_and + 2 * seg);
}

// grid: gblocks * Pb, column fastest (as the gather)
__global__ __launch_bounds__(RANK_BLOCK) void rank_indicators_kernel(
    RankShape r, const double* __restrict__ q, int32_t slot_lo, int32_t slot_hi, double* __restrict__ out,
    int64_t seg_stride, int64_t ld_d, int32_t col_lo, int32_t col_hi) {
    const int32_t jb = blockIdx.x % r.Pb;
    const int64_t e0 = (int64_t)(blockIdx.x / r.Pb) * RANK_GATHER_TILE;
    const double q_lo = q[(int64_t)jb * RANK_Q_SLOTS + slot_lo], q_hi = q[(int64_t)jb * RANK_Q_SLOTS + slot_hi];
#pragma unroll
    for (int it = 0; it < RANK_GATHER_ITEMS; ++it) {
        const int64_t e = e0 + it * RANK_BLOCK + threadIdx.x;
        if (e < r.S) {
            const double x = rank_load(r, (uint32_t)e, r.col0 + jb);
            out[jb * seg_stride + e * ld_d + col_lo] = x <= q_lo ? 1.0 : 0.0;
            out[jb * seg_stride + e * ld_d + col_hi] = x <= q_hi ? 1.0 : 0.0;
        }
    }
}

inline int64_t gather_blocks(const RankShape& r) { return (r.S + RANK_GATHER_TILE - 1) / RANK_GATHER_TILE; }

// the launchers' common refusal: a shape the plan would not have produced
inline bool rank_shape_ok(const RankShape& r) {
    return r.Pb >= 1 && r.S >= 1 && r.S <= RANK_MAX_S && r.n >= 1 && r.S == 2 * (int64_t)r.C * r.n &&
           r.tiles == (r.S + RANK_TILE - 1) / RANK_TILE && r.tiles * RANK_ITEMS * r.Pb <= RANK_MAX_BLOCKS;
}

}  // namespace

hipError_t launch_rank_gather(const RankShape& r, uint64_t* keys, uint32_t* idx, uint64_t* or_and,
                              uint32_t* flags, hipStream_t s) {
    if (!rank_shape_ok(r)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(key_init_kernel, dim3((r.Pb + 255) / 256), dim3(256), 0, s, r.Pb, or_and, flags);
    hipLaunchKernelGGL(key_gather_kernel<RankLoad>, dim3((unsigned)(gather_blocks(r) * r.Pb)), dim3(RANK_BLOCK),
                       0, s, RankLoad{r}, r.S, r.S, r.col0, r.Pb, keys, idx, or_and, flags);
    return hipGetLastError();
}

hipError_t launch_key_gather(const SensSource& src, int64_t S, int64_t seg_stride, int32_t col0, int32_t Pb,
                             uint64_t* keys, uint32_t* idx, uint64_t* or_and, uint32_t* flags, hipStream_t s) {
    const int64_t gblocks = (S + RANK_GATHER_TILE - 1) / RANK_GATHER_TILE;
    if (gblocks * Pb > 0x7fffffffll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(key_init_kernel, dim3((Pb + 255) / 256), dim3(256), 0, s, Pb, or_and, flags);
    hipLaunchKernelGGL(key_gather_kernel<SensLoad>, dim3((unsigned)(gblocks * Pb)), dim3(RANK_BLOCK), 0, s,
                       SensLoad{src}, S, seg_stride, col0, Pb, keys, idx, or_and, flags);
    return hipGetLastError();
}

hipError_t launch_rank_sort_pass(const RankShape& r, int digit, const uint64_t* kin, const uint32_t* iin,
                                 uint64_t* kout, uint32_t* iout, uint32_t* hist, hipStream_t s) {
    if (!rank_shape_ok(r) || digit < 0 || digit >= RANK_PASSES) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(r.tiles * r.Pb));
    const int shift = digit * RANK_DIGIT_BITS;
    hipLaunchKernelGGL(rank_count_kernel, grid, dim3(RANK_BLOCK), 0, s, r.S, r.tiles, shift, kin, hist);
    hipLaunchKernelGGL(rank_scan_kernel, dim3(r.Pb), dim3(RANK_DIGITS), 0, s, r.tiles, hist);
    hipLaunchKernelGGL(rank_scatter_kernel, grid, dim3(RANK_BLOCK), 0, s, r.S, r.tiles, shift, kin, iin, kout,
                       iout, (const uint32_t*)hist);
    return hipGetLastError();
}

hipError_t launch_rank_z(const RankShape& r, const uint64_t* keys, const uint32_t* idx, double* out,
                         int64_t seg_stride, int64_t ld_d, int32_t col, hipStream_t s) {
    if (!rank_shape_ok(r) || col < 0 || col >= ld_d || seg_stride < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rank_z_kernel, dim3((unsigned)(r.tiles * r.Pb)), dim3(RANK_BLOCK), 0, s, r.S, r.tiles,
                       keys, idx, out, seg_stride, ld_d, col);
    return hipGetLastError();
}

hipError_t launch_rank_pick(const RankShape& r, const uint64_t* keys, const RankQuantiles& rq, double* q,
                            hipStream_t s) {
    if (!rank_shape_ok(r) || rq.n < 1 || rq.n > RANK_Q_SLOTS) return hipErrorInvalidValue;
    for (int t = 0; t < rq.n; ++t)
        if (rq.index[t] < 0 || rq.index[t] >= r.S) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rank_pick_kernel, dim3(r.Pb), dim3(64), 0, s, r.S, keys, rq, q);
    return hipGetLastError();
}

hipError_t launch_rank_fold(const RankShape& r, uint64_t* keys, const double* q, int32_t med_slot,
                            uint64_t* or_and, hipStream_t s) {
    if (!rank_shape_ok(r) || med_slot < 0 || med_slot >= RANK_Q_SLOTS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(key_init_kernel, dim3((r.Pb + 255) / 256), dim3(256), 0, s, r.Pb, or_and,
                       (uint32_t*)nullptr);
    hipLaunchKernelGGL(rank_fold_kernel, dim3((unsigned)(gather_blocks(r) * r.Pb)), dim3(RANK_BLOCK), 0, s, r.S,
                       gather_blocks(r), keys, q, med_slot, or_and);
    return hipGetLastError();
}

hipError_t launch_rank_indicators(const RankShape& r, const double* q, int32_t slot_lo, int32_t slot_hi,
                                  double* out, int64_t seg_stride, int64_t ld_d, int32_t col_lo, int32_t col_hi,
                                  hipStream_t s) {
    if (!rank_shape_ok(r) || slot_lo < 0 || slot_lo >= RANK_Q_SLOTS || slot_hi < 0 || slot_hi >= RANK_Q_SLOTS ||
        col_lo < 0 || col_hi < 0 || col_lo >= ld_d || col_hi >= ld_d || seg_stride < 1)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(rank_indicators_kernel, dim3((unsigned)(gather_blocks(r) * r.Pb)), dim3(RANK_BLOCK), 0, s,
                       r, q, slot_lo, slot_hi, out, seg_stride, ld_d, col_lo, col_hi);
    return hipGetLastError();
}

}  // namespace bmc
