// Dev microbenchmark (not part of the product): the poll schedule of the granule all-gather.
// 32 workgroups on one XCD (blocks b = 0 mod 8 of a 256-block launch), P publisher waves each
// (P = 1: the loop kernel; P = 8: the bundles' eight leaders per CU), wave w of every group
// forming ring w: publish two {epoch, 32 bits} words (lanes 0, 1 of one store), gather the
// ring's 64 words one per lane with sc1 loads, sum, and let the next round depend on the sum.
// Between gather and publish a chain of `work` dependent f64 FMAs stands for the rest of an
// iteration (work = 0: the hop alone, polls of the last round still in flight at the store).
// Schedule <DEPTH, GAP0, GAP>: GAP0 wait states between the store and the first poll, GAP between
// the first DEPTH polls; afterwards each poll is re-issued when its predecessor's slot is tested.
// Reported per round: wall time (events), s_memtime ticks from a group's own store to its exit
// from the gather (group 0, wave 0), polls issued.
//   hipcc --offload-arch=gfx950 -O3 -Wno-unused-value -o pollsched pollsched.hip && ./pollsched
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
typedef unsigned long long u64;

constexpr int PAIR_STRIDE = 8;        // words: one 64-byte line per granule pair, as the product
constexpr int RING_WORDS = 32 * PAIR_STRIDE;
constexpr int MAXP = 8;

__device__ __forceinline__ u64 ld(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// N wait states without touching any counter (s_nop k = k + 1 of them)
template <int N>
__device__ __forceinline__ void wait_states() {
    if constexpr (N >= 16) { asm volatile("s_nop 15"); wait_states<N - 16>(); }
    else if constexpr (N > 0) asm volatile("s_nop %0" ::"n"(N - 1));
}

template <int DEPTH, int GAP0, int GAP>
__device__ __forceinline__ bool gather(const u64* p, u64 need, unsigned epoch, u64& x, unsigned& polls) {
    u64 q[DEPTH];
    wait_states<GAP0>();
#pragma unroll
    for (int d = 0; d < DEPTH - 1; ++d) { q[d] = ld(p); wait_states<GAP>(); }
    polls += DEPTH - 1;
    for (unsigned spins = 0;; ++spins) {
#pragma unroll
        for (int d = 0; d < DEPTH; ++d) {
            q[(d + DEPTH - 1) % DEPTH] = ld(p);
            ++polls;
            const u64 w = q[d];
            const u64 hit = __builtin_amdgcn_ballot_w64((unsigned)(w >> 32) == epoch);
            if ((hit & need) == need) { x = w; return true; }
        }
        if (spins > 4000000u) return false;   // (about a second: the host reports it)
    }
}

template <int LOCAL, int DEPTH, int GAP0, int GAP>
__global__ __launch_bounds__(64 * MAXP) void ring(u64* words, int* xcc, int rounds, int work,
                                                  int spread, long long* out, double* sink) {
    const int b = blockIdx.x;
    if (threadIdx.x == 0) xcc[b] = __builtin_amdgcn_s_getreg((3 << 11) | 20) & 0xf;
    // spread: the 32 groups are blocks 0..31, four on each of the 8 XCDs (a chain whose placement
    // check failed, and the pollers of the second level); otherwise blocks 0 mod 8, one XCD
    if (spread ? b >= 32 : b % 8 != 0) return;
    const int g = spread ? b : b / 8, G = 32;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;   // wave < MAXP (launch bounds)
    u64* ringw = words + (size_t)wave * 2 * RING_WORDS;     // [wave][parity][32 pairs x 8 words]
    const bool have = lane < 2 * G;
    const u64 needm = __builtin_amdgcn_ballot_w64(have);
    double total = 1.0;
    long long t_hop = 0, t0 = 0;
    unsigned polls = 0;
    for (int r = 1; r <= rounds; ++r) {
        if (r == 3) { t0 = __builtin_amdgcn_s_memtime(); t_hop = 0; polls = 0; }
        double x = 1.0 + 1e-3 * g + 1e-9 * total;            // depends on the last round
        for (int i = 0; i < work; ++i) x = fma(x, 0.999999, 1e-7);
        u64* slot = ringw + (r & 1) * RING_WORDS;
        const long long ts = __builtin_amdgcn_s_memtime();
        if (lane < 2) {
            const unsigned w = lane == 0 ? (unsigned)__double2hiint(x) : (unsigned)__double2loint(x);
            const u64 word = ((u64)(unsigned)r << 32) | w;
            if (LOCAL) __hip_atomic_store(slot + g * PAIR_STRIDE + lane, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            else __hip_atomic_store(slot + g * PAIR_STRIDE + lane, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        const u64* p = slot + (have ? (lane >> 1) * PAIR_STRIDE + (lane & 1) : 0);
        u64 v;
        if (!gather<DEPTH, GAP0, GAP>(p, needm, (unsigned)r, v, polls)) {
            if (lane == 0) out[3] = r;                       // expired: every ring leaves in turn
            return;
        }
        t_hop += __builtin_amdgcn_s_memtime() - ts;
        const int w = have ? (int)(unsigned)v : 0;
        const int other = __builtin_amdgcn_update_dpp(0, w, 0xB1, 0xf, 0xf, true);
        const int swap = (w ^ other) & -(lane & 1);
        double d = __hiloint2double(w ^ swap, other ^ swap);
        for (int o = 2; o < 64; o <<= 1) d += __shfl_xor(d, o);
        total = d;
    }
    if (g == 0 && threadIdx.x == 0) {
        out[0] = __builtin_amdgcn_s_memtime() - t0;
        out[1] = t_hop;
        out[2] = polls;
        sink[0] = total;
    }
}

// what N wait states really take, in the same ticks
template <int N>
__global__ void wait_cost(long long* out, int reps) {
    const long long t0 = __builtin_amdgcn_s_memtime();
    for (int i = 0; i < reps; ++i) wait_states<N>();
    out[0] = __builtin_amdgcn_s_memtime() - t0;
}

struct Variant {
    const char* name;
    void (*k[2])(u64*, int*, int, int, int, long long*, double*);
};
#define V(D, G0, G) {"depth " #D " first +" #G0 " gap " #G, {ring<0, D, G0, G>, ring<1, D, G0, G>}}

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 20000;
    const Variant vars[] = {
        V(1, 0, 0),   V(2, 0, 0),                                             // (a) = today's
        V(2, 0, 8),   V(2, 0, 16),  V(2, 0, 24),  V(2, 0, 32),  V(2, 0, 40),  V(2, 0, 48),  V(2, 0, 64),
        V(2, 0, 96),  V(2, 0, 128),                                           // (b)
        V(2, 16, 0),  V(2, 32, 0),  V(2, 48, 0),  V(2, 64, 0),  V(2, 96, 0),  V(2, 128, 0), V(2, 192, 0),
        V(2, 256, 0),                                                         // (c) on the clumped pair
        V(2, 16, 32), V(2, 32, 32), V(2, 48, 32), V(2, 64, 32), V(2, 32, 24), V(2, 64, 128), V(2, 192, 128),
        V(1, 64, 0),  V(1, 128, 0), V(1, 256, 0),
        V(3, 0, 0),   V(3, 0, 20),  V(3, 0, 48),  V(3, 64, 20),               // (d)
        V(4, 0, 0),   V(4, 0, 16),  V(4, 0, 32),  V(4, 64, 16),
    };
    const int nv = sizeof(vars) / sizeof(vars[0]);
    u64* words; int* xcc; long long* out; double* sink;
    const size_t wbytes = (size_t)MAXP * 2 * RING_WORDS * sizeof(u64);
    if (hipMalloc(&words, wbytes) != hipSuccess || hipMalloc(&xcc, 256 * sizeof(int)) != hipSuccess ||
        hipMalloc(&out, 64) != hipSuccess || hipMalloc(&sink, 64) != hipSuccess) { printf("hipMalloc failed\n"); return 1; }
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    {   // ticks per wait state
        long long ht;
        hipLaunchKernelGGL(wait_cost<128>, dim3(1), dim3(64), 0, 0, out, 10000);
        hipMemcpy(&ht, out, 8, hipMemcpyDeviceToHost);
        printf("128 wait states: %.1f ticks\n", (double)ht / 10000);
    }
    // the first pass (agent scope, one XCD) also tells whether blocks 0 mod 8 do share an XCD; the
    // workgroup-scope store is only valid (and only run) if they do
    struct Pass { int local, spread, P, work; };
    const Pass passes[] = {{0, 0, 1, 160}, {0, 0, 8, 160}, {0, 1, 1, 160}, {0, 1, 8, 160},
                           {1, 0, 1, 0},   {1, 0, 1, 160}, {1, 0, 8, 160}};
    bool one_xcd = false;
    for (const Pass& ps : passes) {
        if (ps.local && !one_xcd) { printf("blocks 0 mod 8 do not share one XCD: workgroup-scope passes skipped\n"); break; }
        printf("# store scope %s, groups %s, %d poller(s) per CU, %d dependent FMAs per round\n",
               ps.local ? "workgroup" : "agent", ps.spread ? "spread over the XCDs" : "on one XCD", ps.P, ps.work);
        for (int rep = 0; rep < 2; ++rep)
            for (int i = 0; i < nv; ++i) {
                hipMemset(words, 0, wbytes);
                hipMemset(out, 0, 64);
                hipEventRecord(e0);
                hipLaunchKernelGGL(vars[i].k[ps.local], dim3(256), dim3(64 * ps.P), 0, 0, words, xcc, rounds,
                                   ps.work, ps.spread, out, sink);
                hipEventRecord(e1);
                if (hipEventSynchronize(e1) != hipSuccess) { printf("launch failed\n"); return 1; }
                float ms; hipEventElapsedTime(&ms, e0, e1);
                int hx[256]; long long ho[4];
                hipMemcpy(hx, xcc, sizeof(hx), hipMemcpyDeviceToHost);
                hipMemcpy(ho, out, sizeof(ho), hipMemcpyDeviceToHost);
                int same = 1; for (int j = 0; j < 256; j += 8) same &= hx[j] == hx[0];
                if (!ps.spread) one_xcd = same;
                if (ho[3]) { printf("%-28s spin expired in round %lld\n", vars[i].name, ho[3]); return 1; }
                const double n = rounds - 2;
                printf("%-28s rep %d  %7.1f ns/round  store->gathered %7.1f ticks  %5.2f polls  xcc %d one-XCD %d\n",
                       vars[i].name, rep, ms * 1e6 / rounds, ho[1] / n, ho[2] / n, hx[0], same);
                fflush(stdout);
            }
    }
    return 0;
}
