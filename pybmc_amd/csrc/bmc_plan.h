// Launch planning of the Gibbs and simplex loops: which geometry, how the chains are split over
// launches, and which compiled kernel each launch runs.  Plain C++17 (no HIP): the capacity rules
// below decide both what the host plans and which instantiations exist.  A launch's KernelKey
// (gibbs_kernel_key / simplex_kernel_key) names one instantiation; kernel_compiled() says whether
// it is built, and kernels_gibbs.hip instantiates exactly the keys of loop_kernel_keys(), one
// table entry each.  tests/launch_plan_check.cpp runs the planner and the selection on the CPU.
// Also here: plan_score, the draw-split plan of the pointwise log-likelihood kernels
// (kernels_waic.hip; tests/score_plan_check.cpp), and plan_loo, the pass and candidate plan of
// the PSIS-LOO kernels (kernels_loo.hip; tests/loo_plan_check.cpp), with plan_loo_predict for the
// leave-one-out predictive moments (tests/loo_predict_plan_check.cpp), and plan_ppc, the plan of
// the posterior predictive check (kernels_ppc.hip; tests/ppc_plan_check.cpp), and
// plan_predict_orderstat, the sort / selection route of the posterior predictive's order
// statistics (kernels_predict.hip; tests/predict_plan_check.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/pybmc_amd.h"
#include "bmc_psis_plan.h"

namespace bmc {

constexpr size_t LDS_LIMIT = 160 * 1024;
constexpr int MAX_KCH = 4;        // K <= 256 columns (64 per lane-chunk)
constexpr int MAX_GROUPS = 256;   // 8 teams of <= 32 groups (exchange_sum)

// ---- poll schedule of the granule gather (bmc_loop.h: granule_gather1, exchange_sum) ---------
// A group publishes its total and then polls with `depth` reads in flight.  Read d of the first
// `depth` is issued poll_issue_state(s, d) wait states (s_nop; 4.3 shader cycles each on MI355X)
// behind the publication; every later read is issued when its predecessor has been tested, so the
// reads keep that distance for the whole spin.  One schedule per use, each chosen by a same-box
// A/B of the product after the table of scripts/micro/pollsched.hip:
//   POLL_LOCAL   first level, workgroup-scope store (the groups share an XCD), one chain per
//                pass: the first read ~140 cycles behind the store (an earlier one is certain to
//                miss: every group publishes at about the same time and the store needs longer
//                to land), the second ~100 cycles behind the first, so that the pair samples L2
//                every ~half load round trip (~260 cycles) instead of twice at the same instant
//   POLL_AGENT   first level, agent-scope store, one chain per pass: reads that arrive while the
//                write-through is under way delay it, so the first one waits ~345 cycles (80
//                states).  It was 64 until the leader's way from the residual pass to the
//                publication was shortened (the leader's instruction stream): the
//                optimum is sharp and moved with it -- agent scope forced at C2, 64 / 80 / 96
//                states: 1.110 / 0.957 / 0.962 us per iteration (parent, at 64: 0.955), 16 chains
//                1.747 / 1.494 / 1.262 (parent 1.940); 96 lost N = 100 000 x 32 in one call
//   POLL_PLAIN   first level of the passes that serve 4 or 8 chains (their leaders share a CU)
//                and of the simplex sampler: back to back, as before (the spaced pair was 1.9 %
//                slower for 32 chains at C2 and no faster for the simplex sampler)
//   POLL_LEVEL2  team totals and relay of chains over more than 32 groups: back to back, as
//                before (no spaced or delayed schedule was faster in the micro benchmark)
// One POLL_LOCAL for every kernel class (one chain, 16 packed, a team's first level).  On the
// shortened stream 40 / 16 and 32 / 16 were run on every case of the A/B protocol: neither
// cleared the spread at C2 (0.7958 and 0.7984 against 0.7942 [0.0079]), 40 / 16 lost N = 100 000
// x 32 (1.7888 against 1.7753 [0.0100]) and 32 / 16 lost 16 chains (0.9520 against 0.9333
// [0.0155]), so every class keeps 32 / 24 and there is no selection by class.
struct PollSched {
    int depth, first, gap;
};
constexpr int poll_issue_state(PollSched s, int d) { return s.first + d * s.gap; }
#ifndef BMC_POLL_DEPTH2
#define BMC_POLL_DEPTH2 2
#endif
#ifndef BMC_POLL_FIRST_LOCAL
#define BMC_POLL_FIRST_LOCAL 32
#endif
#ifndef BMC_POLL_GAP_LOCAL
#define BMC_POLL_GAP_LOCAL 24
#endif
#ifndef BMC_POLL_FIRST_AGENT
#define BMC_POLL_FIRST_AGENT 80
#endif
constexpr PollSched POLL_LOCAL{2, BMC_POLL_FIRST_LOCAL, BMC_POLL_GAP_LOCAL};
constexpr PollSched POLL_AGENT{2, BMC_POLL_FIRST_AGENT, 0};
constexpr PollSched POLL_PLAIN{2, 0, 0};
constexpr PollSched POLL_LEVEL2{BMC_POLL_DEPTH2, 0, 0};

// ---- capacity rules (host plan and kernel instantiations) ------------------------------------
constexpr int reg_kmax(int k) { return k <= 8 ? 8 : k <= 16 ? 16 : k <= 32 ? 32 : k <= 64 ? 64 : 0; }

// 1 if rows_per_lane (panels per wave x rows per lane of a panel) rows of k columns fit the 128
// data VGPRs per lane that keep the register-resident loop spill-free (f64: two per element)
constexpr bool gibbs_reg_capacity(int k, bool f32, int rows_per_lane) {
    return reg_kmax(k) > 0 && rows_per_lane * reg_kmax(k) * (f32 ? 1 : 2) <= 128;
}

// register residency with several chains per pass: one panel per wave (PPW = 1).  The panel
// (KMAX*VEC values) plus two blocks of u plus the leaders' state must fit 256 VGPRs: the most
// chains per pass that hipcc compiles without scratch, per (columns, storage type, rows per lane)
constexpr int gibbs_reg_multi_cap(int k, bool f32, int vec) {
    if (reg_kmax(k) == 0) return 0;
    if (vec == 1) return 8;
    if (vec == 2) return reg_kmax(k) * (f32 ? 4 : 8) >= 256 ? 4 : 8;   // 128 VGPRs of panel: 4 chains
    return 0;
}

// PACK: the loop kernel held to 128 VGPRs (4 waves per SIMD), so that two 5-wave groups of
// different chains fit a CU side by side.  It exists only for shapes with one panel of at most 64
// data VGPRs per wave (e.g. K = 32 doubles).
constexpr bool gibbs_packable(int k, bool f32, int vec, int ppw) {
    return ppw == 1 && vec == 1 && reg_kmax(k) > 0 && reg_kmax(k) * (f32 ? 1 : 2) <= 64 &&
           !(f32 && reg_kmax(k) == 64);   // (f32, 64 columns spills at 128)
}
// (at 136 VGPRs the unpacked kernel is 3 % faster per iteration, so a single chain keeps that one)
constexpr bool loop_can_pack(bool f32, int vec, int mode, int kmax, int ppw) {
    return mode == 0 && gibbs_packable(kmax, f32, vec, ppw);
}

// bundles of 8 chains in the balanced two-panels-per-wave layout (PanelStore::partial_rss_reg_bal)
constexpr bool gibbs_bundle_bal_shape(int k, bool f32, int vec, int chains_per_pass) {
    return vec == 1 && chains_per_pass == 8 && reg_kmax(k) >= 16 && gibbs_reg_capacity(k, f32, 2);
}

// one-wave-per-chain kernels (gibbs_wave_kernel, simplex_wave_kernel): row panels x columns a
// wave keeps, RMAX * KMAX <= 128 (and at most 16 panels = 1024 rows)
constexpr int wave_kmax(int k) { return k <= 4 ? 4 : k <= 8 ? 8 : k <= 16 ? 16 : k <= 32 ? 32 : 0; }
constexpr int wave_rmax(int np) { return np <= 2 ? 2 : np <= 4 ? 4 : np <= 8 ? 8 : np <= 12 ? 12 : np <= 16 ? 16 : 0; }
// register-resident FMAs per iteration for k columns and npanels panels of 64 rows PER WAVE,
// 0 = no such kernel; a chain runs in 1, 2, 4 or 8 such waves
constexpr int gibbs_wave_capacity(int k, int npanels) {
    const int km = wave_kmax(k), rm = wave_rmax(npanels);
    return (km > 0 && rm > 0 && km * rm <= 128) ? km * rm : 0;
}
// 8 waves: two per SIMD, 256 registers each -- shapes up to 64 FMAs (12 x 8 spills at 256)
constexpr bool gibbs_wave_fits(int fmas, int waves) { return waves <= 4 || fmas <= 64; }

// ---- argument checks of launch_gibbs / launch_simplex ---------------------------------------
constexpr bool geometry_ok(int k, int G, int waves, int nslot) {
    return k <= 64 * MAX_KCH && G <= MAX_GROUPS && G >= 1 && waves >= 1 && waves <= 8 && nslot >= 1 &&
           nslot <= 2048;
}
// chains of one gibbs_loop_kernel launch (chains_per_pass <= 1) or of one gibbs_multi_kernel launch
// (bundles of chains_per_pass chains, one or one per slot; a leader wave per chain)
constexpr bool gibbs_chains_ok(int n_chains, int chains_per_pass, int waves, int nslot, int bundle_slots,
                               int G, int mode) {
    if (chains_per_pass <= 1) return n_chains >= 1 && n_chains <= nslot;
    return waves >= chains_per_pass && n_chains >= chains_per_pass && n_chains % chains_per_pass == 0 &&
           bundle_slots >= 0 && n_chains / chains_per_pass <= (bundle_slots > 0 ? bundle_slots : 1) &&
           !(bundle_slots > 0 && (G > 32 || mode != 0));
}

// ---- the plan ----------------------------------------------------------------------------
struct Shape {
    int64_t n;
    int k, f32, vec, npanels;   // vec: rows per lane of a panel (choose_vec)
};

// Chip shape from the device properties (MI355X in SPX mode: 256 CUs = 8 XCDs x 32; a
// partitioned device exposes fewer CUs, and the co-residency bound must follow it).
struct Chip {
    int groups_max;   // one resident workgroup per CU
    int xcds;         // slots: blocks b and b + xcds share an XCD (observed round-robin)
    int cu_per_xcd;
};
// cu_limit (bmc_tuning.cu_limit, or its environment default; 0 = none): fewer CUs can hold this
// context's persistent workgroups than the device reports (CU-masked queue, a GPU shared with
// another process)
inline Chip chip_of(int n_cu, int cu_limit) {
    Chip ch;
    ch.groups_max = n_cu > 0 ? n_cu : 256;
    if (cu_limit > 0 && cu_limit < ch.groups_max) ch.groups_max = cu_limit;
    if (ch.groups_max > 256) ch.groups_max = 256;   // the gather holds 2 x 256 granules
    ch.xcds = ch.groups_max >= 64 ? ch.groups_max / 32 : 1;
    ch.cu_per_xcd = ch.groups_max / ch.xcds;
    return ch;
}

// rows per lane: one row per lane whenever the whole matrix can stay in the chip's VGPRs
// (256 CUs x 8 waves x ppw panels of 64 rows); otherwise wide (16-byte) reads once there
// are enough panels to occupy the chip, narrower panels for small N.
inline int choose_vec(int64_t n, int32_t k, int f32) {
    // register residency: the narrowest panel that lets every panel have its own wave (more
    // waves = shorter serial FMA phase); two rows per lane (wider reads for the streaming
    // kernels that share the layout) once one row per lane would need two panels per wave
    const int64_t waves_chip = 256 * 8;   // sized for the full chip; geometry re-checks the fit
    if (gibbs_reg_capacity(k, f32, 1) && (n + 63) / 64 <= waves_chip) return 1;
    if (gibbs_reg_capacity(k, f32, 2) && (n + 127) / 128 <= waves_chip) return 2;
    for (int ppw : {2, 4})
        if (gibbs_reg_capacity(k, f32, ppw) && (n + 63) / 64 <= waves_chip * ppw) return 1;
    int vec = f32 ? 4 : 2;
    while (vec > 1 && (n + 64 * vec - 1) / (64 * vec) < 1024) vec >>= 1;
    return vec;
}

// ---- set-up kernels (kernels_setup.hip): the launch classes a shape reaches -------------------
// residual_rss: workgroups of 4 wave slots; slot w walks panels w, w + 4 G, ...
// 4 workgroups per CU: measured best all-round on MI355X (52 MB: 12.1 us/pass,
// 520 MB: 95 us/pass = 5.5 TB/s); more groups only add ramp-up and tail
inline int32_t rss_groups_of(int32_t npanels) {
    int32_t g = (npanels + 3) / 4;
    if (g > 1024) g = 1024;
    if (g < 1) g = 1;
    return g;
}
constexpr unsigned RSS_FLAT_TICKET_MAX = 256;   // more workgroups than this draw tickets in two levels
// the most panels one wave slot of residual_rss walks
inline int32_t rss_trips_of(int32_t npanels) {
    const int32_t slots = 4 * rss_groups_of(npanels);
    return npanels > 0 ? (npanels + slots - 1) / slots : 0;
}
// rotate: column groups per panel (a workgroup of 4 waves x jt output columns each)
inline uint32_t rotate_col_groups(int32_t ko, int32_t jt) { return (uint32_t)((ko + 4 * jt - 1) / (4 * jt)); }

struct Geometry {
    int chains_per_launch, G, waves, ppg, mode, ppw, nslot;
    int one_wave;   // the chain runs in ONE wave (gibbs_wave_kernel)
};

constexpr int RES_AUTO = 0, RES_REG = 1, RES_STREAM = 3;  // 2 = LDS
// one-wave chains: register-resident FMAs per iteration (rows per lane x columns, padded) up to
// which one wave beats the workgroup form.  Same-box, us per iteration, wave / workgroup:
// 12 x 4 (N = 629, K = 3) 0.351 / 0.629, 16 x 4 0.394 / 0.636, 12 x 8 0.469 / 0.633,
// 2 x 32 0.521 / 0.545; 16 x 8 0.675 / 0.636, 8 x 16 0.657 / 0.562, 4 x 32 0.739 / 0.550
constexpr int ONE_WAVE_MAX_FMAS = 96;

// Pick the launch geometry.  Preference order: row panels in VGPRs with each chain on
// one XCD (8 slots x <= 32 groups), then panels pinned in LDS, then streaming.
inline Geometry choose_geometry(const Shape& s, const bmc_tuning& tu, const Chip& chip, int n_chains,
                                bool allow_one_wave = false, int max_waves = 1) {
    const int MAX_GROUPS_PER_LAUNCH = chip.groups_max, XCD_COUNT = chip.xcds,
              CU_PER_XCD = chip.cu_per_xcd;
    const int RP = 64 * s.vec;
    const size_t es = s.f32 ? 4 : 8;
    const size_t panel_bytes = (size_t)(s.k + 1) * RP * es;
    // u slices for up to 8 chains per pass + partial sums + control words + alignment slack.
    // (An upper bound that decides the residency, not lds_plan: the launch itself checks
    // gibbs_lds_bytes against LDS_LIMIT.)
    const size_t fixed = (size_t)((s.k + 63) / 64 * 64) * 8 * 8 + (512 + 8) * 8 + 64;
    const int NP = s.npanels;
    auto lds_fits = [&](int G) {
        const int ppg = (NP + G - 1) / G;
        return fixed + (size_t)ppg * panel_bytes <= LDS_LIMIT;
    };
    Geometry g{};
    g.ppw = 1;
    // ---- register residency: G <= 32 groups of <= 8 waves, 1/2/4 panels per wave ----
    // ---- small problem: ONE workgroup holds the whole chain in registers -------------------
    // No inter-workgroup exchange, no co-residency requirement (measured 0.85 us/iteration at
    // N = 629 against 1.4 with ten single-wave groups), and every chain is an independent
    // workgroup, so hundreds of chains run side by side in one launch.
    // Smaller still (the reference's data set, 629 x 3): the chain in ONE wave, rows and columns
    // in its registers, no hand-over of any kind inside an iteration (gibbs_wave_kernel; measured
    // at N = 629, K = 3: see DESIGN.md 4.1).  waves_per_group = 1 asks for it, > 1 or an
    // explicit panels_per_wave keep the workgroup form.
    if (allow_one_wave && (tu.residency == RES_AUTO || tu.residency == RES_REG) && s.vec == 1 &&
        tu.groups_per_chain <= 1 && tu.waves_per_group <= 1 && tu.panels_per_wave <= 0) {
        // 1, 2, 4 (one per SIMD) or 8 waves: the fewest that keep a wave's FMAs per iteration
        // within the measured crossover
        int nw = 0, fmas = 0;
        for (int w : {1, 2, 4, 8}) {
            if (w > 1 && (w > max_waves || tu.waves_per_group == 1)) break;
            const int f = gibbs_wave_capacity(s.k, (int)((NP + w - 1) / w));
            if (!gibbs_wave_fits(f, w)) break;
            if (f > 0 && (f <= ONE_WAVE_MAX_FMAS || tu.waves_per_group == 1)) { nw = w; fmas = f; break; }
        }
        if (nw > 0 && fmas > 0) {
            g.mode = 0;
            g.ppw = (int)((NP + nw - 1) / nw);
            g.G = 1;
            g.waves = nw;
            g.ppg = (int)NP;
            g.chains_per_launch = n_chains < 2048 ? n_chains : 2048;
            g.nslot = g.chains_per_launch;
            g.one_wave = 1;
            return g;
        }
    }
    if ((tu.residency == RES_AUTO || tu.residency == RES_REG) && s.vec == 1 &&
        tu.groups_per_chain <= 1) {
        for (int want : {4, 8}) {
            for (int ppw : {1, 2, 4}) {
                if (tu.panels_per_wave > 0 && tu.panels_per_wave != ppw) continue;
                if (!gibbs_reg_capacity(s.k, s.f32, ppw)) continue;
                const int waves = (NP + ppw - 1) / ppw;
                if (waves > want || (tu.waves_per_group > 0 && waves > tu.waves_per_group)) continue;
                g.mode = 0;
                g.ppw = ppw;
                g.G = 1;
                g.waves = tu.waves_per_group > 0 ? tu.waves_per_group : waves;
                g.ppg = NP;
                g.chains_per_launch = n_chains < 2048 ? n_chains : 2048;
                g.nslot = g.chains_per_launch;
                return g;
            }
        }
    }
    if ((tu.residency == RES_AUTO || tu.residency == RES_REG) && s.vec <= 2) {
        // Prefer the fewest panels per wave that keep the chain on ONE XCD (32 groups x 8 waves):
        // its exchange is a single hop through that XCD's L2 (~0.4 us) where a chain spread over
        // the chip pays two levels (~1.3 us), which outweighs one or three more panels per wave
        // (~0.2 us each at K = 32); N = 30000, K = 32: 2.1 -> 1.5 us per iteration, and 8 chains
        // then run side by side, one per XCD.
        int first_ppw = 1;
        if (tu.panels_per_wave <= 0 && tu.groups_per_chain <= 0 && s.vec == 1)
            for (int ppw : {1, 2, 4})
                if (gibbs_reg_capacity(s.k, s.f32, ppw) && (int64_t)CU_PER_XCD * 8 * ppw >= NP) {
                    first_ppw = ppw;
                    break;
                }
        for (int ppw : {1, 2, 4}) {
            if (ppw < first_ppw) continue;
            if (tu.panels_per_wave > 0 && tu.panels_per_wave != ppw) continue;
            if (s.vec == 2 && ppw != 1) continue;
            if (!gibbs_reg_capacity(s.k, s.f32, ppw * s.vec)) continue;
            // one XCD (32 CUs) per chain while the panels fit there (measured: 32 groups x 5
            // waves beats 20 x 8 at C2); otherwise the whole chip serves one chain at a time
            int G = tu.groups_per_chain;
            if (G <= 0) {
                G = NP < CU_PER_XCD ? NP : CU_PER_XCD;
                if ((int64_t)G * 8 * ppw < NP) {
                    G = (int)((NP + 8 * ppw - 1) / (8 * ppw));
                    if (G > MAX_GROUPS_PER_LAUNCH) continue;
                }
            }
            if (G > MAX_GROUPS_PER_LAUNCH) continue;
            // a chain over several XCDs: whole teams (groups g mod 8), so that the kernel can
            // put team j on XCD j whichever XCD the launch starts on
            if (tu.groups_per_chain <= 0 && G > CU_PER_XCD && XCD_COUNT == 8 &&
                ((G + 7) & ~7) <= MAX_GROUPS_PER_LAUNCH)
                G = (G + 7) & ~7;
            const int ppg_reg = (NP + G - 1) / G;
            int waves = tu.waves_per_group > 0 ? tu.waves_per_group : (ppg_reg + ppw - 1) / ppw;
            if (waves > 8 || (int64_t)G * waves * ppw < NP) continue;
            g.mode = 0;
            g.ppw = ppw;
            g.G = G;
            g.waves = waves;
            if (G <= CU_PER_XCD) {
                // one chain per XCD (plan_gibbs widens this when more chains fit side by side)
                g.nslot = XCD_COUNT;
                g.chains_per_launch = n_chains < XCD_COUNT ? n_chains : XCD_COUNT;
            } else {
                g.chains_per_launch = MAX_GROUPS_PER_LAUNCH / G;
                if (g.chains_per_launch > n_chains) g.chains_per_launch = n_chains;
                g.nslot = g.chains_per_launch;
            }
            g.ppg = (NP + G - 1) / G;
            return g;
        }
    }
    // ---- LDS residency or streaming ------------------------------------------------------
    const int t_waves = tu.waves_per_group;
    int cpl = n_chains < XCD_COUNT ? n_chains : XCD_COUNT;
    int G;
    if (tu.groups_per_chain > 0) {
        G = tu.groups_per_chain;
        if (G > MAX_GROUPS_PER_LAUNCH) G = MAX_GROUPS_PER_LAUNCH;
        if (cpl > MAX_GROUPS_PER_LAUNCH / G) cpl = MAX_GROUPS_PER_LAUNCH / G;
        if (cpl < 1) cpl = 1;
    } else {
        // fewer chains per launch until the panels fit in LDS (or one chain is left)
        while (cpl > 1 && !lds_fits(MAX_GROUPS_PER_LAUNCH / cpl)) --cpl;
        const int gmax = MAX_GROUPS_PER_LAUNCH / cpl;
        const int want_waves = t_waves > 0 ? t_waves : 4;
        G = (NP + want_waves - 1) / want_waves;
        if (G > gmax) G = gmax;
        if (G < 1) G = 1;
        if (!lds_fits(G) && lds_fits(gmax))
            while (!lds_fits(G)) ++G;
        if (G > CU_PER_XCD && XCD_COUNT == 8 && ((G + 7) & ~7) <= gmax) G = (G + 7) & ~7;   // whole teams
    }
    if (G > NP) G = NP;
    g.G = G;
    g.chains_per_launch = cpl;
    g.ppg = (NP + G - 1) / G;
    const bool want_stream = tu.residency == RES_STREAM;
    g.mode = (!want_stream && lds_fits(G)) ? 1 : 2;
    int waves = t_waves > 0 ? t_waves : (g.ppg < 4 ? g.ppg : (g.mode == 1 ? (g.ppg < 8 ? g.ppg : 8) : 8));
    if (waves > 8) waves = 8;   // 512-thread workgroups: 256 VGPRs per lane, no spills
    if (waves < 1) waves = 1;
    g.waves = waves;
    // one slot per XCD while a chain's groups fit one XCD's CUs; otherwise any placement
    g.nslot = (G <= CU_PER_XCD) ? XCD_COUNT : cpl;
    return g;
}

// One-XCD register residency: each chain on the groups of one XCD, one chain per XCD.  With more
// chains than XCDs, the packed variant's queries (VGPRs <= 128, two groups per CU) decide whether
// chains c and c + xcds may share XCD c % xcds; they are worth asking only when
// gibbs_pack_candidate holds.
inline bool gibbs_one_xcd_reg(const Geometry& geo, const Chip& chip, const bmc_tuning& tu) {
    return geo.mode == 0 && geo.G > 1 && geo.nslot == chip.xcds && chip.xcds > 1 &&
           geo.G <= chip.cu_per_xcd && tu.groups_per_chain <= 0;
}
inline bool gibbs_pack_candidate(const Geometry& geo, const Chip& chip, const bmc_tuning& tu, int n_chains) {
    return gibbs_one_xcd_reg(geo, chip, tu) && n_chains > geo.nslot && 2 * geo.waves <= 16;
}

// One launch of the persistent Gibbs loop: chains c0 .. c0 + n_chains - 1.
struct GibbsLaunch {
    int c0, n_chains, chains_per_pass, waves, nslot, pack, bundle_slots, bundle_bal;
    int resident;   // workgroups that stay in the loop (the residency check)
};
struct GibbsPlan {
    std::vector<GibbsLaunch> launches;
    int max_per_launch;        // the most chains one launch holds (sizes the exchange words)
    int64_t passes = 0;        // X passes per iteration (a pass serving several chains counts once)
    int chains_per_pass = 1;   // the largest of the launches
    int waves_per_group = 0;   // the largest of the launches (geo.waves without any)
};

// Split n_chains over launches of the geometry.  pack_ok: the packed variant exists for this
// geometry and two of its groups fit a CU (the device's answer; only used where
// gibbs_pack_candidate holds).
inline GibbsPlan plan_gibbs(const Geometry& geo, const Shape& s, const bmc_tuning& tu, const Chip& chip,
                            int n_chains, bool pack_ok) {
    // One-XCD register residency with more than 8 chains.
    // (a) 16 chains or more: the register-resident panels of an XCD's 32 groups serve a BUNDLE of
    //     2 / 4 / 8 chains per pass (gibbs_multi_kernel, one bundle per XCD: 16 .. 64 chains in one
    //     launch); every chain bit-identical to its solo run.
    // (b) 9 .. 15 chains left: chains c and c + 8 share XCD c % 8, two workgroups per CU side by
    //     side.  That needs 4 waves per SIMD (two 5-wave groups must fit whatever SIMDs their
    //     waves land on), i.e. the kernel variant held to 128 VGPRs, which exists for light
    //     shapes only.  (Three or four per XCD are not used: measured, the launch then stalls.)
    const int xcds = chip.xcds, K = s.k;
    const bool xcd_bundles = gibbs_one_xcd_reg(geo, chip, tu) && geo.ppw == 1 && s.vec == 1 && geo.G <= 32 &&
                             tu.chains_per_pass != 1 && gibbs_reg_multi_cap(K, s.f32, s.vec) >= 2;
    pack_ok = pack_ok && gibbs_pack_candidate(geo, chip, tu, n_chains);
    GibbsPlan p;
    p.max_per_launch = geo.chains_per_launch;
    if (pack_ok) p.max_per_launch = 2 * geo.nslot;
    if (xcd_bundles) p.max_per_launch = 8 * xcds;
    if (p.max_per_launch < 8) p.max_per_launch = 8;
    // chains per pass: when the panels are NOT register-resident one read of X can serve up to
    // 8 chains (one leader wave per chain); 0 = automatic, 1 = off
    int cpp_max = 1, waves_multi = geo.waves;
    // (register residency: only the whole-chip form, one chain bundle per launch, one panel per
    // wave; the one-XCD-per-chain form already runs 8 chains side by side)
    const bool reg_multi_ok = geo.mode == 0 && geo.nslot < 8 && geo.G > 1 && geo.ppw == 1;
    if ((geo.mode != 0 || reg_multi_ok) && n_chains > 1 && tu.chains_per_pass != 1) {
        // every chain of a pass needs a leader wave: widen the workgroup if the panels alone
        // would ask for fewer waves (the extra waves own no panel, they only lead a chain)
        int want = n_chains >= 8 ? 8 : n_chains >= 4 ? 4 : 2;
        if (tu.chains_per_pass > 1 && tu.chains_per_pass < want) want = tu.chains_per_pass >= 4 ? 4 : 2;
        if (waves_multi < want && tu.waves_per_group <= 0) waves_multi = want;
        cpp_max = waves_multi >= 8 ? 8 : waves_multi >= 4 ? 4 : waves_multi >= 2 ? 2 : 1;
        if (cpp_max > want) cpp_max = want;
        if (reg_multi_ok) {
            const int cap = gibbs_reg_multi_cap(K, s.f32, s.vec);
            if (cpp_max > cap) cpp_max = cap < 2 ? 1 : cap;
        }
    }
    for (int c0 = 0; c0 < n_chains;) {
        const int left = n_chains - c0;
        GibbsLaunch l{};
        l.c0 = c0;
        l.chains_per_pass = 1;
        l.nslot = geo.nslot;
        // bundles pay from 4 chains per XCD on (measured at C2, us per iteration for all chains:
        // 16 chains 1.37 as bundles of 2 against 1.05 packed two per XCD; 32 chains 1.81 as
        // bundles of 4 against 2 x 1.05; 64 chains 2.33 as bundles of 8); with fewer they are
        // used when asked for (chains_per_pass = 2) or when the shape has no packed variant
        if (xcd_bundles && left >= 2 * xcds && (left >= 4 * xcds || !pack_ok || tu.chains_per_pass > 1)) {
            // one bundle per XCD: as many chains per bundle as keep all XCDs busy
            int cap = gibbs_reg_multi_cap(K, s.f32, s.vec);
            if (tu.chains_per_pass > 1 && tu.chains_per_pass < cap) cap = tu.chains_per_pass;
            int cpp = 2;
            while (cpp * 2 <= cap && cpp * 2 * xcds <= left) cpp *= 2;
            // 40 .. 63 chains: bundles of 8 on 5 .. 7 XCDs in one launch (2.3 us per iteration at C2)
            // rather than bundles of 4 on all 8 (1.8 us for 32 of them) plus a second launch
            if (cap >= 8 && cpp == 4 && left >= 5 * 8) cpp = 8;
            const int bundles = left / cpp < xcds ? left / cpp : xcds;
            l.chains_per_pass = cpp;
            l.n_chains = bundles * cpp;
            l.bundle_slots = xcds;
            l.waves = geo.waves > cpp ? geo.waves : cpp;   // a leader wave per chain
            // bundles of 8 on 8 waves, at most 5 panels per group, two panels of K columns in a
            // wave's registers: the balanced layout (4 chains of panel w % 4 + 1 chain of the
            // fifth panel per wave instead of 8 chains of one panel on waves 0 .. 3)
            // (panels_per_wave = 1 asked for explicitly keeps the one-panel layout: the A/B knob)
            l.bundle_bal = gibbs_bundle_bal_shape(K, s.f32, s.vec, cpp) && l.waves == 8 && geo.ppg <= 5 &&
                           tu.panels_per_wave != 1;
            l.resident = bundles * geo.G;
            p.passes += bundles;
        } else if (cpp_max > 1 && left >= 2) {
            int cpp = 1;
            while (cpp * 2 <= left && cpp * 2 <= cpp_max) cpp *= 2;
            l.chains_per_pass = cpp;
            l.n_chains = cpp;
            l.waves = waves_multi;
            l.resident = geo.G;
            p.passes += 1;
        } else {
            l.waves = geo.waves;
            if (pack_ok && left > geo.nslot) {
                l.pack = 1;
                l.nslot = 2 * geo.nslot;
            }
            const int cap = l.pack ? l.nslot : geo.chains_per_launch;
            l.n_chains = left < cap ? left : cap;
            l.resident = l.n_chains * geo.G;
            p.passes += l.n_chains;
        }
        if (l.chains_per_pass > p.chains_per_pass) p.chains_per_pass = l.chains_per_pass;
        if (l.waves > p.waves_per_group) p.waves_per_group = l.waves;
        p.launches.push_back(l);
        c0 += l.n_chains;
    }
    if (p.waves_per_group == 0) p.waves_per_group = geo.waves;   // widened for leader waves
    return p;
}

// ---- which compiled kernel a launch runs ----------------------------------------------------
// One key per instantiation of the loop kernels of kernels_gibbs.hip (T = f32 ? float : double):
//   KF_LOOP          gibbs_loop_kernel<T, vec, mode, kmax, ppw, single, pack, smallg>
//   KF_MULTI         gibbs_multi_kernel<T, vec, mode, cpp, kmax, ppw, slotted, bal>
//   KF_WAVE          gibbs_wave_kernel<T, rmax, kmax, nw>
//   KF_SIMPLEX_LOOP  simplex_loop_kernel<T, vec, mode, kmax, ppw, single>
//   KF_SIMPLEX_WAVE  simplex_wave_kernel<T, rmax, kmax, nw > 1>   (MANY)
enum KernelFamily { KF_NONE, KF_LOOP, KF_MULTI, KF_WAVE, KF_SIMPLEX_LOOP, KF_SIMPLEX_WAVE };
struct KernelKey {
    int family = KF_NONE, f32 = 0;
    int vec = 0, mode = 0, kmax = 0, ppw = 0, cpp = 0, rmax = 0, nw = 0;
    bool single = false, pack = false, smallg = false, slotted = false, bal = false;
};
constexpr bool operator==(const KernelKey& a, const KernelKey& b) {
    return a.family == b.family && a.f32 == b.f32 && a.vec == b.vec && a.mode == b.mode && a.kmax == b.kmax &&
           a.ppw == b.ppw && a.cpp == b.cpp && a.rmax == b.rmax && a.nw == b.nw && a.single == b.single &&
           a.pack == b.pack && a.smallg == b.smallg && a.slotted == b.slotted && a.bal == b.bal;
}

// The instantiation rules.  LDS / streaming (mode 1, 2): one kernel per rows per lane (4 for f32
// only).  Registers: kmax = reg_kmax, rows per lane (ppw x vec; vec 2: one panel per wave) within
// gibbs_reg_capacity; the single-chain loop as the general kernel, SINGLE (G = 1), SMALLG
// (G <= 32) and, where packable, PACK; bundles of cpp <= gibbs_reg_multi_cap chains, SLOTTED
// (one bundle per XCD) for one row per lane, BAL for gibbs_bundle_bal_shape.  One wave per chain:
// rmax x kmax within gibbs_wave_capacity on 1, 2 / 4 (nw 4) or, if gibbs_wave_fits, 8 waves;
// the simplex sampler has no 8-wave kernel.
constexpr bool kernel_compiled(const KernelKey& k) {
    const bool mem_vec = k.vec == 1 || k.vec == 2 || (k.vec == 4 && k.f32);
    const bool reg_ok = k.kmax > 0 && reg_kmax(k.kmax) == k.kmax && (k.vec == 1 || k.vec == 2);
    switch (k.family) {
        case KF_LOOP:
        case KF_SIMPLEX_LOOP:
            if (k.mode != 0)
                return (k.mode == 1 || k.mode == 2) && mem_vec && k.kmax == 0 && k.ppw == 0 && !k.single &&
                       !k.pack && !k.smallg;
            if (!reg_ok || !(k.ppw == 1 || k.ppw == 2 || k.ppw == 4) || (k.vec == 2 && k.ppw != 1) ||
                !gibbs_reg_capacity(k.kmax, k.f32, k.ppw * k.vec))
                return false;
            if (k.family == KF_SIMPLEX_LOOP) return !k.pack && !k.smallg;
            return k.pack ? k.smallg && !k.single && loop_can_pack(k.f32, k.vec, k.mode, k.kmax, k.ppw)
                          : !(k.single && k.smallg);
        case KF_MULTI:
            if (k.cpp != 2 && k.cpp != 4 && k.cpp != 8) return false;
            if (k.mode != 0)
                return (k.mode == 1 || k.mode == 2) && mem_vec && k.kmax == 0 && k.ppw == 0 && !k.slotted && !k.bal;
            if (!reg_ok || !gibbs_reg_capacity(k.kmax, k.f32, k.vec) || k.cpp > gibbs_reg_multi_cap(k.kmax, k.f32, k.vec))
                return false;
            if (k.bal) return k.slotted && k.ppw == 2 && gibbs_bundle_bal_shape(k.kmax, k.f32, k.vec, k.cpp);
            return k.ppw == 1 && (!k.slotted || k.vec == 1);
        case KF_WAVE:
        case KF_SIMPLEX_WAVE:
            if (wave_kmax(k.kmax) != k.kmax || wave_rmax(k.rmax) != k.rmax || gibbs_wave_capacity(k.kmax, k.rmax) == 0)
                return false;
            return k.nw == 1 || k.nw == 4 || (k.family == KF_WAVE && k.nw == 8 && gibbs_wave_fits(k.rmax * k.kmax, 8));
    }
    return false;
}

// Every compiled key, in a fixed order: the key space enumerated once, filtered by kernel_compiled
struct KernelKeys {
    KernelKey key[512];
    int n = 0;
};
constexpr KernelKeys loop_kernel_keys() {
    KernelKeys ks{};
    auto add = [&ks](const KernelKey& k) {
        if (kernel_compiled(k)) ks.key[ks.n++] = k;
    };
    for (int f32 = 0; f32 < 2; ++f32) {
        for (int vec : {1, 2, 4})
            for (int mode : {0, 1, 2})
                for (int kmax : {0, 8, 16, 32, 64})
                    for (int ppw : {0, 1, 2, 4})
                        for (int v = 0; v < 8; ++v) {
                            const bool b0 = v & 1, b1 = v & 2, b2 = v & 4;
                            add({KF_LOOP, f32, vec, mode, kmax, ppw, 0, 0, 0, b0, b1, b2, false, false});
                            add({KF_SIMPLEX_LOOP, f32, vec, mode, kmax, ppw, 0, 0, 0, b0, b1, b2, false, false});
                            for (int cpp : {2, 4, 8})
                                if (v < 4) add({KF_MULTI, f32, vec, mode, kmax, ppw, cpp, 0, 0, false, false, false, b0, b1});
                        }
        for (int rmax : {2, 4, 8, 12, 16})
            for (int kmax : {4, 8, 16, 32})
                for (int nw : {1, 4, 8}) {
                    add({KF_WAVE, f32, 0, 0, kmax, 0, 0, rmax, nw, false, false, false, false, false});
                    add({KF_SIMPLEX_WAVE, f32, 0, 0, kmax, 0, 0, rmax, nw, false, false, false, false, false});
                }
    }
    return ks;
}

// The one-wave kernels: rmax x kmax of the panels a wave keeps, 1 / 4 / 8 waves (KF_NONE: none)
inline KernelKey wave_kernel_key(int family, const Shape& s, int waves, int n_blocks) {
    const int nw = waves > 1 ? waves : 1;
    const int rpw = (s.npanels + nw - 1) / nw;
    if (s.vec != 1 || !gibbs_wave_capacity(s.k, rpw) || n_blocks < 1 || (nw != 1 && nw != 2 && nw != 4 && nw != 8))
        return KernelKey{};
    KernelKey key;
    key.family = family;
    key.f32 = s.f32 != 0;
    key.kmax = wave_kmax(s.k);
    key.rmax = wave_rmax(rpw);
    key.nw = nw > 4 ? 8 : nw > 1 ? 4 : 1;
    return key;
}

// The single-chain loop kernels of both samplers: registers (kmax, ppw; SINGLE for one workgroup)
// or LDS / streaming
inline KernelKey loop_kernel_key(int family, const Shape& s, const Geometry& g) {
    KernelKey key;
    key.family = family;
    key.f32 = s.f32 != 0;
    key.vec = s.vec;
    key.mode = g.mode == 0 ? 0 : g.mode == 1 ? 1 : 2;
    if (key.mode == 0) {
        key.kmax = reg_kmax(s.k);
        key.ppw = g.ppw;
        key.single = g.G == 1;
    }
    return key;
}

// The kernel of one launch of a Gibbs plan (launch_gibbs).  The key may name a kernel that is not
// compiled: check kernel_compiled().
inline KernelKey gibbs_kernel_key(const Shape& s, const Geometry& g, const GibbsLaunch& l) {
    if (g.one_wave) return wave_kernel_key(KF_WAVE, s, l.waves, l.n_chains);
    KernelKey key = loop_kernel_key(KF_LOOP, s, g);
    if (l.chains_per_pass > 1) {   // bundles of chains: registers with one panel per wave (BAL: two)
        key.family = KF_MULTI;
        key.cpp = l.chains_per_pass;
        key.single = false;
        if (key.mode == 0) {
            if (g.ppw != 1) return KernelKey{};
            key.slotted = l.bundle_slots > 0;
            key.bal = l.bundle_bal != 0;
            key.ppw = key.bal ? 2 : 1;
        }
    } else if (key.mode == 0 && g.G > 1) {
        // PACK where the packed variant exists (two chains per XCD: SMALLG), else SMALLG for the
        // one-level exchange
        key.pack = l.pack && loop_can_pack(key.f32, key.vec, key.mode, key.kmax, key.ppw);
        key.smallg = key.pack || g.G <= 32;
    }
    return key;
}

// The kernel of the simplex sampler's launch (launch_simplex)
inline KernelKey simplex_kernel_key(const Shape& s, const Geometry& g) {
    if (g.one_wave) return wave_kernel_key(KF_SIMPLEX_WAVE, s, g.waves, 1);
    return loop_kernel_key(KF_SIMPLEX_LOOP, s, g);
}

// ---- simplex chains over launches -----------------------------------------------------------
// One launch of the simplex loop: chains c0 .. c0 + n_chains - 1 of the call.
struct SimplexLaunch {
    int c0, n_chains;
    int nslot;      // workgroup form: grid = nslot x G, chain = block % nslot (wave form: unused)
    int resident;   // workgroups that wait for one another inside the loop: n_chains x G
};
struct SimplexPlan {
    Geometry geo;   // of ONE chain: every chain of every launch runs simplex_kernel_key(shape, geo)
    std::vector<SimplexLaunch> launches;
    int max_per_launch = 0;   // the most chains one launch holds (sizes the exchange words)
};

// Split n_chains simplex chains over launches.  The geometry is the one a single chain gets
// (choose_geometry for one chain; the one-wave form needs a model per lane), so a chain runs the
// same kernel on the same grid shape whatever its neighbours: that is what makes chain c of a call
// bit for bit its solo run.
//   one-wave form   one block per chain, all chains in one launch up to the 2048 blocks the Gibbs
//                   one-wave launches use as well
//   workgroup form  a chain needs G co-resident workgroups, and the device holds groups_max (one
//                   per CU, cu_limit): groups_max / G chain slots per launch.  Where one chain
//                   gets the XCD labelling (geo.nslot = the XCD count: its groups are the blocks
//                   b = slot mod 8, which share an XCD) every chain keeps it: one chain per XCD,
//                   slot c for chain c, as plan_gibbs batches its single-chain loops.
inline SimplexPlan plan_simplex_launches(const Shape& s, const bmc_tuning& tu, const Chip& chip, int n_models,
                                         int n_chains) {
    SimplexPlan p;
    p.geo = choose_geometry(s, tu, chip, 1, n_models <= 64, 4);
    const bool xcd_slots = !p.geo.one_wave && chip.xcds > 1 && p.geo.nslot == chip.xcds;
    int cap = 2048;
    if (!p.geo.one_wave) {
        cap = xcd_slots ? chip.xcds : chip.groups_max / p.geo.G;
        if (cap < 1) cap = 1;
    }
    for (int c0 = 0; c0 < n_chains;) {
        SimplexLaunch l{};
        l.c0 = c0;
        l.n_chains = n_chains - c0 < cap ? n_chains - c0 : cap;
        l.nslot = xcd_slots ? chip.xcds : l.n_chains;
        l.resident = l.n_chains * p.geo.G;
        if (l.n_chains > p.max_per_launch) p.max_per_launch = l.n_chains;
        p.launches.push_back(l);
        c0 += l.n_chains;
    }
    return p;
}

// The key as the demangled kernel name, e.g. gibbs_loop_kernel<double, 1, 0, 32, 1, false, false, true>
inline std::string kernel_name(const KernelKey& k) {
    const char* T = k.f32 ? "float" : "double";
    auto b = [](bool x) { return x ? "true" : "false"; };
    char buf[128];
    switch (k.family) {
        case KF_LOOP:
            std::snprintf(buf, sizeof buf, "gibbs_loop_kernel<%s, %d, %d, %d, %d, %s, %s, %s>", T, k.vec, k.mode,
                          k.kmax, k.ppw, b(k.single), b(k.pack), b(k.smallg));
            break;
        case KF_MULTI:
            std::snprintf(buf, sizeof buf, "gibbs_multi_kernel<%s, %d, %d, %d, %d, %d, %s, %s>", T, k.vec, k.mode,
                          k.cpp, k.kmax, k.ppw, b(k.slotted), b(k.bal));
            break;
        case KF_WAVE:
            std::snprintf(buf, sizeof buf, "gibbs_wave_kernel<%s, %d, %d, %d>", T, k.rmax, k.kmax, k.nw);
            break;
        case KF_SIMPLEX_LOOP:
            std::snprintf(buf, sizeof buf, "simplex_loop_kernel<%s, %d, %d, %d, %d, %s>", T, k.vec, k.mode, k.kmax,
                          k.ppw, b(k.single));
            break;
        case KF_SIMPLEX_WAVE:
            std::snprintf(buf, sizeof buf, "simplex_wave_kernel<%s, %d, %d, %s>", T, k.rmax, k.kmax, b(k.nw > 1));
            break;
        default:
            return "none";
    }
    return buf;
}

// ---- pointwise log-likelihood (kernels_waic.hip) -------------------------------
// A workgroup owns SCORE_TILE points and walks draw tiles of SCORE_TILE draws.  Few points and
// many draws is the common case (377 training rows, 50 000 draws: 6 point tiles for 256 CUs), so
// the draw tiles are split over `splits` workgroups per point tile; their partials are merged in
// split order by a second kernel.  The plan depends on the shapes and the CU count only:
//   * target: SCORE_GROUPS_PER_CU workgroups per CU (two 4-wave groups keep every SIMD supplied
//     while the other group waits at its slab barrier);
//   * a split walks at least SCORE_MIN_TILES draw tiles (below that the per-group set-up and the
//     lane merge at its end outweigh the work), and no split is empty;
//   * point tiles alone reaching the target means one split.
constexpr int SCORE_TILE = 64;
constexpr int SCORE_GROUPS_PER_CU = 2;
constexpr int SCORE_MIN_TILES = 4;
constexpr int SCORE_MAX_K = 256;

struct ScorePlan {
    int64_t point_tiles;      // ceil(n_points / 64)
    int64_t draw_tiles;       // ceil(n_draws / 64)
    int64_t tiles_per_split;  // draw tiles of every split but the last
    int64_t splits;           // split j walks draw tiles [j * tiles_per_split, ...), none empty
    int32_t k_pad;            // columns rounded up to whole 16-column slabs
};

inline ScorePlan plan_score(int64_t n_points, int64_t n_draws, int32_t k, int n_cu) {
    ScorePlan p;
    p.point_tiles = (n_points + SCORE_TILE - 1) / SCORE_TILE;
    p.draw_tiles = (n_draws + SCORE_TILE - 1) / SCORE_TILE;
    p.k_pad = (k + 15) / 16 * 16;
    const int64_t target = (int64_t)SCORE_GROUPS_PER_CU * (n_cu > 0 ? n_cu : 1);
    int64_t want = (target + p.point_tiles - 1) / p.point_tiles;   // 1 when the point tiles suffice
    const int64_t most = p.draw_tiles / SCORE_MIN_TILES;   // (every split at least that long)
    if (want > most) want = most;
    if (want < 1) want = 1;
    p.tiles_per_split = (p.draw_tiles + want - 1) / want;
    p.splits = (p.draw_tiles + p.tiles_per_split - 1) / p.tiles_per_split;
    return p;
}

// ---- PSIS-LOO (kernels_loo.hip) ------------------------------------------------
// Per point the M smallest ll[i][.] (the M largest importance ratios) and the next one, of a
// matrix that is never stored.  Every pass over the matrix is the tile loop of the score kernels
// with the same draw splits (plan_score).  The passes:
//   1        the score kernels themselves (lppd_i; they also pad A, y and make the draw constants)
//   1        range: smallest and largest order-preserving 64-bit key of ll per point
//   0 .. 8   radix select on the key bits below the point's common prefix, LOO_DIGIT_BITS per
//            pass, digits counted in LDS per 64-point tile; a point is settled once the bucket
//            that holds rank M + 1, plus everything below it, fits `cap` candidates, or once all
//            64 bits are fixed (then the bucket is ONE value, repeated).  A workgroup whose 64
//            points are settled returns at once, so the launches past the second or third are
//            empty for ordinary input; 64 / LOO_DIGIT_BITS bounds them for any input.
//   1        append: keys below the bucket (at most M, by the definition of the bucket) and, if
//            it fits, the bucket itself go to the point's candidate slots; exp(lw) of everything
//            above is summed in a fixed order.  At most `cap` slots are ever written.
// then one workgroup per point sorts its candidates and does the fit.  No select pass is needed
// when S <= cap (everything is a candidate) or when S < 25 (no tail).
constexpr int LOO_DIGIT_BITS = 8;
constexpr int LOO_MAX_SELECT_PASSES = 64 / LOO_DIGIT_BITS;
constexpr int64_t LOO_MIN_CAP = 64;
constexpr int64_t LOO_MAX_CAP = 16384;   // the per-point sort is done in LDS: 128 KiB of doubles

// the tail of the fit (bmc_psis_plan.h); 0 when that is below the minimum: nothing is smoothed
constexpr int LOO_MIN_TAIL = PSIS_MIN_TAIL;
inline int64_t loo_tail(int64_t n_draws) {
    const int64_t M = psis_tail_length(n_draws);
    return M < LOO_MIN_TAIL ? 0 : M;
}

struct LooPlan {
    ScorePlan score;         // tiles and draw splits of every pass over the matrix
    int64_t tail;            // M; 0: no smoothing (S < 25)
    int32_t grid_points;     // of the generalised Pareto fit on the tail (0: no tail)
    int64_t cap;             // candidate slots per point: a power of two >= 2 (M + 1)
    int32_t select_passes;   // launches of the select kernel (0 or LOO_MAX_SELECT_PASSES)
    int32_t matrix_passes;   // all launches that walk the matrix: score, range, select, append
    bool ok;                 // cap <= LOO_MAX_CAP (about 7.4 million draws)
};

inline LooPlan plan_loo(int64_t n_points, int64_t n_draws, int32_t k, int n_cu) {
    LooPlan p;
    p.score = plan_score(n_points, n_draws, k, n_cu);
    p.tail = loo_tail(n_draws);
    p.grid_points = p.tail > 0 ? psis_grid_points(p.tail) : 0;
    p.cap = LOO_MIN_CAP;
    while (p.cap < 2 * (p.tail + 1)) p.cap <<= 1;
    p.ok = p.cap <= LOO_MAX_CAP;
    p.select_passes = (p.tail > 0 && n_draws > p.cap) ? LOO_MAX_SELECT_PASSES : 0;
    p.matrix_passes = 3 + p.select_passes;
    return p;
}

// Device work space of launch_loo besides the score kernels' own (score_buffers), in bytes:
// O(n_points (M + 256 + splits)).
struct LooBuffers {
    size_t range;    // [splits][n_pad][3] u64: smallest key, largest key, non-finite seen
    size_t prefix;   // [n_pad] u64: the fixed high bits of the threshold key
    size_t kmin;     // [n_pad] u64: the smallest key (c_i = -ll of it)
    size_t meta;     // [n_pad][4] u32: bits fixed, keys below the bucket, keys in it, flags
    size_t hist;     // [n_pad][256] u32: digit counts of the current select pass
    size_t count;    // [n_pad] u32: candidates appended
    size_t cand;     // [n_pad][cap] f64
    size_t body;     // [splits][n_pad] f64: sum of exp(lw) above the bucket
    size_t out;      // [2][n_points] f64: elpd_loo_i, pareto_k
    size_t total() const { return range + prefix + kmin + meta + hist + count + cand + body + out; }
};
inline LooBuffers loo_buffers(const LooPlan& p, int64_t n_points) {
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t n_pad = (size_t)p.score.point_tiles * SCORE_TILE, sp = (size_t)p.score.splits;
    LooBuffers b;
    b.range = up(sp * n_pad * 3 * 8);
    b.prefix = up(n_pad * 8);
    b.kmin = up(n_pad * 8);
    b.meta = up(n_pad * 16);
    b.hist = up(n_pad * ((size_t)1 << LOO_DIGIT_BITS) * 4);
    b.count = up(n_pad * 4);
    b.cand = up(n_pad * (size_t)p.cap * 8);
    b.body = up(sp * n_pad * 8);
    b.out = up((size_t)n_points * 2 * 8);
    return b;
}

// ---- PSIS-LOO predictive moments (kernels_loo.hip) ------------------------------
// The passes of plan_loo with the PREDICT variants of append and fit, and between them one more
// pass over the matrix for the points whose bucket is one repeated value (only when the select
// runs; a workgroup without such a point returns at once).  The fit sorts (value, draw) pairs and
// keeps every sorted candidate next to the tail's weights: LOO_PREDICT_SLOT_LDS bytes of LDS per
// candidate slot (8 value, 4 tail, 4 draw index) where plan_loo needs 8, so of gfx950's 160 KiB
// (less the fit's LOO_FIT_STATIC_LDS of reduction and grid arrays) the largest cap is 8192:
// M = ceil(3 sqrt(S)) <= 4095, S <= 4095^2 / 9 = LOO_PREDICT_MAX_DRAWS.
constexpr int64_t LOO_PREDICT_SLOT_LDS = 16;
constexpr int64_t LOO_PREDICT_MAX_CAP = 8192;
constexpr int64_t LOO_PREDICT_MAX_DRAWS = 1863225;
constexpr int64_t LOO_FIT_STATIC_LDS = 6144;       // (an upper bound: 5 KiB of arrays and a few scalars)
constexpr int64_t LOO_LDS_BYTES = 160 * 1024;
constexpr int LOO_PREDICT_OUTS = 6;     // elpd_loo_i, pareto_k, loo_mean, loo_sd, loo_pit, ess
constexpr int LOO_PREDICT_SUMS = 4;     // per point besides sum w: w r, w (sigma^2 + r^2), w Phi, w^2
constexpr int LOO_BUCKET_SUMS = 3;      // of a one-value bucket: r, sigma^2 + r^2, Phi
// Under the Student-t likelihood (student) the append runs in LOO_PREDICT_T_PHASES
// phases, each one more pass over the matrix: the first sums everything but w F and writes the
// candidates, the second recomputes the weights and sums w F alone (the t distribution function of
// bmc_math.h on top of the t density does not fit the registers of one kernel).  Both write the same
// LOO_PREDICT_SUMS slots.  The passes read LOO_PREDICT_T_ROWS more constants per draw: the variance
// term sigma_s^2 nu_s / (nu_s - 2) (0 where the call's loo_sd is +inf) and nu_s.
constexpr int LOO_PREDICT_T_PHASES = 2;
constexpr int LOO_PREDICT_T_ROWS = 2;

struct LooPredictPlan {
    LooPlan loo;             // the passes both calls share
    int64_t record_bytes;    // global memory per candidate: the value and its draw index
    int64_t fit_lds;         // dynamic LDS of the fit: cap * LOO_PREDICT_SLOT_LDS
    int32_t bucket_pass;     // 1: the one-value-bucket pass is launched
    int32_t append_phases;   // launches of the append: 1, or LOO_PREDICT_T_PHASES under the t likelihood
    int64_t draw_rows;       // doubles of further per-draw constants: LOO_PREDICT_T_ROWS * n_draws, or 0
    int32_t matrix_passes;   // all launches that walk the matrix
    bool ok;                 // loo.cap <= LOO_PREDICT_MAX_CAP (LOO_PREDICT_MAX_DRAWS draws)
};

inline LooPredictPlan plan_loo_predict(int64_t n_points, int64_t n_draws, int32_t k, int n_cu,
                                       bool student = false) {
    LooPredictPlan p;
    p.loo = plan_loo(n_points, n_draws, k, n_cu);
    p.record_bytes = 8 + 4;
    p.fit_lds = p.loo.cap * LOO_PREDICT_SLOT_LDS;
    p.bucket_pass = p.loo.select_passes > 0 ? 1 : 0;
    p.append_phases = student ? LOO_PREDICT_T_PHASES : 1;
    p.draw_rows = student ? (int64_t)LOO_PREDICT_T_ROWS * n_draws : 0;
    p.matrix_passes = p.loo.matrix_passes + p.bucket_pass + (p.append_phases - 1);
    p.ok = p.loo.cap <= LOO_PREDICT_MAX_CAP;
    return p;
}

// Device work space of launch_loo_predict: loo_buffers, then
struct LooPredictBuffers {
    LooBuffers loo;
    size_t candidx;   // [n_pad][cap] u32: the draw of every candidate
    size_t pay;       // [splits][n_pad][4] f64: the payload sums above the bucket
    size_t bucket;    // [splits][n_pad][3] f64: the payload sums of a one-value bucket
    size_t out;       // [6][n_points] f64
    size_t tc;        // [LOO_PREDICT_T_ROWS][n_draws] f64: the t passes' further constants (0: Gaussian)
    size_t total() const { return loo.total() + candidx + pay + bucket + out + tc; }
};
inline LooPredictBuffers loo_predict_buffers(const LooPredictPlan& p, int64_t n_points) {
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t n_pad = (size_t)p.loo.score.point_tiles * SCORE_TILE, sp = (size_t)p.loo.score.splits;
    LooPredictBuffers b;
    b.loo = loo_buffers(p.loo, n_points);
    b.candidx = up(n_pad * (size_t)p.loo.cap * 4);
    b.pay = up(sp * n_pad * LOO_PREDICT_SUMS * 8);
    b.bucket = up(sp * n_pad * LOO_BUCKET_SUMS * 8);
    b.out = up((size_t)n_points * LOO_PREDICT_OUTS * 8);
    b.tc = up((size_t)p.draw_rows * 8);
    return b;
}

// ---- posterior predictive check (kernels_ppc.hip) -------------------------------
// The same never-stored points x draws matrix, reduced over the POINTS, per draw: a workgroup owns
// SCORE_TILE draws and walks every point tile, so the roles of plan_score are swapped and there
// is no split: one workgroup per draw tile, whatever the CU count (fewer than 64 x CUs draws leave
// CUs idle; the bits do not depend on the device).  Both operands are padded to whole tiles: the
// draws [S_pad][k_pad] (with sigma_s, 1 / sigma_s and the centre c_s per draw) and the design
// [n_pad][k_pad] (with y and the offset per point, and its column means).  Refused (ok = false): fewer than PPC_MIN_POINTS points (skew and
// kurt of fewer are constants), fewer than 2 draws, k outside 1 .. SCORE_MAX_K, more points than
// PPC_MAX_POINTS (the noise counter carries the point pair in one 32-bit word).
constexpr int PPC_STATS = 8;      // min, max, mean, sd, skew, kurt, chi2, max_abs_z (replicated)
constexpr int PPC_OBS = 2;        // chi2, max_abs_z (observed: the two that depend on the draw)
constexpr int64_t PPC_MIN_POINTS = 3;
constexpr int64_t PPC_MAX_POINTS = (int64_t)1 << 31;

struct PpcPlan {
    int64_t point_tiles, draw_tiles;   // ceil(n / 64), ceil(S / 64)
    int64_t n_pad, S_pad;              // whole tiles
    int32_t k_pad;                     // whole 16-column slabs
    int64_t grid;                      // workgroups: draw_tiles
    int64_t rounds;                    // ceil(grid / (SCORE_GROUPS_PER_CU * n_cu)): 1 = one wave of groups
    bool ok;
};

inline PpcPlan plan_ppc(int64_t n_points, int64_t n_draws, int32_t k, int n_cu) {
    PpcPlan p{};
    p.ok = n_points >= PPC_MIN_POINTS && n_points <= PPC_MAX_POINTS && n_draws >= 2 && k >= 1 &&
           k <= SCORE_MAX_K && (n_draws + SCORE_TILE - 1) / SCORE_TILE <= 0x7fffffffll;
    if (!p.ok) return p;
    p.point_tiles = (n_points + SCORE_TILE - 1) / SCORE_TILE;
    p.draw_tiles = (n_draws + SCORE_TILE - 1) / SCORE_TILE;
    p.n_pad = p.point_tiles * SCORE_TILE;
    p.S_pad = p.draw_tiles * SCORE_TILE;
    p.k_pad = (k + 15) / 16 * 16;
    p.grid = p.draw_tiles;
    const int64_t slots = (int64_t)SCORE_GROUPS_PER_CU * (n_cu > 0 ? n_cu : 1);
    p.rounds = (p.grid + slots - 1) / slots;
    return p;
}

// Device work space of launch_ppc, in bytes
struct PpcBuffers {
    size_t Ap;    // [n_pad][k_pad] f64: the design, zero in the padding
    size_t yo;    // [2][n_pad] f64: y, then the offset
    size_t Tp;    // [S_pad][k_pad] f64: the coefficients of every draw, zero in the padding
    size_t sg;    // [3][S_pad] f64: sigma_s, 1 / sigma_s (1 in the padding; NaN marks a bad draw) and
                  // the draw's centre c_s; then [k_pad + 16]: the column means of the design and,
                  // at k_pad, the mean offset
    size_t out;   // [S][PPC_STATS] then [S][PPC_OBS] f64
    size_t total() const { return Ap + yo + Tp + sg + out; }
};
inline PpcBuffers ppc_buffers(const PpcPlan& p, int64_t n_draws) {
    PpcBuffers b;
    b.Ap = (size_t)p.n_pad * (size_t)p.k_pad * 8;
    b.yo = (size_t)p.n_pad * 2 * 8;
    b.Tp = (size_t)p.S_pad * (size_t)p.k_pad * 8;
    b.sg = ((size_t)p.S_pad * 3 + (size_t)p.k_pad + 16) * 8;
    b.out = (size_t)n_draws * (PPC_STATS + PPC_OBS) * 8;
    return b;
}
// The Student-t check with a nu per draw (PpcArgs::nus) needs one buffer more, [2][S_pad] f64: nu_s,
// then 2 / nu_s (4 and 1/2 in the padding).  A function of its own: no size above depends on the
// noise.  At most PPC_MAX_NU_VALUES distinct values, the limit of the scorers' nu_draws.
constexpr int32_t PPC_MAX_NU_VALUES = 4096;
inline size_t ppc_nu_bytes(const PpcPlan& p) { return (size_t)p.S_pad * 2 * 8; }

// ---- posterior predictive order statistics (kernels_predict.hip) ----------------
// Which kernels read the requested ranks off the S draws of each of M points, and with what grid,
// block and LDS.  Two routes:
//   sort     predict_orderstat_kernel<nsort>: bitonic sort in LDS over nsort = the power of two
//            >= max(S, 64), one thread per pair up to 1024 threads and never fewer than 128 (thread
//            t < n_q writes a percentile, thread 64 + c counts interval c: 128 threads serve the
//            request limits n_q = n_cov = 64).
//   select   predict_select_kernel<vpt>: SEL_THREADS threads keep vpt draws each in registers
//            (vpt = ceil(S / SEL_THREADS) rounded up to 8, 12, .. 32), histogram them over SEL_BINS
//            bins and rank only the members of the requested bins (<= SEL_CAP each).  Taken for
//            2048 <= S <= 32 SEL_THREADS and at most PREDICT_SELECT_MAX_RANKS requested ranks
//            (2 n_q + 2 n_cov: every rank owns a list of SEL_CAP doubles in LDS).  Points it cannot
//            resolve are handed to the sort kernel, which then runs second over that list with
//            fewer workgroups.
// Both kernels walk the points with a stride of their grid.  Refused (ok = false): S outside
// 1 .. PREDICT_MAX_DRAWS (the sort holds a point's draws in LDS), n_q or n_cov outside
// 0 .. PREDICT_MAX_Q / PREDICT_MAX_COV, no points.  `launch` is false when nothing is asked.
#ifndef BMC_SEL_BINS
#define BMC_SEL_BINS 4096
#endif
constexpr int SEL_BINS = BMC_SEL_BINS, SEL_CAP = 64, SEL_THREADS = 512;
constexpr int PREDICT_MAX_DRAWS = 16384;          // 128 KiB of doubles in LDS; 32 draws x SEL_THREADS
constexpr int PREDICT_MAX_Q = 64, PREDICT_MAX_COV = 64;
constexpr int PREDICT_SELECT_MIN_DRAWS = 2048;
constexpr int PREDICT_SELECT_MAX_VPT = 32;
constexpr int PREDICT_SELECT_MAX_RANKS = 128;
constexpr int64_t PREDICT_MAX_BLOCKS = 2048;      // workgroups of the first (or only) pass
constexpr int64_t PREDICT_FALLBACK_BLOCKS = 256;  // workgroups of the sort behind the selection

struct PredictOrderstatPlan {
    bool ok, launch, select;
    int vpt;                              // draws per thread of the selection (8 .. 32), or 0
    int nsort, sort_threads;              // the sort: primary, or second pass behind the selection
    int64_t blocks_select, blocks_sort;   // workgroups (blocks_select = 0 without the selection)
    size_t lds_select, lds_sort;          // dynamic LDS, bytes
};

inline PredictOrderstatPlan plan_predict_orderstat(int32_t S, int32_t n_q, int32_t n_cov, int64_t M,
                                                   bool have_fail_list = true) {
    PredictOrderstatPlan p{};
    p.ok = S >= 1 && S <= PREDICT_MAX_DRAWS && n_q >= 0 && n_q <= PREDICT_MAX_Q && n_cov >= 0 &&
           n_cov <= PREDICT_MAX_COV && M >= 1;
    if (!p.ok) return p;
    p.launch = n_q > 0 || n_cov > 0;
    p.nsort = 64;
    while (p.nsort < S) p.nsort <<= 1;
    p.sort_threads = p.nsort / 2 < 1024 ? (p.nsort / 2 < 128 ? 128 : p.nsort / 2) : 1024;
    p.lds_sort = (size_t)p.nsort * sizeof(double);
    // selection when there are many draws and few requested ranks, otherwise the sort
    const int n_t = 2 * n_q + 2 * n_cov;
    p.select = S >= PREDICT_SELECT_MIN_DRAWS && S <= PREDICT_SELECT_MAX_VPT * SEL_THREADS &&
               n_t <= PREDICT_SELECT_MAX_RANKS && have_fail_list;
    int64_t blocks = M < PREDICT_MAX_BLOCKS ? M : PREDICT_MAX_BLOCKS;
    if (blocks < 1) blocks = 1;
    p.blocks_sort = blocks;
    if (p.select) {
        // hist + slot | min / max per wave | wave totals + flag | prefix per thread | cnt, tbin, tk,
        // trank per rank | alignment | one list per rank
        p.lds_select = (size_t)SEL_BINS * 8 + 16 * 8 + 16 * 4 + SEL_THREADS * 4 + (size_t)n_t * 16 + 16 +
                       (size_t)n_t * SEL_CAP * 8;
        // draws per thread in steps of 4 (10 000 draws: 20, not 24 -- the slots past the row
        // cost every per-draw step of the kernel)
        const int vpt = (S + SEL_THREADS - 1) / SEL_THREADS;
        p.vpt = vpt <= 8 ? 8 : (vpt + 3) / 4 * 4;
        p.blocks_select = blocks;
        p.blocks_sort = blocks < PREDICT_FALLBACK_BLOCKS ? blocks : PREDICT_FALLBACK_BLOCKS;
    }
    return p;
}

}  // namespace bmc
