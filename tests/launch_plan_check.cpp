// CPU check of pybmc_amd/csrc/bmc_plan.h, the launch planner of the Gibbs loop.
//   (no argument)  one line per named case: the shape, the geometry and every launch of the plan
//                  with the kernel it runs; tests/test_launch_plan.py compares them with the plans
//                  of the parent commit.
//   sweep          plans over a grid of shapes x chain counts x cu_limit x tunings; every plan
//                  must cover its chains once and in order, fit its exchange words, pass the
//                  argument checks of launch_gibbs and run compiled kernels only (the simplex
//                  sampler's geometries too).  Prints the compiled kernels no plan reaches, then
//                  "sweep <plans> <failures>" last.
//   names          the demangled names of every compiled loop kernel (kernels_gibbs.hip's table)
//   census         for every compiled loop kernel the cheapest recipe (smallest n * k * chains) of a
//                  grid of shapes x chain counts x cu_limit x tunings whose plan launches it, as
//                  "name | recipe", or "name | unreached"; tests/kernel_census.txt pins the output
//                  (regenerate: g++ -std=c++17 -O2 -o /tmp/lpc tests/launch_plan_check.cpp &&
//                  /tmp/lpc census > tests/kernel_census.txt)
//   replan FILE    re-plans every recipe of such a table: "name | the launches in order, joined by
//                  ;, each kernel@first chain+chains:chains per pass | the same had the device
//                  given the other pack answer"
//   setup N K F32 [N K F32 ...]
//                  per triple the launch class of the set-up kernels (kernels_setup.hip) for an
//                  (N x K) problem of that storage type: rows per lane (choose_vec), panels, rows
//                  of the last panel; residual_rss: workgroups, flat or two-level ticket, the most
//                  panels one wave slot walks; rotate to K output columns: column groups per
//                  panel and the columns of the last wave (tests/test_setup_plan.py)
#include "../pybmc_amd/csrc/bmc_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <set>
#include <array>
#include <iterator>
#include <string>
#include <unordered_map>
#include <vector>

using namespace bmc;

struct Case {
    const char* name;
    int64_t n;
    int k, f32, n_chains, cu_limit;
    int groups, waves, residency, ppw, cpp;   // bmc_tuning fields (0: automatic)
    int pack_ok;                              // what the device queries of run_common answer
};

static const Case CASES[] = {
    // name                 n       k   f32 chains cu  G   W  res ppw cpp pack
    {"ref629x3",            629,    3,  0,  1,     0,  0,  0, 0,  0,  0,  0},
    {"ref629x3_256ch",      629,    3,  0,  256,   0,  0,  0, 0,  0,  0,  0},
    {"ref629x3_f32",        629,    3,  1,  1,     0,  0,  0, 0,  0,  0,  0},
    {"n2500x8_4waves",      2500,   8,  0,  1,     0,  0,  0, 0,  0,  0,  0},
    {"n2500x8_256ch",       2500,   8,  0,  256,   0,  0,  0, 0,  0,  0,  0},
    {"n8000x4_8waves",      8000,   4,  0,  1,     0,  0,  0, 0,  0,  0,  0},
    {"golden64x8",          64,     8,  0,  1,     0,  0,  0, 0,  0,  0,  0},
    {"golden3x2",           3,      2,  0,  1,     0,  0,  0, 0,  0,  0,  0},
    {"c2_1",                10000,  32, 0,  1,     0,  0,  0, 0,  0,  0,  0},
    {"c2_1_pack",           10000,  32, 0,  1,     0,  0,  0, 0,  0,  0,  1},
    {"c2_8",                10000,  32, 0,  8,     0,  0,  0, 0,  0,  0,  0},
    {"c2_8_pack",           10000,  32, 0,  8,     0,  0,  0, 0,  0,  0,  1},
    {"c2_9",                10000,  32, 0,  9,     0,  0,  0, 0,  0,  0,  0},
    {"c2_9_pack",           10000,  32, 0,  9,     0,  0,  0, 0,  0,  0,  1},
    {"c2_15",               10000,  32, 0,  15,    0,  0,  0, 0,  0,  0,  0},
    {"c2_15_pack",          10000,  32, 0,  15,    0,  0,  0, 0,  0,  0,  1},
    {"c2_16",               10000,  32, 0,  16,    0,  0,  0, 0,  0,  0,  0},
    {"c2_16_pack",          10000,  32, 0,  16,    0,  0,  0, 0,  0,  0,  1},
    {"c2_32",               10000,  32, 0,  32,    0,  0,  0, 0,  0,  0,  0},
    {"c2_32_pack",          10000,  32, 0,  32,    0,  0,  0, 0,  0,  0,  1},
    {"c2_40",               10000,  32, 0,  40,    0,  0,  0, 0,  0,  0,  0},
    {"c2_40_pack",          10000,  32, 0,  40,    0,  0,  0, 0,  0,  0,  1},
    {"c2_63",               10000,  32, 0,  63,    0,  0,  0, 0,  0,  0,  0},
    {"c2_63_pack",          10000,  32, 0,  63,    0,  0,  0, 0,  0,  0,  1},
    {"c2_64",               10000,  32, 0,  64,    0,  0,  0, 0,  0,  0,  0},
    {"c2_64_pack",          10000,  32, 0,  64,    0,  0,  0, 0,  0,  0,  1},
    {"c2_130_pack",         10000,  32, 0,  130,   0,  0,  0, 0,  0,  0,  1},
    {"c2_cu128_1",          10000,  32, 0,  1,     128, 0, 0, 0,  0,  0,  0},
    {"c2_cu128_16_pack",    10000,  32, 0,  16,    128, 0, 0, 0,  0,  0,  1},
    {"c2_cu32_1",           10000,  32, 0,  1,     32, 0,  0, 0,  0,  0,  0},
    {"c2_cu32_8",           10000,  32, 0,  8,     32, 0,  0, 0,  0,  0,  0},
    {"c4_1",                200000, 64, 1,  1,     0,  0,  0, 0,  0,  0,  0},
    {"c4_8",                200000, 64, 1,  8,     0,  0,  0, 0,  0,  0,  0},
    {"c5_1",                50000,  256, 0, 1,     0,  0,  0, 0,  0,  0,  0},
    {"c5_8",                50000,  256, 0, 8,     0,  0,  0, 0,  0,  0,  0},
    {"hbm410mb_1",          400000, 256, 1, 1,     0,  0,  0, 0,  0,  0,  0},
    // the tuning knobs the GPU tests set
    {"ref629x4_w1",         629,    4,  0,  2,     0,  0,  1, 0,  0,  0,  0},
    {"ref629x4_g10_w1",     629,    4,  0,  2,     0,  10, 1, 0,  0,  0,  0},
    {"n1000x4_g1_w4",       1000,   4,  0,  2,     0,  1,  4, 0,  0,  0,  0},
    {"n8000x4_w8",          8000,   4,  0,  2,     0,  0,  8, 0,  0,  0,  0},
    {"n3000x8_res3_8ch",    3000,   8,  0,  8,     0,  0,  0, 3,  0,  0,  0},
    {"n3000x8_res3_cpp1",   3000,   8,  0,  8,     0,  0,  0, 3,  0,  1,  0},
    {"n3000x8_res2_5ch",    3000,   8,  0,  5,     0,  0,  0, 2,  0,  0,  0},
    {"n700x130_res3_3ch",   700,    130, 0, 3,     0,  0,  0, 3,  0,  0,  0},
    {"n3000x8_g3_w2_res2",  3000,   8,  0,  2,     0,  3,  2, 2,  0,  0,  0},
    {"c2_19_cpp2_pack",     10000,  32, 0,  19,    0,  0,  0, 0,  0,  2,  1},
    {"c2_40_cpp4_pack",     10000,  32, 0,  40,    0,  0,  0, 0,  0,  4,  1},
    {"c2_64_cpp1_pack",     10000,  32, 0,  64,    0,  0,  0, 0,  0,  1,  1},
    {"c2_64_ppw1",          10000,  32, 0,  64,    0,  0,  0, 0,  1,  0,  0},
    {"n9000x16f32_64ch",    9000,   16, 1,  64,    0,  0,  0, 0,  0,  0,  0},
    {"n9000x16f32_64ch_ppw1", 9000, 16, 1,  64,    0,  0,  0, 0,  1,  0,  0},
    {"c2_res3_8ch",         10000,  32, 0,  8,     0,  0,  0, 3,  0,  0,  0},
    {"n100000x32_4ch",      100000, 32, 0,  4,     0,  0,  0, 0,  0,  0,  0},
};

static Shape shape_of(int64_t n, int k, int f32) {
    const int vec = choose_vec(n, k, f32);
    return Shape{n, k, f32, vec, (int)((n + 64 * vec - 1) / (64 * vec))};
}

static bmc_tuning tuning(int groups, int waves, int residency, int ppw, int cpp, int cu_limit) {
    bmc_tuning t;
    std::memset(&t, 0, sizeof t);
    t.groups_per_chain = groups;
    t.waves_per_group = waves;
    t.residency = residency;
    t.panels_per_wave = ppw;
    t.chains_per_pass = cpp;
    t.cu_limit = cu_limit;
    return t;
}

static void print_case(const Case& c) {
    const Shape s = shape_of(c.n, c.k, c.f32);
    const bmc_tuning tu = tuning(c.groups, c.waves, c.residency, c.ppw, c.cpp, c.cu_limit);
    const Chip chip = chip_of(256, c.cu_limit);
    const Geometry g = choose_geometry(s, tu, chip, c.n_chains, true, 8);
    const GibbsPlan p = plan_gibbs(g, s, tu, chip, c.n_chains, c.pack_ok != 0);
    std::printf("%s: vec=%d np=%d | G=%d waves=%d ppg=%d mode=%d ppw=%d nslot=%d cpl=%d one_wave=%d | "
                "max=%d passes=%lld cpp=%d wpg=%d |",
                c.name, s.vec, s.npanels, g.G, g.waves, g.ppg, g.mode, g.ppw, g.nslot, g.chains_per_launch,
                g.one_wave, p.max_per_launch, (long long)p.passes, p.chains_per_pass, p.waves_per_group);
    // c0+chains cpp/waves/nslot/pack/bundle_slots/bundle_bal/resident=kernel
    for (const GibbsLaunch& l : p.launches)
        std::printf(" %d+%d:%d/%d/%d/%d/%d/%d/%d=%s", l.c0, l.n_chains, l.chains_per_pass, l.waves, l.nslot, l.pack,
                    l.bundle_slots, l.bundle_bal, l.resident, kernel_name(gibbs_kernel_key(s, g, l)).c_str());
    std::printf("\n");
}

static long failures = 0;
static void fail(const char* what, const Shape& s, const bmc_tuning& tu, int n_chains, bool pack) {
    if (++failures <= 20)
        std::printf("FAIL %s: n=%lld k=%d f32=%d chains=%d cu_limit=%d G=%d W=%d res=%d ppw=%d cpp=%d pack=%d\n",
                    what, (long long)s.n, s.k, s.f32, n_chains, tu.cu_limit, tu.groups_per_chain,
                    tu.waves_per_group, tu.residency, tu.panels_per_wave, tu.chains_per_pass, (int)pack);
}

static std::set<std::string> reached;
static bool compiled(const KernelKey& k) {
    if (!kernel_compiled(k)) return false;
    static KernelKey last;   // (consecutive plans mostly share their kernel)
    if (!(k == last)) reached.insert(kernel_name(last = k));
    return true;
}

static long sweep() {
    const int64_t ns[] = {1, 3, 64, 100, 629, 1000, 2500, 4000, 8000, 10000, 16000, 30000, 65000,
                          100000, 200000, 400000, 1000000};
    const int ks[] = {1, 3, 4, 8, 12, 16, 24, 32, 48, 64, 65, 128, 256};
    const int cu_limits[] = {0, 128, 64, 32, 16};
    const int chains[] = {1, 2, 3, 4, 5, 7, 8, 9, 12, 15, 16, 17, 19, 24, 31, 32, 33, 37, 40, 45, 48,
                          63, 64, 65, 100, 130, 256, 300, 2048, 3000};
    const int knobs[][5] = {{0, 0, 0, 0, 0}, {0, 1, 0, 0, 0}, {0, 2, 0, 0, 0}, {0, 4, 0, 0, 0}, {0, 8, 0, 0, 0},
                            {1, 0, 0, 0, 0}, {10, 0, 0, 0, 0}, {32, 0, 0, 0, 0}, {10, 1, 0, 0, 0},
                            {1, 4, 0, 0, 0}, {3, 2, 2, 0, 0}, {0, 0, 1, 0, 0}, {0, 0, 2, 0, 0},
                            {0, 0, 3, 0, 0}, {0, 0, 3, 0, 1}, {0, 0, 1, 0, 1}, {0, 0, 0, 0, 1},
                            {0, 0, 0, 0, 2}, {0, 0, 0, 0, 4}, {0, 0, 0, 0, 8}, {0, 0, 0, 1, 0},
                            {0, 0, 0, 2, 0}, {0, 0, 0, 4, 0}};
    long plans = 0;
    for (int64_t n : ns)
        for (int k : ks)
            for (int f32 : {0, 1}) {
                const Shape s = shape_of(n, k, f32);
                for (const auto& kn : knobs)
                    for (int cl : cu_limits) {
                        const bmc_tuning tu = tuning(kn[0], kn[1], kn[2], kn[3], kn[4], cl);
                        const Chip chip = chip_of(256, cl);
                        if (tu.groups_per_chain > chip.groups_max) continue;   // run_common: BMC_EINVAL
                        for (bool one_wave_ok : {false, true}) {   // the simplex sampler (Km > 64, Km <= 64)
                            const Geometry g = choose_geometry(s, tu, chip, 1, one_wave_ok, 4);
                            if (!g.one_wave && !geometry_ok(s.k, g.G, g.waves, g.nslot))
                                fail("launch_simplex argument checks", s, tu, 1, false);
                            if (!compiled(simplex_kernel_key(s, g))) fail("simplex kernel not compiled", s, tu, 1, false);
                        }
                        for (int nc : chains) {
                            const Geometry g = choose_geometry(s, tu, chip, nc, true, 8);
                            for (bool flag : {false, true}) {
                                // the device queries answer yes only for a shape the packed kernel exists for
                                const bool pack_ok = flag && gibbs_packable(s.k, s.f32, s.vec, g.ppw);
                                const GibbsPlan p = plan_gibbs(g, s, tu, chip, nc, pack_ok);
                                ++plans;
                                int next = 0;
                                for (const GibbsLaunch& l : p.launches) {
                                    if (l.c0 != next || l.n_chains < 1) fail("chains not covered in order", s, tu, nc, pack_ok);
                                    next = l.c0 + l.n_chains;
                                    if (l.n_chains > p.max_per_launch) fail("exceeds max_per_launch", s, tu, nc, pack_ok);
                                    if (l.chains_per_pass > p.chains_per_pass || l.waves > p.waves_per_group)
                                        fail("summary", s, tu, nc, pack_ok);
                                    if (!compiled(gibbs_kernel_key(s, g, l)))
                                        fail("kernel not compiled", s, tu, nc, pack_ok);
                                    if (l.pack && !gibbs_kernel_key(s, g, l).pack)
                                        fail("packed variant", s, tu, nc, pack_ok);
                                    if (g.one_wave) {
                                        if (l.chains_per_pass != 1 || l.n_chains > l.nslot || l.nslot > 2048)
                                            fail("one-wave launch size", s, tu, nc, pack_ok);
                                        continue;
                                    }
                                    if (!geometry_ok(s.k, g.G, l.waves, l.nslot) ||
                                        !gibbs_chains_ok(l.n_chains, l.chains_per_pass, l.waves, l.nslot,
                                                         l.bundle_slots, g.G, g.mode))
                                        fail("launch_gibbs argument checks", s, tu, nc, pack_ok);
                                    if ((g.G > 1 || l.chains_per_pass > 1) &&
                                        l.resident > chip.groups_max * (l.pack ? 2 : 1))
                                        fail("co-resident workgroups", s, tu, nc, pack_ok);
                                }
                                if (next != nc) fail("chains not all covered", s, tu, nc, pack_ok);
                            }
                        }
                    }
            }
    return plans;
}

// ---- census: the cheapest recipe that launches each compiled kernel ---------------------------
// A recipe is a problem the samplers accept and the parity tests can perturb: k >= 2 (one column
// cannot show a column mix-up, nor lose a column), n >= 2 k + 2 (X'X stays regular with the last
// row dropped); the simplex sampler needs k < n_models, and its
// one-wave kernels n_models <= 64 (ow = 1), so k <= 62 there.  Recipes assume a 256-CU device.
struct Recipe {
    int sampler = 0;   // 0 Gibbs, 1 simplex
    int64_t n = 0;
    int k = 0, f32 = 0, chains = 0, cu = 0, G = 0, W = 0, res = 0, ppw = 0, cpp = 0, pack = 0, ow = 0;
    double cost() const { return (double)n * k * chains; }
};

static std::vector<std::string> plan_recipe(const Recipe& r, bool pack_answer) {
    const Shape s = shape_of(r.n, r.k, r.f32);
    const bmc_tuning tu = tuning(r.G, r.W, r.res, r.ppw, r.cpp, r.cu);
    const Chip chip = chip_of(256, r.cu);
    std::vector<std::string> out;
    if (r.sampler == 1) {
        const Geometry g = choose_geometry(s, tu, chip, 1, r.ow != 0, 4);
        out.push_back(kernel_name(simplex_kernel_key(s, g)) + "@0+1:1");
        return out;
    }
    const Geometry g = choose_geometry(s, tu, chip, r.chains, true, 8);
    const bool pack_ok = pack_answer && gibbs_packable(s.k, s.f32, s.vec, g.ppw);
    for (const GibbsLaunch& l : plan_gibbs(g, s, tu, chip, r.chains, pack_ok).launches)
        out.push_back(kernel_name(gibbs_kernel_key(s, g, l)) + "@" + std::to_string(l.c0) + "+" +
                      std::to_string(l.n_chains) + ":" + std::to_string(l.chains_per_pass));
    return out;
}

static void print_recipe(const Recipe& r) {
    std::printf("%s n=%lld k=%d f32=%d chains=%d cu=%d G=%d W=%d res=%d ppw=%d cpp=%d pack=%d ow=%d",
                r.sampler ? "simplex" : "gibbs", (long long)r.n, r.k, r.f32, r.chains, r.cu, r.G, r.W, r.res,
                r.ppw, r.cpp, r.pack, r.ow);
}

static void census(const KernelKeys& keys) {
    // the sweep's grid, the multiples of 64 also one row short (a ragged last panel costs less and
    // wins), small n for the one-wave shapes (2 / 4 / 8 panels per wave in 1, 2, 4 or 8 waves), the
    // rows-per-lane boundaries of choose_vec, k in every kmax bracket
    const int64_t ns[] = {1, 3, 63, 64, 100, 127, 200, 255, 300, 400, 511, 629, 767, 1000, 1023, 1500, 2047,
                          2500, 3000, 3999, 4000, 5000, 6000, 7999, 8000, 10000, 12000, 15999, 16000, 20000,
                          30000, 40000, 65000, 100000, 131071, 131137, 140000, 199999, 200000, 262143, 262209,
                          300000, 399999, 400000, 600000, 999999, 1000000};
    const int ks[] = {1, 2, 3, 4, 5, 8, 9, 12, 16, 17, 24, 32, 33, 48, 64, 65, 128, 256};
    const int cu_limits[] = {0, 128, 64, 32, 16};
    const int chains[] = {1, 2, 3, 4, 5, 7, 8, 9, 12, 15, 16, 17, 19, 24, 31, 32, 33, 37, 40, 45, 48,
                          63, 64, 65, 100, 130, 256, 300, 2048, 3000};
    std::vector<std::array<int, 5>> knobs = {
        {0, 0, 0, 0, 0}, {0, 1, 0, 0, 0}, {0, 2, 0, 0, 0}, {0, 4, 0, 0, 0}, {0, 8, 0, 0, 0}, {1, 0, 0, 0, 0},
        {10, 0, 0, 0, 0}, {32, 0, 0, 0, 0}, {10, 1, 0, 0, 0}, {1, 4, 0, 0, 0}, {3, 2, 2, 0, 0}, {0, 0, 1, 0, 0},
        {0, 0, 2, 0, 0}, {0, 0, 3, 0, 0}, {0, 0, 3, 0, 1}, {0, 0, 1, 0, 1}, {0, 0, 0, 0, 1}, {0, 0, 0, 0, 2},
        {0, 0, 0, 0, 4}, {0, 0, 0, 0, 8}, {0, 0, 0, 1, 0}, {0, 0, 0, 2, 0}, {0, 0, 0, 4, 0}};
    // and what the sweep's 23 tunings leave out: groups x waves x residency x panels per wave x
    // chains per pass in combination
    for (int G : {0, 1, 3, 40, 200})
        for (int W : {0, 2, 8})
            for (int res : {0, 1, 2, 3})
                for (int ppw : {0, 1, 2, 4})
                    for (int cpp : {0, 2, 4}) knobs.push_back({G, W, res, ppw, cpp});
    const size_t n_sweep_knobs = 23;   // (the tunings added above run with the chain counts below only)
    const int few_chains[] = {1, 2, 4, 8, 9};
    std::vector<Recipe> best(keys.n);
    std::unordered_map<uint64_t, int> index;
    auto packed = [](const KernelKey& k) {
        return (uint64_t)k.family | (uint64_t)k.f32 << 3 | (uint64_t)k.vec << 4 | (uint64_t)k.mode << 7 |
               (uint64_t)k.kmax << 9 | (uint64_t)k.ppw << 17 | (uint64_t)k.cpp << 20 | (uint64_t)k.rmax << 24 |
               (uint64_t)k.nw << 29 | (uint64_t)k.single << 33 | (uint64_t)k.pack << 34 | (uint64_t)k.smallg << 35 |
               (uint64_t)k.slotted << 36 | (uint64_t)k.bal << 37;
    };
    for (int i = 0; i < keys.n; ++i) index[packed(keys.key[i])] = i;
    auto offer = [&](const KernelKey& key, const Recipe& r) {
        const auto it = index.find(packed(key));
        if (it == index.end()) return;
        Recipe& b = best[it->second];
        if (b.chains == 0 || r.cost() < b.cost()) b = r;
    };
    for (int64_t n : ns)
        for (int k : ks) {
            if (k < 2 || n < 2 * k + 2) continue;
            for (int f32 : {0, 1}) {
                const Shape s = shape_of(n, k, f32);
                for (size_t ki = 0; ki < knobs.size(); ++ki)
                    for (int cl : cu_limits) {
                        const auto& kn = knobs[ki];
                        const bmc_tuning tu = tuning(kn[0], kn[1], kn[2], kn[3], kn[4], cl);
                        const Chip chip = chip_of(256, cl);
                        if (tu.groups_per_chain > chip.groups_max) continue;   // run_common: BMC_EINVAL
                        Recipe r;
                        r.n = n; r.k = k; r.f32 = f32; r.cu = cl;
                        r.G = kn[0]; r.W = kn[1]; r.res = kn[2]; r.ppw = kn[3]; r.cpp = kn[4];
                        if (kn[4] == 0)   // (the simplex sampler has no chains per pass)
                            for (int ow : {1, 0}) {
                                if (ow && k > 62) continue;
                                const Geometry g = choose_geometry(s, tu, chip, 1, ow != 0, 4);
                                if (!g.one_wave && !geometry_ok(s.k, g.G, g.waves, g.nslot)) continue;
                                r.sampler = 1; r.chains = 1; r.ow = ow; r.pack = 0;
                                offer(simplex_kernel_key(s, g), r);
                            }
                        r.sampler = 0; r.ow = 0;
                        const int* nc_begin = ki < n_sweep_knobs ? std::begin(chains) : std::begin(few_chains);
                        const int* nc_end = ki < n_sweep_knobs ? std::end(chains) : std::end(few_chains);
                        for (const int* pnc = nc_begin; pnc != nc_end; ++pnc) {
                            const int nc = *pnc;
                            const Geometry g = choose_geometry(s, tu, chip, nc, true, 8);
                            for (int flag : {0, 1}) {
                                const bool pack_ok = flag && gibbs_packable(s.k, s.f32, s.vec, g.ppw);
                                if (flag && !pack_ok) continue;   // (the same plan as without)
                                // where the packed variant exists and the plan asks the device, a
                                // recipe counts on its yes (128 VGPRs, two groups per CU)
                                if (!flag && gibbs_packable(s.k, s.f32, s.vec, g.ppw) &&
                                    gibbs_pack_candidate(g, chip, tu, nc))
                                    continue;
                                r.chains = nc; r.pack = flag;
                                for (const GibbsLaunch& l : plan_gibbs(g, s, tu, chip, nc, pack_ok).launches)
                                    offer(gibbs_kernel_key(s, g, l), r);
                            }
                        }
                    }
            }
        }
    for (int i = 0; i < keys.n; ++i) {
        std::printf("%s | ", kernel_name(keys.key[i]).c_str());
        if (best[i].chains == 0) std::printf("unreached");
        else print_recipe(best[i]);
        std::printf("\n");
    }
}

static int replan(const char* file) {
    std::ifstream in(file);
    if (!in) return 2;
    std::string line;
    while (std::getline(in, line)) {
        const size_t bar = line.find(" | ");
        if (bar == std::string::npos) continue;
        const std::string name = line.substr(0, bar), rec = line.substr(bar + 3);
        if (rec == "unreached") {
            std::printf("%s | unreached\n", name.c_str());
            continue;
        }
        Recipe r;
        char sampler[16];
        long long n;
        if (std::sscanf(rec.c_str(), "%15s n=%lld k=%d f32=%d chains=%d cu=%d G=%d W=%d res=%d ppw=%d cpp=%d pack=%d ow=%d",
                        sampler, &n, &r.k, &r.f32, &r.chains, &r.cu, &r.G, &r.W, &r.res, &r.ppw, &r.cpp, &r.pack,
                        &r.ow) != 13)
            return 3;
        r.n = n;
        r.sampler = std::strcmp(sampler, "simplex") == 0;
        std::printf("%s |", name.c_str());
        for (int other : {0, 1}) {
            const std::vector<std::string> ks = plan_recipe(r, other ? !r.pack : r.pack != 0);
            for (size_t i = 0; i < ks.size(); ++i) std::printf("%s%s", i ? ";" : " ", ks[i].c_str());
            std::printf(other ? "\n" : " |");
        }
    }
    return 0;
}

// ---- setup: the launch class of the set-up kernels for one (n, k, f32) ------------------------
static void setup_class(int64_t n, int k, int f32) {
    const Shape s = shape_of(n, k, f32);
    const int32_t G = rss_groups_of(s.npanels);
    std::printf("setup n=%lld k=%d f32=%d: vec=%d np=%d rows_per_panel=%d last_rows=%lld | rss G=%d ticket=%s "
                "trips=%d | rotate ncg=%u last_wave_cols=%d\n",
                (long long)n, k, f32, s.vec, s.npanels, 64 * s.vec,
                (long long)(n - (int64_t)(s.npanels - 1) * 64 * s.vec), G,
                (unsigned)G > RSS_FLAT_TICKET_MAX ? "two-level" : "flat", rss_trips_of(s.npanels),
                rotate_col_groups(k, 8), (k - 1) % 8 + 1);
}

int main(int argc, char** argv) {
    static constexpr KernelKeys keys = loop_kernel_keys();
    if (argc > 4 && (argc - 2) % 3 == 0 && std::strcmp(argv[1], "setup") == 0) {
        for (int a = 2; a + 2 < argc; a += 3)
            setup_class(std::atoll(argv[a]), std::atoi(argv[a + 1]), std::atoi(argv[a + 2]));
        return 0;
    }
    if (argc > 1 && std::strcmp(argv[1], "census") == 0) {
        census(keys);
        return 0;
    }
    if (argc > 2 && std::strcmp(argv[1], "replan") == 0) return replan(argv[2]);
    if (argc > 1 && std::strcmp(argv[1], "sweep") == 0) {
        const long plans = sweep();
        int unreached = 0;
        for (int i = 0; i < keys.n; ++i) unreached += reached.count(kernel_name(keys.key[i])) == 0;
        std::printf("compiled loop kernels %d, reached by no plan of the sweep %d\n", keys.n, unreached);
        std::printf("sweep %ld %ld\n", plans, failures);
        return failures != 0;
    }
    if (argc > 1 && std::strcmp(argv[1], "names") == 0) {
        for (int i = 0; i < keys.n; ++i) std::printf("%s\n", kernel_name(keys.key[i]).c_str());
        return 0;
    }
    for (const Case& c : CASES) print_case(c);
    return 0;
}
