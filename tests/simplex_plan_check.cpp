// CPU check of plan_simplex_launches (pybmc_amd/csrc/bmc_plan.h): how the chains of one
// bmc_simplex_run_chains call are split over launches of the simplex loop kernels.
//   plan <n> <k> <f32> <n_models> <chains> <cu_limit> <G> <W> <res> <ppw>
//          the geometry, the kernel and the launches as "c0+chains/nslot/resident;..."
//   sweep  a grid of shapes x model counts x chain counts x cu_limit x tuning: every chain is in
//          exactly one launch, in order; geometry and kernel are the one-chain plan's, which is what
//          bmc_simplex_run computed before there were chains (choose_geometry for one chain); no
//          launch keeps more workgroups resident than the CUs allow; one chain is one launch on
//          the one-chain grid.  Prints "sweep <plans> <failures>" last.
#include "../pybmc_amd/csrc/bmc_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace bmc;

static Shape shape_of(int64_t n, int k, int f32) {
    const int vec = choose_vec(n, k, f32);
    return Shape{n, k, f32, vec, (int)((n + 64 * vec - 1) / (64 * vec))};
}

static bmc_tuning tuning(int groups, int waves, int residency, int ppw, int cu_limit) {
    bmc_tuning t;
    std::memset(&t, 0, sizeof t);
    t.groups_per_chain = groups;
    t.waves_per_group = waves;
    t.residency = residency;
    t.panels_per_wave = ppw;
    t.cu_limit = cu_limit;
    return t;
}

static bool same_geometry(const Geometry& a, const Geometry& b) {
    return a.chains_per_launch == b.chains_per_launch && a.G == b.G && a.waves == b.waves && a.ppg == b.ppg &&
           a.mode == b.mode && a.ppw == b.ppw && a.nslot == b.nslot && a.one_wave == b.one_wave;
}

static int check(const Shape& s, const bmc_tuning& tu, const Chip& chip, int km, int C) {
    const SimplexPlan p = plan_simplex_launches(s, tu, chip, km, C);
    const Geometry one = choose_geometry(s, tu, chip, 1, km <= 64, 4);   // what one chain gets
    int bad = 0;
    bad += !same_geometry(p.geo, one);
    bad += !(simplex_kernel_key(s, p.geo) == simplex_kernel_key(s, one));
    bad += !kernel_compiled(simplex_kernel_key(s, p.geo));
    // every chain exactly once, in order
    int next = 0, most = 0;
    for (const SimplexLaunch& l : p.launches) {
        bad += l.c0 != next || l.n_chains < 1;
        next = l.c0 + l.n_chains;
        if (l.n_chains > most) most = l.n_chains;
        bad += l.resident != l.n_chains * p.geo.G;
        if (p.geo.one_wave) {
            bad += l.n_chains > 2048;
        } else {
            // co-residency: one workgroup per CU; and what launch_simplex checks
            bad += l.resident > chip.groups_max;
            bad += l.n_chains > l.nslot || !geometry_ok(s.k, p.geo.G, p.geo.waves, l.nslot);
            // the XCD labelling where one chain has it: one chain per XCD, slot c = chain c
            if (one.nslot == chip.xcds && chip.xcds > 1) bad += l.nslot != chip.xcds;
        }
    }
    bad += next != C || most != p.max_per_launch;
    // no launch is split off while the previous one has room
    for (size_t i = 0; i + 1 < p.launches.size(); ++i) bad += p.launches[i].n_chains != p.max_per_launch;
    if (C == 1) bad += p.launches.size() != 1 || (!p.geo.one_wave && p.launches[0].nslot != one.nslot);
    if (bad)
        std::printf("FAIL n=%lld k=%d f32=%d km=%d chains=%d cu=%d G=%d W=%d res=%d ppw=%d\n", (long long)s.n, s.k,
                    s.f32, km, C, tu.cu_limit, tu.groups_per_chain, tu.waves_per_group, tu.residency,
                    tu.panels_per_wave);
    return bad != 0;
}

int main(int argc, char** argv) {
    if (argc == 12 && !std::strcmp(argv[1], "plan")) {
        int v[10];
        for (int i = 0; i < 10; ++i) v[i] = std::atoi(argv[2 + i]);
        const Shape s = shape_of(std::atoll(argv[2]), v[1], v[2]);
        const bmc_tuning tu = tuning(v[6], v[7], v[8], v[9], v[5]);
        const SimplexPlan p = plan_simplex_launches(s, tu, chip_of(256, v[5]), v[3], v[4]);
        std::printf("G=%d waves=%d mode=%d ppw=%d one_wave=%d max_per_launch=%d | %s | ", p.geo.G, p.geo.waves,
                    p.geo.mode, p.geo.ppw, p.geo.one_wave, p.max_per_launch,
                    kernel_name(simplex_kernel_key(s, p.geo)).c_str());
        for (size_t i = 0; i < p.launches.size(); ++i)
            std::printf("%s%d+%d/%d/%d", i ? ";" : "", p.launches[i].c0, p.launches[i].n_chains,
                        p.launches[i].nslot, p.launches[i].resident);
        std::printf("\n");
        return 0;
    }
    if (argc == 2 && !std::strcmp(argv[1], "sweep")) {
        const int64_t ns[] = {3, 64, 150, 629, 1024, 2500, 4000, 10000, 30000, 100000, 400000, 2000000};
        const int ks[] = {1, 3, 8, 32, 64, 100, 256};
        const int kms[] = {4, 64, 65, 300};
        const int chains[] = {1, 2, 5, 7, 8, 9, 16, 64, 255, 256, 257, 2048, 2049, 5000};
        const int cus[] = {0, 1, 7, 8, 32, 63, 64, 100, 128, 256, 304};
        const int knobs[][4] = {{0, 0, 0, 0}, {1, 0, 0, 0}, {1, 1, 0, 0}, {1, 3, 1, 1}, {1, 8, 0, 0}, {2, 2, 2, 0},
                                {3, 1, 1, 1}, {4, 4, 0, 0}, {8, 0, 0, 0}, {32, 0, 0, 0}, {40, 0, 0, 0},
                                {1, 4, 3, 0}, {0, 0, 3, 0}, {0, 0, 2, 0}, {0, 0, 1, 2}};
        long plans = 0, fails = 0;
        for (int64_t n : ns)
            for (int k : ks)
                for (int f32 : {0, 1}) {
                    const Shape s = shape_of(n, k, f32);
                    for (const auto& kn : knobs)
                        for (int cu : cus) {
                            const bmc_tuning tu = tuning(kn[0], kn[1], kn[2], kn[3], cu);
                            const Chip chip = chip_of(256, cu);
                            if (tu.groups_per_chain > chip.groups_max) continue;   // the run: BMC_EINVAL
                            for (int km : kms) {
                                const Geometry one = choose_geometry(s, tu, chip, 1, km <= 64, 4);
                                // (a geometry the chip cannot hold or no kernel serves is refused by
                                // the run itself, for one chain as for many)
                                if (one.G > chip.groups_max || !kernel_compiled(simplex_kernel_key(s, one)))
                                    continue;
                                for (int C : chains) {
                                    ++plans;
                                    fails += check(s, tu, chip, km, C);
                                }
                            }
                        }
                }
        std::printf("sweep %ld %ld\n", plans, fails);
        return fails != 0;
    }
    std::fprintf(stderr, "usage: simplex_plan_check plan <n> <k> <f32> <km> <chains> <cu> <G> <W> <res> <ppw> | sweep\n");
    return 2;
}
