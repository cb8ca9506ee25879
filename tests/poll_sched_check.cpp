// CPU check of the poll schedules of the granule gather (pybmc_amd/csrc/bmc_plan.h: PollSched,
// poll_issue_state): prints one line per schedule, "name depth first gap t0 t1 ...".
#include <cstdio>

#include "../pybmc_amd/csrc/bmc_plan.h"

static void show(const char* name, bmc::PollSched s) {
    std::printf("%s %d %d %d", name, s.depth, s.first, s.gap);
    for (int d = 0; d < s.depth; ++d) std::printf(" %d", bmc::poll_issue_state(s, d));
    std::printf("\n");
}

int main() {
    show("local", bmc::POLL_LOCAL);
    show("agent", bmc::POLL_AGENT);
    show("plain", bmc::POLL_PLAIN);
    show("level2", bmc::POLL_LEVEL2);
    return 0;
}
