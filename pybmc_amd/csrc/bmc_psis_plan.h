// Host-only: the tail of Pareto-smoothed importance sampling (Vehtari et al. 2024), one rule for
// every caller (plan_loo, plan_loo_predict, plan_sens).  No HIP types: the plan checks under tests/
// compile it with g++.  The fit itself is bmc_psis.h.
#pragma once
#include <cstdint>

namespace bmc {

constexpr int PSIS_MIN_TAIL = 5;   // no fit on a shorter tail

// M = min(floor(S / 5), ceil(3 sqrt(S))), in integers
inline int64_t psis_tail_length(int64_t S) {
    if (S < 1) return 0;
    int64_t t = 0;   // ceil(sqrt(9 S)): the smallest t with t^2 >= 9 S
    for (int64_t bit = (int64_t)1 << 31; bit > 0; bit >>= 1)
        if ((t + bit - 1) * (t + bit - 1) < 9 * S) t += bit;
    return S / 5 < t ? S / 5 : t;
}

// grid points of the generalised Pareto fit on a tail of M: 30 + floor(sqrt(M))
inline int32_t psis_grid_points(int64_t M) {
    int64_t rt = 0;
    while ((rt + 1) * (rt + 1) <= M) ++rt;
    return (int32_t)(30 + rt);
}

}  // namespace bmc
