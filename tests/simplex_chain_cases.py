"""Replay cases of the simplex chain tests (test_simplex_chains_gpu.py on the GPU; the seed lists are
checked on the CPU by test_simplex_plan.py).  Problems and streams are census_common's.

One call has one step size, so a case takes the step size census_common.simplex_case finds for its
problem, and its chains replay the streams of the first N_CHAINS stream seeds that, at that step
size, satisfy simplex_case's rule: acceptances over burn + T strictly between 1/8 and 7/8 of it,
smallest accept/reject margin at least census_common.MARGIN.  The lists below are what that search
gives; the tests recompute the search and assert every chain's margin and acceptance."""
import census_common as cc

N_CHAINS = 5

# (n, k, f32, one-wave form) -> tuning (groups, waves, residency, panels per wave, agent scope,
# cu_limit), stream seeds of the chains
CASES = {
    "one_wave_629x3": dict(problem=(629, 3, 0, 1), tuning=(0, 0, 0, 0, 0, 0), seeds=[1, 2, 3, 4, 5]),
    "four_waves_2500x3": dict(problem=(2500, 3, 0, 1), tuning=(0, 0, 0, 0, 0, 0), seeds=[1, 2, 3, 5, 6]),
    "workgroup_single_300x4": dict(problem=(300, 4, 0, 0), tuning=(0, 0, 0, 0, 0, 0), seeds=[1, 2, 3, 4, 5]),
    "workgroup_3_groups_300x4": dict(problem=(300, 4, 0, 0), tuning=(3, 2, 1, 1, 0, 6), seeds=[1, 2, 3, 4, 5]),
}


def chains_of(case):
    """The case's data, step size and per-chain dicts (seed, streams, oracle chain, counts, margin),
    chosen by the rule above -- independent of the pinned list, which the caller compares."""
    n, k, f32, ow = case["problem"]
    base = cc.simplex_case(n, k, f32, ow)
    tt = cc.BURN_SIMPLEX + cc.T_SIMPLEX
    chains = []
    for seed in range(1, 60):
        Z, U, G = cc.simplex_streams(n, k, seed, tt)
        chain, acc, used, acc_all, margin = cc.simplex_chain(base["y"], base["X"], base["Vt_hat"], base["S_hat"],
                                                             base["stepsize"], Z, U, G)
        if tt / 8 < acc_all < 7 * tt / 8 and margin >= cc.MARGIN:
            chains.append(dict(seed=seed, Z=Z, U=U, G=G, chain=chain, acc=acc, used=used, acc_all=acc_all,
                               margin=margin))
        if len(chains) == N_CHAINS:
            return base, chains
    raise AssertionError("fewer than %d stream seeds follow the rule" % N_CHAINS)
