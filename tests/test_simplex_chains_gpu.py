"""Several simplex chains per call on the GPU (-m gpu): bmc_simplex_run_chains and what is built on it.

The contract under test: chain c of a device-mode call is bit for bit the one-chain run with
seed = seeds[c], whatever its index, its launch or its neighbours; a replay-mode chain is the solo
replay of its three streams, within the project's replay bar 1e-9 * max(1, |ref|.max()) of the
oracle with equal acceptance and consumption counts."""
import os

import numpy as np
import pytest

import census_common as cc
import simplex_chain_cases as S
from conftest import load_golden
from gpu_common import gpu_ctx
from pybmc_amd import gibbs_sampler_simplex

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SEEDS = [11, (1 << 40) + 5, 3, (1 << 63) + 9, 77]      # distinct; two of them above 2^32
PRIOR = (1.0, 0.02)


def synth(n, k, km):
    """The problems of test_simplex_gpu.py's two- and four-wave test."""
    rng = np.random.default_rng(n + k)
    A = rng.standard_normal((n, km))
    truth = A @ np.full(km, 1.0 / km) + 0.05 * rng.standard_normal(n)
    Ac = A - A.mean(1, keepdims=True)
    U, Sv, Vt = np.linalg.svd(Ac, full_matrices=False)
    S_hat = Sv[:k]
    return truth - A.mean(1), U[:, :k], Vt[:k] / S_hat[:, None], S_hat


def golden150():
    g = load_golden("simplex_synth150x4")
    return g["y"], g["X"], g["Vt_hat"], g["S_hat"]


# name: (problem, tuning (groups, waves, residency, panels per wave, agent scope, cu_limit), step size,
#        expected (groups per chain, waves per group, launches for 5 chains))
SOLO_CASES = {
    "one_wave_golden150x4": (golden150, (0, 0, 0, 0, 0, 0), 0.002, (1, 1, 1)),
    "four_waves_2500x3": (lambda: synth(2500, 3, 4), (0, 0, 0, 0, 0, 0), 0.001, (1, 4, 1)),
    "two_waves_1024x8": (lambda: synth(1024, 8, 9), (0, 0, 0, 0, 0, 0), 0.001, (1, 2, 1)),
    "workgroup_single": (golden150, (1, 3, 1, 1, 0, 0), 0.002, (1, 3, 1)),
    "workgroup_single_2_cus": (golden150, (1, 3, 1, 1, 0, 2), 0.002, (1, 3, 3)),
    "workgroup_3_groups_xcd_slots": (golden150, (3, 1, 1, 1, 0, 0), 0.002, (3, 1, 1)),
    "workgroup_3_groups_6_cus": (golden150, (3, 1, 1, 1, 0, 6), 0.002, (3, 1, 3)),
    "workgroup_3_groups_agent_scope": (golden150, (3, 1, 1, 1, 1, 0), 0.002, (3, 1, 1)),
    "workgroup_3_groups_agent_scope_6_cus": (golden150, (3, 1, 1, 1, 1, 6), 0.002, (3, 1, 3)),
    "workgroup_2_groups_lds_4_cus": (golden150, (2, 2, 2, 0, 0, 4), 0.002, (2, 2, 3)),
}


def tune(ctx, t):
    ctx.set_tuning(groups_per_chain=t[0], waves_per_group=t[1], residency=t[2], panels_per_wave=t[3],
                   force_agent_scope=t[4], cu_limit=t[5])


def census_names():
    return {name for name, _ in cc.read_table()}


@pytest.mark.parametrize("name", list(SOLO_CASES))
def test_every_chain_is_its_solo_run(name):
    make, tuning, stepsize, (G, W, launches) = SOLO_CASES[name]
    y, X, Vt_hat, S_hat = make()
    ctx = gpu_ctx()
    ctx.set_problem(y, X)
    tune(ctx, tuning)
    burn, T = 100, 300          # kept rows are staged 64 at a time: T is not a multiple of 64
    args = (Vt_hat, S_hat)
    rest = (T, *PRIOR, burn, stepsize)
    try:
        def solo():
            return [ctx.simplex_run(*args, *rest, seed=s, return_stats=True) for s in SEEDS]
        before = solo()
        kernels_solo = ctx.last_kernels()
        out, acc, used, st = ctx.simplex_run_chains(*args, len(SEEDS), *rest, seeds=SEEDS, return_stats=True)
        kernels = ctx.last_kernels()
        after = solo()
    finally:
        ctx.set_tuning()
    assert out.shape == (len(SEEDS), T, X.shape[1] + 1) and np.isfinite(out).all()
    assert (st["groups_per_chain"], st["waves_per_group"], st["launches"]) == (G, W, launches), st
    assert st["n_chains"] == len(SEEDS) and st["passes"] == used.sum()
    assert len(kernels) == launches and set(kernels) == set(kernels_solo) and set(kernels) <= census_names()
    for c, s in enumerate(SEEDS):
        for when, runs in (("before", before), ("after", after)):
            o1, a1, u1, st1 = runs[c]
            assert np.array_equal(out[c], o1), (name, c, when)
            assert acc[c] == a1 and used[c] == u1, (name, c, when)
            assert st1["n_chains"] == 1 and st1["launches"] == 1
    # distinct seeds give distinct chains, and the sampler both moved and stayed on the simplex
    assert len({out[c].tobytes() for c in range(len(SEEDS))}) == len(SEEDS)
    assert (acc > 0).all() and (used <= burn + T).all()
    w = out[..., :-1] @ Vt_hat + 1.0 / Vt_hat.shape[1]
    assert (w >= 0).all()


def replay_arrays(chains, exact_for):
    tt = cc.BURN_SIMPLEX + cc.T_SIMPLEX
    xi = np.stack([c["Z"] for c in chains])
    g = np.stack([c["G"] for c in chains])
    unif = np.stack([c["U"] for c in chains])
    # some chains get exactly the uniforms they consume, the others all tt
    n_unif = np.array([c["used"] if i in exact_for else tt for i, c in enumerate(chains)], dtype=np.int64)
    return xi, unif, n_unif, g


@pytest.mark.parametrize("name", list(S.CASES))
def test_replay_against_the_oracle(name):
    case = S.CASES[name]
    base, chains = S.chains_of(case)
    tt = cc.BURN_SIMPLEX + cc.T_SIMPLEX
    assert [c["seed"] for c in chains] == case["seeds"]
    for c in chains:     # no chain is excluded: each one decides clear of the rounding of its ratio
        assert c["margin"] >= cc.MARGIN and tt / 8 < c["acc_all"] < 7 * tt / 8, (name, c["seed"], c["margin"])
    ctx = gpu_ctx()
    ctx.set_problem(base["y"], base["X"])
    tune(ctx, case["tuning"])
    xi, unif, n_unif, g = replay_arrays(chains, exact_for=(0, 2, 3))
    try:
        out, acc, used, st = ctx.simplex_run_chains(
            base["Vt_hat"], base["S_hat"], len(chains), cc.T_SIMPLEX, *PRIOR, cc.BURN_SIMPLEX, base["stepsize"],
            xi=xi, unif=unif, n_unif=n_unif, g=g, return_stats=True)
        kernels = ctx.last_kernels()
    finally:
        ctx.set_tuning()
    assert len(kernels) == st["launches"] and set(kernels) <= census_names()
    if case["tuning"][5]:
        assert st["launches"] > 1, st      # the case is meant to cross a launch boundary
    for i, c in enumerate(chains):
        ref = c["chain"]
        err = np.abs(out[i] - ref).max()
        print(f"{name} chain {i} (stream seed {c['seed']}): max|err| {err:.3e}, margin {c['margin']:.2e}, "
              f"accepted {acc[i]}, used {used[i]}")
        assert err <= cc.F64_BAR * max(1.0, np.abs(ref).max()), (name, i, err)
        assert acc[i] == c["acc"] and used[i] == c["used"], (name, i)


def test_one_short_stream_names_its_chain():
    """Chain 2 alone gets one uniform too few: BMC_EINVAL naming chain 2 (the kernel's own
    end-of-stream path, not a fault), and the context is fine afterwards."""
    case = S.CASES["workgroup_single_300x4"]
    base, chains = S.chains_of(case)
    ctx = gpu_ctx()
    ctx.set_problem(base["y"], base["X"])
    xi, unif, n_unif, g = replay_arrays(chains, exact_for=(0, 1, 2, 3, 4))
    args = (base["Vt_hat"], base["S_hat"], len(chains), cc.T_SIMPLEX, *PRIOR, cc.BURN_SIMPLEX, base["stepsize"])
    short = n_unif.copy()
    short[2] -= 1
    with pytest.raises(ValueError, match=r"fewer uniforms supplied.*\(chain 2\)"):
        ctx.simplex_run_chains(*args, xi=xi, unif=unif, n_unif=short, g=g)
    with pytest.raises(ValueError):
        ctx.simplex_run_chains(*args[:2], 0, *args[3:], xi=xi[:0], unif=unif[:0], n_unif=short[:0], g=g[:0])
    out, acc, used = ctx.simplex_run_chains(*args, xi=xi, unif=unif, n_unif=n_unif, g=g)
    for i, c in enumerate(chains):
        assert np.abs(out[i] - c["chain"]).max() <= cc.F64_BAR * max(1.0, np.abs(c["chain"]).max())
        assert acc[i] == c["acc"] and used[i] == c["used"]


@pytest.mark.parametrize("tuning", [(0, 0, 0, 0, 0, 0), (3, 1, 1, 1, 0, 0), (3, 1, 1, 1, 0, 9)],
                         ids=["one_wave", "3_groups_xcd_slots", "3_groups_9_cus"])
def test_neighbours_do_not_matter(tuning):
    y, X, Vt_hat, S_hat = golden150()
    ctx = gpu_ctx()
    ctx.set_problem(y, X)
    tune(ctx, tuning)
    seeds = [5, 6, (1 << 33) + 7, 8, 9, 10, 11]
    rest = (200, *PRIOR, 60, 0.002)
    try:
        out7, acc7, used7 = ctx.simplex_run_chains(Vt_hat, S_hat, 7, *rest, seeds=seeds)
        for c in (0, 2, 3, 6):
            out2, acc2, used2 = ctx.simplex_run_chains(Vt_hat, S_hat, 2, *rest, seeds=[seeds[c], 12345])
            assert np.array_equal(out7[c], out2[0]), c
            assert acc7[c] == acc2[0] and used7[c] == used2[0], c
    finally:
        ctx.set_tuning()


def test_sampler_surface(capsys):
    y, X, Vt_hat, S_hat = golden150()
    seeds = [21, 22, 23, 24]
    out = gibbs_sampler_simplex(y, X, Vt_hat, S_hat, 500, PRIOR, burn=200, stepsize=0.002, n_chains=4, seeds=seeds)
    lines = capsys.readouterr().out.strip().splitlines()
    assert out.shape == (4, 500, X.shape[1] + 1) and np.isfinite(out).all()
    assert ((out[..., :-1] @ Vt_hat + 1.0 / Vt_hat.shape[1]) >= 0).all()
    assert len(lines) == 2 and lines[0].startswith("Acceptance rate: ") and "min" in lines[1] and "max" in lines[1]
    for c, s in enumerate(seeds):
        one = gibbs_sampler_simplex(y, X, Vt_hat, S_hat, 500, PRIOR, burn=200, stepsize=0.002, seed=s)
        assert one.shape == (500, X.shape[1] + 1) and np.array_equal(one, out[c])
    assert len(capsys.readouterr().out.strip().splitlines()) == 4      # the reference's single line each
    # default seeds come from numpy's global stream: repeatable, and chain 0 of two is not the
    # one-chain run (two draws of the stream per seed, hi halves first)
    np.random.seed(3)
    a = gibbs_sampler_simplex(y, X, Vt_hat, S_hat, 100, PRIOR, burn=50, stepsize=0.002, n_chains=3)
    np.random.seed(3)
    b = gibbs_sampler_simplex(y, X, Vt_hat, S_hat, 100, PRIOR, burn=50, stepsize=0.002, n_chains=3)
    assert a.shape == (3, 100, X.shape[1] + 1) and np.array_equal(a, b)


def _standin_bmc():
    from pybmc_amd import BayesianModelCombination, Dataset
    models = ["FRDM", "HFB24", "UNEDF1", "SKM"]
    ds = Dataset(os.path.join(HERE, "golden", "dataset_standin.csv"))
    data = ds.load_data(models + ["truth"], keys=["BE"], domain_keys=["N", "Z"])
    train_df, val_df, _ = ds.split_data(data, "BE", splitting_algorithm="random", train_size=0.6,
                                        val_size=0.2, test_size=0.2)
    b = BayesianModelCombination(models, data, truth_column_name="truth")
    b.orthogonalize("BE", train_df, components_kept=3, method="svd")
    return b, models, val_df


def test_train_pools_simplex_chains_in_chain_order():
    from pybmc_amd import _lib
    b, models, val_df = _standin_bmc()
    T, burn, seeds = 3000, 500, [31, 32, 33, 34]
    opts = {"iterations": T, "sampler": "simplex", "burn": burn, "stepsize": 0.001,
            "b_mean_prior": np.zeros(3), "b_mean_cov": np.eye(3), "nu0_chosen": 1.0, "sigma20_chosen": 0.02}
    b.train({**opts, "n_chains": 4, "seeds": seeds})
    assert b.n_chains == 4 and b.samples.shape == (4 * T, 4)
    assert b.last_stats["n_chains"] == 4 and b.last_stats["launches"] == 1
    kernels = _lib.default_context(b.device).last_kernels()
    assert len(kernels) == b.last_stats["launches"]
    assert all(k.startswith("simplex_") for k in kernels) and set(kernels) <= census_names()
    solo = [gibbs_sampler_simplex(b.centered_experiment_train, b.U_hat, b.Vt_hat, b.S_hat, T, [1.0, 0.02],
                                  burn=burn, stepsize=0.001, seed=s, device=b.device) for s in seeds]
    assert np.array_equal(b.samples, np.concatenate(solo))
    # the readers of chains take the pooled simplex chains as they are
    df = b.diagnostics()
    assert list(df.index) == ["beta_0", "beta_1", "beta_2", "sigma"] + models
    assert np.isfinite(df["r_hat"].to_numpy()).all() and np.isfinite(df["ess"].to_numpy()).all()
    assert (df["ess"] > 0).all()
    w = b.waic()
    assert np.isfinite(w["elpd_waic"]) and w["n_points"] == len(b.centered_experiment_train)
    loo = b.loo()
    assert np.isfinite(loo["elpd_loo"])
    lpd = b.log_predictive_density(val_df)
    assert np.isfinite(lpd["elpd"]) and lpd["n_points"] == len(val_df)
    rndm_m, lo, med, up = b.predict(val_df[models + ["N", "Z"]])
    assert np.isfinite(rndm_m).all() and len(med) == len(val_df)
    # devices with the simplex sampler is an error, not a silent single-GPU run
    with pytest.raises(ValueError, match="simplex"):
        b.train({**opts, "devices": [0, 1]})


def test_train_without_n_chains_is_unchanged():
    b, _, _ = _standin_bmc()
    opts = {"iterations": 800, "sampler": "simplex", "burn": 200, "stepsize": 0.001,
            "b_mean_prior": np.zeros(3), "b_mean_cov": np.eye(3), "nu0_chosen": 1.0, "sigma20_chosen": 0.02}
    np.random.seed(11)
    b.train(opts)
    got = b.samples.copy()
    assert b.n_chains == 1 and got.shape == (800, 4) and b.last_stats["n_chains"] == 1
    # what train() has always done on this branch: one seed from numpy's global stream (two
    # draws, the high half first), one chain through the one-chain entry point
    np.random.seed(11)
    hi = np.random.randint(0, 2 ** 32, size=1, dtype=np.uint64)
    lo = np.random.randint(0, 2 ** 32, size=1, dtype=np.uint64)
    seed = int((hi << np.uint64(32)) | lo)
    ctx = gpu_ctx()
    ctx.set_problem(np.asarray(b.centered_experiment_train, dtype=np.float64), b.U_hat)
    want, _ = ctx.simplex_run(b.Vt_hat, b.S_hat, 800, 1.0, 0.02, 200, 0.001, seed=seed)
    assert np.array_equal(got, want)
