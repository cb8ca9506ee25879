"""Parity of the HIP Gibbs path with the reference, through the C ABI  (-m gpu).

Tiers:
  T1 step-wise      Gram, OLS sigma2_0, mean/cov of beta | sigma2, rss        1e-12 rel
  T2 whole chain    the reference's own chain (golden fixture) replayed with its
                    variates; posterior summaries                            1e-6 rel
                    (north-star bar; the observed error is ~1e-15)
  T3 distributional on-device Philox variates vs the oracle with numpy variates,
                    within 5 Monte-Carlo standard errors
"""
import numpy as np
import pytest

import census_common as cc
from gpu_common import golden_case, gpu_ctx, replay_inputs
from oracle import bmc_oracle as O
from pybmc_amd.chains import posterior_summary
from pybmc_amd.synthetic import synth_problem

pytestmark = pytest.mark.gpu

CASES = ["gibbs_tiny3x2", "gibbs_dense64x8", "gibbs_ortho629x3", "gibbs_ragged1237x5",
         "gibbs_c2_10000x32"]
REL_BAR = 1e-6      # north-star tolerance on posterior summaries (float64)
STEP_TOL = 1e-12    # T1


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.mark.parametrize("name", CASES)
def test_t1_stepwise(name):
    ctx = gpu_ctx()
    g, y, X, prior = golden_case(name)
    Xf = np.asarray(X, float)
    ctx.set_problem(y, X)
    ctx.set_prior(*prior)
    Xa = np.column_stack([Xf, y])
    assert rel(ctx.gram(), Xa.T @ Xa) < STEP_TOL                    # f64 MFMA Gram
    st = O.chain_setup(y, Xf, prior)
    W, lam, s2i = ctx.basis()
    assert abs(s2i - st["sigma2_init"]) <= STEP_TOL * st["sigma2_init"]
    # mean / cov of beta | sigma2 against the oracle's inv(X'X/s2 + P + 1e-6 I)
    # (inference_utils.py:41-44).  SURVEY 8(c) T1 asks for 1e-12; an explicit inverse is only
    # accurate to about kappa * eps relative (kappa = condition number of the matrix inverted,
    # eps = 2.2e-16) -- on BOTH sides of the comparison -- so the bar is
    # max(1e-12, 32 kappa eps): 1e-12 itself on the orthonormal designs train() produces
    # (kappa ~ 1), looser only where the fixture is ill-conditioned, and by how much is printed.
    b0, C0 = np.asarray(prior[0], float), np.asarray(prior[1], float)
    eps = np.finfo(float).eps
    for s2 in (st["sigma2_init"], 0.37, 5.0, float(g["samples"][-1, -1] ** 2)):
        m, c = ctx.conditional_moments(s2)
        mo, co = O.conditional_moments(st, y, Xf, s2)
        kappa = np.linalg.cond(Xf.T @ Xf / s2 + np.linalg.inv(C0) + 1e-6 * np.eye(len(b0)))
        bar = max(STEP_TOL, 32 * kappa * eps)
        assert rel(m, mo) < bar and rel(c, co) < bar, (name, s2, kappa, rel(m, mo), rel(c, co))
    betas = g["samples"][:7, :-1]
    got = ctx.residual_rss(betas)
    want = np.array([O.residual_rss(y, Xf, b) for b in betas])
    assert rel(got, want) < STEP_TOL


@pytest.mark.parametrize("name", CASES)
def test_t2_replay_whole_chain(name):
    ctx = gpu_ctx()
    g, y, X, prior = golden_case(name)
    ctx.set_problem(y, X)
    ctx.set_prior(*prior)
    T = int(g["T"])
    st, xi, ref = replay_inputs(ctx, g, y, X, prior, T)
    out, stats = ctx.gibbs_run(1, T, xi=xi[None], g=g["G"][None, :T])
    out = out[0]
    assert np.abs(out - ref).max() < 1e-9 * max(1.0, np.abs(ref).max())
    Vt_hat = (g["Vt"] / g["S_hat"][:, None]) if "Vt" in g else None
    a, b = posterior_summary(out, Vt_hat), posterior_summary(ref, Vt_hat)
    for key in b:
        assert rel(a[key], b[key]) < REL_BAR, key


def test_t2_replay_is_geometry_independent():
    """Same chain under different launch geometries (groups, waves, LDS-resident or
    streaming): the reduction order changes, the chain must not (beyond rounding)."""
    ctx = gpu_ctx()
    g, y, X, prior = golden_case("gibbs_c2_10000x32")
    ctx.set_problem(y, X)
    ctx.set_prior(*prior)
    T = 300
    st, xi, ref = replay_inputs(ctx, g, y, X, prior, T)
    outs = []
    # (groups, waves, residency 1 reg/2 lds/3 stream, panels per wave, force agent scope)
    seen = set()
    for G, W, res, ppw, agent in [(0, 0, 0, 0, 0), (0, 0, 0, 0, 1), (20, 8, 1, 1, 0),
                                  (32, 5, 1, 1, 1), (10, 8, 1, 2, 0), (16, 5, 1, 2, 1),
                                  (157, 1, 2, 0, 0), (8, 8, 2, 0, 0), (32, 5, 2, 0, 1),
                                  (64, 3, 3, 0, 0), (256, 1, 2, 0, 0), (1, 8, 3, 0, 0)]:
        ctx.set_tuning(G, W, res, ppw, agent)
        o, stats = ctx.gibbs_run(1, T, xi=xi[None], g=g["G"][None, :T])
        assert np.abs(o[0] - ref).max() < 1e-9, (G, W, res, ppw, agent)
        if agent:
            assert stats["xcd_local_chains"] == 0
        seen.add((stats["residency"], stats["xcd_local_chains"]))
        outs.append(o[0])
    assert {1, 2, 3} <= {r for r, _ in seen}
    ctx.set_tuning(0, 0)
    for o in outs[1:]:
        assert np.abs(o - outs[0]).max() < 1e-11


def test_t2_replay_many_chains_in_one_launch():
    """Eight copies of the reference chain in one launch (one per XCD): all equal."""
    ctx = gpu_ctx()
    g, y, X, prior = golden_case("gibbs_ortho629x3")
    ctx.set_problem(y, X)
    ctx.set_prior(*prior)
    T = 500
    st, xi, ref = replay_inputs(ctx, g, y, X, prior, T)
    out, stats = ctx.gibbs_run(8, T, xi=np.repeat(xi[None], 8, 0), g=np.repeat(g["G"][None, :T], 8, 0))
    for c in range(8):
        assert np.abs(out[c] - ref).max() < 1e-9
    assert stats["n_chains"] == 8


def test_t2_float32_storage():
    """f32 storage of X and y (f64 accumulation): a NEW capability; the tolerance is
    the storage rounding (1e-5 relative), not the 1e-6 float64 bar."""
    ctx = gpu_ctx()
    g, y, X, prior = golden_case("gibbs_ortho629x3")
    ctx.set_problem(y, X, dtype=np.float32)
    ctx.set_prior(*prior)
    T = 1000
    # innovations are defined against the f32-rounded problem the device actually holds
    X32, y32 = np.asarray(X, np.float32).astype(float), np.asarray(y, np.float32).astype(float)
    W, lam, s2i = ctx.basis()
    Z, G = g["Z"][:T], g["G"][:T]
    ref = O.gibbs_replay(y32, X32, T, prior, Z, G)
    st = O.chain_setup(y32, X32, prior)
    trace = np.concatenate([[st["sigma2_init"]], ref[:, -1] ** 2])
    xi = O.innovations_in_basis(st, y32, X32, ref, W, lam, trace)
    out, _ = ctx.gibbs_run(1, T, xi=xi[None], g=G[None])
    a, b = posterior_summary(out[0]), posterior_summary(ref)
    for key in b:
        assert rel(a[key], b[key]) < 1e-5, key


def mcse(x):
    """Monte-Carlo standard error by batch means (50 batches)."""
    x = np.asarray(x)
    nb = 50
    m = x[: len(x) // nb * nb].reshape(nb, -1, *x.shape[1:]).mean(1)
    return m.std(0, ddof=1) / np.sqrt(nb)


def test_t3_device_rng_matches_oracle_distribution():
    ctx = gpu_ctx()
    g, y, X, prior = golden_case("gibbs_dense64x8")
    ctx.set_problem(y, X)
    ctx.set_prior(*prior)
    T = 40000
    st = O.chain_setup(y, X, prior)
    Z, G = O.reference_streams(123, 456, T, X.shape[1], O.gamma_shape(st))
    ref = O.gibbs_replay(y, X, T, prior, Z, G)
    out, _ = ctx.gibbs_run(4, T, seeds=[11, 12, 13, 14])
    pooled = out.reshape(-1, out.shape[-1])
    for stat in (lambda s: s, lambda s: s ** 2):
        a, b = stat(pooled), stat(ref)
        se = np.sqrt(mcse(a) ** 2 + mcse(b) ** 2)
        assert np.all(np.abs(a.mean(0) - b.mean(0)) < 5 * se)
    # Gelman-Rubin across the four device chains
    m = out.mean(1)
    Wv = out.var(1, ddof=1).mean(0)
    Bv = T * m.var(0, ddof=1)
    rhat = np.sqrt(((T - 1) / T * Wv + Bv / T) / Wv)
    assert np.all(rhat < 1.01)


def test_chain_depends_on_its_seed_only():
    """A chain's samples are a function of (problem, prior, seed): running it alone,
    among other chains, or under another geometry gives the same chain."""
    ctx = gpu_ctx()
    p = synth_problem(3000, 9, 8, seed=2)
    ctx.set_problem(p["y"], p["X"])
    ctx.set_prior(*p["prior"])
    T = 400
    alone, _ = ctx.gibbs_run(1, T, seeds=[77])
    many, _ = ctx.gibbs_run(5, T, seeds=[5, 77, 6, 77, 8])
    assert np.array_equal(many[1], many[3])
    assert np.abs(many[1] - alone[0]).max() < 1e-11
    assert np.abs(many[0] - many[1]).max() > 1e-3
    ctx.set_tuning(3, 2, 2)
    other, _ = ctx.gibbs_run(1, T, seeds=[77])
    ctx.set_tuning(0, 0)
    assert np.abs(other[0] - alone[0]).max() < 1e-11
    again, _ = ctx.gibbs_run(1, T, seeds=[77])
    assert np.array_equal(again, alone)            # bit-reproducible run to run


def test_more_chains_than_one_launch_holds():
    ctx = gpu_ctx()
    p = synth_problem(20000, 6, 5, seed=4)           # 313 panels: several groups per chain
    ctx.set_problem(p["y"], p["X"])
    ctx.set_prior(*p["prior"])
    out, stats = ctx.gibbs_run(19, 200, seeds=np.arange(19) + 1)
    assert stats["groups_per_chain"] > 1 and stats["launches"] >= 3 and np.isfinite(out).all()
    solo, _ = ctx.gibbs_run(1, 200, seeds=[19])
    assert np.abs(out[18] - solo[0]).max() < 1e-11


def test_small_problem_runs_in_one_workgroup_per_chain():
    """N <= a few thousand rows: the chain lives in ONE workgroup (no exchange, no co-residency
    requirement), so hundreds of chains share a launch; results equal the multi-group kernel's."""
    ctx = gpu_ctx()
    p = synth_problem(629, 4, 3, seed=3)
    ctx.set_problem(p["y"], p["X"])
    ctx.set_prior(*p["prior"])
    T = 400
    seeds = np.arange(300) + 1
    many, st = ctx.gibbs_run(300, T, seeds=seeds)
    assert st["groups_per_chain"] == 1 and st["launches"] == 1 and st["residency"] == 1
    ctx.set_tuning(groups_per_chain=10, waves_per_group=1)
    multi, st2 = ctx.gibbs_run(3, T, seeds=seeds[[0, 150, 299]])
    ctx.set_tuning()
    assert st2["groups_per_chain"] == 10
    for i, c in enumerate((0, 150, 299)):
        assert np.abs(many[c] - multi[i]).max() < 1e-11


@pytest.mark.parametrize("n,k,dt", [(629, 3, np.float64), (64, 1, np.float64), (100, 4, np.float64),
                                    (1000, 4, np.float64), (700, 8, np.float64), (500, 16, np.float64),
                                    (250, 32, np.float64), (1024, 8, np.float64), (629, 3, np.float32),
                                    (300, 13, np.float32)])
def test_one_wave_chains(n, k, dt):
    """A chain of a few hundred rows and a few columns runs in ONE wave (gibbs_wave_kernel: rows
    and columns in the wave's registers, no LDS hand-over, no barrier; output rows staged 64 at
    a time).  Every register shape (rows per lane x columns), both storage types: equal to the
    one-workgroup form to rounding, independent of how many chains share the launch, for
    iteration counts around the 64-row staging block, and equal to the replayed oracle chain."""
    ctx = gpu_ctx()
    rng = np.random.default_rng(7 * n + k)
    X = (rng.standard_normal((n, k)) / np.sqrt(n)).astype(dt)
    y = (X.astype(np.float64) @ rng.standard_normal(k) + 0.1 * rng.standard_normal(n)).astype(dt)
    prior = (np.zeros(k), np.eye(k) * 10.0, 1.0, 0.02)
    ctx.set_problem(y, np.asfortranarray(X), dtype=dt)
    ctx.set_prior(*prior)
    seeds = np.arange(70) + 3
    ctx.set_tuning(waves_per_group=1)
    for T in (1, 63, 64, 65, 130):
        many, st = ctx.gibbs_run(70, T, seeds=seeds)
        assert st["waves_per_group"] == 1 and st["groups_per_chain"] == 1 and st["launches"] == 1, st
        assert st["xcd_local_chains"] == 70 and np.isfinite(many).all()
        solo, _ = ctx.gibbs_run(1, T, seeds=seeds[33:34])
        assert np.array_equal(many[33], solo[0]), T
        if T > 1:   # (a prefix of a longer run: the variates of iteration t do not depend on T)
            assert np.array_equal(many[33][:1], ctx.gibbs_run(1, 1, seeds=seeds[33:34])[0][0])
    ctx.set_tuning(waves_per_group=4, groups_per_chain=1)
    group, stg = ctx.gibbs_run(3, 130, seeds=seeds[[0, 33, 69]])
    ctx.set_tuning()
    assert stg["waves_per_group"] == 4 and stg["groups_per_chain"] == 1
    scale = max(1.0, np.abs(group).max())
    for i, c in enumerate((0, 33, 69)):
        assert np.abs(many[c] - group[i]).max() < 1e-11 * scale, c
    if dt == np.float64:
        Xd = X.astype(np.float64)
        st_o = O.chain_setup(y, Xd, prior)
        Z, G = O.reference_streams(11, 12, 70, k, O.gamma_shape(st_o))
        ref, trace = O.gibbs_replay(y, Xd, 70, prior, Z, G, return_sigma2=True)
        W, lam, _ = ctx.basis()
        xi = O.innovations_in_basis(st_o, y, Xd, ref, W, lam, trace)
        ctx.set_tuning(waves_per_group=1)
        out, st = ctx.gibbs_run(2, 70, xi=np.repeat(xi[None], 2, 0), g=np.repeat(G[None], 2, 0))
        ctx.set_tuning()
        assert st["waves_per_group"] == 1
        assert np.array_equal(out[0], out[1])
        assert np.abs(out[0] - ref).max() < 1e-9 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("n,k,dt,nw", [(1024, 8, np.float64, 2), (2500, 8, np.float64, 4),
                                       (4000, 4, np.float64, 4), (1500, 3, np.float32, 2),
                                       (2100, 7, np.float32, 4), (8000, 4, np.float64, 8),
                                       (6000, 3, np.float32, 8), (4096, 8, np.float64, 8)])
def test_chains_in_two_or_four_waves(n, k, dt, nw):
    """A few thousand rows and a few columns: the chain runs in 2, 4 or 8 waves of ONE workgroup
    (gibbs_wave_kernel), every wave with its share of the rows in registers and every wave
    running the whole iteration; the waves exchange one double per iteration through LDS.
    Equal to the workgroup form (gibbs_loop_kernel) to rounding, to the replayed oracle chain,
    independent of the number of chains in the launch and of the iteration count."""
    ctx = gpu_ctx()
    rng = np.random.default_rng(5 * n + k)
    X = (rng.standard_normal((n, k)) / np.sqrt(n)).astype(dt)
    y = (X.astype(np.float64) @ rng.standard_normal(k) + 0.1 * rng.standard_normal(n)).astype(dt)
    prior = (np.zeros(k), np.eye(k) * 10.0, 1.0, 0.02)
    ctx.set_problem(y, np.asfortranarray(X), dtype=dt)
    ctx.set_prior(*prior)
    seeds = np.arange(40) + 9
    for T in (1, 64, 65, 200):
        many, st = ctx.gibbs_run(40, T, seeds=seeds)
        assert st["waves_per_group"] == nw and st["groups_per_chain"] == 1 and st["launches"] == 1, st
        solo, _ = ctx.gibbs_run(1, T, seeds=seeds[17:18])
        assert np.array_equal(many[17], solo[0]), T
    ctx.set_tuning(waves_per_group=8)
    group, stg = ctx.gibbs_run(2, 200, seeds=seeds[[0, 39]])
    ctx.set_tuning()
    assert stg["waves_per_group"] == 8
    scale = max(1.0, np.abs(group).max())
    assert np.abs(many[0] - group[0]).max() < 1e-11 * scale
    assert np.abs(many[39] - group[1]).max() < 1e-11 * scale
    if dt == np.float64:
        st_o = O.chain_setup(y, X, prior)
        Z, G = O.reference_streams(21, 22, 70, k, O.gamma_shape(st_o))
        ref, trace = O.gibbs_replay(y, X, 70, prior, Z, G, return_sigma2=True)
        W, lam, _ = ctx.basis()
        xi = O.innovations_in_basis(st_o, y, X, ref, W, lam, trace)
        out, st = ctx.gibbs_run(2, 70, xi=np.repeat(xi[None], 2, 0), g=np.repeat(G[None], 2, 0))
        assert st["waves_per_group"] == nw
        assert np.array_equal(out[0], out[1])
        assert np.abs(out[0] - ref).max() < 1e-9 * max(1.0, np.abs(ref).max())


# ---------------------------------------------------------------- edge cases
def test_edge_shapes():
    ctx = gpu_ctx()
    rng = np.random.default_rng(0)
    for n, k in [(1, 1), (2, 1), (63, 2), (64, 3), (65, 3), (129, 7), (4097, 64), (700, 65),
                 (600, 130)]:
        X = rng.standard_normal((n, k))
        y = rng.standard_normal(n)
        if n < k:
            continue
        prior = (np.zeros(k), np.eye(k), 1.0, 1.0)
        ctx.set_problem(y, X)
        if n == k == 1:
            pass
        ctx.set_prior(*prior)
        st = O.chain_setup(y, X, prior)
        T = 50
        Z, G = O.reference_streams(1, 2, T, k, O.gamma_shape(st))
        ref = O.gibbs_replay(y, X, T, prior, Z, G)
        W, lam, s2i = ctx.basis()
        trace = np.concatenate([[st["sigma2_init"]], ref[:, -1] ** 2])
        xi = O.innovations_in_basis(st, y, X, ref, W, lam, trace)
        out, _ = ctx.gibbs_run(1, T, xi=xi[None], g=G[None])
        assert np.abs(out[0] - ref).max() < 1e-8 * max(1.0, np.abs(ref).max()), (n, k)


def test_zero_iterations_and_layouts():
    ctx = gpu_ctx()
    rng = np.random.default_rng(1)
    X = rng.standard_normal((300, 4))
    y = rng.standard_normal(300)
    prior = (np.zeros(4), np.eye(4), 1.0, 1.0)
    ctx.set_problem(y, X)
    ctx.set_prior(*prior)
    out, _ = ctx.gibbs_run(1, 0, seeds=[1])
    assert out.shape == (1, 0, 5)
    a, _ = ctx.gibbs_run(1, 100, seeds=[3])
    ctx.set_problem(y, np.asfortranarray(X))       # column-major, what U_hat is
    ctx.set_prior(*prior)
    b, _ = ctx.gibbs_run(1, 100, seeds=[3])
    assert np.array_equal(a, b)
    ctx.set_problem(y, X[:, ::-1][:, ::-1])        # a non-contiguous view is copied
    ctx.set_prior(*prior)
    c, _ = ctx.gibbs_run(1, 100, seeds=[3])
    assert np.array_equal(a, c)


def test_error_behaviour_matches_the_reference():
    ctx = gpu_ctx()
    rng = np.random.default_rng(2)
    X = rng.standard_normal((50, 3))
    y = rng.standard_normal(50)
    ctx.set_problem(y, X)
    with pytest.raises(np.linalg.LinAlgError):     # inv(b_mean_cov), inference_utils.py:22
        ctx.set_prior(np.zeros(3), np.zeros((3, 3)), 1.0, 1.0)
    Xs = np.column_stack([X[:, 0], X[:, 0], X[:, 1]])
    ctx.set_problem(y, Xs)
    with pytest.raises(np.linalg.LinAlgError):     # inv(X'X), inference_utils.py:26
        ctx.set_prior(np.zeros(3), np.eye(3), 1.0, 1.0)
    with pytest.raises(ValueError):
        ctx.set_problem(y[:10], X)
    with pytest.raises(ValueError):
        ctx.set_prior(np.zeros(2), np.eye(2), 1.0, 1.0)
    ctx.set_problem(y, X)
    from pybmc_amd import _lib
    with pytest.raises(_lib.BmcError):             # run before set_prior
        ctx.gibbs_run(1, 10, seeds=[1])
    ctx.set_prior(np.zeros(3), np.eye(3), 1.0, 1.0)
    with pytest.raises(ValueError):
        ctx.gibbs_run(0, 10, seeds=[])


def test_sigma2_floor():
    """A perfect fit drives sigma2 to the 1e-6 floor of inference_utils.py:37,52."""
    ctx = gpu_ctx()
    X = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    y = X @ np.array([1.0, 2.0])
    ctx.set_problem(y, X)
    ctx.set_prior(np.zeros(2), np.eye(2) * 1e6, 1e-9, 1e-9)
    _, _, s2i = ctx.basis()
    assert s2i == 1e-6
    out, _ = ctx.gibbs_run(1, 50, seeds=[1])
    assert np.all(out[0, :, -1] >= 1e-3 - 1e-18)   # sigma >= sqrt(1e-6)


# ------------------------------------------------------- full-size properties
def test_full_size_c2_properties():
    """BASELINE config C2/C3 at full length (8 chains x 50000): size-independent
    properties -- chains agree (R-hat), the posterior mean of beta equals the
    closed-form conditional mean at the posterior-mean precision, weights sum to 1."""
    ctx = gpu_ctx()
    p = synth_problem(10000, 33, 32, seed=0)
    ctx.set_problem(p["y"], p["X"])
    ctx.set_prior(*p["prior"])
    T = 50000
    out, stats = ctx.gibbs_run(8, T, seeds=np.arange(1, 9))
    assert np.isfinite(out).all() and stats["residency"] == 1
    burn = 1000
    s = out[:, burn:]
    m = s.mean(1)
    Wv = s.var(1, ddof=1).mean(0)
    Bv = s.shape[1] * m.var(0, ddof=1)
    rhat = np.sqrt(((s.shape[1] - 1) / s.shape[1] * Wv + Bv / s.shape[1]) / Wv)
    assert np.all(rhat < 1.005)
    pooled = s.reshape(-1, 33)
    # E[beta] = E[ mean(beta | sigma2) ]: average the closed form over the sigma2 draws
    sig2 = pooled[::997, -1] ** 2
    means = np.mean([ctx.conditional_moments(v)[0] for v in sig2], axis=0)
    se = pooled[:, :-1].std(0) / np.sqrt(len(pooled) / 2)
    assert np.all(np.abs(pooled[:, :-1].mean(0) - means) < 6 * se)
    Vt_hat = p["Vt"] / p["S_hat"][:, None]
    w = posterior_summary(pooled, Vt_hat)["weights_mean"]
    assert abs(w.sum() - 1.0) < 1e-9
    assert abs(pooled[:, -1].mean() - 0.1) < 0.005


def test_c_abi_leading_dimensions_and_device_inputs():
    """Straight through the C ABI: padded leading dimensions in both layouts, float32 storage,
    and device-resident inputs (bmc_set_problem_device) must all describe the same problem."""
    import ctypes as C
    import torch
    from pybmc_amd import _lib
    ctx = gpu_ctx()
    lib = _lib.load_library()
    rng = np.random.default_rng(11)
    n, k = 777, 6
    X = rng.standard_normal((n, k))
    y = rng.standard_normal(n)
    ctx.set_problem(y, X)
    want = ctx.gram()
    # row-major with ldx = k + 3, col-major with ldx = n + 5
    Xr = np.zeros((n, k + 3)); Xr[:, :k] = X
    Xc = np.zeros((k, n + 5)); Xc[:, :n] = X.T
    for buf, ldx, layout in ((Xr, k + 3, _lib.BMC_ROW_MAJOR), (Xc, n + 5, _lib.BMC_COL_MAJOR)):
        rc = lib.bmc_set_problem(ctx._h, buf.ctypes.data_as(C.c_void_p), n, k, ldx, layout,
                                 y.ctypes.data_as(C.c_void_p), _lib.BMC_F64)
        assert rc == 0
        ctx.n, ctx.k = n, k
        assert np.array_equal(ctx.gram(), want)
    # device-resident inputs (a torch tensor's storage), both layouts
    for arr, ldx, layout in ((X, k, _lib.BMC_ROW_MAJOR), (np.ascontiguousarray(X.T), n, _lib.BMC_COL_MAJOR)):
        tx = torch.from_numpy(arr).cuda()
        ty = torch.from_numpy(y).cuda()
        torch.cuda.synchronize()
        ctx.set_problem_device(tx.data_ptr(), n, k, ldx, layout, ty.data_ptr())
        assert np.array_equal(ctx.gram(), want)
    # bad leading dimension / NULL pointers -> BMC_EINVAL, not a crash
    assert lib.bmc_set_problem(ctx._h, Xr.ctypes.data_as(C.c_void_p), n, k, k - 1, 0,
                               y.ctypes.data_as(C.c_void_p), 0) == _lib.BMC_EINVAL
    assert lib.bmc_set_problem(ctx._h, None, n, k, k, 0, y.ctypes.data_as(C.c_void_p), 0) == _lib.BMC_EINVAL
    assert lib.bmc_set_problem(ctx._h, Xr.ctypes.data_as(C.c_void_p), n, 300, 300, 0,
                               y.ctypes.data_as(C.c_void_p), 0) == _lib.BMC_EINVAL
    # float32 storage sees the float32-rounded matrix
    ctx.set_problem(y, X, dtype=np.float32)
    X32, y32 = X.astype(np.float32).astype(float), y.astype(np.float32).astype(float)
    Xa = np.column_stack([X32, y32])
    assert np.abs(ctx.gram() - Xa.T @ Xa).max() < 1e-10 * np.abs(Xa.T @ Xa).max()


def test_residual_kernel_properties_at_full_size():
    """Size-independent properties of the residual-reduction kernel at the C4 shape
    (N = 200000, K = 64, float32 storage): rss(0) = y'y, scaling, and the Gram identity
    rss(b) = y'y - 2 b'X'y + b'X'X b (all against the kernel's own MFMA Gram)."""
    ctx = gpu_ctx()
    rng = np.random.Generator(np.random.PCG64(4))
    n, k = 200000, 64
    X = np.asfortranarray(rng.standard_normal((n, k), dtype=np.float32))
    y = rng.standard_normal(n, dtype=np.float32)
    ctx.set_problem(y, X, dtype=np.float32)
    G = ctx.gram()
    A, c, yty = G[:k, :k], G[:k, k], G[k, k]
    assert abs(ctx.residual_rss(np.zeros(k))[0] - yty) <= 1e-12 * yty
    B = rng.standard_normal((5, k)) * 0.1
    got = ctx.residual_rss(B)
    want = np.array([yty - 2 * b @ c + b @ A @ b for b in B])
    assert np.abs(got - want).max() < 1e-10 * yty
    # more vectors than one launch takes (8): launches back to back, one copy each way; every
    # vector's result is that of asking for it alone
    B = rng.standard_normal((21, k)) * 0.1
    many = ctx.residual_rss(B)
    assert many.shape == (21,)
    for i in (0, 7, 8, 15, 16, 20):
        assert many[i] == ctx.residual_rss(B[i])[0]
    assert np.abs(np.linalg.eigvalsh(A)).min() > 0 and np.allclose(A, A.T, rtol=0, atol=0)


def test_t2_long_chain_at_c2_size():
    """5000 iterations at N = 10000, K = 32 (ten times the committed golden prefix): the oracle
    chain (numpy streams, computed here) replayed through the HIP loop; rounding differences must
    not accumulate (the chain map contracts) -- north-star bar 1e-6 on the summaries."""
    ctx = gpu_ctx()
    p = synth_problem(10000, 33, 32, seed=0)
    y, X, prior = p["y"], p["X"], p["prior"]
    T = 5000
    st = O.chain_setup(y, X, prior)
    Z, G = O.reference_streams(101, 102, T, 32, O.gamma_shape(st))
    ref, trace = O.gibbs_replay(y, X, T, prior, Z, G, return_sigma2=True)
    ctx.set_problem(y, X)
    ctx.set_prior(*prior)
    W, lam, _ = ctx.basis()
    xi = O.innovations_in_basis(st, y, X, ref, W, lam, trace)
    out, stats = ctx.gibbs_run(1, T, xi=xi[None], g=G[None])
    assert stats["residency"] == 1 and stats["xcd_local_chains"] in (0, 1)
    err = np.abs(out[0] - ref)
    assert err.max() < 1e-11
    assert err[-500:].max() <= 10 * max(err[:500].max(), 1e-15)      # no drift
    Vt_hat = p["Vt"] / p["S_hat"][:, None]
    a, b = posterior_summary(out[0], Vt_hat), posterior_summary(ref, Vt_hat)
    for key in b:
        assert rel(a[key], b[key]) < REL_BAR, key


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    return cc.build_planner(tmp_path_factory.mktemp("planner"))


def replay_distinct_streams(ctx, planner, tmp_path, y, X, prior, dt, nch, T, **tune):
    """nch chains of the problem set on ctx in replay mode, the first, one middle and the last slot
    of every launch and of every bundle on DIFFERENT streams (census_common.colour_slots, from the
    launches the CPU planner predicts; Context.last_kernels() must agree with one of its two pack
    answers), every slot compared with its OWN oracle chain: a kernel that reads another slot's
    variates, or a bundle that swaps two chains, fails.  f64 storage: the replay bar 1e-9; f32:
    test_t2_float32_storage's bar on posterior_summary, the oracle run on the f32-rounded data.
    Returns (stats, launches)."""
    f32 = np.dtype(dt) == np.float32
    Xd, yd = np.asarray(X, dt).astype(np.float64), np.asarray(y, dt).astype(np.float64)
    plans = cc.plan_launches(planner, tmp_path, Xd.shape[0], Xd.shape[1], f32, nch,
                             res=tune.get("residency", 0), cpp=tune.get("chains_per_pass", 0))
    n_streams = cc.N_STREAMS if nch > 2 else nch
    colour = cc.colour_slots(plans[0], n_streams, plans[1])
    streams = cc.gibbs_streams(yd, Xd, prior, n_streams, T)
    chains = [cc.gibbs_chain(yd, Xd, prior, Z, G) for Z, G in streams]
    W, lam, _ = ctx.basis()
    st_o = O.chain_setup(yd, Xd, prior)
    xis = [O.innovations_in_basis(st_o, yd, Xd, ref, W, lam, trace) for ref, trace in chains]
    ctx.set_tuning(**tune)
    try:
        out, st = ctx.gibbs_run(nch, T, xi=np.stack([xis[colour[c]] for c in range(nch)]),
                                g=np.stack([streams[colour[c]][1] for c in range(nch)]))
        got = ctx.last_kernels()
    finally:
        ctx.set_tuning()
    took = [p for p in plans if [l[0] for l in p] == got]
    assert took, (got, plans)
    cc.assert_separated(colour, took[0])
    assert len({colour[c] for c in range(nch)}) == min(nch, n_streams)
    for c in range(nch):
        ref = chains[colour[c]][0]
        if f32:
            a, b = posterior_summary(out[c]), posterior_summary(ref)
            for key in b:
                assert rel(a[key], b[key]) < 1e-5, (c, key)
        else:
            assert np.abs(out[c] - ref).max() < 1e-9 * max(1.0, np.abs(ref).max()), c
    return st, took[0]


@pytest.mark.parametrize("n,k,res,nch", [(3000, 8, 3, 8), (3000, 8, 2, 5), (700, 130, 3, 3),
                                         (5000, 33, 3, 8)])
def test_several_chains_per_pass(n, k, res, nch):
    """Streamed / LDS-pinned panels: one read of X serves up to 8 chains (gibbs_multi_kernel).
    A chain must not notice how many chains share its pass."""
    ctx = gpu_ctx()
    rng = np.random.default_rng(n + k)
    X = rng.standard_normal((n, k)) / np.sqrt(n)
    y = X @ rng.standard_normal(k) + 0.1 * rng.standard_normal(n)
    prior = (np.zeros(k), np.eye(k) * 10.0, 1.0, 0.02)
    ctx.set_problem(y, X)
    ctx.set_prior(*prior)
    T = 300
    seeds = np.arange(nch) + 3
    ctx.set_tuning(residency=res, chains_per_pass=1)
    solo, st1 = ctx.gibbs_run(nch, T, seeds=seeds)
    assert st1["chains_per_pass"] == 1
    ctx.set_tuning(residency=res, chains_per_pass=0)
    shared, st = ctx.gibbs_run(nch, T, seeds=seeds)
    ctx.set_tuning()
    assert st["residency"] == res and st["chains_per_pass"] in (2, 4, 8)
    # bit for bit: per chain the shared pass performs the operations of the single-chain kernel in
    # the same order (same groups per chain on both sides)
    assert st["groups_per_chain"] == st1["groups_per_chain"]
    assert np.array_equal(shared, solo)
    # and the replay tier through the shared pass: the oracle chain in every slot
    st_o = O.chain_setup(y, X, prior)
    Z, G = O.reference_streams(5, 6, 100, k, O.gamma_shape(st_o))
    ref, trace = O.gibbs_replay(y, X, 100, prior, Z, G, return_sigma2=True)
    W, lam, _ = ctx.basis()
    xi = O.innovations_in_basis(st_o, y, X, ref, W, lam, trace)
    ctx.set_tuning(residency=res)
    out, st = ctx.gibbs_run(4, 100, xi=np.repeat(xi[None], 4, 0), g=np.repeat(G[None], 4, 0))
    ctx.set_tuning()
    assert st["chains_per_pass"] in (2, 4)
    for c in range(4):
        assert np.abs(out[c] - ref).max() < 1e-9 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("n,k,res,nch", [(3000, 8, 3, 8), (3000, 8, 2, 5), (700, 130, 3, 3),
                                         (5000, 33, 3, 8)])
def test_several_chains_per_pass_distinct_streams(n, k, res, nch, planner, tmp_path):
    """test_several_chains_per_pass's shapes and chain counts with a different stream per slot:
    each chain of a shared pass against its own oracle chain."""
    ctx = gpu_ctx()
    rng = np.random.default_rng(n + k)
    X = rng.standard_normal((n, k)) / np.sqrt(n)
    y = X @ rng.standard_normal(k) + 0.1 * rng.standard_normal(n)
    prior = (np.zeros(k), np.eye(k) * 10.0, 1.0, 0.02)
    ctx.set_problem(y, X)
    ctx.set_prior(*prior)
    st, launches = replay_distinct_streams(ctx, planner, tmp_path, y, X, prior, np.float64, nch, 100,
                                           residency=res)
    assert st["residency"] == res and st["chains_per_pass"] in (2, 4, 8)
    assert any(l[0].startswith("gibbs_multi_kernel<") for l in launches)


def c2_like_problem(ctx, n=10000, k=32, seed=7):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, k)) / np.sqrt(n)
    y = X @ rng.standard_normal(k) + 0.1 * rng.standard_normal(n)
    ctx.set_problem(y, X)
    ctx.set_prior(np.zeros(k), np.eye(k) * 10.0, 1.0, 0.02)


def test_two_chains_per_xcd_when_more_than_eight_chains():
    """One-XCD register residency with 9 .. 15 chains: chains c and c + 8 share XCD c (two
    workgroups per CU side by side, the 128-VGPR variant of the kernel).  Every chain is
    bit-identical to the same seed run alone."""
    ctx = gpu_ctx()
    c2_like_problem(ctx)
    T = 400
    seeds = np.arange(13) + 100
    out, st = ctx.gibbs_run(13, T, seeds=seeds)
    assert st["residency"] == 1 and st["groups_per_chain"] <= 32 and st["chains_per_pass"] == 1
    assert st["launches"] == 1 and st["xcd_local_chains"] in (0, 13)
    for c in (0, 7, 8, 12):
        solo, _ = ctx.gibbs_run(1, T, seeds=seeds[c:c + 1])
        assert np.array_equal(out[c], solo[0])


@pytest.mark.parametrize("nch,cpp,launches,ask", [(64, 8, 1, 0), (19, 2, 2, 2), (37, 4, 2, 0),
                                                  (130, 8, 3, 0), (40, 4, 2, 4), (48, 8, 1, 0),
                                                  (45, 8, 2, 0)])
def test_bundles_of_chains_per_xcd(nch, cpp, launches, ask):
    """One-XCD register residency with 16 chains or more (the headline size): the resident
    panels of an XCD's 32 workgroups serve a bundle of 2 / 4 / 8 chains per pass, one bundle per
    XCD, 16 .. 64 chains per launch (gibbs_multi_kernel with bundle slots); what is left over
    runs as before.  Bundles of 2 are slower than the two-per-XCD packing and only used when
    asked for (`ask` = bmc_tuning.chains_per_pass).  Every chain -- first and last of a bundle, of a launch, and the left-overs
    -- is BIT-identical to the same seed run alone: the lane-wise group sum of the bundle kernel
    is operation for operation that of the single-chain kernel."""
    ctx = gpu_ctx()
    c2_like_problem(ctx)
    T = 300
    seeds = np.arange(nch) + 1000
    ctx.set_tuning(chains_per_pass=ask)
    out, st = ctx.gibbs_run(nch, T, seeds=seeds)
    ctx.set_tuning()
    assert st["residency"] == 1 and st["groups_per_chain"] == 32
    assert st["chains_per_pass"] == cpp and st["launches"] == launches, st
    assert st["xcd_local_chains"] in (0, nch)
    assert st["passes"] < nch * T               # a pass that serves a bundle counts once
    probe = sorted(c for c in {0, 1, cpp - 1, cpp, 8 * cpp - 1, min(8 * cpp, nch - 1), nch // 2,
                               nch - 2, nch - 1} if c < nch)
    for c in probe:
        solo, st1 = ctx.gibbs_run(1, T, seeds=seeds[c:c + 1])
        assert st1["chains_per_pass"] == 1
        assert np.array_equal(out[c], solo[0]), c
    # chains_per_pass = 1 switches the bundles off: the 16-per-launch packing of round 2
    ctx.set_tuning(chains_per_pass=1)
    off, st_off = ctx.gibbs_run(min(nch, 20), T, seeds=seeds[:20])
    ctx.set_tuning()
    assert st_off["chains_per_pass"] == 1
    assert np.array_equal(off, out[:min(nch, 20)])


@pytest.mark.parametrize("n,k,dt", [(10000, 32, np.float64), (9000, 16, np.float32), (5000, 20, np.float64),
                                    (8000, 32, np.float32), (10100, 16, np.float64)])
def test_bundles_of_eight_balanced_and_one_panel_layouts_agree(n, k, dt):
    """Bundles of 8 chains with at most 5 panels per workgroup run in the balanced layout (every
    wave holds two panels: 4 chains of panel w % 4 and one chain of the fifth,
    PanelStore::partial_rss_reg_bal); panels_per_wave = 1 keeps the one-panel-per-wave layout.
    Both must give the same bits (the lane-wise group sum is indexed by panel in both), ragged
    last groups included (N = 5000: 3 panels at most; N = 10100: the last group has fewer)."""
    ctx = gpu_ctx()
    rng = np.random.default_rng(3 * n + k)
    X = (rng.standard_normal((n, k)) / np.sqrt(n)).astype(dt)
    y = (X.astype(np.float64) @ rng.standard_normal(k) + 0.1 * rng.standard_normal(n)).astype(dt)
    ctx.set_problem(y, np.asfortranarray(X), dtype=dt)
    ctx.set_prior(np.zeros(k), np.eye(k) * 10.0, 1.0, 0.02)
    T, nch = 250, 64
    seeds = np.arange(nch) + 5
    bal, st = ctx.gibbs_run(nch, T, seeds=seeds)
    ctx.set_tuning(panels_per_wave=1)
    one, st1 = ctx.gibbs_run(nch, T, seeds=seeds)
    ctx.set_tuning()
    for s_ in (st, st1):
        assert s_["residency"] == 1 and s_["chains_per_pass"] == 8 and s_["launches"] == 1, s_
    assert st["groups_per_chain"] == st1["groups_per_chain"]
    assert np.isfinite(bal).all()
    assert np.array_equal(bal, one)
    solo, _ = ctx.gibbs_run(1, T, seeds=seeds[41:42])
    assert np.array_equal(bal[41], solo[0])


@pytest.mark.parametrize("n,k,dt", [(10000, 8, np.float64), (10000, 64, np.float64), (9000, 16, np.float32),
                                    (12000, 64, np.float32), (5000, 20, np.float64)])
def test_bundles_other_widths_and_storage(n, k, dt):
    """The bundle kernel's other instantiations (8 / 16 / 32 / 64 columns, f32 storage; 64 columns
    load the chains' u in two chunks; N = 5000 leaves some waves without a panel of their own and
    several sharing the last one): 64 chains in one launch, probes bit-identical to solo runs."""
    ctx = gpu_ctx()
    rng = np.random.default_rng(n + k)
    X = (rng.standard_normal((n, k)) / np.sqrt(n)).astype(dt)
    y = (X.astype(np.float64) @ rng.standard_normal(k) + 0.1 * rng.standard_normal(n)).astype(dt)
    ctx.set_problem(y, np.asfortranarray(X), dtype=dt)
    ctx.set_prior(np.zeros(k), np.eye(k) * 10.0, 1.0, 0.02)
    T, nch = 200, 64
    seeds = np.arange(nch) + 77
    out, st = ctx.gibbs_run(nch, T, seeds=seeds)
    assert st["residency"] == 1 and st["chains_per_pass"] == 8 and st["launches"] == 1, st
    assert np.isfinite(out).all()
    for c in (0, 7, 8, 33, 63):
        solo, st1 = ctx.gibbs_run(1, T, seeds=seeds[c:c + 1])
        assert st1["groups_per_chain"] == st["groups_per_chain"]
        assert np.array_equal(out[c], solo[0]), (c, st, st1)


def test_bundles_replay_the_reference_chain():
    """The reference's own C2 chain (golden fixture, its innovations expressed in the library's
    basis) replayed in all 32 slots of a launch of bundles (4 chains per XCD): every slot must
    reproduce it (T2 bar) and all slots must agree bit for bit."""
    ctx = gpu_ctx()
    g, y, X, prior = golden_case("gibbs_c2_10000x32")
    ctx.set_problem(y, X)
    ctx.set_prior(*prior)
    T = int(g["T"])
    st, xi, ref = replay_inputs(ctx, g, y, X, prior, T)
    nch = 32
    out, stats = ctx.gibbs_run(nch, T, xi=np.repeat(xi[None], nch, 0), g=np.repeat(g["G"][None, :T], nch, 0))
    assert stats["chains_per_pass"] == 4 and stats["launches"] == 1 and stats["residency"] == 1
    for c in range(nch):
        assert np.array_equal(out[c], out[0])
    assert np.abs(out[0] - ref).max() < 1e-9 * max(1.0, np.abs(ref).max())
    Vt_hat = (g["Vt"] / g["S_hat"][:, None]) if "Vt" in g else None
    a, b = posterior_summary(out[0], Vt_hat), posterior_summary(ref, Vt_hat)
    for key in b:
        assert rel(a[key], b[key]) < REL_BAR, key


@pytest.mark.parametrize("nch,cpp", [(32, 4), (64, 8), (19, 2)])
def test_bundles_replay_distinct_streams(nch, cpp, planner, tmp_path):
    """The C2 fixture's problem in a launch of bundles (4 chains per XCD as above, the balanced
    bundles of 8, and bundles of 2 with a remainder launch), a different stream in the first, a
    middle and the last slot of every bundle and launch, each slot against its own oracle chain."""
    ctx = gpu_ctx()
    g, y, X, prior = golden_case("gibbs_c2_10000x32")
    ctx.set_problem(y, X)
    ctx.set_prior(*prior)
    tune = dict(chains_per_pass=2) if cpp == 2 else {}
    st, launches = replay_distinct_streams(ctx, planner, tmp_path, y, np.asarray(X, float), prior, np.float64,
                                           nch, 130, **tune)
    assert st["chains_per_pass"] == cpp and st["residency"] == 1
    assert launches[0][3] == cpp and "true" in launches[0][0]   # (slotted bundles)


@pytest.mark.parametrize("n,k,dt,nch", [(100000, 32, np.float64, 8), (120000, 7, np.float64, 5),
                                        (200000, 64, np.float32, 8), (150000, 20, np.float32, 4)])
def test_several_chains_per_pass_register_residency(n, k, dt, nch):
    """Whole-chip register residency (one panel per wave, the chain spread over all XCDs): the
    resident panels serve up to 8 chains per pass.  Each chain must reproduce, to rounding of the
    exchange-free arithmetic, what it draws when it has the chip to itself, and the replayed
    oracle chain (float64 storage) in every slot."""
    ctx = gpu_ctx()
    rng = np.random.default_rng(n + k)
    X = (rng.standard_normal((n, k)) / np.sqrt(n)).astype(dt)
    y = (X.astype(np.float64) @ rng.standard_normal(k) + 0.1 * rng.standard_normal(n)).astype(dt)
    prior = (np.zeros(k), np.eye(k) * 10.0, 1.0, 0.02)
    ctx.set_problem(y, np.asfortranarray(X), dtype=dt)
    ctx.set_prior(*prior)
    T = 300
    seeds = np.arange(nch) + 11
    ctx.set_tuning(residency=1, chains_per_pass=1)
    solo, st1 = ctx.gibbs_run(nch, T, seeds=seeds)
    assert st1["chains_per_pass"] == 1 and st1["residency"] == 1
    ctx.set_tuning(residency=1, chains_per_pass=0)
    shared, st = ctx.gibbs_run(nch, T, seeds=seeds)
    ctx.set_tuning()
    assert st["residency"] == 1 and st["chains_per_pass"] in (2, 4, 8)
    assert st["launches"] < st1["launches"]
    # bit for bit (one row per lane: the shared pass reduces lane-wise exactly like the
    # single-chain kernel; two rows per lane: a wave sum per wave on both sides)
    assert st["groups_per_chain"] == st1["groups_per_chain"]
    assert np.array_equal(shared, solo)
    if dt == np.float64:
        Xd, yd = X.astype(np.float64), y.astype(np.float64)
        st_o = O.chain_setup(yd, Xd, prior)
        Z, G = O.reference_streams(5, 6, 60, k, O.gamma_shape(st_o))
        ref, trace = O.gibbs_replay(yd, Xd, 60, prior, Z, G, return_sigma2=True)
        W, lam, _ = ctx.basis()
        xi = O.innovations_in_basis(st_o, yd, Xd, ref, W, lam, trace)
        out, st = ctx.gibbs_run(4, 60, xi=np.repeat(xi[None], 4, 0), g=np.repeat(G[None], 4, 0))
        assert st["chains_per_pass"] in (2, 4) and st["residency"] == 1
        for c in range(4):
            assert np.abs(out[c] - ref).max() < 1e-9 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("n,k,dt,nch", [(100000, 32, np.float64, 8), (120000, 7, np.float64, 5),
                                        (200000, 64, np.float32, 8), (150000, 20, np.float32, 4)])
def test_several_chains_per_pass_register_residency_distinct_streams(n, k, dt, nch, planner, tmp_path):
    """test_several_chains_per_pass_register_residency's shapes, storage types and chain counts
    with a different stream per slot, each chain against its own oracle chain (f32 storage: the
    oracle on the f32-rounded data, summary bar 1e-5)."""
    ctx = gpu_ctx()
    rng = np.random.default_rng(n + k)
    X = (rng.standard_normal((n, k)) / np.sqrt(n)).astype(dt)
    y = (X.astype(np.float64) @ rng.standard_normal(k) + 0.1 * rng.standard_normal(n)).astype(dt)
    prior = (np.zeros(k), np.eye(k) * 10.0, 1.0, 0.02)
    ctx.set_problem(y, np.asfortranarray(X), dtype=dt)
    ctx.set_prior(*prior)
    st, launches = replay_distinct_streams(ctx, planner, tmp_path, y, X, prior, dt, nch, 60)
    assert st["residency"] == 1 and st["chains_per_pass"] in (2, 4, 8)
    assert any(l[0].startswith("gibbs_multi_kernel<") for l in launches)


@pytest.mark.parametrize("n,k,dt,res", [(200000, 64, np.float32, 1), (50000, 256, np.float64, 3),
                                        (210000, 256, np.float32, 3)])
def test_full_size_c4_c5_properties(n, k, dt, res):
    """BASELINE configs C4 (N = 200000, K = 64, float32 storage, panels in registers across the
    chip) and C5 (N = 50000, K = 256, streamed, 8 chains per pass) at full width, and a 215 MB
    matrix (beyond the 190 MB that the streaming loop keeps cached: its last panels are read
    with non-temporal loads): the posterior
    mean of beta equals the closed-form conditional mean averaged over the sigma2 draws, sigma
    recovers the generating noise level, chains agree, and the recorded sigma of every row is
    consistent with an independent residual pass over the recorded beta."""
    ctx = gpu_ctx()
    rng = np.random.Generator(np.random.PCG64(8))
    X = (rng.standard_normal((n, k)) / np.sqrt(n)).astype(dt)
    beta = rng.standard_normal(k)
    y = (X.astype(np.float64) @ beta + 0.1 * rng.standard_normal(n)).astype(dt)
    ctx.set_problem(y, np.asfortranarray(X), dtype=dt)
    prior = (np.zeros(k), np.eye(k) * 100.0, 1.0, 0.02)
    ctx.set_prior(*prior)
    T, C = 1500, 8
    out, st = ctx.gibbs_run(C, T, seeds=np.arange(C) + 1)
    assert st["residency"] == res and np.isfinite(out).all()
    if res == 3:
        assert st["chains_per_pass"] == 8 and st["launches"] == 1
    s = out[:, 300:]
    assert abs(s[..., -1].mean() - 0.1) < 2e-3
    pooled = s.reshape(-1, k + 1)
    sig2 = pooled[::601, -1] ** 2
    means = np.mean([ctx.conditional_moments(v)[0] for v in sig2[:12]], axis=0)
    se = pooled[:, :-1].std(0) / np.sqrt(len(pooled))
    assert np.all(np.abs(pooled[:, :-1].mean(0) - means) < 6 * se + 1e-9)
    m = s.mean(1)
    assert np.all(np.abs(m[:, :-1] - m[:, :-1].mean(0)).max(0) < 8 * se * np.sqrt(C))
    # rss(beta_t) through the stand-alone residual kernel bounds sigma_{t}: the Gibbs draw is
    # sigma2_t = (nu0 s20 + rss(beta_t)) / (2 g_t) with g_t ~ Gamma((nu0+n)/2): ratio ~ 1 +- few/sqrt(n)
    rows = out[0, [10, 500, 1499]]
    rss = ctx.residual_rss(rows[:, :-1])
    ratio = rows[:, -1] ** 2 / ((0.02 + rss) / (1.0 + n))
    assert np.all(np.abs(ratio - 1) < 8 / np.sqrt(n / 2))
