"""Device-generated variates and device-RNG runs pinned to the host reference (-m gpu).

Everything between "Philox bits" (tests/test_rng_gpu.py, bit for bit) and "a chain, a simplex walk
or a predictive draw" is a deterministic function of those bits, so it is checked element by
element here, not by distribution:

  A  the fill kernels (normal_fill_kernel, gamma_fill_kernel) against tests/rng_reference.py and
     against the CPU build of bmc_math.h, across the capacity of their capped grids;
  B  device-mode gibbs_run == replay-mode gibbs_run fed by the fill kernels, per kernel family,
     and one case end to end against the numpy oracle on the reference's variates;
  C  the same for the simplex sampler, whose third stream (uniforms) has no entry point of its
     own and comes from the reference;
  D  the predictive noise against the (point, draw) formula of the reference.

tests/test_rng_reference_host.py guards the reference itself on the CPU, including the condition
that lets A compare EVERY gamma variate (no element within 1e-9 of an accept / reject boundary).

Not covered, and why: the counter's high word (pair >> 32) needs more than 2^33 variates per chain
(64 GB); the predictive counter stays below 2^32 even at 10 000 draws x 50 000 points; the
64-attempt fall-through of the gamma sampler has probability about 0.03^64.  These paths are not
faked here.
"""
import functools

import numpy as np
import pandas as pd
import pytest

import rng_host_build as H
import rng_reference as R
from conftest import load_golden
from gpu_common import golden_case, gpu_ctx
from oracle import bmc_oracle as O
from pybmc_amd import coverage

pytestmark = pytest.mark.gpu

U52 = 2.0 ** -52
SEEDS = [0, 12345, 2 ** 32 + 7, 2 ** 64 - 1]
N_MAX = 2_100_001


# ------------------------------------------------------------------------------------------
# A. fill kernels
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_normals(seed):
    """(long-double reference, CPU build of bmc_math.h) of the longest case; both are prefix-stable
    (tests/test_rng_reference_host.py), shorter cases slice them."""
    return R.normals(seed, N_MAX), H.normals(seed, N_MAX)


@pytest.mark.parametrize("seed", SEEDS)
def test_normal_fill_matches_the_reference(seed):
    """n = 1, 2, 3, 1001 (odd tails), 1 048 576 + 3 and 2 100 001: the grid is capped at 2048 x 256
    threads, one Box-Muller pair each, so 1 048 576 elements are its exact capacity and the two
    long cases cross one and two wraps of the stride loop.  Bit for bit the CPU build of
    bmc_math.h ("the same bits"), and within 4 units of 2^-52 |z| of the long-double reference:
    the 1.98 of the CPU build plus one ulp each for a device sqrt and division that need not be
    correctly rounded.  Observed on an MI355X: DESIGN.md, "Variate streams"."""
    ctx = gpu_ctx()
    ref, cpu = host_normals(seed)
    for n in (1, 2, 3, 1001, 1_048_576 + 3, N_MAX):
        z, _ = ctx.rng_fill(seed, n_normal=n)
        assert z.shape == (n,)
        d = np.abs(z.astype(R.LD) - ref[:n]) / np.abs(ref[:n])
        worst = float(d.max()) / U52
        differ = int((z != cpu[:n]).sum())
        print(f"normals seed {seed} n {n}: {worst:.3f} units of 2^-52 |z| from the reference, "
              f"{differ} elements differ from the CPU build")
        assert worst <= 4.0, (seed, n, int(d.argmax()))
        assert np.array_equal(z, cpu[:n]), (seed, n, differ)


@pytest.mark.parametrize("shape", R.GAMMA_SHAPES)
def test_gamma_fill_matches_the_reference(shape):
    """600 001 elements (past the 524 288 of the capped grid) per shape, every element compared
    (tests/test_rng_reference_host.py: none is near a decision boundary); the value implies the
    number of attempts.  Bar: relative 16 x 2^-52 -- a 4-unit x enters v = (1 + c x)^3 with the
    factor 3 |c x / (1 + c x)|, at most 3 while 1 + c x >= 1/2, plus the roundings of the cube,
    of d v and of the power -- and, only for the elements whose factor exceeds that, the
    propagated error 3 x 4 x 2^-52 |c x / (1 + c x)| itself."""
    ctx = gpu_ctx()
    ref, attempts, margin, amp = R.gammas(R.GAMMA_SEED, shape, R.GAMMA_N, detail=True)
    assert int((margin < R.MARGIN_FLOOR).sum()) == 0
    _, g = ctx.rng_fill(R.GAMMA_SEED, shape=shape, n_gamma=R.GAMMA_N)
    rel = np.abs(g - ref) / ref
    bar = np.maximum(16.0, 12.0 * amp) * U52
    i = int((rel / bar).argmax())
    print(f"gammas shape {shape}: worst {rel.max() / U52:.3f} units of 2^-52 relative "
          f"(element {int(rel.argmax())}, {attempts[rel.argmax()]} attempts); worst against its bar: "
          f"element {i}, {rel[i] / U52:.3f} of {bar[i] / U52:.1f}; {int((amp > 4 / 3).sum())} elements "
          f"on the propagated bound")
    assert np.all(rel <= bar), (shape, i, rel[i] / U52, bar[i] / U52, int(attempts[i]))
    # a second seed with both key words non-zero, and the chain's own prefix
    seed2 = 2 ** 32 + 7
    ref2, _, margin2, amp2 = R.gammas(seed2, shape, 5000, detail=True)
    assert margin2.min() >= R.MARGIN_FLOOR        # (3e-5 at the least over the shapes)
    _, g2 = ctx.rng_fill(seed2, shape=shape, n_gamma=5000)
    assert np.all(np.abs(g2 - ref2) / ref2 <= np.maximum(16.0, 12.0 * amp2) * U52)
    _, g3 = ctx.rng_fill(R.GAMMA_SEED, shape=shape, n_gamma=1000)
    assert np.array_equal(g3, g[:1000])


# ------------------------------------------------------------------------------------------
# B. device mode is replay mode fed by the fill kernels
# ------------------------------------------------------------------------------------------
def same_or_close(ctx_kernels_a, ctx_kernels_b, a, b):
    """array_equal where both runs launched the same kernels, else the suite's bar between
    geometries."""
    if ctx_kernels_a == ctx_kernels_b:
        assert np.array_equal(a, b), float(np.abs(a - b).max())
    else:
        assert np.abs(a - b).max() < 1e-11 * max(1.0, np.abs(b).max())


def device_vs_replay(ctx, seeds, T, nu0, **tune):
    """gibbs_run(seeds) against gibbs_run(xi, g) with every chain's variates fetched from the
    fill kernels under that chain's seed.  Returns (device chains, stats, kernel names)."""
    seeds = np.asarray(seeds, dtype=np.uint64)
    C, K = len(seeds), ctx.k
    shape = (nu0 + ctx.n) / 2.0
    ctx.set_tuning(**tune)
    try:
        dev, st = ctx.gibbs_run(C, T, seeds=seeds)
        kd = ctx.last_kernels()
        xi, g = np.empty((C, T, K)), np.empty((C, T))
        for c, s in enumerate(seeds):
            z, gg = ctx.rng_fill(int(s), n_normal=T * K, shape=shape, n_gamma=T)
            xi[c], g[c] = z.reshape(T, K), gg
        rep, st2 = ctx.gibbs_run(C, T, xi=xi, g=g)
        kr = ctx.last_kernels()
    finally:
        ctx.set_tuning()
    assert np.isfinite(dev).all() and st["launches"] == st2["launches"]
    same_or_close(kd, kr, dev, rep)
    return dev, st, kd


def synth(n, k, seed, dt=np.float64):
    rng = np.random.default_rng([n, k, seed])
    X = (rng.standard_normal((n, k)) / np.sqrt(n)).astype(dt)
    y = (X.astype(np.float64) @ rng.standard_normal(k) + 0.1 * rng.standard_normal(n)).astype(dt)
    return y, X, (np.zeros(k), np.eye(k) * 10.0, 1.0, 0.02)


def mixed_seeds(C):
    """Distinct seeds, one duplicate pair in the launch (where C allows), one seed >= 2^32."""
    s = [int(v) for v in np.arange(C) * 7919 + 5]
    s[-1] = 2 ** 32 + 11
    if C >= 3:
        s[C // 2] = s[0]
    return s


# (n, k, chains, T, tuning, storage, kernel family the launches must come from, launches)
FAMILIES = {
    "one_wave": (629, 3, 5, 200, dict(waves_per_group=1), np.float64, "gibbs_wave_kernel<", 1),
    "four_waves": (2500, 8, 3, 200, {}, np.float64, "gibbs_wave_kernel<", 1),
    "workgroup": (3000, 8, 3, 200, dict(waves_per_group=8), np.float64, "gibbs_loop_kernel<", 1),
    "c2_one_chain": (10000, 32, 1, 200, {}, np.float64, "gibbs_loop_kernel<", 1),
    "c2_bundles": (10000, 32, 16, 130, dict(chains_per_pass=2), np.float64, "gibbs_multi_kernel<", 1),
    "shared_pass": (3000, 8, 8, 200, dict(residency=3), np.float64, "gibbs_multi_kernel<", 1),
    "several_launches": (20000, 6, 19, 130, {}, np.float64, "gibbs_loop_kernel<", 3),
    "rss_mode_1": (10000, 32, 5, 200, dict(rss_mode=1), np.float64, None, 1),
    "f32_storage": (629, 3, 4, 200, {}, np.float32, "gibbs_wave_kernel<float", 1),
}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_device_mode_is_replay_of_the_fill_kernels(family):
    """With A this pins every device chain to the host reference: chain c of a device-mode run
    consumes elements [0, T K) of the normal stream and [0, T) of the gamma stream (shape
    (nu0 + n) / 2) of ITS seed, whatever its index, launch, bundle or neighbours."""
    n, k, C, T, tune, dt, prefix, launches = FAMILIES[family]
    ctx = gpu_ctx()
    y, X, prior = synth(n, k, 1, dt)
    ctx.set_problem(y, np.asfortranarray(X), dtype=dt)
    ctx.set_prior(*prior)
    seeds = mixed_seeds(C)
    dev, st, kernels = device_vs_replay(ctx, seeds, T, prior[2], **tune)
    if prefix is None:
        assert kernels == [] and st["residency"] == 4
    else:
        assert kernels and all(name.startswith(prefix) for name in kernels), kernels
    assert st["launches"] >= launches, st
    if C >= 3:       # equal seeds, equal chains; different seeds, different chains
        assert np.array_equal(dev[C // 2], dev[0])
        assert np.abs(dev[C - 1] - dev[0]).max() > 1e-3


@pytest.mark.parametrize("family", ["one_wave", "workgroup", "shared_pass"])
def test_device_mode_prefix_is_stable(family):
    """The first 100 rows of a T = 400 run are the T = 100 run: the variates of iteration t do not
    depend on T (per-chain buffers are [chain][T K] and [chain][T])."""
    n, k, C, _, tune, dt, _, _ = FAMILIES[family]
    ctx = gpu_ctx()
    y, X, prior = synth(n, k, 1, dt)
    ctx.set_problem(y, np.asfortranarray(X), dtype=dt)
    ctx.set_prior(*prior)
    seeds = np.asarray(mixed_seeds(C), dtype=np.uint64)
    ctx.set_tuning(**tune)
    try:
        long_run, _ = ctx.gibbs_run(C, 400, seeds=seeds)
        kl = ctx.last_kernels()
        short_run, _ = ctx.gibbs_run(C, 100, seeds=seeds)
        ks = ctx.last_kernels()
    finally:
        ctx.set_tuning()
    same_or_close(kl, ks, long_run[:, :100], short_run)


def test_device_chain_end_to_end_against_the_oracle():
    """Host reference -> numpy oracle -> chain, no device variate involved: the oracle runs on
    rng_reference's normals and gammas, its draw mapped into the library's basis (beta = mean +
    W (sqrt(d) xi), cov = W diag(d) W', the inverse of what replay_inputs does), and the device
    chain of the same seed must be that chain at the replay bar."""
    ctx = gpu_ctx()
    g, y, X, prior = golden_case("gibbs_ortho629x3")
    Xf = np.asarray(X, float)
    ctx.set_problem(y, X)
    ctx.set_prior(*prior)
    T, K = 300, Xf.shape[1]
    W, lam, _ = ctx.basis()
    Winv = np.linalg.inv(W)
    st = O.chain_setup(y, Xf, prior)
    for seed in (12345, 2 ** 32 + 7):
        xi = R.normals(seed, T * K).astype(np.float64).reshape(T, K)
        G, _, margin = R.gammas(seed, O.gamma_shape(st), T)
        assert margin.min() >= R.MARGIN_FLOOR
        real = O.mvn_draw_svd
        O.mvn_draw_svd = lambda mean, cov, z: mean + W @ (np.sqrt(np.diag(Winv @ cov @ Winv.T)) * z)
        try:
            ref = O.gibbs_replay(y, Xf, T, prior, xi, G)
        finally:
            O.mvn_draw_svd = real
        out, _ = ctx.gibbs_run(1, T, seeds=[seed])
        err = np.abs(out[0] - ref).max()
        print(f"device chain vs oracle on reference variates, seed {seed}: {err:.3e}")
        assert err < 1e-9 * max(1.0, np.abs(ref).max())


# ------------------------------------------------------------------------------------------
# C. simplex
# ------------------------------------------------------------------------------------------
def simplex_cases():
    g = load_golden("simplex_synth150x4")
    yield "synth150x4", g["y"], g["X"], g["Vt_hat"], g["S_hat"], 0.002, 1
    n, k, km = 2500, 3, 4                      # test_simplex_gpu.py's four-wave shape
    rng = np.random.default_rng(n + k)
    A = rng.standard_normal((n, km))
    truth = A @ np.full(km, 1.0 / km) + 0.05 * rng.standard_normal(n)
    U, S, Vt = np.linalg.svd(A - A.mean(1, keepdims=True), full_matrices=False)
    yield "four_waves", truth - A.mean(1), U[:, :k], Vt[:k] / S[:k, None], S[:k], 0.001, 4


@pytest.mark.parametrize("case", ["synth150x4", "four_waves"])
def test_simplex_device_mode_is_replay_of_the_streams(case):
    """simplex_run(seed) against simplex_run(xi, unif, g).  The kernel indexes the uniform stream
    by CONSUMPTION (a running counter advanced only by proposals inside the simplex), as replay
    semantics say, so device mode is the replay of uniforms(seed, burn + T).  First with the
    normals and gammas of the fill kernels (A pins them) and the reference's uniforms: same
    kernel, same bits.  Then with all three streams from the reference: the same decisions, and
    the chain at the simplex replay tier's 1e-9 (its variates differ from the device's by the few
    units of 2^-52 A measures, so bit equality is not to be had there)."""
    name, y, X, Vt_hat, S_hat, stepsize, nw = next(c for c in simplex_cases() if c[0] == case)
    ctx = gpu_ctx()
    ctx.set_problem(y, X)
    n, k = X.shape
    nu0, s20, burn, T = 1.0, 0.02, 300, 1000
    tt = burn + T
    shape = (nu0 + n) / 2.0
    for seed in (7, 2 ** 32 + 7):
        out, acc, used, st = ctx.simplex_run(Vt_hat, S_hat, T, nu0, s20, burn, stepsize, seed=seed,
                                             return_stats=True)
        kd = ctx.last_kernels()
        assert st["waves_per_group"] == nw and 0 < acc < T and 0 < used <= tt, (st, acc, used)
        if case == "synth150x4":   # proposals do leave the simplex: consumption lags the iteration
            assert used < tt - 50
        unif = R.uniforms(seed, tt)
        z, gg = ctx.rng_fill(seed, n_normal=tt * k, shape=shape, n_gamma=tt)
        rep, acc2, used2, _ = ctx.simplex_run(Vt_hat, S_hat, T, nu0, s20, burn, stepsize,
                                              xi=z.reshape(tt, k), unif=unif, g=gg, return_stats=True)
        kr = ctx.last_kernels()
        assert (acc2, used2) == (acc, used)
        same_or_close(kd, kr, out, rep)
        # only what was consumed matters: the uniforms past `used` are never read
        cut, acc3, used3, _ = ctx.simplex_run(Vt_hat, S_hat, T, nu0, s20, burn, stepsize,
                                              xi=z.reshape(tt, k), unif=unif[:used], g=gg,
                                              return_stats=True)
        assert (acc3, used3) == (acc, used) and np.array_equal(cut, rep)
        # all three streams from the host reference
        G, _, margin = R.gammas(seed, shape, tt)
        assert margin.min() >= R.MARGIN_FLOOR
        xi = R.normals(seed, tt * k).astype(np.float64).reshape(tt, k)
        ref, acc4, used4, _ = ctx.simplex_run(Vt_hat, S_hat, T, nu0, s20, burn, stepsize,
                                              xi=xi, unif=unif, g=G, return_stats=True)
        assert (acc4, used4) == (acc, used)
        err = np.abs(out - ref).max()
        print(f"simplex {name} seed {seed}: accepted {acc}, uniforms used {used}, "
              f"device mode vs reference streams {err:.3e}")
        assert err < 1e-9
        # and through the numpy oracle (the diagonal proposal map of the library)
        real = O.mvn_draw_svd
        step = S_hat * stepsize
        O.mvn_draw_svd = lambda mean, cov, zz: mean + step * zz
        try:
            oref, oacc, oused = O.simplex_replay(y, X, Vt_hat, S_hat, T, [nu0, s20], burn, stepsize,
                                                 xi, unif, G)
        finally:
            O.mvn_draw_svd = real
        assert (oacc, oused) == (acc, used)
        assert np.abs(out - oref).max() < 1e-9


# ------------------------------------------------------------------------------------------
# D. predictive noise
# ------------------------------------------------------------------------------------------
PREDICT_SHAPES = [(1, 2, 1, 64), (65, 5, 3, 1000), (130, 33, 32, 10000), (7, 257, 9, 4097),
                  (200, 4, 2, 2048), (13, 6, 3, 100)]


@pytest.mark.parametrize("M,Km,k,S", PREDICT_SHAPES)
def test_predict_device_noise_is_the_reference_noise(M, Km, k, S):
    """predict(seed) against predict(noise = predict_noise(seed, S, M)): entry (draw s, point p)
    is half (p >> 2) & 1 of the pair of counter (p - 4 ((p >> 2) & 1)) S + s, whatever the tile.
    (13, 6, 3, 100): M is no multiple of 8 and S none of 64, so the sine halves of points 8 .. 12
    and the counters of columns 100 .. 127 fall into the padding."""
    ctx = gpu_ctx()
    rng = np.random.default_rng(M + Km)
    preds = rng.standard_normal((M, Km)) + 3
    theta = np.column_stack([rng.standard_normal((S, k)) * 0.1, rng.uniform(0.5, 1.5, S)])
    Vt = rng.standard_normal((k, Km))
    truth = preds.mean(1) + rng.standard_normal(M)
    pct = np.arange(0, 101, 5)
    q = (2.5, 50, 97.5, 0, 100, 33.3)
    for seed in (11, 2 ** 32 + 7):
        dev, bands, cov = ctx.predict(preds, theta, Vt, seed=seed, q=q, truth=truth, cov_percentiles=pct)
        assert dev.shape == (S, M)
        # the CPU build of the transform: the bits the device computes (A), so the same draws
        cpu, _, _ = ctx.predict(preds, theta, Vt, noise=H.predict_noise(seed, S, M), q=q)
        assert np.array_equal(dev, cpu), float(np.abs(dev - cpu).max())
        # the long-double reference, rounded: the replay tier's bar
        ref, _, _ = ctx.predict(preds, theta, Vt, q=q,
                                noise=R.predict_noise(seed, S, M).astype(np.float64))
        assert np.abs(dev - ref).max() < 1e-12 * np.abs(ref).max()
        # bands and coverage are numpy's on the returned draws
        assert np.array_equal(bands, np.percentile(dev, q, axis=0))
        assert coverage(pct, dev, pd.DataFrame({"truth": truth}), "truth") == cov


@pytest.mark.parametrize("M,S", [(96, 10000), (200, 2048), (13, 100), (130, 1000)])
def test_predict_noise_matrix_has_no_counter_collisions(M, S):
    """Zero weights and preds = 0 isolate the noise: draws / sigma IS the noise matrix (sigma = 2,
    exact).  No two of its entries are equal -- a 53-bit stream makes a repeat practically
    impossible, a counter shared by two (point, draw) entries makes it certain -- and every entry
    is the reference's."""
    ctx = gpu_ctx()
    Km, k, seed = 4, 2, 2 ** 32 + 7
    theta = np.column_stack([np.zeros((S, k)), np.full(S, 2.0)])
    dev, _, _ = ctx.predict(np.zeros((M, Km)), theta, np.zeros((k, Km)), seed=seed, q=())
    z = dev / 2.0
    assert len(np.unique(z)) == z.size
    assert len(np.unique(np.abs(z))) == z.size          # nor equal up to the sign
    assert np.array_equal(z, H.predict_noise(seed, S, M))
    ref = R.predict_noise(seed, S, M)
    worst = float((np.abs(z.astype(R.LD) - ref) / np.abs(ref)).max()) / U52
    print(f"predictive noise {S} x {M}: {worst:.3f} units of 2^-52 |z| from the reference")
    assert worst <= 4.0
