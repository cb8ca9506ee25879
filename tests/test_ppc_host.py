"""CPU checks of the posterior predictive check (pybmc_amd.ppc, kernels_ppc.hip): argument
validation without a device, ppc_summary against a hand case, the fifth variate stream of
ppc_reference.py (moments, pair structure, independence of the draw count), the margin proof that
lets test_ppc_gpu.py demand equal p-values, and the public surface."""
import os

import numpy as np
import pytest

import ppc_reference as P
import rng_reference as G

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- arguments -------------------------------------------------------------------------------------
def test_every_bad_argument_is_a_value_error_before_any_gpu_work():
    """No GPU is needed for any of these: on a machine without one a call that reached the device
    would raise BmcError, not ValueError."""
    from pybmc_amd import posterior_predictive_check as ppc
    A = np.zeros((5, 3))
    y = np.zeros(5)
    th = np.ones((10, 4))
    bad = [
        ((np.zeros((2, 3)), np.zeros(2), th), {}, "at least 3 points"),
        ((np.zeros((0, 3)), np.zeros(0), th), {}, "at least one point"),
        ((np.zeros((5, 257)), y, np.ones((10, 258))), {}, "k must be"),
        ((np.zeros((5, 3), dtype=np.float32), y, th), {}, "float64"),
        ((A, y.astype(np.float32), th), {}, "float64"),
        ((A, y, th.astype(np.float32)), {}, "float64"),
        ((A, np.zeros(4), th), {}, "y must be"),
        ((A, y, np.ones((10, 5))), {}, "columns"),
        ((A, y, np.ones((1, 4))), {}, "at least 2 draws"),
        ((A, y, np.ones(4)), {}, "dimensions"),
        ((np.zeros(5), y, th), {}, "dimensions"),
        ((A, y, th), {"burn": 9}, "at least 2 draws"),
        ((A, y, th), {"burn": -1}, "burn"),
        ((A, y, th), {"thin": 0}, "thin"),
        ((A, y, th), {"offset": np.zeros(4)}, "offset must be"),
        ((A, y, th), {"offset": np.zeros((5, 1))}, "offset must be"),
        ((A, y, th), {"offset": np.zeros(5, dtype=np.float32)}, "offset must be float64"),
        ((A, y, th), {"seed": -1}, "seed"),
        ((A, y, th), {"seed": 2 ** 64}, "seed"),
        ((A, y, th), {"seed": 1.5}, "seed"),
    ]
    for args, kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            ppc(*args, **kw)


def test_scoring_messages_are_unchanged_by_the_shared_argument_handling():
    from pybmc_amd import scoring
    with pytest.raises(ValueError, match="at least one point"):
        scoring._check_shapes((0, 3), (0,), (10, 4), 0, 1)
    assert scoring._check_shapes((1, 3), (1,), (10, 4), 0, 1) == (1, 3, 1, 10, 10)
    assert scoring._check_shapes((2, 3), (2,), (2, 10, 4), 1, 2) == (2, 3, 2, 10, 5)
    with pytest.raises(ValueError, match="at least 3 points; got 2"):
        scoring._check_shapes((2, 3), (2,), (10, 4), 0, 1, 3)


def test_bmc_method_guards_call_order():
    import pandas as pd
    from pybmc_amd import BayesianModelCombination
    df = pd.DataFrame({"a": [1.0, 2.0, 3.5], "b": [1.5, 2.5, 3.0], "truth": [1.2, 2.2, 3.1]})
    bmc = BayesianModelCombination(["a", "b"], {"p": df}, "truth")
    with pytest.raises(ValueError, match="orthogonalize"):
        bmc.posterior_predictive_check()
    with pytest.raises(ValueError, match="orthogonalize"):
        bmc.posterior_predictive_check(df)
    bmc.orthogonalize("p", df, components_kept=1)
    with pytest.raises(ValueError, match="train"):
        bmc.posterior_predictive_check()
    bmc.samples = np.ones((10, 2))
    with pytest.raises(ValueError, match="DataFrame"):
        bmc.posterior_predictive_check(np.zeros((3, 3)))
    with pytest.raises(ValueError, match="truth column"):
        bmc.posterior_predictive_check(df[["a", "b"]])


# ---- the summary -----------------------------------------------------------------------------------
def test_ppc_summary_hand_case():
    from pybmc_amd import PPC_STATS, ppc_summary
    assert PPC_STATS == P.PPC_STATS == ("min", "max", "mean", "sd", "skew", "kurt", "chi2", "max_abs_z")
    t_rep = np.zeros((4, 8))
    t_obs = np.zeros((4, 8))
    t_rep[:, 0] = [1, 2, 3, 4]
    t_obs[:, 0] = 2.5                      # two of four at or above
    t_rep[:, 1] = [1, 2, 3, 4]
    t_obs[:, 1] = [1, 2, 3, 4]             # equality counts: 1
    t_rep[:, 2] = -1                       # never: 0
    t_rep[:, 6] = [5, 0, 0, 0]
    t_obs[:, 6] = [4, 1, 1, 1]             # per-draw T_obs: one of four
    t_rep[:, 7] = np.nan                   # a NaN is never >=
    p = ppc_summary(t_rep, t_obs)
    assert list(p) == list(PPC_STATS)
    assert p == {"min": 0.5, "max": 1.0, "mean": 0.0, "sd": 1.0, "skew": 1.0, "kurt": 1.0, "chi2": 0.25,
                 "max_abs_z": 0.0}
    assert p == P.p_values(t_rep, t_obs)
    for bad in ((np.zeros((4, 7)), np.zeros((4, 7))), (t_rep, t_obs[:3]), (np.zeros((0, 8)), np.zeros((0, 8)))):
        with pytest.raises(ValueError):
            ppc_summary(*bad)


def test_host_marginal_statistics_are_the_reference():
    from pybmc_amd.ppc import marginal_stats
    x = np.random.default_rng(3).standard_normal(629) * 2.5 + 17
    np.testing.assert_allclose(marginal_stats(x), P.marginal(x).astype(np.float64), rtol=1e-12, atol=1e-12)
    # by hand: 1, 2, 3, 6 -> mean 3, m2 3.5, m3 4.5, m4 24.5
    got = marginal_stats(np.array([1.0, 2.0, 3.0, 6.0]))
    np.testing.assert_allclose(got, [1, 6, 3, np.sqrt(3.5), 4.5 / 3.5 ** 1.5, 24.5 / 3.5 ** 2 - 3], rtol=1e-15)


# ---- the fifth stream ------------------------------------------------------------------------------
def test_stream_id_and_pair_layout():
    assert P.STREAM_PPC == int.from_bytes(b"PPCS", "big") == 0x50504353
    assert P.STREAM_PPC not in (G.STREAM_NORMAL, G.STREAM_GAMMA, G.STREAM_PRED_NORMAL, G.STREAM_UNIFORM)
    i = np.arange(200)
    pair, half = P.pair_index(i), P.half_index(i)
    assert list(pair[:34]) == list(range(32)) + [0, 1] and pair[64] == 32 and pair[127] == 63
    assert list(half[[0, 31, 32, 63, 64, 96]]) == [0, 0, 1, 1, 0, 1]
    # points i and i + 32 of a tile share a counter and take different halves; nothing else shares
    lo = i[half == 0]
    for a in lo:
        if a + 32 < 200:
            assert pair[a] == pair[a + 32] and half[a + 32] == 1
    key = pair * 2 + half.astype(np.uint64)
    assert len(np.unique(key)) == 200


def test_points_32_apart_are_the_two_halves_of_one_box_muller_pair():
    seed, n, draws = 77, 100, np.arange(5)
    z = P.noise(seed, n, draws)
    index, sub = P.noise_counters(n, draws)
    u1, u2 = G.pair_uniforms(G.stream_words(seed, index, P.STREAM_PPC, sub))
    z0, z1, rad = G.box_muller(u1, u2)
    for i in (0, 5, 31, 64, 67):           # cosine-half points whose partner exists (i + 32 < 100)
        assert np.array_equal(u1[i], u1[i + 32]) and np.array_equal(u2[i], u2[i + 32])
        assert np.array_equal(z[i], z0[i]) and np.array_equal(z[i + 32], z1[i])
        np.testing.assert_allclose((z[i] ** 2 + z[i + 32] ** 2).astype(np.float64),
                                   (rad[i] ** 2).astype(np.float64), rtol=1e-15)
    # a cosine-half point whose partner is past n is simply alone: 70 + 32 > 99
    assert np.array_equal(z[70], z0[70])


def test_noise_depends_on_seed_point_and_draw_only():
    a = P.noise(5, 65, np.arange(70))
    b = P.noise(5, 65, np.arange(130))
    assert np.array_equal(a, b[:, :70])                       # not on S
    assert np.array_equal(P.noise(5, 33, np.arange(70)), a[:33])   # not on n
    assert np.array_equal(P.noise(5, 65, np.array([69, 3])), a[:, [69, 3]])
    assert not np.array_equal(P.noise(6, 65, np.arange(70)), a)
    # a draw index past 2^32 reaches the second counter word
    big = P.noise(5, 4, np.array([3, 3 + 2 ** 32]))
    assert not np.array_equal(big[:, 0], big[:, 1])


def test_noise_moments():
    z = P.noise(2024, 640, np.arange(500)).astype(np.float64)      # 320 000 variates
    n = z.size
    assert abs(z.mean()) < 4 / np.sqrt(n)
    assert abs(z.var() - 1) < 4 * np.sqrt(2 / n)
    assert abs((z ** 3).mean()) < 4 * np.sqrt(15 / n)
    assert abs((z ** 4).mean() - 3) < 4 * np.sqrt(96 / n)
    # the halves of a pair, neighbouring points and neighbouring draws are uncorrelated
    for x, w in ((z[:32], z[32:64]), (z[:-1], z[1:]), (z[:, :-1], z[:, 1:])):
        assert abs(np.mean(x * w)) < 4 / np.sqrt(x.size)


# ---- the margin proof ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", P.CASES, ids=lambda c: "n%d_k%d_S%d" % c[:3])
def test_no_statistic_of_a_gpu_case_sits_on_its_comparison(case):
    """For every GPU case no |T_rep - T_obs| / max(1, |T_rep|, |T_obs|) of the reference is under
    MARGIN_FLOOR = 1e-9, ten times the largest bar the GPU test may use: a device value within its
    bar of the reference is on the same side of T_obs, so the p-values must be EQUAL."""
    n = case[0]
    _, _, _, _, t_rep, t_obs = P.case(*case)
    assert P.MARGIN_FLOOR == 1e-9
    m = P.margins(t_rep, t_obs)
    cols = P.compared(n)
    print(case, "smallest margin", m[:, cols].min(), "per statistic", m[:, cols].min(axis=0))
    assert np.isfinite(np.asarray(t_rep, dtype=np.float64)).all()
    assert np.isfinite(np.asarray(t_obs, dtype=np.float64)).all()
    assert m[:, cols].min() >= P.MARGIN_FLOOR
    assert len(cols) == 8 - len(P.DEGENERATE.get(n, ()))


def assert_margins(cases, tag):
    worst = np.inf
    for n, S, A, y, th, off, seed, t_rep, t_obs in cases:
        assert np.isfinite(np.asarray(t_rep, dtype=np.float64)).all()
        assert np.isfinite(np.asarray(t_obs, dtype=np.float64)).all()
        assert t_rep.shape == t_obs.shape == (S, 8) and A.shape[0] == n
        worst = min(worst, P.margins(t_rep, t_obs)[:, P.compared(n)].min())
    print(tag, "smallest margin", worst)
    assert worst >= P.MARGIN_FLOOR
    return worst


@pytest.mark.parametrize("k", P.GRID_K)
def test_no_statistic_of_the_shape_grid_sits_on_its_comparison(k):
    """The same proof for the 45 (n, S) of the grid at this k (smallest margin of the whole grid:
    1.9e-7), and the table itself: n-major case numbers, seeds with a non-zero high word, an offset
    on every third case."""
    shapes = P.grid_shapes(k)
    assert len(shapes) == 45 and [c for c, _, _, _ in shapes] == list(range(45))
    assert [(n, S) for _, n, S, _ in shapes] == [(n, S) for n in P.GRID_N for S in P.GRID_S]
    assert all(d == 40000 + 100 * k + c for c, _, _, d in shapes)
    cases = [P.grid_case(k, c) for c in range(45)]
    for (c, n, S, d), got in zip(shapes, cases):
        assert got[6] == (0x9E3779B9 << 32) | (d * 2654435761 % 2 ** 32) and got[6] >> 32 != 0
        assert (got[5] is not None) == (c % 3 == 0)
    assert_margins(cases, "grid k=%d" % k)


def test_no_statistic_of_the_seed_edges_or_the_biased_fits_sits_on_its_comparison():
    assert P.SEED_EDGES == (0, 2 ** 64 - 1) and P.BIASED == (0.3, 3.0)
    assert_margins([P.seed_edge_case(s) for s in P.SEED_EDGES], "seed edges")
    assert assert_margins([P.biased_case(d) for d in P.BIASED], "biased") > 2e-5
    # the two keys are not the key of any other case, and give other variates
    a, b = (P.seed_edge_case(s)[7] for s in P.SEED_EDGES)
    assert not np.array_equal(a, b) and not np.array_equal(a, P.case(65, 3, 130, 11)[4])


@pytest.mark.parametrize("delta", P.BIASED)
def test_the_biased_fits_are_biased(delta):
    """A condition on the INPUT of the biased cases: every draw's replicated mean lies more than 10
    (delta = 0.3) or 150 (delta = 3) of the draw's sigma_s from mean(y), the scalar the power sums
    were once taken about -- and 11.8 or 119 of the replicate's own sd, whose fourth power is what
    one-pass moments about a shared centre lose of kurt."""
    n, S, A, y, th, off, seed, t_rep, t_obs = P.biased_case(delta)
    assert (n, S, A.shape, seed) == (200, 64, (200, 2), (7 << 32) | 5) and np.all(A[:, 0] == 1)
    shift = np.abs(t_rep[:, 2] - y.mean())
    in_sigma, in_sd = (shift / th[:, 2]).min(), (shift / t_rep[:, 3]).min()
    print(delta, "shift in sigma_s", in_sigma, "in sd(y_rep)", in_sd)
    assert in_sigma > P.BIASED_SD[delta] and P.BIASED_SD == {0.3: 10.0, 3.0: 150.0}
    assert in_sd > (10 if delta == 0.3 else 100)
    # the cases of CASES never see this: their draws scatter about the least-squares point
    A0, y0, _, _, r0, _ = P.case(200, 33, 257, 17)
    assert (np.abs(r0[:, 2] - y0.mean()) / r0[:, 3]).max() < 0.1


# ---- the floors --------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", P.GROUPS)
def test_floors_are_not_exceeded_when_recomputed(group):
    """FLOORS holds, per group and per value of TEN, the larger of the float64 reference's deviation
    from the long-double one and the effect of the generator's accuracy on the long-double one
    (ppc_reference.measured_floors): nothing of the device.  The GPU test's bars are 64 x these."""
    got = P.measured_floors(group)
    print(group, " ".join("%s %.2e" % kv for kv in zip(P.TEN, got)))
    assert len(P.TEN) == 10 and len(P.FLOORS[group]) == 10 and set(P.FLOORS) == set(P.GROUPS)
    for name, v, floor in zip(P.TEN, got, P.FLOORS[group]):
        assert 0 < v <= floor, (group, name, v, floor)
        assert floor <= 1.25 * v, (group, name, "the constant is looser than its provenance says")


def test_bars_are_64_floors_rounded_up_to_one_digit():
    assert P.BAR_FACTOR == 64
    assert [P.round_up_one_digit(x) for x in (9.6e-14, 1e-12, 1.01e-12, 5.2e-11, 2.3e-13)] == \
        [1e-13, 1e-12, 2e-12, 6e-11, 3e-13]
    for group in P.GROUPS:
        b = P.bars(group)
        assert tuple(b) == P.TEN
        for name, floor in zip(P.TEN, P.FLOORS[group]):
            assert 64 * floor <= b[name] < 128 * floor and b[name] <= P.MARGIN_FLOOR / 10


# ---- bad input on the reference ----------------------------------------------------------------------
def test_reference_nan_rules():
    """What test_ppc_gpu.py asks of the device, on the reference first: a bad draw is NaN in all
    ten values and nowhere else; a bad point spoils what the definitions say it spoils."""
    A, y, th, seed, t_rep, t_obs = P.case(65, 3, 130, 11)
    for bad in (np.nan, np.inf, -np.inf):
        t = th.copy()
        t[7, 1] = bad
        r, o = P.reference(A, y, t, seed)
        assert np.isnan(r[7]).all() and np.isnan(o[7, 6:]).all() and np.isfinite(o[7, :6]).all()
        assert np.array_equal(np.delete(r, 7, 0), np.delete(t_rep, 7, 0))
        assert np.array_equal(np.delete(o, 7, 0), np.delete(t_obs, 7, 0))
    for bad in (np.nan, 0.0, -0.3, np.inf):
        t = th.copy()
        t[129, 3] = bad
        r, o = P.reference(A, y, t, seed)
        assert np.isnan(r[129]).all() and np.isnan(o[129, 6:]).all()
        assert np.array_equal(r[:129], t_rep[:129]) and np.array_equal(o[:129], t_obs[:129])
    assert list(P.bad_draws(np.array([[1.0, 1.0], [np.nan, 1.0], [1.0, 0.0], [1.0, -1.0], [1.0, np.inf]]))) == \
        [False, True, True, True, True]
    An = A.copy()
    An[40, 2] = np.nan
    r, o = P.reference(An, y, th, seed)
    assert np.isnan(r[:, :6]).all() and np.isnan(o[:, 6:]).all() and np.isfinite(o[:, :6]).all()
    assert np.array_equal(r[:, 6:], t_rep[:, 6:])
    yn = y.copy()
    yn[64] = np.nan
    r, o = P.reference(A, yn, th, seed)
    assert np.array_equal(r, t_rep) and np.isnan(o).all()
    yn[64] = np.inf
    r, o = P.reference(A, yn, th, seed)
    assert np.array_equal(r, t_rep) and np.all(o[:, 6:] == np.inf)
    off = np.zeros(65)
    off[0] = np.nan
    r, o = P.reference(A, y, th, seed, offset=off)
    assert np.isnan(r[:, :6]).all() and np.isnan(o[:, :6]).all()
    assert np.array_equal(r[:, 6:], t_rep[:, 6:]) and np.array_equal(o[:, 6:], t_obs[:, 6:])
    # a NaN never counts as >=
    assert P.p_values(r, o)["mean"] == 0.0


def test_kurtosis_of_three_values_is_a_constant():
    """Why (3, 1, 2) leaves kurt out of the comparisons and (4, 1, 2) stands beside it."""
    assert P.DEGENERATE == {3: ("kurt",)}
    rng = np.random.default_rng(0)
    for _ in range(20):
        k = P.marginal(rng.standard_normal(3) * 10 ** rng.uniform(-3, 3))[5]
        assert abs(float(k) + 1.5) < 1e-15
    _, _, _, _, t_rep, t_obs = P.case(*P.CASES[0])
    assert np.all(np.abs(t_rep[:, 5] + 1.5) < 1e-15) and np.all(np.abs(t_obs[:, 5] + 1.5) < 1e-15)
    assert abs(float(P.marginal(rng.standard_normal(4))[5]) + 1.5) > 1e-3


def test_the_well_specified_case_is_not_flagged_and_the_misspecified_one_is():
    """On the reference, before the GPU test asks the same of the device."""
    _, _, _, _, t_rep, t_obs = P.case(*P.CASES[-1])
    assert P.CASES[-1][:3] == (629, 3, 300)
    p = P.p_values(t_rep, t_obs)
    print(p)
    assert all(0.02 < v < 0.98 for v in p.values()), p
    A, y, th = P.make_case(200, 3, 300, 29, noise=0.9)        # 3 x the noise the draws' sigma claims
    q = P.p_values(*P.reference(A, y, th, 1))
    assert q["chi2"] == 0.0 and q["sd"] == 0.0


# ---- the surface -----------------------------------------------------------------------------------
def test_new_entry_points_are_bound():
    import pybmc_amd
    from pybmc_amd import _lib
    header = open(os.path.join(HERE, "..", "include", "pybmc_amd.h")).read()
    for name in ("bmc_ppc", "bmc_ppc_device"):
        assert name in _lib.PROTOTYPES and name + "(" in header
        assert len(_lib.PROTOTYPES[name][1]) == 15
    for name in ("posterior_predictive_check", "ppc_summary", "PPC_STATS"):
        assert name in pybmc_amd.__all__ and hasattr(pybmc_amd, name)
    assert callable(pybmc_amd.BayesianModelCombination.posterior_predictive_check)
    assert callable(_lib.Context.ppc) and callable(_lib.Context.ppc_device)
    assert "loo_pit" in pybmc_amd.posterior_predictive_check.__doc__       # the scope note
    lib = _lib.load_library()
    assert lib.bmc_abi_version() == 4
    # a NULL context is refused before anything touches a device
    null = (None, None, 3, 1, 1, 0, None, None, None, 2, 2, 0, 0.0, None, None)
    assert lib.bmc_ppc(*null) == 1
    assert lib.bmc_ppc_device(*null) == 1
