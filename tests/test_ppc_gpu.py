"""The posterior predictive check on the MI355X (kernels_ppc.hip, pybmc_amd.ppc) against the
long-double reference of tests/ppc_reference.py: every draw, every statistic.

Accuracy is |device - reference| / max(1, |reference|) per value: the eight of t_rep and the two
observed ones that depend on the draw (P.TEN).  The cases fall into three groups (P.GROUPS): the
seven hand-picked shapes with the offset case, the shape grid with the two edge seeds, and the
biased fits.  A group's bar for a value is 64 x its FLOOR, rounded up to one significant digit
(P.bars); the floor is the larger of the float64 reference's deviation from the long-double one
and the effect of the generator's accuracy on the long-double one, over the
group's cases: tests/test_ppc_host.py recomputes it on the CPU, and nothing of the device enters
it.  64 covers the MFMA's and the lane tree's summation order, the one-pass moments about the
draw's own centre, and exp / log / sincos that are not correctly rounded.  No bar exceeds 1e-10, a
tenth of the 1e-9 floor that test_ppc_host.py proves for |T_rep - T_obs| on every case -- which is
why the p-values must be EQUAL to the reference's, not close -- and no bar of the first two groups
is wider than the worst-case rounding bounds this file held before a device had run it
(WIDEST_BEFORE).  The biased fits are a group of their own: |y_rep| / sd is about 250 there, so
skew and kurt have floors of 1.0e-12 and 3.2e-13 whatever the arithmetic after y_rep.

MEASURED holds the largest deviation seen on an MI355X per group and value.  It is a record, not
a bar: check() prints the figures of every case, and the running maxima per group, before it
asserts.

At n = 3 the kurtosis of any three values is -3/2 (ppc_reference.DEGENERATE): there it is checked
as a value and left out of the p-value comparison; (4, 1, 2) is the smallest case with all eight.
"""
import numpy as np
import pytest

import ppc_reference as P
import score_reference as R

pytestmark = pytest.mark.gpu

BARS = {group: P.bars(group) for group in P.GROUPS}
BAR_CAP = 1e-10
# the bars of this file before any run (worst-case rounding bounds), per statistic
WIDEST_BEFORE = {"min": 1e-12, "max": 1e-12, "mean": 1e-12, "sd": 1e-12, "skew": 1e-11, "kurt": 1e-11,
                 "chi2": 1e-11, "max_abs_z": 1e-11, "chi2_obs": 1e-11, "max_abs_e": 1e-11}

# Largest |device - reference| / max(1, |reference|) on an MI355X, the order of P.TEN
MEASURED = {
    "cases": (5.09e-16, 4.90e-16, 3.13e-16, 2.27e-16, 5.29e-16, 2.87e-15, 2.60e-16, 2.70e-16, 1.11e-15, 4.22e-15),
    "grid": (1.57e-15, 1.74e-15, 4.35e-15, 5.19e-16, 2.63e-15, 7.56e-15, 3.45e-16, 2.81e-16, 2.12e-14, 3.48e-14),
    "biased": (1.37e-16, 2.04e-16, 1.11e-16, 1.26e-16, 2.40e-14, 3.26e-14, 1.75e-16, 1.56e-16, 4.66e-16, 1.39e-15),
}
# The same two biased cases with the power sums about ONE centre for all draws, mean(y + offset), as
# the kernel took them before: delta = 0.3: sd 9.2e-16, skew 3.3e-12, kurt 7.0e-11 (bar 3e-11);
# delta = 3: sd 1.0e-13 (bar 9e-15), skew 2.7e-9, kurt 6.1e-7.  test_biased_fits failed on both.
WORST = {group: np.zeros(len(P.TEN)) for group in P.GROUPS}


def test_no_bar_exceeds_a_tenth_of_the_margin_floor():
    assert BAR_CAP == P.MARGIN_FLOOR / 10
    for group in P.GROUPS:
        assert tuple(BARS[group]) == P.TEN and all(0 < v <= BAR_CAP for v in BARS[group].values())
        assert BARS[group] == {name: P.round_up_one_digit(64 * f) for name, f in zip(P.TEN, P.FLOORS[group])}
    for group in ("cases", "grid"):
        assert all(BARS[group][name] <= WIDEST_BEFORE[name] for name in P.TEN), group
    assert max(max(b.values()) for b in BARS.values()) == BARS["biased"]["skew"] == 7e-11
    for group in P.GROUPS:       # the record is of runs that passed
        assert all(0 < m <= BARS[group][name] for name, m in zip(P.TEN, MEASURED[group])), group


def errors(dev, ref):
    """(columns,) float64: the largest |dev - ref| / max(1, |ref|) of every column."""
    ref = np.asarray(ref, dtype=P.LD)
    e = np.abs(np.asarray(dev, dtype=P.LD) - ref) / np.maximum(P.LD(1), np.abs(ref))
    return e.max(axis=0).astype(np.float64)


def check(out, t_rep, t_obs, n, tag, group="cases"):
    """The device's t_rep and t_obs within the group's bars, its p-values equal to the reference's;
    prints the figures before it asserts."""
    bars = BARS[group]
    assert out["t_rep"].shape == out["t_obs"].shape == t_rep.shape and out["stats"] == P.PPC_STATS
    assert out["n_points"] == n and out["n_draws"] == t_rep.shape[0]
    assert np.isfinite(out["t_rep"]).all() and np.isfinite(out["t_obs"]).all()
    e_rep, e_obs = errors(out["t_rep"], t_rep), errors(out["t_obs"], t_obs)
    WORST[group] = np.maximum(WORST[group], np.concatenate([e_rep, e_obs[6:]]))
    print(f"{tag}: t_rep " + " ".join(f"{k} {v:.2e}" for k, v in zip(P.PPC_STATS, e_rep)))
    print(f"{tag}: t_obs " + " ".join(f"{k} {v:.2e}" for k, v in zip(P.PPC_STATS, e_obs)))
    print(f"WORST {group} " + " ".join(f"{v:.2e}" for v in WORST[group]))
    for j, key in enumerate(P.PPC_STATS):
        assert e_rep[j] <= bars[key], (tag, "t_rep", key, e_rep[j])
        assert e_obs[j] <= bars[P.TEN[j + 2] if j >= 6 else key], (tag, "t_obs", key, e_obs[j])
    want = P.p_values(t_rep, t_obs)
    from pybmc_amd import ppc_summary
    assert out["p_value"] == ppc_summary(out["t_rep"], out["t_obs"])
    for j in P.compared(n):
        key = P.PPC_STATS[j]
        assert out["p_value"][key] == want[key], (tag, key)
    return e_rep, e_obs


def run(A, y, th, seed, **kw):
    from pybmc_amd import posterior_predictive_check
    return posterior_predictive_check(A, y, th, seed=seed, **kw)


def same_bits(a, b):
    return (np.array_equal(a["t_rep"], b["t_rep"]) and np.array_equal(a["t_obs"], b["t_obs"])
            and a["p_value"] == b["p_value"])


@pytest.mark.parametrize("case", P.CASES, ids=lambda c: "n%d_k%d_S%d" % c[:3])
def test_cases_against_the_reference(case):
    A, y, th, seed, t_rep, t_obs = P.case(*case)
    out = run(A, y, th, seed)
    assert out["seed"] == seed
    check(out, t_rep, t_obs, case[0], "n=%d k=%d S=%d" % case[:3])
    assert same_bits(out, run(A, y, th, seed))             # two calls, the same bits
    assert not np.array_equal(run(A, y, th, seed + 1)["t_rep"], out["t_rep"])
    if case[0] == 3:
        assert np.all(np.abs(out["t_rep"][:, 5] + 1.5) <= BARS["cases"]["kurt"])
        assert np.all(np.abs(out["t_obs"][:, 5] + 1.5) <= BARS["cases"]["kurt"])


def via_abi(A, y, th, seed, offset=None, col_major=False, pad_a=0, pad_t=0):
    """The same call through the C ABI (ctx.ppc), so that layout and strides can be set: A in either
    layout with lda wider than its rows by pad_a, theta with ldt wider by pad_t, the slack NaN."""
    from pybmc_amd import _lib, ppc_summary
    from pybmc_amd.ppc import marginal_stats
    ctx = _lib.default_context(0)
    n, k = A.shape
    S = th.shape[0]
    if col_major:
        buf = np.full((k, n + pad_a), np.nan)
        buf[:, :n] = A.T
        lda, layout = n + pad_a, _lib.BMC_COL_MAJOR
    else:
        buf = np.full((n, k + pad_a), np.nan)
        buf[:, :k] = A
        lda, layout = k + pad_a, _lib.BMC_ROW_MAJOR
    tb = np.full((S, k + 1 + pad_t), np.nan)
    tb[:, :k + 1] = th
    yo = y if offset is None else y + offset
    with ctx.lock:
        got = ctx.ppc(buf, n, k, lda, layout, np.ascontiguousarray(y), tb, S, k + 1 + pad_t,
                      None if offset is None else np.ascontiguousarray(offset), seed, float(np.mean(yo)))
    t_obs = np.empty((S, 8))
    t_obs[:, :6] = marginal_stats(yo)
    t_obs[:, 6:] = got["t_obs2"]
    return {"p_value": ppc_summary(got["t_rep"], t_obs), "t_rep": got["t_rep"], "t_obs": t_obs,
            "stats": P.PPC_STATS, "n_points": n, "n_draws": S, "seed": seed}


@pytest.mark.parametrize("k", P.GRID_K)
def test_shapes_on_both_sides_of_every_rule(k):
    """Points on both sides of the 64-point tile and of the Box-Muller partner 32 further on, the
    full-tile branch exactly (64, 128); k around the 16-column slab with and without a spare slab
    column (16 and 32: k_pad == k) up to the limit; draws around the 64-draw tile; a noise seed with
    a non-zero high word in every case; both layouts, lda and ldt wider than the rows with NaN in the
    slack; an offset on every third case."""
    for case, n, S, data_seed in P.grid_shapes(k):
        n_, S_, A, y, th, off, seed, t_rep, t_obs = P.grid_case(k, case)
        assert (n_, S_) == (n, S) and seed >> 32 == 0x9E3779B9
        pad_a, pad_t = (case % 3) * 2, (case % 2) * 3
        out = via_abi(A, y, th, seed, offset=off, col_major=bool(case % 2), pad_a=pad_a, pad_t=pad_t)
        check(out, t_rep, t_obs, n, f"k={k} case={case} n={n} S={S} col_major={case % 2} pad_a={pad_a} "
              f"pad_t={pad_t} offset={off is not None}", "grid")


@pytest.mark.parametrize("seed", P.SEED_EDGES, ids=("seed_0", "seed_2^64-1"))
def test_the_first_and_the_last_seed(seed):
    n, S, A, y, th, off, seed_, t_rep, t_obs = P.seed_edge_case(seed)
    out = run(A, y, th, seed)
    assert out["seed"] == seed == seed_
    check(out, t_rep, t_obs, n, "seed=%d" % seed, "grid")


@pytest.mark.parametrize("delta", P.BIASED, ids=lambda d: "biased_%g" % d)
def test_biased_fits(delta):
    """Draws whose replicated mean sits 15 or 150 sd from mean(y): power sums about one centre for
    all draws lose (shift / sd)^4 u of kurt (3.2e-10 and 3.1e-6 in float64 on these two cases); about
    the draw's own centre a_bar . beta_s + mean(offset) they lose nothing that the floor sees."""
    n, S, A, y, th, off, seed, t_rep, t_obs = P.biased_case(delta)
    out = run(A, y, th, seed)
    check(out, t_rep, t_obs, n, "biased delta=%g" % delta, "biased")
    assert out["p_value"]["mean"] == 1.0 and out["p_value"]["min"] == 1.0      # and it is flagged


def test_every_input_form_gives_the_bits_of_the_plain_call():
    import torch
    A, y, th, seed, _, _ = P.case(65, 3, 130, 11)
    plain = run(A, y, th, seed)
    assert same_bits(plain, run(np.asfortranarray(A), y, th, seed)), "Fortran-ordered A"
    wide = np.full((260, 6), np.nan)
    wide[::2, :4] = th
    assert same_bits(plain, run(A, y, wide[:, :4], seed, thin=2)), "draws thinned in place (ldt = 12)"
    assert same_bits(plain, run(A, y, th.reshape(2, 65, 4), seed)), "(C, T, k+1)"
    dev = torch.as_tensor(th.copy(), device="cuda:0")
    assert same_bits(plain, run(A, y, dev, seed)), "CUDA tensor"
    assert same_bits(plain, run(A, y, dev.reshape(2, 65, 4), seed)), "CUDA tensor, chains"
    # burn and thin pool as the scoring calls do
    chains = np.concatenate([np.full((2, 3, 4), np.nan), th.reshape(2, 65, 4)], axis=1)
    assert same_bits(plain, run(A, y, chains, seed, burn=3))


def test_a_draw_does_not_depend_on_the_draw_count():
    A, y, th, seed, _, _ = P.case(65, 3, 130, 11)
    a, b = run(A, y, th, seed), run(A, y, th[:70], seed)
    assert np.array_equal(a["t_rep"][:70], b["t_rep"]) and np.array_equal(a["t_obs"][:70], b["t_obs"])


def test_offset_moves_the_marginal_statistics_only():
    _, _, _, _, t_rep0, _ = P.case(150, 17, 64, 13)
    _, _, A, y, th, off, seed, t_rep, t_obs = P.offset_case()
    base, out = run(A, y, th, seed), run(A, y, th, seed, offset=off)
    check(out, t_rep, t_obs, 150, "offset")
    # min, max and mean move by the reference's amounts: each side is within its bar of its reference
    for name, j in (("min", 0), ("max", 1), ("mean", 2)):
        moved = out["t_rep"][:, j].astype(P.LD) - base["t_rep"][:, j].astype(P.LD)
        ref_moved = t_rep[:, j] - t_rep0[:, j]
        room = BARS["cases"][name] * (np.maximum(1, np.abs(t_rep[:, j])) + np.maximum(1, np.abs(t_rep0[:, j])))
        assert np.all(np.abs(ref_moved) > 1) and np.all(np.abs(moved - ref_moved) <= room), name
    for j in (6, 7):
        assert np.array_equal(out["t_rep"][:, j], base["t_rep"][:, j])
        assert np.array_equal(out["t_obs"][:, j], base["t_obs"][:, j])
    # zeros are the default
    assert same_bits(base, run(A, y, th, seed, offset=np.zeros(150)))


def test_a_misspecified_fit_is_flagged():
    """Targets with 3 x the noise the draws' sigma claims."""
    A, y, th = P.make_case(200, 3, 300, 29, noise=0.9)
    out = run(A, y, th, 1)
    print(out["p_value"])
    assert out["p_value"]["chi2"] == 0.0
    assert out["p_value"] == P.p_values(*P.reference(A, y, th, 1))


def test_a_well_specified_fit_is_not_flagged():
    A, y, th, seed, _, _ = P.case(629, 3, 300, 19)
    p = run(A, y, th, seed)["p_value"]
    print(p)
    assert all(0.02 < v < 0.98 for v in p.values()), p


def test_seed_none_draws_from_numpys_global_stream_and_returns_it():
    A, y, th, _, _, _ = P.case(33, 1, 70, 7)
    np.random.seed(123)
    a = run(A, y, th, None)
    np.random.seed(123)
    b = run(A, y, th, None)
    assert a["seed"] == b["seed"] and 0 <= a["seed"] < 2 ** 64 and same_bits(a, b)
    assert same_bits(a, run(A, y, th, a["seed"]))
    assert run(A, y, th, None)["seed"] != a["seed"]


def test_c_abi_refuses_bad_arguments():
    from pybmc_amd import _lib
    ctx = _lib.default_context(0)
    A, y, th, _, _, _ = P.case(33, 1, 70, 7)
    for args, msg in (((A, 2, 1, 1, 0, y, th, 70, 2, None, 0, 0.0), "n_points"),
                      ((A, 33, 1, 1, 0, y, th, 1, 2, None, 0, 0.0), "n_draws"),
                      ((A, 33, 1, 0, 0, y, th, 70, 2, None, 0, 0.0), "lda"),
                      ((A, 33, 1, 1, 0, y, th, 70, 1, None, 0, 0.0), "ldt"),
                      ((A, 33, 0, 1, 0, y, th, 70, 2, None, 0, 0.0), "k must"),
                      ((A, 33, 1, 1, 2, y, th, 70, 2, None, 0, 0.0), "layout")):
        with pytest.raises(ValueError, match=msg):
            ctx.ppc(*args)
    with pytest.raises(ValueError, match="n_points"):
        ctx.ppc_device(1, 2 ** 31 + 1, 1, 1, 0, 1, 1, 70, 2, None, 0, 0.0)


# ---- bad input ------------------------------------------------------------------------------------
# A value is NaN exactly where the definitions of ppc.py give NaN; a bad draw spoils its own row and
# no other; a bad point spoils what depends on it and nothing else.  Non-finite values are data:
# every index of the kernels comes from the shapes.
BAD_N, BAD_K, BAD_S = 130, 3, 130


def clean_run():
    A, y, th = P.make_case(BAD_N, BAD_K, BAD_S, 77)
    return A, y, th, run(A, y, th, 4242)


def summary_holds(out):
    from pybmc_amd import ppc_summary
    assert out["p_value"] == ppc_summary(out["t_rep"], out["t_obs"])
    for j, name in enumerate(P.PPC_STATS):      # a NaN never counts as >=
        both = ~(np.isnan(out["t_rep"][:, j]) | np.isnan(out["t_obs"][:, j]))
        counted = np.zeros(BAD_S, dtype=bool)
        counted[both] = out["t_rep"][both, j] >= out["t_obs"][both, j]
        assert out["p_value"][name] == float(np.mean(counted)), name


@pytest.mark.parametrize("column,value", [(1, np.nan), (0, np.inf), (2, -np.inf), (3, np.nan), (3, 0.0),
                                          (3, -0.3), (3, np.inf)],
                         ids=("beta_nan", "beta_inf", "beta_-inf", "sigma_nan", "sigma_0", "sigma_-0.3",
                              "sigma_inf"))
def test_a_bad_draw_is_nan_in_all_ten_values_and_spoils_no_other(column, value):
    """In the middle of a draw tile, at index 0 and at S - 1 (a partly filled tile)."""
    A, y, th, clean = clean_run()
    assert np.isfinite(clean["t_rep"]).all() and np.isfinite(clean["t_obs"]).all()
    for d in (67, 0, BAD_S - 1):
        t = th.copy()
        t[d, column] = value
        out = run(A, y, t, 4242)
        print(d, out["t_rep"][d], out["t_obs"][d, 6:])
        assert np.isnan(out["t_rep"][d]).all() and np.isnan(out["t_obs"][d, 6:]).all(), d
        keep = np.arange(BAD_S) != d
        assert np.array_equal(out["t_rep"][keep], clean["t_rep"][keep]), d
        assert np.array_equal(out["t_obs"][keep], clean["t_obs"][keep]), d
        assert np.array_equal(out["t_obs"][d, :6], clean["t_obs"][d, :6])
        summary_holds(out)
        for j, name in enumerate(P.PPC_STATS):
            counted = clean["t_rep"][keep, j] >= clean["t_obs"][keep, j]
            assert out["p_value"][name] == float(np.mean(np.append(counted, False))), (d, name)
        r, o = P.reference(A, y, t, 4242)
        assert np.array_equal(np.isnan(out["t_rep"]), np.isnan(r))
        assert np.array_equal(np.isnan(out["t_obs"]), np.isnan(o))


def test_a_bad_point_spoils_what_depends_on_it():
    """NaN in A[i, j], i in a full tile, at a tile's first point and in the partly filled last one."""
    A, y, th, clean = clean_run()
    for i, j in ((5, 0), (64, 2), (BAD_N - 1, 1)):
        An = A.copy()
        An[i, j] = np.nan
        out = run(An, y, th, 4242)
        assert np.isnan(out["t_rep"][:, :6]).all() and np.isnan(out["t_obs"][:, 6:]).all(), (i, j)
        assert np.array_equal(out["t_rep"][:, 6:], clean["t_rep"][:, 6:]), (i, j)
        assert np.array_equal(out["t_obs"][:, :6], clean["t_obs"][:, :6]), (i, j)
        summary_holds(out)
        assert all(out["p_value"][name] == 0.0 for name in P.PPC_STATS[:6])


def test_a_nan_target_spoils_the_observed_values_only():
    A, y, th, clean = clean_run()
    for i in (5, BAD_N - 1):
        yn = y.copy()
        yn[i] = np.nan
        out = run(A, yn, th, 4242)
        assert np.isnan(out["t_obs"]).all(), i
        assert np.array_equal(out["t_rep"], clean["t_rep"]), i
        summary_holds(out)
        assert set(out["p_value"].values()) == {0.0}


def test_a_nan_offset_spoils_the_marginal_values_only():
    A, y, th, clean = clean_run()
    for i in (5, BAD_N - 1):
        off = np.zeros(BAD_N)
        off[i] = np.nan
        out = run(A, y, th, 4242, offset=off)
        assert np.isnan(out["t_rep"][:, :6]).all() and np.isnan(out["t_obs"][:, :6]).all(), i
        assert np.array_equal(out["t_rep"][:, 6:], clean["t_rep"][:, 6:]), i
        assert np.array_equal(out["t_obs"][:, 6:], clean["t_obs"][:, 6:]), i
        summary_holds(out)


def test_an_infinite_target_gives_infinite_observed_discrepancies():
    A, y, th, clean = clean_run()
    yn = y.copy()
    yn[70] = np.inf
    out = run(A, yn, th, 4242)
    assert np.all(out["t_obs"][:, 6:] == np.inf)
    assert np.array_equal(out["t_rep"], clean["t_rep"])
    summary_holds(out)
    assert out["p_value"]["chi2"] == 0.0 and out["p_value"]["max_abs_z"] == 0.0


# ---- the BayesianModelCombination surface ---------------------------------------------------------
def test_bmc_posterior_predictive_check():
    from pybmc_amd import BayesianModelCombination, posterior_predictive_check
    train, models = R.three_component_frame(400, seed=1)
    val, _ = R.three_component_frame(150, seed=2)
    b = BayesianModelCombination(models, {"p": train}, truth_column_name="truth")
    b.orthogonalize("p", train, components_kept=3, method="svd")
    b.train({"iterations": 1500, "burn": 300, "n_chains": 2, "seeds": [1, 2]})
    s = np.asarray(b.samples).reshape(2, -1, 4)
    yc = np.asarray(b.centered_experiment_train, dtype=np.float64)
    mu = np.asarray(b._predictions_mean_train, dtype=np.float64)
    a = b.posterior_predictive_check(seed=7, burn=100)
    w = posterior_predictive_check(b.U_hat, yc, s, burn=100, offset=mu, seed=7)
    assert same_bits(a, w) and a["n_points"] == 400 and a["n_draws"] == 2 * (s.shape[1] - 100) and a["seed"] == 7
    # in the truth's units: the observed marginal statistics are those of the truth column
    truth = train["truth"].to_numpy()
    np.testing.assert_allclose(a["t_obs"][0, :3], [truth.min(), truth.max(), truth.mean()], rtol=1e-13)
    # held out, as log_predictive_density builds it
    preds = val[models].to_numpy(dtype=np.float64)
    h = b.posterior_predictive_check(val, seed=8)
    wh = posterior_predictive_check(preds @ np.asarray(b.Vt_hat).T, val["truth"].to_numpy() - preds.mean(axis=1),
                                    s, offset=preds.mean(axis=1), seed=8)
    assert same_bits(h, wh) and h["n_points"] == 150 and h["n_draws"] == 2 * s.shape[1] == 3000
    print(a["p_value"], h["p_value"])
    assert all(0.0 <= v <= 1.0 for v in h["p_value"].values())
