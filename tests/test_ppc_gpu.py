"""The posterior predictive check on the MI355X (kernels_ppc.hip, pybmc_amd.ppc) against the
long-double reference of tests/ppc_reference.py: every draw, every statistic.

Accuracy is |device - reference| / max(1, |reference|) per statistic.  No bar may exceed 1e-10, a
tenth of the 1e-9 floor that test_ppc_host.py proves for |T_rep - T_obs| on these cases -- which is
why the p-values must be EQUAL to the reference's, not close.

The design asks for bars of 64 x the largest value observed on the MI355X.  No GPU run was
possible when this file was written, so nothing has been observed; until a run replaces them the
bars are WORST-CASE rounding bounds for the shapes of this file (u = 2^-53 = 1.1e-16), a
tightening being the only change a measurement can bring:

  element   z is within 4.2 u |z| of the reference (2.1 units of 2^-52, measured for
            these bmc_math.h functions).  a_i . beta_s is a sum of k <= 33 products in the MFMA's
            order: |error| <= k u sum_j |a_ij beta_sj|, and sum_j |a_ij beta_sj| <= 60 here; with the
            noise, offset and centring roundings |error of y_rep| <= (k + 8) u 60 = 2.7e-13.
  min max mean   an element's error, relative to max(1, |.|) <= 2.7e-13                   bar 1e-12
  sd        the sums run over <= 40 elements per lane and a 4-step tree, 45 u relative to the sum of
            magnitudes; sd >= 1 here, so the elements' 2.7e-13 dominates                 bar 1e-12
  skew kurt m3 / m2^1.5 and m4 / m2^2 move by 3 and 4 times an element's error over sd times the
            absolute moments E|x/sd|^2, E|x/sd|^3 (<= 2.5): <= 3e-12                     bar 1e-11
  chi2 max_abs_z   replicated: 8.4 u + 45 u.  Observed: e = (y - a . beta) / sigma with |y - a . beta|
            about sigma = 0.3, so an element's 2.7e-13 is 9e-13 of e and 1.8e-12 of e^2    bar 1e-11

At n = 3 the kurtosis of any three values is -3/2 (ppc_reference.DEGENERATE): there it is checked
as a value and left out of the p-value comparison; (4, 1, 2) is the smallest case with all eight.
"""
import numpy as np
import pytest

import ppc_reference as P
import score_reference as R

pytestmark = pytest.mark.gpu

BARS = {"min": 1e-12, "max": 1e-12, "mean": 1e-12, "sd": 1e-12, "skew": 1e-11, "kurt": 1e-11,
        "chi2": 1e-11, "max_abs_z": 1e-11}
BAR_CAP = 1e-10


def test_no_bar_exceeds_a_tenth_of_the_margin_floor():
    assert BAR_CAP == P.MARGIN_FLOOR / 10
    assert set(BARS) == set(P.PPC_STATS) and all(0 < v <= BAR_CAP for v in BARS.values())


def errors(dev, ref):
    """(8,) float64: the largest |dev - ref| / max(1, |ref|) of every statistic."""
    ref = np.asarray(ref, dtype=P.LD)
    e = np.abs(np.asarray(dev, dtype=P.LD) - ref) / np.maximum(P.LD(1), np.abs(ref))
    return e.max(axis=0).astype(np.float64)


def check(out, t_rep, t_obs, n, tag):
    """The device's t_rep and t_obs within the bars, its p-values equal to the reference's; prints
    the figures before it asserts."""
    assert out["t_rep"].shape == out["t_obs"].shape == t_rep.shape and out["stats"] == P.PPC_STATS
    assert out["n_points"] == n and out["n_draws"] == t_rep.shape[0]
    assert np.isfinite(out["t_rep"]).all() and np.isfinite(out["t_obs"]).all()
    e_rep, e_obs = errors(out["t_rep"], t_rep), errors(out["t_obs"], t_obs)
    print(f"{tag}: t_rep " + " ".join(f"{k} {v:.2e}" for k, v in zip(P.PPC_STATS, e_rep)))
    print(f"{tag}: t_obs " + " ".join(f"{k} {v:.2e}" for k, v in zip(P.PPC_STATS, e_obs)))
    for j, key in enumerate(P.PPC_STATS):
        assert e_rep[j] <= BARS[key], (tag, "t_rep", key, e_rep[j])
        assert e_obs[j] <= BARS[key], (tag, "t_obs", key, e_obs[j])
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
        assert np.all(np.abs(out["t_rep"][:, 5] + 1.5) <= BARS["kurt"])
        assert np.all(np.abs(out["t_obs"][:, 5] + 1.5) <= BARS["kurt"])


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
    A, y, th, seed, t_rep0, _ = P.case(150, 17, 64, 13)
    off = 20.0 + 5.0 * np.random.default_rng(1).standard_normal(150)
    t_rep, t_obs = P.reference(A, y, th, seed, offset=off)
    base, out = run(A, y, th, seed), run(A, y, th, seed, offset=off)
    check(out, t_rep, t_obs, 150, "offset")
    # min, max and mean move by the reference's amounts: each side is within its bar of its reference
    for name, j in (("min", 0), ("max", 1), ("mean", 2)):
        moved = out["t_rep"][:, j].astype(P.LD) - base["t_rep"][:, j].astype(P.LD)
        ref_moved = t_rep[:, j] - t_rep0[:, j]
        room = BARS[name] * (np.maximum(1, np.abs(t_rep[:, j])) + np.maximum(1, np.abs(t_rep0[:, j])))
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
