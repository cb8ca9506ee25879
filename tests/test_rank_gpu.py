"""Rank-normalised diagnostics on the GPU (-m gpu): kernels_rank.hip through the C ABI and the
Python API against the scipy / numpy reference (tests/rank_reference.py).

Bars.  Ranks are exact, so z differs from the reference by the two ndtri's alone: 1e-14 absolute
(tests/test_rank_host.py).  r_hat (rtol 1e-12), ess_bulk / ess_tail / mcse_mean (rtol 1e-9) are the
bars of tests/test_diagnostics_gpu.py for the same estimators; each case first asserts, from the
reference alone, that no ESS scan stopped on a pair sum within 1e-9 of 0 (an input on which a
rounding could move the stopping lag is ill-posed: the seeds below were chosen on the CPU).
Quantiles: 1 ulp of np.quantile.  The split draws of a column number S = 2 C n, an even number: the
tile-edge shapes are one sort tile and one tile + 2."""
import os
import re

import numpy as np
import pytest

import diag_reference as D
import rank_reference as RR
from conftest import GOLDEN, ROOT
from pybmc_amd import chain_diagnostics, rank_diagnostics, rank_normalize

pytestmark = pytest.mark.gpu

Z_BAR = 1e-14


def sort_tile():
    text = open(os.path.join(ROOT, "pybmc_amd", "csrc", "bmc_rank_plan.h")).read()
    block = int(re.search(r"RANK_BLOCK = (\d+);", text).group(1))
    items = int(re.search(r"RANK_ITEMS = (\d+);", text).group(1))
    assert re.search(r"RANK_TILE = RANK_BLOCK \* RANK_ITEMS;", text)
    return block * items


TILE = sort_tile()


def _ties(rng, C, T, tops):
    return np.stack([rng.integers(0, top + 1, size=(C, T)).astype(np.float64) for top in tops], axis=-1)


def _zeros(rng):
    x = rng.standard_normal((2, 600, 2))
    x[rng.random(x.shape) < 0.3] = 0.0
    x[rng.random(x.shape) < 0.3] = -0.0
    assert np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()
    return x


NORMALIZE_CASES = {
    "ar1": lambda rng: np.concatenate([D.ar1(rng, 4, 2000, 2, 0.0), D.ar1(rng, 4, 2000, 1, 0.9)], axis=-1),
    "minimum": lambda rng: rng.standard_normal((1, 9, 1)),                      # n = 4
    "one_tile": lambda rng: rng.standard_normal((1, TILE, 2)),                  # S = tile
    "tile_plus_2": lambda rng: rng.standard_normal((1, TILE + 2, 2)),           # S = tile + 2
    "tile_minus_2_odd": lambda rng: rng.standard_normal((1, TILE - 1, 1)),      # S = tile - 2, T' odd
    # runs of ~ S/4 and ~ S/2 equal keys over S = 3 tiles + 112: they cross tile boundaries, and
    # the longer ones hold a whole tile; the third column is one run
    "ties": lambda rng: _ties(rng, 2, 3 * TILE // 2 + 56, (3, 1, 0)),
    "zeros": _zeros,
    "constant": lambda rng: np.full((2, 40, 1), 2.5),                           # no digit differs: no pass
}


@pytest.mark.parametrize("folded", [False, True])
@pytest.mark.parametrize("name", sorted(NORMALIZE_CASES))
def test_rank_normalize_matches_reference(name, folded):
    rng = np.random.default_rng(200 + sorted(NORMALIZE_CASES).index(name))
    x = NORMALIZE_CASES[name](rng)
    want = RR.rank_normalize(x, folded=folded)
    got = rank_normalize(x, folded=folded)
    assert got.shape == want.shape
    err = np.abs(got - want).max()
    print(f"{name} folded={folded}: max |z - z_ref| = {err:.3e}")
    assert err <= Z_BAR
    if name == "zeros" and not folded:
        s = RR.split(x)
        for j in range(x.shape[-1]):
            assert len(set(got[:, :, j][s[:, :, j] == 0])) == 1        # -0.0 and +0.0: one rank


def test_rank_normalize_device_input_and_burn():
    import torch
    rng = np.random.default_rng(3)
    x = D.ar1(rng, 3, 701, 4, 0.5)
    want = RR.rank_normalize(x, burn=100)                 # T' = 601: the middle draw has no rank
    got = rank_normalize(torch.as_tensor(x, device="cuda:0"), burn=100)
    assert got.shape == (6, 300, 4) and np.abs(got - want).max() <= Z_BAR
    assert np.array_equal(got, rank_normalize(x, burn=100))


def _shifted(rng):
    x = rng.standard_normal((4, 2000, 2))
    x[1, 1000:] += 2.0            # one chain moves by 2 sd in its second half
    return x


DIAG_CASES = {
    "white": (lambda rng: D.ar1(rng, 4, 3000, 3, 0.0), 300),
    "ar1_0.9": (lambda rng: D.ar1(rng, 4, 3000, 3, 0.9), 301),
    "large_mean": (lambda rng: D.ar1(rng, 4, 2000, 2, 0.3, loc=1e4, scale=1e-2), 302),
    "cauchy": (lambda rng: rng.standard_cauchy((4, 2000, 2)), 303),
    "shifted": (_shifted, 304),
}


def check_against_reference(x, burn=0, probs=(0.05, 0.5, 0.95), got=None, well_posed=True):
    ref = RR.diagnostics(np.asarray(x), burn=burn, probs=probs)
    if well_posed:      # a condition on the input, from the reference alone
        stop = ref["stop"][np.isfinite(ref["stop"])]
        assert np.all(np.abs(stop) > 1e-9), ref["stop"]
    got = rank_diagnostics(x, burn=burn, probs=probs) if got is None else got
    assert list(got) == ["mean", "sd", "mcse_mean", "ess_bulk", "ess_tail", "r_hat", "quantiles"]
    for key, rtol in (("r_hat", 1e-12), ("ess_bulk", 1e-9), ("ess_tail", 1e-9), ("mcse_mean", 1e-9)):
        with np.errstate(invalid="ignore"):
            rel = np.nanmax(np.abs(got[key] / ref[key] - 1.0)) if np.isfinite(ref[key]).any() else 0.0
        print(f"  {key}: max rel err {rel:.3e}")
        np.testing.assert_allclose(got[key], ref[key], rtol=rtol, atol=0, equal_nan=True, err_msg=key)
    assert got["quantiles"].shape == ref["quantiles"].shape
    fin = np.isfinite(ref["quantiles"])
    assert np.array_equal(np.isnan(got["quantiles"]), ~fin)
    ulps = np.abs(got["quantiles"][fin] - ref["quantiles"][fin]) / np.spacing(np.abs(ref["quantiles"][fin]))
    print(f"  quantiles: max {ulps.max() if ulps.size else 0:.2f} ulp")
    assert np.all(ulps <= 1.0)
    return got, ref


@pytest.mark.parametrize("name", sorted(DIAG_CASES))
def test_rank_diagnostics_matches_reference(name):
    make, seed = DIAG_CASES[name]
    x = make(np.random.default_rng(seed))
    got, ref = check_against_reference(x)
    # the indicator counts, from the quantiles that came back
    s = RR.split(x)
    for row, k in ((0, 0), (1, 2)):
        assert np.array_equal((s <= got["quantiles"][k]).sum((0, 1)), ref["counts"][row])
    classic = chain_diagnostics(x)
    assert np.array_equal(got["mean"], classic["mean"]) and np.array_equal(got["sd"], classic["sd"])
    if name == "shifted":
        assert np.all(ref["r_hat"] > 1.05) and np.all(got["r_hat"] > 1.05)
    if name == "cauchy":
        assert np.all(got["r_hat"] < 1.01)      # what the rank normalisation is for: heavy tails mix fine


def test_odd_kept_draws_with_burn():
    rng = np.random.default_rng(310)
    x = D.ar1(rng, 3, 1001, 4, 0.7)
    got, _ = check_against_reference(x, burn=100)          # T' = 901
    # the middle draw of each chain: out of the ranks and quantiles, inside mean and sd
    y = x.copy()
    y[:, 100 + 450] = 1e6
    moved = rank_diagnostics(y, burn=100)
    for key in ("r_hat", "ess_bulk", "ess_tail", "quantiles"):
        assert np.array_equal(moved[key], got[key]), key
    assert np.all(moved["mean"] > got["mean"] + 100) and np.all(moved["sd"] > 1000)
    check_against_reference(x, burn=0)


def test_column_subset_ld_greater_than_n_cols():
    import torch
    rng = np.random.default_rng(311)
    full = D.ar1(rng, 2, 400, 70, 0.6)
    sub = full[:, :, 3:68]                       # a view: row stride 70; 65 columns: past one 64-column tile
    got, _ = check_against_reference(sub)
    t = torch.as_tensor(full, device="cuda:0")[:, :, 3:68]
    assert t.stride() == (400 * 70, 70, 1)
    dev = rank_diagnostics(t)
    for key in got:
        assert np.array_equal(got[key], dev[key], equal_nan=True), key


def test_degenerate_columns():
    rng = np.random.default_rng(312)
    x = rng.standard_normal((2, 300, 6))
    x[:, :, 1] = 3.0
    x[0, 10, 3] = np.nan
    x[1, 200, 4] = np.inf
    got, ref = check_against_reference(x)
    for key in ("r_hat", "ess_bulk", "ess_tail", "mcse_mean"):
        assert np.isnan(got[key][[1, 3, 4]]).all(), key
        assert np.isfinite(got[key][[0, 2, 5]]).all(), key
    assert np.array_equal(got["quantiles"][:, 1], [3.0, 3.0, 3.0])
    assert np.isnan(got["quantiles"][:, [3, 4]]).all() and np.isfinite(got["quantiles"][:, [0, 2, 5]]).all()
    # the neighbours are what they are without the bad columns
    alone = rank_diagnostics(np.ascontiguousarray(x[:, :, [0, 2, 5]]))
    for key in ("r_hat", "ess_bulk", "ess_tail", "quantiles"):
        assert np.array_equal(alone[key], got[key][..., [0, 2, 5]]), key
    z = rank_normalize(x)
    assert np.isnan(z[:, :, [3, 4]]).all() and np.isfinite(z[:, :, [0, 1, 2, 5]]).all()
    assert np.all(z[:, :, 1] == 0.0)


def test_bitwise_deterministic_host_equals_device_and_batching():
    import torch
    from pybmc_amd import _lib
    rng = np.random.default_rng(313)
    x = D.ar1(rng, 4, 2 * TILE + 10, 5, 0.9)           # 16 tiles and a bit per column
    x[:, :, 4] = np.round(x[:, :, 4])                  # ties too
    a = rank_diagnostics(x, burn=3)
    b = rank_diagnostics(x, burn=3)
    c = rank_diagnostics(torch.as_tensor(x, device="cuda:0"), burn=3)
    one = rank_diagnostics(x, burn=3, cols_per_batch=1)
    two = rank_diagnostics(x, burn=3, cols_per_batch=2)
    for key in a:
        for other in (b, c, one, two):
            assert np.array_equal(a[key], other[key], equal_nan=True), key
    za, zb = rank_normalize(x, burn=3, folded=True), rank_normalize(x, burn=3, folded=True)
    assert np.array_equal(za, zb)
    ms = _lib.default_context(0).rank_last_timing()
    assert set(ms) == {"sort_ms", "rank_ms", "classic_ms", "moments_ms"} and all(v > 0 for v in ms.values())


def test_quantile_requests():
    rng = np.random.default_rng(314)
    x = D.ar1(rng, 2, 500, 3, 0.5)
    probs = [0.0, 1.0, 0.5, 0.025, 0.975, 0.25, 0.75, 1 / 3, 0.1, 0.9, 0.2, 0.8, 0.3, 0.7, 0.4, 0.6]
    got, ref = check_against_reference(x, probs=probs)
    s = RR.split(x).reshape(-1, 3)
    assert np.array_equal(got["quantiles"][0], s.min(0)) and np.array_equal(got["quantiles"][1], s.max(0))
    base = rank_diagnostics(x)
    for key in ("r_hat", "ess_bulk", "ess_tail"):        # q05 / q95 are internal: not what was asked for
        assert np.array_equal(got[key], base[key]), key


def test_bad_arguments_raise():
    import torch
    x = np.zeros((2, 100, 3))
    with pytest.raises(ValueError, match="n = "):
        rank_diagnostics(np.zeros((2, 9, 3)), burn=2)
    with pytest.raises(ValueError, match="n = "):
        rank_normalize(np.zeros((2, 7, 3)))
    with pytest.raises(ValueError, match="probabilities"):
        rank_diagnostics(x, probs=np.linspace(0.1, 0.9, 17))
    with pytest.raises(ValueError, match="probabilities"):
        rank_diagnostics(x, probs=[])
    for bad in (1.5, -0.1, np.nan):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            rank_diagnostics(x, probs=[0.5, bad])
    with pytest.raises(ValueError, match="float64"):
        rank_diagnostics(x.astype(np.float32))
    with pytest.raises(ValueError, match="float64"):
        rank_normalize(torch.zeros((2, 90, 3), dtype=torch.float32, device="cuda:0"))
    t = torch.zeros((2, 90, 6), dtype=torch.float64, device="cuda:0")[:, :, ::2]
    with pytest.raises(ValueError, match="contiguous last dimension"):
        rank_diagnostics(t)
    with pytest.raises(ValueError, match="contiguous last dimension"):
        rank_normalize(t)
    # and the C ABI's own checks
    from pybmc_amd import _lib
    ctx = _lib.default_context(0)
    with pytest.raises(ValueError, match="ld must be >= n_cols"):
        ctx.rank_diagnostics(x, 2, 100, 3, 2)
    with pytest.raises(ValueError, match=">= 4 draws"):
        ctx.rank_diagnostics(x, 2, 100, 3, 3, burn=93)
    with pytest.raises(ValueError, match="n_chains"):
        ctx.rank_normalize(x, 0, 100, 3, 3)
    with pytest.raises(ValueError, match="between 1 and 16"):
        ctx.rank_diagnostics(x, 2, 100, 3, 3, probs=np.full(17, 0.5))
    with pytest.raises(ValueError, match="outside"):
        ctx.rank_diagnostics(x, 2, 100, 3, 3, probs=[0.5, 1.0000001])
    with pytest.raises(ValueError, match="cols_per_batch"):
        ctx.rank_diagnostics(x, 2, 100, 3, 3, cols_per_batch=-1)


def test_bmc_summary_on_the_standin_dataset():
    from pybmc_amd import BayesianModelCombination, Dataset
    models = ["FRDM", "HFB24", "UNEDF1", "SKM"]
    ds = Dataset(os.path.join(GOLDEN, "dataset_standin.csv"))
    data = ds.load_data(models + ["truth"], keys=["BE"], domain_keys=["N", "Z"])
    train_df, _, _ = ds.split_data(data, "BE", splitting_algorithm="random", train_size=0.6, val_size=0.2,
                                   test_size=0.2)
    b = BayesianModelCombination(models, data, truth_column_name="truth")
    b.orthogonalize("BE", train_df, components_kept=3, method="svd")
    b.train({"iterations": 3000, "burn": 0, "n_chains": 4, "seeds": [1, 2, 3, 4]})
    df = b.summary()
    assert list(df.index) == ["beta_0", "beta_1", "beta_2", "sigma"] + models
    assert list(df.columns) == ["mean", "sd", "q5", "q50", "q95", "mcse_mean", "ess_bulk", "ess_tail", "r_hat"]
    classic = b.diagnostics()
    assert np.array_equal(df["mean"].to_numpy(), classic["mean"].to_numpy())
    assert np.array_equal(df["sd"].to_numpy(), classic["sd"].to_numpy())
    assert np.all(df["q5"] <= df["q50"]) and np.all(df["q50"] <= df["q95"])
    assert np.all(df["r_hat"] < 1.05) and np.all(df["ess_bulk"] > 100) and np.all(df["ess_tail"] > 100)
    # the same numbers as the reference on the same [beta, sigma, weights] series (the weights as
    # summary() forms them: a device matmul, whose last bits a host matmul need not share)
    from pybmc_amd.bmc import _series_tensor
    series = _series_tensor(b.samples.reshape(4, -1, 4), b.Vt_hat, b.device).cpu().numpy()
    got = {key: df[key].to_numpy() for key in ("mean", "sd", "mcse_mean", "ess_bulk", "ess_tail", "r_hat")}
    got["quantiles"] = df[["q5", "q50", "q95"]].to_numpy().T
    check_against_reference(series, got=got)
    assert list(b.summary(probs=(0.025, 0.975)).columns)[2:4] == ["q2.5", "q97.5"]
