"""The posterior predictive check with Student-t replicated noise on the MI355X (kernels_ppc.hip,
the PPC_T and PPC_TV instantiations; pybmc_amd.ppc) against the long-double reference of
tests/ppc_t_reference.py: every draw, every statistic.

Accuracy is |device - reference| / max(1, |reference|) per value of T.TEN, as in test_ppc_gpu.py.
A group's bar for a value is 64 x its floor, rounded up to one significant digit (T.bars); the
floor is the larger of the float64 reference's deviation from the long-double one and the effect
of the generator's accuracy (T.T_ACCURACY, per nu) on the long-double one, over the group's cases:
tests/test_ppc_t_host.py recomputes it on the CPU, and nothing of the device enters it.  No bar
exceeds 1e-10, a tenth of the 1e-9 that test_ppc_t_host.py proves for |T_rep - T_obs| on every
case, which is why the p-values must be EQUAL to the reference's.

check() prints the figures of every case, and the running maxima per group beside the floors,
before it asserts.  MEASURED is the record of an MI355X run.
"""
import numpy as np
import pytest

import ppc_reference as P
import ppc_t_reference as T
import robust_reference as RR

pytestmark = pytest.mark.gpu

BARS = {group: T.bars(group) for group in T.GROUPS}
WORST = {group: np.zeros(len(T.TEN)) for group in T.GROUPS}

# Largest |device - reference| / max(1, |reference|) on an MI355X, the order of T.TEN
MEASURED = {
    "grid": (1.08e-15, 1.47e-15, 1.05e-15, 1.28e-15, 2.12e-15, 4.65e-15, 2.84e-15, 1.49e-15, 1.69e-15, 3.31e-15),
    "biased": (1.13e-16, 1.99e-16, 1.19e-16, 1.10e-16, 1.82e-14, 6.14e-14, 2.47e-16, 2.64e-16, 2.80e-16, 4.03e-16),
}


def test_the_record_is_of_runs_that_passed():
    for group in T.GROUPS:
        assert all(0 < m <= BARS[group][name] for name, m in zip(T.TEN, MEASURED[group])), group


def errors(dev, ref):
    ref = np.asarray(ref, dtype=P.LD)
    e = np.abs(np.asarray(dev, dtype=P.LD) - ref) / np.maximum(P.LD(1), np.abs(ref))
    return e.max(axis=0).astype(np.float64)


def check(out, t_rep, t_obs, n, tag, group="grid"):
    """The device's t_rep and t_obs within the group's bars, its p-values equal to the reference's;
    prints the figures before it asserts."""
    bars = BARS[group]
    assert out["t_rep"].shape == out["t_obs"].shape == t_rep.shape and out["stats"] == P.PPC_STATS
    assert out["n_points"] == n and out["n_draws"] == t_rep.shape[0] and out["likelihood"] == "student_t"
    assert np.isfinite(out["t_rep"]).all() and np.isfinite(out["t_obs"]).all()
    e_rep, e_obs = errors(out["t_rep"], t_rep), errors(out["t_obs"], t_obs)
    WORST[group] = np.maximum(WORST[group], np.concatenate([e_rep, e_obs[6:]]))
    print(f"{tag}: t_rep " + " ".join(f"{k} {v:.2e}" for k, v in zip(P.PPC_STATS, e_rep)))
    print(f"{tag}: t_obs " + " ".join(f"{k} {v:.2e}" for k, v in zip(P.PPC_STATS, e_obs)))
    print(f"WORST {group} " + " ".join(f"{v:.2e}" for v in WORST[group]))
    print(f"FLOOR {group} " + " ".join(f"{v:.2e}" for v in T.FLOORS[group]))
    for j, key in enumerate(P.PPC_STATS):
        assert e_rep[j] <= bars[key], (tag, "t_rep", key, e_rep[j])
        assert e_obs[j] <= bars[T.TEN[j + 2] if j >= 6 else key], (tag, "t_obs", key, e_obs[j])
    want = P.p_values(t_rep, t_obs)
    from pybmc_amd import ppc_summary
    assert out["p_value"] == ppc_summary(out["t_rep"], out["t_obs"])
    for j in P.compared(n):
        key = P.PPC_STATS[j]
        assert out["p_value"][key] == want[key], (tag, key)


def lik(nus):
    """The keyword of posterior_predictive_check for a case's nu."""
    return {"nu_draws": nus} if isinstance(nus, np.ndarray) else {"nu": nus}


def run(A, y, th, seed, nus, **kw):
    from pybmc_amd import posterior_predictive_check
    return posterior_predictive_check(A, y, th, seed=seed, **lik(nus), **kw)


def same_bits(a, b):
    return (np.array_equal(a["t_rep"], b["t_rep"]) and np.array_equal(a["t_obs"], b["t_obs"])
            and a["p_value"] == b["p_value"])


def table_of(nus, S):
    """(values, int32 index) as the _tv entry points take a nu per draw."""
    values, index = np.unique(T.nu_of_draws(nus, S), return_inverse=True)
    return values, np.ascontiguousarray(index, dtype=np.int32)


def via_abi(A, y, th, seed, nus, offset=None, col_major=False, pad_a=0, pad_t=0, device=False):
    """The same call through the C ABI (ctx.ppc_t / ctx.ppc_tv and their _device forms), so that
    layout and strides can be set: A in either layout with lda wider than its rows by pad_a, theta
    with ldt wider by pad_t, the slack NaN."""
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
    per_draw = isinstance(nus, np.ndarray)
    noise = table_of(nus, S) if per_draw else (float(nus),)
    name = "ppc_tv" if per_draw else "ppc_t"
    yc = np.ascontiguousarray(y)
    oc = None if offset is None else np.ascontiguousarray(offset)
    if device:
        import torch
        held = [torch.as_tensor(a, device="cuda:0") for a in (buf, yc, tb)]
        od = None if oc is None else torch.as_tensor(oc, device="cuda:0")
        if per_draw:
            idx = torch.as_tensor(noise[1], device="cuda:0")
            noise = (noise[0], idx.data_ptr())
        torch.cuda.synchronize()
        with ctx.lock:
            got = getattr(ctx, name + "_device")(held[0].data_ptr(), n, k, lda, layout, held[1].data_ptr(),
                                                 held[2].data_ptr(), S, k + 1 + pad_t,
                                                 None if od is None else od.data_ptr(), seed, *noise)
    else:
        with ctx.lock:
            got = getattr(ctx, name)(buf, n, k, lda, layout, yc, tb, S, k + 1 + pad_t, oc, seed, *noise)
    t_obs = np.empty((S, 8))
    t_obs[:, :6] = marginal_stats(y if offset is None else y + offset)
    t_obs[:, 6:] = got["t_obs2"]
    return {"p_value": ppc_summary(got["t_rep"], t_obs), "t_rep": got["t_rep"], "t_obs": t_obs,
            "stats": P.PPC_STATS, "n_points": n, "n_draws": S, "seed": seed, "likelihood": "student_t"}


@pytest.mark.parametrize("c", T.CASES, ids=T.case_id)
def test_cases_against_the_reference(c):
    """Points on both sides of the 64-point tile (nothing at i + 32 may depend on point i), k around
    the 16-column slab, draws around the 64-draw tile, every nu and the cycle of all three, the
    first and the last seed and seeds with a non-zero high word, offsets; and every input form gives
    the bits of the plain call: host arrays, device tensors, column-major and padded lda / ldt
    through the raw ABI, a second call."""
    import torch
    n, S, A, y, th, off, seed, nus, t_rep, t_obs = T.case(c)
    out = run(A, y, th, seed, nus, offset=off)
    assert out["seed"] == seed and out["nu_estimated"] is isinstance(nus, np.ndarray)
    check(out, t_rep, t_obs, n, T.case_id(c))
    assert same_bits(out, run(A, y, th, seed, nus, offset=off)), "two calls"
    assert same_bits(out, run(A, y, torch.as_tensor(th.copy(), device="cuda:0"), seed, nus, offset=off)), "CUDA tensor"
    assert same_bits(out, via_abi(A, y, th, seed, nus, offset=off, col_major=True, pad_a=3, pad_t=2)), "col-major"
    assert same_bits(out, via_abi(A, y, th, seed, nus, offset=off, pad_a=2, pad_t=3, device=True)), "device, padded"
    if n == 3:
        assert np.all(np.abs(out["t_rep"][:, 5] + 1.5) <= BARS["grid"]["kurt"])


def test_biased_fit():
    """The replicated mean 150 sd from mean(y), t_4 noise: the moments about the draw's own centre
    lose nothing that the floor sees, and the fit is flagged."""
    n, S, A, y, th, off, seed, nu, t_rep, t_obs = T.biased_case()
    out = run(A, y, th, seed, nu)
    check(out, t_rep, t_obs, n, "biased delta=%g nu=%g" % (T.BIASED_DELTA, nu), "biased")
    assert out["p_value"]["mean"] == 1.0 and out["p_value"]["min"] == 1.0


def test_one_value_per_draw_is_the_single_nu_call():
    n, S, A, y, th, off, seed, nus, _, _ = T.case(T.CASES[3])          # 65 x 1, 130 draws, nu = 4
    assert same_bits(run(A, y, th, seed, nus), run(A, y, th, seed, np.full(S, nus)))
    assert same_bits(run(A, y, th, seed, nus), via_abi(A, y, th, seed, np.full(S, nus), device=True))


def test_a_draw_depends_on_its_own_nu_and_on_no_other_draw():
    n, S, A, y, th, off, seed, nus, _, _ = T.case(T.CASES[9])          # 65 x 16, 130 draws, the cycle
    whole = run(A, y, th, seed, nus, offset=off)
    part = run(A, y, th[:70], seed, nus[:70], offset=off)               # not on the draw count
    assert np.array_equal(whole["t_rep"][:70], part["t_rep"]) and np.array_equal(whole["t_obs"][:70], part["t_obs"])
    for j, nu in enumerate(T.NUS):                                      # nor on the other draws' nu
        one = run(A, y, th, seed, nu, offset=off)
        rows = np.arange(S) % 3 == j
        assert np.array_equal(one["t_rep"][rows], whole["t_rep"][rows]), nu
        assert not np.array_equal(one["t_rep"][~rows][:, 6], whole["t_rep"][~rows][:, 6]), nu
    assert not np.array_equal(run(A, y, th, seed + 1, nus, offset=off)["t_rep"], whole["t_rep"])


def test_without_nu_the_call_is_the_plain_gaussian_one():
    from pybmc_amd import posterior_predictive_check
    A, y, th, seed, t_rep, t_obs = P.case(65, 3, 130, 11)
    plain = posterior_predictive_check(A, y, th, seed=seed)
    explicit = posterior_predictive_check(A, y, th, seed=seed, nu=None, nu_draws=None)
    assert same_bits(plain, explicit) and plain["likelihood"] == "gaussian" and plain["nu_estimated"] is False
    assert plain["p_value"] == P.p_values(t_rep, t_obs)
    assert not np.array_equal(run(A, y, th, seed, 50.0)["t_rep"], plain["t_rep"])   # a stream of its own


# ---- bad input: the rules of the Gaussian check, one case each, n = 65, S = 70 -------------------------
BAD_N, BAD_K, BAD_S, BAD_SEED = 65, 3, 70, 4242


def bad_clean():
    A, y, th = P.make_case(BAD_N, BAD_K, BAD_S, 77)
    nus = T.case_nu(T.CYCLE, BAD_S)
    return A, y, th, nus, run(A, y, th, BAD_SEED, nus)


def test_a_bad_draw_is_nan_in_all_ten_values_and_spoils_no_other():
    A, y, th, nus, clean = bad_clean()
    assert np.isfinite(clean["t_rep"]).all() and np.isfinite(clean["t_obs"]).all()
    for d, column, value in ((67, 1, np.nan), (0, 3, 0.0), (BAD_S - 1, 0, np.inf)):
        t = th.copy()
        t[d, column] = value
        out = run(A, y, t, BAD_SEED, nus)
        assert np.isnan(out["t_rep"][d]).all() and np.isnan(out["t_obs"][d, 6:]).all(), d
        keep = np.arange(BAD_S) != d
        assert np.array_equal(out["t_rep"][keep], clean["t_rep"][keep]), d
        assert np.array_equal(out["t_obs"][keep], clean["t_obs"][keep]), d
        r, o = T.reference(A, y, t, BAD_SEED, nus)
        assert np.array_equal(np.isnan(out["t_rep"]), np.isnan(r)) and np.array_equal(np.isnan(out["t_obs"]), np.isnan(o))


def test_nan_in_a_point_spoils_what_it_enters():
    A, y, th, nus, clean = bad_clean()
    An = A.copy()
    An[64, 2] = np.nan                       # the one point of the partly filled last tile
    out = run(An, y, th, BAD_SEED, nus)
    assert np.isnan(out["t_rep"][:, :6]).all() and np.isnan(out["t_obs"][:, 6:]).all()
    assert np.array_equal(out["t_rep"][:, 6:], clean["t_rep"][:, 6:])
    yn = y.copy()
    yn[5] = np.nan
    out = run(A, yn, th, BAD_SEED, nus)
    assert np.isnan(out["t_obs"]).all() and np.array_equal(out["t_rep"], clean["t_rep"])
    off = np.zeros(BAD_N)
    off[63] = np.nan
    out = run(A, y, th, BAD_SEED, nus, offset=off)
    assert np.isnan(out["t_rep"][:, :6]).all() and np.isnan(out["t_obs"][:, :6]).all()
    assert np.array_equal(out["t_rep"][:, 6:], clean["t_rep"][:, 6:])
    assert np.array_equal(out["t_obs"][:, 6:], clean["t_obs"][:, 6:])


def test_c_abi_refuses_bad_arguments():
    import torch
    from pybmc_amd import _lib
    ctx = _lib.default_context(0)
    A, y, th = P.make_case(33, 1, 70, 7)
    common = (A, 33, 1, 1, 0, y, th, 70, 2, None, 0)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="nu must be positive and finite"):
            ctx.ppc_t(*common, bad)
    with pytest.raises(ValueError, match="n_points"):
        ctx.ppc_t(A, 2, 1, 1, 0, y, th, 70, 2, None, 0, 4.0)
    idx = (np.arange(70) % 2).astype(np.int32)
    for vals in ([4.0, 0.0], [4.0, np.nan], [np.inf, 4.0], [-1.0, 2.0]):
        with pytest.raises(ValueError, match="nu_values must be positive and finite"):
            ctx.ppc_tv(*common, np.array(vals), idx)
    for bad in (-1, 2, 2 ** 30):                      # host index: before anything runs
        with pytest.raises(ValueError, match="nu_index must index"):
            ctx.ppc_tv(*common, np.array([4.0, 5.0]), np.r_[idx[:69], bad].astype(np.int32))
    with pytest.raises(ValueError, match="n_values must be >= 1"):
        ctx.ppc_tv(*common, np.empty(0), idx)
    with pytest.raises(ValueError, match="n_values must be at most 4096"):
        ctx.ppc_tv(*common, np.linspace(1, 2, 4097), idx)
    ok = ctx.ppc_tv(*common, np.linspace(1, 2, 4096), idx)      # the limit itself is taken
    assert np.isfinite(ok["t_rep"]).all()
    Ad, yd, td = (torch.as_tensor(a, device="cuda:0") for a in (A, y, th))
    bidx = torch.as_tensor(np.r_[idx[:69], 7].astype(np.int32), device="cuda:0")
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="nu_index must index"):   # device index: clamped, reported after
        ctx.ppc_tv_device(Ad.data_ptr(), 33, 1, 1, 0, yd.data_ptr(), td.data_ptr(), 70, 2, None, 0,
                          np.array([4.0, 5.0]), bidx.data_ptr())


# ---- the planted 200 x 3 problem ---------------------------------------------------------------------------
def planted_bmc():
    """A BayesianModelCombination standing on robust_reference.planted_problem(200, 3, 0.05, 11): the
    orthonormal design as U_hat, the planted targets as the centred truth, no offset."""
    import pandas as pd
    from pybmc_amd import BayesianModelCombination
    y, X, prior, _, planted = RR.planted_problem(200, 3, 0.05, 11)
    df = pd.DataFrame({"a": [0.0], "b": [0.0], "c": [0.0], "d": [0.0], "truth": [0.0]})
    b = BayesianModelCombination(["a", "b", "c", "d"], {"p": df}, truth_column_name="truth")
    b.U_hat = X
    b.S_hat = np.sqrt(np.diag(prior[1]))
    b.Vt_hat = np.zeros((3, 4))
    b.centered_experiment_train = y
    b._predictions_mean_train = np.zeros(200)
    return b, y, X


def test_check_of_three_fits_of_the_planted_problem():
    """4 chains, 2 000 sweeps, the first 200 of each dropped by the check; b.check() after a Gaussian fit, a Student-t fit with nu = 4
    and one that estimates nu.  Every p-value equals the long-double reference's on the same draws
    and seed.  The reference run is computed and printed first, and a direction is asserted only
    where the reference clears its threshold by 0.02: expected are max_abs_z and kurt outside
    [0.02, 0.98] for the Gaussian fit and all eight inside (0.02, 0.98) for the estimated-nu fit; the
    nu = 4 row is printed, not asserted."""
    b, y, X = planted_bmc()
    common = {"iterations": 2000, "n_chains": 4, "seeds": [21, 22, 23, 24]}
    fits = (("gaussian", {}), ("t4", {"sampler": "student_t", "nu": 4}),
            ("t_est", {"sampler": "student_t", "nu": "estimate"}))
    for tag, opts in fits:
        b.train(dict(common, **opts))
        th = np.asarray(b.samples, dtype=np.float64).reshape(4, 2000, 4)[:, 200:].reshape(-1, 4)
        if tag == "gaussian":
            t_rep, t_obs = P.reference(X, y, th, 99)
        else:
            nus = np.asarray(b.nu_samples, dtype=np.float64).reshape(4, 2000)[:, 200:].reshape(-1) if tag == "t_est" else 4.0
            t_rep, t_obs = T.reference(X, y, th, 99, nus)
        want = P.p_values(t_rep, t_obs)
        margin = float(P.margins(t_rep, t_obs).min())
        print(f"{tag}: {th.shape[0]} draws, median sigma {np.median(th[:, -1]):.3f}, reference p "
              + " ".join(f"{k} {v:.4f}" for k, v in want.items()) + f"; smallest margin {margin:.2e}")
        out = b.check(burn=200, seed=99)
        print(f"{tag}: device    p " + " ".join(f"{k} {v:.4f}" for k, v in out["p_value"].items()))
        assert out["n_draws"] == th.shape[0] == 7200 and out["n_points"] == 200
        assert out["likelihood"] == ("gaussian" if tag == "gaussian" else "student_t")
        assert out["nu_estimated"] is (tag == "t_est")
        if tag == "t_est":
            print(f"t_est: median nu {np.median(nus):.2f}, mean {out['nu']:.3f}")
            assert out["nu"] == pytest.approx(float(np.mean(nus)), rel=1e-14)
        assert margin > P.MARGIN_FLOOR, margin     # ten times the widest bar: the p-values must be equal
        assert out["p_value"] == want, tag
        if tag == "gaussian":      # expected outside [0.02, 0.98]; clear of it by 0.02 means at 0 or 1
            for key in ("max_abs_z", "kurt"):
                if want[key] <= 0.0 or want[key] >= 1.0:
                    assert not 0.02 <= out["p_value"][key] <= 0.98, (tag, key)
                else:
                    print(f"{tag}: {key} not asserted: the reference gives {want[key]:.4f}")
        if tag == "t_est":         # expected inside (0.02, 0.98); clear of its ends by 0.02
            for key, v in want.items():
                if 0.04 <= v <= 0.96:
                    assert 0.02 < out["p_value"][key] < 0.98, (tag, key)
                else:
                    print(f"{tag}: {key} not asserted: the reference gives {v:.4f}")
