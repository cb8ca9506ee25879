"""Every width class, chunk edge, staging flush and grid-stride trip of the cross-validation kernels
on the device (-m gpu): the rows of tests/cv_class_cases.py through pybmc_amd.cv.kfold_cv and
cv_component_path.  tests/test_cv_classes_host.py proves on the CPU that each row reaches what the
table says.

Bars (none taken from the code under test; those of test_cv_gpu.py and test_cvpath_gpu.py):
  chains   against gibbs_sampler on the training rows under the same seed, the data-pass loop:
           1e-8 x the column's scale.  All chains where a case has at most 16, the chains of
           cv_class_cases.PICKS otherwise (both sides of every boundary the case is about);
  scores   elpd_cv_i of EVERY row against cv_reference.cv_reference (numpy on the returned draws):
           1e-11 max(1, |ref|); cv_mean_i against A[held] @ mean(draws): 1e-12 relative to the fold's
           largest |mean|; the summary against cv_reference.summary, rel 1e-13; n_fold exactly.
           unrotate_wrap pools 19 200 draws where the 1e-12 was argued for 600: its reference mean is
           formed in long double, and the bar is the larger of 1e-12 and 100 x the distance of
           numpy's float64 mean from it on the same draws;
  bits     a shorter run is the prefix of a longer one under the same seeds; strided views of A, and
           repeated calls, give the same bits; every candidate of a path is kfold_cv on the leading
           columns.
Measured on the MI355X: chains 2.2e-14 / 1.6e-14 / 5.7e-14 / 4.1e-14 / 4.3e-14 / 4.3e-14 / 4.9e-13
(width_15 .. width_63), 7.9e-11 (nt4_tight; mean sigma draw / sigma 0.94), 1.0e-14 (chunk_edges),
2.3e-15 (loo), 6.6e-16 (max_folds), 1.2e-13 (gather_wrap), 1.1e-13 (unrotate_wrap, chains 0, 107,
108, 127), 3.1e-15 / 5.0e-15 / 5.0e-15 / 5.0e-15 / 5.3e-15 (t_edges, T = 1, 63, 64, 65, 128), path
9.2e-14 (tile_fill, 14 chains) and 1.2e-14 (split_classes, 8 chains).  elpd_cv_i at most 2.2e-15
(unrotate_wrap; 1.3e-15 elsewhere; 8.9e-16 on the 786 rows of gather_wrap behind the wrap).
cv_mean_i at most 1.1e-15 where folds hold several rows; in the one-row folds the scale is the
row's own |mean|, which can cancel: 1.0e-14 (loo) and 5.7e-13 (max_folds, 1024 rows of two
columns).  unrotate_wrap: numpy's float64 mean lies 3.5e-15 from the long-double one, so the bar
stays 1e-12; the device is 7.5e-16 from the long-double one.  No element differs in any of the
bit-for-bit comparisons.  Every test runs in under 0.3 s.
"""
import os
import re

import numpy as np
import pytest

import cv_class_cases as CC
import cv_reference as CV
import test_cv_gpu as G
import test_cvpath_gpu as P
from pybmc_amd import cv

pytestmark = pytest.mark.gpu

TOL_CHAIN, TOL_ELPD, TOL_MEAN = G.TOL_CHAIN, G.TOL_ELPD, G.TOL_MEAN


def _constant(name):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "pybmc_amd", "csrc", "bmc_cv_plan.h")).read()
    return int(re.search(name + r" = (\d+);", text).group(1))


STRIDE = _constant("CV_STRIDE_BLOCKS") * _constant("CV_STRIDE_THREADS")   # elements of one grid-stride trip
_runs, _t_runs, _path_runs = {}, {}, {}


def run(name):
    """One kfold_cv call per row of the table, shared by the tests and left unchanged."""
    if name not in _runs:
        A, y, prior, folds, F, C, T = CC.case(name)
        out = cv.kfold_cv(A, y, prior, folds, T, n_chains=C, seed=5, return_draws=True)
        _runs[name] = (A, y, prior, folds, F, C, T, out)
    return _runs[name]


def t_run(T):
    """The t_edges runs: cv_reference's `unequal` with two chains and T iterations."""
    if T not in _t_runs:
        A, y, prior, folds, F, C = CC.t_edge_case()
        out = cv.kfold_cv(A, y, prior, folds, T, n_chains=C, seed=5, return_draws=True)
        _t_runs[T] = (A, y, prior, folds, F, C, T, out)
    return _t_runs[T]


def check_chains(tag, A, y, prior, folds, F, C, T, out, picks=None):
    assert out["draws"].shape == (F, C, T, A.shape[1] + 1) and out["seeds"].shape == (F, C)
    assert np.isfinite(out["draws"]).all()
    chains = range(F * C) if picks is None else picks
    assert picks is not None or F * C <= 16
    worst = 0.0
    for g in chains:
        f, c = divmod(g, C)
        worst = max(worst, G.chain_error(out["draws"][f, c], A, y, prior, folds, f, out["seeds"][f, c], T))
    print(f"{tag}: worst chain difference / column scale = {worst:.3e} over {len(chains)} chains (bar {TOL_CHAIN:.0e})")
    assert worst < TOL_CHAIN


def check_scores(tag, A, y, folds, F, C, T, out, long_double_mean=False):
    """elpd_cv_i and cv_mean_i of every row, the summary and the counts; returns the two row-wise
    error vectors (elpd relative to max(1, |ref|), mean relative to the fold's largest |mean|)."""
    elpd, mean = CV.cv_reference(A, y, folds, F, out["draws"])
    err_e = np.abs(out["elpd_cv_i"] - elpd) / np.maximum(1.0, np.abs(elpd))
    tol_mean = TOL_MEAN
    if long_double_mean:
        mean_ld = np.empty(len(y), dtype=np.longdouble)
        for f in range(F):
            th = out["draws"][f].reshape(-1, out["draws"].shape[-1])[:, :-1].astype(np.longdouble)
            mean_ld[folds == f] = A[folds == f].astype(np.longdouble) @ th.mean(axis=0)
        between = max(float(np.abs(mean[folds == f] - mean_ld[folds == f]).max() / np.abs(mean_ld[folds == f]).max())
                      for f in range(F))
        tol_mean = max(TOL_MEAN, 100.0 * between)
        print(f"{tag}: numpy's float64 mean is {between:.3e} from the long-double one: bar {tol_mean:.3e}")
        mean = mean_ld
    err_m = np.empty(len(y))
    for f in range(F):
        held = folds == f
        err_m[held] = (np.abs(out["cv_mean_i"][held] - mean[held]) / np.abs(mean[held]).max()).astype(np.float64)
    print(f"{tag}: elpd_cv_i {err_e.max():.3e} (bar {TOL_ELPD:.0e}), cv_mean_i {err_m.max():.3e} (bar {tol_mean:.3e}), "
          f"all {len(y)} rows")
    assert np.isfinite(out["elpd_cv_i"]).all() and np.isfinite(out["cv_mean_i"]).all()
    assert err_e.max() <= TOL_ELPD and err_m.max() <= tol_mean
    ref = CV.summary(y, folds, F, out["elpd_cv_i"], out["cv_mean_i"])
    for key in ("elpd_cv", "se", "cv_rmse"):
        assert out[key] == pytest.approx(ref[key], rel=1e-13)
    assert np.array_equal(out["n_fold"], ref["n_fold"]) and out["n_fold"].sum() == len(y)
    assert out["n_points"] == len(y) and out["n_folds"] == F and out["n_draws"] == C * T
    return err_e, err_m, tol_mean


@pytest.mark.parametrize("name", list(CC.CASES))
def test_chains_are_the_subsets_chains(name):
    A, y, prior, folds, F, C, T, out = run(name)
    check_chains(name, A, y, prior, folds, F, C, T, out, CC.PICKS.get(name))
    if name == "nt4_tight":
        # the assertion of test_cv_gpu.py's tight_scaled: no floor binds, so sigma is the data's.
        # n_train = 120 rows and 50 coefficients put E sigma^2 near 70/119 of the true one
        # (sigma x 0.77); a cancelled rss0 would be off by orders of magnitude
        n, k, _, _, _, snr, scale = CC.CASES[name]
        sig = CV.problem(n, k, snr, scale)[3]
        ratio = out["draws"][..., -1].mean() / sig
        print(f"{name}: sigma^2 = {sig ** 2:.3e}, mean sigma draw / sigma = {ratio:.3f} (0.5 .. 1.5)")
        assert sig ** 2 > 1e-5 and 0.5 < ratio < 1.5


@pytest.mark.parametrize("name", list(CC.CASES))
def test_scores_of_every_row(name):
    A, y, prior, folds, F, C, T, out = run(name)
    err_e, err_m, tol_mean = check_scores(name, A, y, folds, F, C, T, out, long_double_mean=name == "unrotate_wrap")
    if name == "gather_wrap":
        # the gathered rows with an element at or behind 8192 x 256 of Z: the second trip of the
        # gather's loop.  Fold order puts them at the end of fold 1: its last 786 rows
        behind = CC.rows_behind(folds, F, A.shape[1], STRIDE)
        last = np.flatnonzero(folds == 1)[-len(behind):]
        assert len(behind) == 786 and np.array_equal(behind, last)
        print(f"{name}: the {len(behind)} rows behind element {STRIDE}: elpd_cv_i {err_e[behind].max():.3e}, "
              f"cv_mean_i {err_m[behind].max():.3e}")
        assert err_e[behind].max() <= TOL_ELPD and err_m[behind].max() <= tol_mean


@pytest.mark.parametrize("T", CC.T_EDGES)
def test_staging_flush_at_every_edge(T):
    """T = 63, 64, 65 and 128 around the 64-row staging of cv_chain, and T = 1: with two chains the
    two pooled draws the C ABI asks for.  All 10 chains and every row's scores."""
    A, y, prior, folds, F, C, T, out = t_run(T)
    check_chains(f"t_edges T={T}", A, y, prior, folds, F, C, T, out)
    check_scores(f"t_edges T={T}", A, y, folds, F, C, T, out)


@pytest.mark.parametrize("T", [t for t in CC.T_EDGES if t < 128])
def test_a_shorter_run_is_the_prefix_of_the_longest(T):
    """The variates are prefix-stable (test_rng_streams_gpu.py), so under the same seeds iteration t
    does not depend on T: a flush at the wrong row, or of the wrong count, would show here."""
    long, short = t_run(128)[-1], t_run(T)[-1]
    assert np.array_equal(long["seeds"], short["seeds"])
    differ = int((short["draws"] != long["draws"][:, :, :T]).sum())
    print(f"t_edges T={T}: {differ} of {short['draws'].size} elements differ from the prefix of T=128")
    assert np.array_equal(short["draws"], long["draws"][:, :, :T])


def test_strided_views_of_A_give_the_same_bits():
    """_host_matrix hands a view with lda > k (row-major) or lda > n (column-major) to the C ABI in
    place; the space between the rows / columns is NaN, so one element read at the wrong stride or
    one byte too few uploaded cannot go unnoticed."""
    A, y, prior, folds, F, C, T, base = t_run(128)
    n, k = A.shape
    big = np.full((n, k + 7), np.nan)
    big[:, 3:3 + k] = A
    row_view = big[:, 3:3 + k]
    assert row_view.strides == (8 * (k + 7), 8) and not row_view.flags["C_CONTIGUOUS"]
    bigF = np.full((n + 5, k), np.nan, order="F")
    bigF[:n] = A
    col_view = bigF[:n, :]
    assert col_view.strides == (8, 8 * (n + 5)) and not col_view.flags["F_CONTIGUOUS"]
    for tag, view in (("row-major, lda = k + 7", row_view), ("column-major, lda = n + 5", col_view)):
        got = cv.kfold_cv(view, y, prior, folds, T, n_chains=C, seed=5, return_draws=True)
        differ = sum(int((np.asarray(got[key]) != np.asarray(base[key])).sum()) for key in base)
        print(f"{tag}: {differ} elements differ from the contiguous call")
        assert set(got) == set(base) and G.same(base, got)
    path = cv.cv_component_path(A, y, prior, folds, T, n_chains=C, seed=5, return_draws=True)
    got = cv.cv_component_path(row_view, y, prior, folds, T, n_chains=C, seed=5, return_draws=True)
    assert P.same(path, got)
    assert np.array_equal(got["draws"][-1], base["draws"])
    assert np.array_equal(got["elpd_cv_i"][-1], base["elpd_cv_i"]) and np.array_equal(got["cv_mean_i"][-1], base["cv_mean_i"])


@pytest.mark.parametrize("name", ["gather_wrap", "max_folds"])
def test_the_largest_calls_repeat_bit_for_bit(name):
    A, y, prior, folds, F, C, T, out = run(name)
    again = cv.kfold_cv(A, y, prior, folds, T, n_chains=C, seed=5, return_draws=True)
    assert set(again) == set(out) and G.same(out, again)


# ---- the component path ------------------------------------------------------------------------------
def path_run(name):
    """One cv_component_path call per row of PATH_CASES and the kfold_cv call of every candidate."""
    if name not in _path_runs:
        A, y, prior, folds, C, T, comps, picks = CC.path_case(name)
        out = cv.cv_component_path(A, y, prior, folds, T, components=comps, n_chains=C, seed=5, return_draws=True)
        singles = [cv.kfold_cv(np.ascontiguousarray(A[:, :k]), y, P.sub_prior(prior, k), folds, T, n_chains=C,
                               seeds=out["seeds"], return_draws=True) for k in out["components"]]
        _path_runs[name] = (A, y, prior, folds, C, T, comps, picks, out, singles)
    return _path_runs[name]


@pytest.mark.parametrize("name", list(CC.PATH_CASES))
def test_every_candidate_of_a_path_is_the_single_call(name):
    A, y, prior, folds, C, T, comps, picks, out, singles = path_run(name)
    assert np.array_equal(out["components"], comps)
    F = int(folds.max()) + 1
    for j, k in enumerate(out["components"]):
        one = singles[j]
        assert out["draws"][j].shape == (F, C, T, k + 1)
        for key, got in (("draws", out["draws"][j]), ("elpd_cv_i", out["elpd_cv_i"][j]), ("cv_mean_i", out["cv_mean_i"][j])):
            differ = int((np.asarray(got) != one[key]).sum())
            print(f"{name} k={k} {key}: {differ} of {one[key].size} elements differ from kfold_cv")
        assert np.array_equal(out["draws"][j], one["draws"])
        assert np.array_equal(out["elpd_cv_i"][j], one["elpd_cv_i"])
        assert np.array_equal(out["cv_mean_i"][j], one["cv_mean_i"])


@pytest.mark.parametrize("name", list(CC.PATH_CASES))
def test_path_chains_are_the_subsets_chains(name):
    A, y, prior, folds, C, T, comps, picks, out, singles = path_run(name)
    F = int(folds.max()) + 1
    worst, count = 0.0, 0
    for j, k in enumerate(out["components"]):
        assert np.isfinite(out["draws"][j]).all()
        Ak, pk = np.ascontiguousarray(A[:, :k]), P.sub_prior(prior, k)
        chains = [divmod(g, C) for g in range(F * C)] if picks is None else \
            [divmod(g - j * F * C, C) for g in picks if j * F * C <= g < (j + 1) * F * C]
        for f, c in chains:
            worst = max(worst, G.chain_error(out["draws"][j][f, c], Ak, y, pk, folds, f, out["seeds"][f, c], T))
        count += len(chains)
    print(f"path {name}: worst chain difference / column scale = {worst:.3e} over {count} chains (bar {TOL_CHAIN:.0e})")
    assert count == (len(picks) if picks else len(comps) * F * C)
    assert worst < TOL_CHAIN
