"""Host-side mirror of the reference's ``pybmc/sampling_utils.py`` surface."""
from __future__ import annotations

import numpy as np

from . import _lib

N_PREDICTIVE_DRAWS = 10000  # reference sampling_utils.py:57


def _choose(rng, samples, noise_df):
    """The 10000 rows of ``samples`` the generator picks (``choice`` picks rows by count alone), and
    the degrees of freedom of their noise: ``noise_df`` itself, or, when it is one value per row of
    ``samples`` (a fit with nu estimated), the chosen rows' values as a (10000, 1) column."""
    if noise_df is None or np.ndim(noise_df) == 0:
        return rng.choice(samples, N_PREDICTIVE_DRAWS, replace=False), noise_df     # :57
    df = np.asarray(noise_df, dtype=np.float64).reshape(-1)
    if df.shape[0] != samples.shape[0]:
        raise ValueError("noise_df must be a number or one value per row of samples")
    both = rng.choice(np.column_stack([samples, df]), N_PREDICTIVE_DRAWS, replace=False)
    return np.ascontiguousarray(both[:, :-1]), both[:, -1:]


def _t_noise(rng, noise_df, n_points):
    """Student-t predictive noise for the replay ``noise=`` argument of ``Context.predict``, drawn on
    the host from the generator that made the ``choice``, right after it (``noise_source="host"``).
    This path is host-bound: 80 kB of variates per point are generated and uploaded;
    ``noise_source="device"`` makes the noise in the predictive kernel instead."""
    if np.ndim(noise_df) == 0:
        noise_df = float(noise_df)
    if not np.all(np.asarray(noise_df) > 0):
        raise ValueError("noise_df must be positive")
    return rng.standard_t(noise_df, (N_PREDICTIVE_DRAWS, n_points))


def _noise_args(rng, noise_df, noise_source, n_points):
    """What ``Context.predict`` gets for the noise, as keywords: nothing (normal noise), the host's
    ``standard_t`` array as ``noise=``, or, for the device's own t variates, ``nu=`` / ``nu_draws=``
    (the chosen rows' values)."""
    if noise_df is None:
        return {}
    if noise_source == "host":
        return {"noise": _t_noise(rng, noise_df, n_points)}
    if np.ndim(noise_df) == 0:
        return {"nu": float(noise_df)}
    return {"nu_draws": np.ascontiguousarray(noise_df, dtype=np.float64).reshape(-1)}


def _check_noise_source(noise_source):
    if noise_source not in ("host", "device"):
        raise ValueError(f'noise_source must be "host" or "device"; got {noise_source!r}')


def rndm_m_random_calculator(filtered_model_predictions, samples, Vt_hat, *, seed=None,
                             device=0, noise_df=None, noise_source="host"):
    """Posterior-predictive draws and 2.5/50/97.5 % bands on the GPU
    (reference sampling_utils.py:40-84).

    Returns ``(rndm_m, [lower, median, upper])`` with ``rndm_m`` of shape
    ``(10000, n_points)`` (C-ordered, like the reference's: sampling_utils.py:77).  Needs at least 10000 posterior samples, like the
    reference (``ValueError`` otherwise, :57).  The reference's side effect of
    re-seeding numpy's global stream (:54, quirk Q2) is not reproduced.

    ``noise_df`` (after a Student-t fit, ``gibbs_sampler_robust``): the predictive noise is
    ``sigma_s * t_nu`` instead of ``sigma_s * z``.  ``noise_df`` may also hold one value per row
    of ``samples`` (a fit with nu estimated): the rows are then chosen from ``samples`` with that
    column appended, and draw s gets ``t`` noise of its own degrees of freedom.

    ``noise_source`` says where the t noise is made (ignored when ``noise_df`` is None):
    ``"host"`` (default) takes ``Generator(PCG64(seed)).standard_t(noise_df, (10000, n_points))``
    from the generator that made the ``choice``, right after it, and replays it through the
    predictive kernels: 80 kB of variates per point, generated and uploaded.  ``"device"`` makes
    the same ``choice`` and hands the chosen rows' degrees of freedom to the predictive kernel, which
    draws the variates itself from ``seed`` (``Context.predict(nu=)`` / ``nu_draws=``; every value
    finite and at least 0.06): nothing but the inputs is uploaded.  The two are different variates
    of the same distribution.
    """
    _check_noise_source(noise_source)
    preds = np.ascontiguousarray(filtered_model_predictions, dtype=np.float64)
    samples = np.ascontiguousarray(samples, dtype=np.float64)
    Vt_hat = np.ascontiguousarray(Vt_hat, dtype=np.float64)
    if samples.shape[0] < N_PREDICTIVE_DRAWS:
        raise ValueError("Cannot take a larger sample than population when replace is False")
    if seed is None:
        seed = int(np.random.randint(0, 2 ** 32, dtype=np.uint64)) << 32 | int(
            np.random.randint(0, 2 ** 32, dtype=np.uint64))
    ctx = _lib.default_context(device)
    rng = np.random.Generator(np.random.PCG64(seed))
    theta, noise_df = _choose(rng, samples, noise_df)
    noise = _noise_args(rng, noise_df, noise_source, preds.shape[0])
    with ctx.lock:
        rndm_m, bands, _ = ctx.predict(preds, theta, Vt_hat, seed=seed, **noise)
    return rndm_m, [bands[0], bands[1], bands[2]]


def predictive_coverage(percentiles, filtered_model_predictions, samples, Vt_hat, truth, *,
                        seed=None, device=0, noise_df=None, noise_source="host"):
    """``coverage(percentiles, rndm_m_random_calculator(...)[0], ...)`` fused on the GPU:
    the draws are sorted where they were produced and only the hit counts come back
    (what ``BayesianModelCombination.evaluate`` needs, reference bmc.py:366-376).  ``noise_df`` and
    ``noise_source``: Student-t noise as in ``rndm_m_random_calculator``, replayed from the host
    or made on the device."""
    _check_noise_source(noise_source)
    preds = np.ascontiguousarray(filtered_model_predictions, dtype=np.float64)
    samples = np.ascontiguousarray(samples, dtype=np.float64)
    if samples.shape[0] < N_PREDICTIVE_DRAWS:
        raise ValueError("Cannot take a larger sample than population when replace is False")
    if seed is None:
        seed = int(np.random.randint(0, 2 ** 32, dtype=np.uint64)) << 32 | int(
            np.random.randint(0, 2 ** 32, dtype=np.uint64))
    rng = np.random.Generator(np.random.PCG64(seed))
    theta, noise_df = _choose(rng, samples, noise_df)
    noise = _noise_args(rng, noise_df, noise_source, preds.shape[0])
    ctx = _lib.default_context(device)
    with ctx.lock:
        _, _, cov = ctx.predict(preds, theta, Vt_hat, seed=seed, q=(), truth=truth,
                                cov_percentiles=list(percentiles), want_draws=False, **noise)
    return cov


def coverage(percentiles, rndm_m, models_output, truth_column):
    """Share of points whose truth lies inside the central p % credible interval,
    for each p (reference sampling_utils.py:4-37).  Index arithmetic (truncation
    towards zero, p = 0 never covers) is the reference's; each column is sorted
    once instead of once per percentile."""
    rndm_m = np.asarray(rndm_m)
    n_draws, n_points = rndm_m.shape
    truth = np.asarray(models_output[truth_column].tolist())
    srt = np.sort(rndm_m, axis=0)
    res = []
    for p in percentiles:
        lo = int((0.5 - p / 200) * n_draws)
        hi = int((0.5 + p / 200) * n_draws) - 1
        inside = (srt[lo] <= truth) & (truth <= srt[hi])
        res.append(int(np.count_nonzero(inside)) / n_points * 100)
    return res
