"""Posterior predictive checks of a sampled fit on the GPU: do data replicated from the fitted
model look like the observed data?

The reference package has no such check; this is a capability of this build.  The model is the
one the samplers draw from, ``y_i ~ N(a_i . beta, sigma^2)`` (the Student-t one: below).  For design rows ``A`` (n x k),
targets ``y``, offsets and S posterior draws ``(beta_s, sigma_s)``, replicated data are

    y_rep[i, s] = a_i . beta_s + sigma_s z[i, s] + offset_i

with ``z[i, s]`` a standard normal that depends on ``(seed, i, s)`` alone (the
fifth variate stream: Philox4x32-10 keyed by the seed, counter ``(s lo, s hi, "PPCS", pair(i))``,
``pair(i) = (i >> 6) * 32 + (i & 31)``, Box-Muller, the cosine half to the point with bit 5 of i
clear, the sine half to point i + 32).  Eight test quantities are taken per draw, ``PPC_STATS``:

* ``min``, ``max``, ``mean``, ``sd``, ``skew``, ``kurt``: ``T_rep[s]`` of ``y_rep[:, s]``, ``T_obs`` the
  same function of ``y + offset`` (constant in s; host, float64).  With ``m_r = mean((x - mean x)^r)``
  (ddof 0): ``sd = sqrt(m2)``, ``skew = m3 / m2^1.5``, ``kurt = m4 / m2^2 - 3``.
* ``chi2``: ``T_rep[s] = sum_i z[i, s]^2``, ``T_obs[s] = sum_i ((y_i - a_i . beta_s) / sigma_s)^2``.
* ``max_abs_z``: ``T_rep[s] = max_i |z[i, s]|``, ``T_obs[s] = max_i |y_i - a_i . beta_s| / sigma_s``.

The Bayesian p-value of a quantity is ``mean_s 1[T_rep[s] >= T_obs[s]]`` (A. Gelman, X.-L. Meng,
H. Stern, "Posterior predictive assessment of model fitness via realized discrepancies",
Statistica Sinica 6, 1996): values near 0 or 1 say that the data are unlike what the fit
replicates -- a noise model too narrow (``chi2``, ``sd`` near 0) or too wide (near 1), skewed or
heavy-tailed residuals (``skew``, ``kurt``), a single outlier (``max_abs_z``, ``min``, ``max``).
At least 3 points are needed; with exactly 3 ``kurt`` is -3/2 for any data, so its p-value compares
two equal numbers and says nothing.

With ``nu=`` or ``nu_draws=`` the same check is of a Student-t fit (``gibbs_sampler_robust``,
``train({"sampler": "student_t"})``): ``y_i ~ a_i . beta + sigma t_nu``, and ``z[i, s]`` is a
Student-t variate with ``nu`` (``nu_s`` with ``nu_draws``) degrees of freedom, made on the device
by Bailey's polar form (the eighth variate stream: counter ``(s lo, s hi, "PPCT",
i)``, the point index itself, ``z = sqrt(nu expm1(-(2 / nu) log u1)) cos(2 pi u2)``; only the
cosine half, since the sine half shares its radius).  It depends on ``(seed, i, s, nu_s)`` alone.
The eight quantities and their definitions do not change; what they mean for a t fit:

* ``sigma_s`` is the SCALE of the t noise, not its standard deviation (which is
  ``sigma sqrt(nu / (nu - 2))`` for ``nu > 2`` and infinite below), so ``chi2`` and ``max_abs_z``
  compare the standardised t variates ``z`` with the standardised residuals
  ``(y_i - a_i . beta_s) / sigma_s``: under the model both are ``t_nu``.  ``chi2`` is no longer
  chi-squared distributed -- its replicated values are heavy-tailed sums -- but it is the same
  function of replicated and observed data, which is all a posterior predictive p-value needs.
* For ``nu <= 4`` the kurtosis, for ``nu <= 3`` the skewness and for ``nu <= 2`` the variance of the
  replicated data have no finite expectation: ``sd``, ``skew`` and ``kurt`` are then statistics of
  the n replicated values at hand, widely spread over the draws, and a p-value near 0 or 1 says
  the more for it.

The check is what says whether ``nu`` is small enough.  On the planted problem of the robust
sampler's tests (200 x 3, 5 % of the targets shifted by 8 to 16 sigma; 4 chains of 2 000 sweeps,
the first 200 of each dropped, MI355X; every p-value equal to the long-double reference's):

    fit                      sigma   p(sd)    p(kurt)  p(chi2)  p(max_abs_z)
    Gaussian                 0.293   0.510    0.005    0.489    0.000
    t, nu = 4 (the default)  0.101   0.001    0.008    0.001    0.016
    t, nu estimated (1.8)    0.081   0.250    0.393    0.322    0.532

The Gaussian fit is flagged by its tails (``kurt``, ``max_abs_z``).  The ``nu = 4`` fit is still
rejected: its sigma has shrunk to the clean rows, and ``t_4`` tails at that scale do not reach the
planted ones.  The fit that estimated ``nu`` passes all eight.

On the device (``kernels_ppc.hip``) the n x S matrix is never stored: the f64 MFMA GEMM of the
scoring kernels with the noise made in the epilogue and the tile reduced over the points, per
draw; one workgroup per 64 draws and no combine across workgroups, so the result does not depend
on the device.  The moments come from power sums of ``y_rep[:, s] - c_s`` about the draw's own
centre ``c_s = mean_i(a_i) . beta_s + mean(offset)``, formed on the device, so that a fit whose
predictions are biased loses nothing of ``skew`` and ``kurt`` to cancellation.

Non-finite input is data, and a value is NaN exactly where the definitions above give NaN (``min``
and ``max`` of values with a NaN among them are NaN, as numpy's are):

* A draw with a non-finite coefficient, or without a finite ``sigma_s > 0``, is NaN in all ten of
  its values (the eight of ``t_rep`` and the observed ``chi2`` and ``max_abs_z``), as the scoring
  and sensitivity calls treat such a draw.  Every other draw is what it is without it.
* A NaN in ``A[i, :]`` makes ``min`` .. ``kurt`` of ``t_rep`` and the observed ``chi2`` and
  ``max_abs_z`` NaN for every draw; the replicated ``chi2`` and ``max_abs_z`` do not read ``A``.
* A NaN in ``y[i]`` makes ``t_obs`` NaN and leaves ``t_rep`` as it is; ``+inf`` there makes the
  observed ``chi2`` and ``max_abs_z`` ``+inf``.
* A NaN in ``offset[i]`` makes the six marginal columns of ``t_rep`` and ``t_obs`` NaN and nothing
  else.
* A NaN is never ``>=``: such a draw does not count towards a p-value.

Out of scope: per-point posterior predictive p-values.  They reduce along the other axis, and they
use every point twice (to fit and to check); ``psis_loo_predict()["loo_pit"]`` is the honest
version of those.
"""
from __future__ import annotations

import numpy as np

from .scoring import _likelihood_call, _pointwise_call

PPC_STATS = ("min", "max", "mean", "sd", "skew", "kurt", "chi2", "max_abs_z")
MIN_POINTS = 3


def marginal_stats(x):
    """``min, max, mean, sd, skew, kurt`` of a vector as defined in the module docstring (host,
    float64, moments about the mean with ddof 0)."""
    x = np.asarray(x, dtype=np.float64)
    mean = float(np.mean(x))
    d = x - mean
    m2, m3, m4 = (float(np.mean(d ** r)) for r in (2, 3, 4))
    return np.array([np.min(x), np.max(x), mean, np.sqrt(m2), m3 / m2 ** 1.5, m4 / m2 ** 2 - 3.0])


def ppc_summary(t_rep, t_obs):
    """``{name: p-value}`` for the columns of ``t_rep`` and ``t_obs`` (both ``(S, 8)``, columns
    ``PPC_STATS``): the share of draws with ``t_rep >= t_obs`` (host)."""
    t_rep = np.asarray(t_rep, dtype=np.float64)
    t_obs = np.asarray(t_obs, dtype=np.float64)
    if t_rep.ndim != 2 or t_rep.shape[1] != len(PPC_STATS) or t_obs.shape != t_rep.shape:
        raise ValueError(f"t_rep and t_obs must both be (n_draws, {len(PPC_STATS)}); got "
                         f"{t_rep.shape} and {t_obs.shape}")
    if t_rep.shape[0] < 1:
        raise ValueError("t_rep must hold at least one draw")
    return {name: float(np.mean(t_rep[:, j] >= t_obs[:, j])) for j, name in enumerate(PPC_STATS)}


def _draw_seed():
    # (as sampling_utils.rndm_m_random_calculator: 64 bits of numpy's global stream)
    return int(np.random.randint(0, 2 ** 32, dtype=np.uint64)) << 32 | int(
        np.random.randint(0, 2 ** 32, dtype=np.uint64))


def posterior_predictive_check(A, y, samples, burn=0, thin=1, offset=None, seed=None, device=0,
                               nu=None, nu_draws=None):
    """Posterior predictive check of a fit (module docstring).

    ``A``, ``y``, ``samples``, ``burn``, ``thin`` and ``device`` as
    ``pointwise_log_likelihood``, with at least 3 points.  ``offset`` is ``(n_points,)`` float64
    (default zeros): added to the replicated and to the observed data of the six marginal
    quantities, so that they can be read in the units of an un-centred target.  ``seed`` (uint64)
    fixes the replicated noise; None draws one from numpy's global stream, and it is returned.
    ``nu`` and ``nu_draws`` as ``pointwise_log_likelihood``: ``nu=None, nu_draws=None`` replicates
    Gaussian noise; a positive finite ``nu`` Student-t noise with that many degrees of freedom;
    ``nu_draws`` (instead of ``nu``) Student-t noise with a ``nu`` per draw, for a fit that
    estimated it (shaped like the leading dimensions of ``samples``, at most 4096 distinct values).

    Returns a dict: ``p_value`` (``{name: p}`` for ``PPC_STATS``), ``t_rep`` and ``t_obs``
    (``(n_draws, 8)``; the marginal columns of ``t_obs`` repeat one value), ``stats``
    (``PPC_STATS``), ``n_points``, ``n_draws``, ``seed``, ``likelihood`` (``"gaussian"`` or
    ``"student_t"``) and ``nu_estimated`` (True with ``nu_draws``).  Per-point p-values are out of
    scope: see ``psis_loo_predict()["loo_pit"]``."""
    if seed is None:
        seed = _draw_seed()
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < 2 ** 64:
        raise ValueError("seed must be an integer in [0, 2^64) or None")
    seed = int(seed)

    host, dev, noise, held = _likelihood_call("ppc", nu, nu_draws, samples, burn, thin)
    if not noise:
        noise = (0.0,)   # (the C ABI's `center`, which the device no longer reads)
    out = _pointwise_call(host, dev, A, y, samples, burn, thin, device, min_points=MIN_POINTS,
                          vectors=(("offset", offset),), scalars=(seed,) + tuple(noise))
    del held
    y = np.asarray(y)
    obs = marginal_stats(y if offset is None else y + np.asarray(offset))
    t_rep = out["t_rep"]
    t_obs = np.empty_like(t_rep)
    t_obs[:, :6] = obs
    t_obs[:, 6:] = out["t_obs2"]
    return {"p_value": ppc_summary(t_rep, t_obs), "t_rep": t_rep, "t_obs": t_obs,
            "stats": PPC_STATS, "n_points": int(y.shape[0]), "n_draws": int(t_rep.shape[0]),
            "seed": seed, "likelihood": "gaussian" if nu is None and nu_draws is None else "student_t",
            "nu_estimated": nu_draws is not None}
