"""Rank-normalised convergence diagnostics on the GPU: folded split R-hat, bulk-ESS, tail-ESS and
quantiles (Vehtari, Gelman, Simpson, Carpenter, Buerkner 2021; Stan's and ArviZ's defaults).

``C``, ``T``, ``burn``, ``T' = T - burn`` and ``n = T' // 2`` are those of ``diagnostics.py``.  A
column's *split draws* are the ``S = 2 C n`` values of its ``M = 2C`` half-chain sequences; with an
odd ``T'`` the middle draw of each chain takes no part in anything rank-based (it still counts for
``mean`` and ``sd``).  ``R`` and ``E`` below are exactly the split R-hat and the ESS of the
``diagnostics.py`` docstring, steps 1-5, floor included, applied to the ``M`` sequences of length
``n`` of a derived series.

* Rank normalisation ``z(v)`` of a series ``v`` over the ``S`` split draws: ``r`` is the 1-based
  rank of the value among the ``S``; equal values share the mean of the ranks they occupy
  (``scipy.stats.rankdata(method="average")``); equality is by value, ``-0.0`` ties with ``+0.0``;
  ``z = ndtri((r - 3/8) / (S + 1/4))``.
* Quantiles ``q_p`` for up to 16 probabilities ``p`` in [0, 1] (default ``(0.05, 0.5, 0.95)``):
  over the ``S`` split draws with numpy's ``method="linear"`` -- virtual index ``(S - 1) p``, its
  floor and fraction as ``_lib.order_stat_plan`` computes them, and the interpolation
  ``t >= 0.5 ? b - (b - a)(1 - t) : a + (b - a) t`` of the predictive leg.
* ``q05`` and ``q95`` are always computed, whatever ``p`` was asked for, and so is the median
  ``med = q_0.5`` (by that interpolation, not ``(a + b) / 2``); the folded series is
  ``f = |x - med|``.
* Per column: ``r_hat = max(R(z(x)), R(z(f)))``, ``ess_bulk = E(z(x))``,
  ``ess_tail = min(E(1[x <= q05]), E(1[x <= q95]))``, ``mcse_mean = sd / sqrt(ess_bulk)``;
  ``mean`` and ``sd`` are ``chain_diagnostics``'s, bit for bit.
* Values, not errors: a column with any non-finite value gets NaN in every rank-based output and
  in its quantiles; a derived series with ``W = 0`` (an all-equal column, an indicator constant
  within every half) gives NaN for the outputs built on it.

On the device (``kernels_rank.hip``), per batch of columns sized from the free memory: the split
draws become (64-bit order-preserving key, u32 index) pairs, one segment per column; a stable LSD
radix sort (8-bit digits, 4096-key tiles; digits that are constant in every segment are skipped)
orders them; runs of equal keys give the average ranks, ``ndtri`` (Wichura's AS 241, ``bmc_math.h``)
the z-scores, written back at the draw's own place; the same sorted keys give the quantiles; the
keys are folded in place and sorted again.  ``z(x)``, ``z(f)`` and the two indicators of a column
go into a buffer ``[C][2n][4]`` in the samplers' layout and the classic kernels of
``diagnostics.py`` run on it unchanged, column by column, so that nothing depends on the batch.
The only atomics are integer counters and masks: two calls return the same bits.
"""
from __future__ import annotations

import numpy as np

from .diagnostics import _prepare

KEYS = ("mean", "sd", "mcse_mean", "ess_bulk", "ess_tail", "r_hat", "quantiles")
MAX_PROBS = 16
DEFAULT_PROBS = (0.05, 0.5, 0.95)


def _check_probs(probs):
    p = np.atleast_1d(np.asarray(probs, dtype=np.float64))
    if p.ndim != 1 or not 1 <= p.size <= MAX_PROBS:
        raise ValueError(f"need between 1 and {MAX_PROBS} probabilities; got {p.size}")
    if not np.all((p >= 0.0) & (p <= 1.0)):
        raise ValueError("every probability must be inside [0, 1]")
    return p


def rank_diagnostics(samples, burn=0, probs=DEFAULT_PROBS, device=0, cols_per_batch=0):
    """Rank-normalised split R-hat, bulk / tail ESS, MCSE and quantiles of every column.

    ``samples`` follows the rules of ``chain_diagnostics``: float64, ``(T, P)`` or ``(C, T, P)``,
    a numpy array or a CUDA torch tensor with a contiguous last dimension (strided column subsets
    are read in place).  Returns a dict of ``[P]`` arrays ``mean``, ``sd``, ``mcse_mean``,
    ``ess_bulk``, ``ess_tail``, ``r_hat`` and ``quantiles`` of shape ``[len(probs), P]``.
    ``cols_per_batch`` (0: sized from the free device memory) does not change the results.  The
    estimator is the module docstring's."""
    p = _check_probs(probs)
    ctx, on_device, a, C, T, P, ld = _prepare(samples, burn, device)
    with ctx.lock:
        if on_device:
            d = ctx.rank_diagnostics_device(a.data_ptr(), C, T, P, ld, int(burn), p, int(cols_per_batch))
        else:
            d = ctx.rank_diagnostics(a, C, T, P, ld, int(burn), p, int(cols_per_batch))
    return {k: d[k] for k in KEYS}


def rank_normalize(samples, burn=0, folded=False, device=0):
    """z-scores of the exact ranks of every column's split draws, ``(2C, n, P)``: sequence
    ``2c + h`` is half ``h`` of chain ``c``.  ``folded=True`` ranks ``|x - median|`` instead.
    A column with a non-finite value is all NaN.  Input rules as for ``rank_diagnostics``."""
    ctx, on_device, a, C, T, P, ld = _prepare(samples, burn, device)
    with ctx.lock:
        if on_device:
            return ctx.rank_normalize_device(a.data_ptr(), C, T, P, ld, int(burn), bool(folded))
        return ctx.rank_normalize(a, C, T, P, ld, int(burn), bool(folded))


def quantile_names(probs):
    """Column names of ``BayesianModelCombination.summary``: ``q5``, ``q50``, ``q97.5``, ..."""
    return ["q" + format(100.0 * float(p), ".10g") for p in np.atleast_1d(probs)]
