"""Convergence diagnostics of sampled chains on the GPU: split R-hat and effective sample size.

The reference package has no diagnostics; this is a capability of this build.  The estimator is
the classic (not rank-normalised) split R-hat and the "mean" ESS (the rank-normalised ones built
on it are in ``rankdiag.py``) of

    A. Vehtari, A. Gelman, D. Simpson, B. Carpenter, P.-C. Buerkner, "Rank-normalization,
    folding, and localization: an improved R-hat for assessing convergence of MCMC",
    Bayesian Analysis 16(2), 2021,

i.e. Stan's and ArviZ's ``method="split"`` / ``method="mean"``.  For one column:

* Split.  ``C`` chains of ``T`` draws; the first ``burn`` of each are dropped.  With
  ``T' = T - burn`` and ``n = T' // 2`` each chain gives two sequences, its first ``n`` and its
  last ``n`` kept draws (the middle draw of an odd ``T'`` is in neither): ``M = 2C`` sequences
  of length ``n``; ``n >= 4`` is required.
* Per sequence: ``mean_m``; ``s2_m``, the centred (two-pass) variance with ddof 1;
  ``acov_m(t) = (1/n) sum_{i=0}^{n-1-t} (x_i - mean_m)(x_{i+t} - mean_m)``.
* R-hat: ``W = mean_m s2_m``, ``B/n = var(mean_m, ddof=1)``,
  ``var_plus = (n-1)/n W + B/n``, ``r_hat = sqrt(var_plus / W)``.
* ESS: ``a(t) = mean_m acov_m(t)``, ``rho(t) = 1 - (W - a(t)) / var_plus``; ``rho[.]`` is a zeroed
  array of length ``n`` with ``rho[0] = 1``.

  1. ``re = 1``, ``ro = rho(1)``, ``rho[1] = ro``, ``t = 1``.
  2. While ``t < n - 3`` and ``re + ro > 0``: ``re = rho(t+1)``, ``ro = rho(t+2)``; if
     ``re + ro >= 0`` set ``rho[t+1] = re``, ``rho[t+2] = ro``; ``t += 2``.
  3. ``max_t = t - 2``; if ``re > 0`` set ``rho[max_t+1] = re``.
  4. Geyer's monotone sequence: for ``t = 1, 3, 5, ...`` while ``t <= max_t - 2``, if
     ``rho[t+1] + rho[t+2] > rho[t-1] + rho[t]`` set both to ``(rho[t-1] + rho[t]) / 2``.
  5. ``tau = -1 + 2 sum_{t=0}^{max_t} rho[t] + rho[max_t+1]``,
     ``tau = max(tau, 1/log10(M n))``, ``ess = M n / tau``.

* Also: ``mean`` and ``sd`` (ddof 1) over all kept draws of all chains (the middle draw of an odd
  ``T'`` included), ``mcse_mean = sd / sqrt(ess)``, and ``max_lag = max_t + 2``, the largest
  autocovariance lag the scan read.
* A column with ``W == 0`` or any non-finite value gets NaN ``r_hat``, ``ess`` and ``mcse_mean``
  (and ``max_lag`` 0): a value, not an error.

On the device (``kernels_diag.hip``): one moments pass over the samples, then ``a(t)`` in blocks
of lags -- 64 first, doubling -- for the columns whose scan ran past the lags computed so far.
"""
from __future__ import annotations

import numpy as np

KEYS = ("mean", "sd", "mcse_mean", "ess", "r_hat", "max_lag")
FIRST_BLOCK = 64


def _is_torch(x):
    return type(x).__module__.split(".")[0] == "torch"


def _check_shape(shape, burn):
    if len(shape) not in (2, 3):
        raise ValueError(f"samples must be (T, P) or (C, T, P); got {len(shape)} dimensions")
    if isinstance(burn, bool) or not isinstance(burn, (int, np.integer)) or burn < 0:
        raise ValueError("burn must be an integer >= 0")
    C, T, P = (1, *shape) if len(shape) == 2 else tuple(shape)
    if C < 1 or P < 1:
        raise ValueError("samples must hold at least one chain and one column")
    n = (T - int(burn)) // 2
    if n < 4:
        raise ValueError(f"need n = (T - burn) // 2 >= 4 draws per split half-chain "
                         f"(T = {T}, burn = {burn})")
    return C, T, P


def _prepare(samples, burn, device):
    """The input rules of ``chain_diagnostics``: (context, on_device, array or tensor, C, T, P, ld).
    A numpy array is read in place when it is a column subset of a C-ordered array, else copied;
    a CUDA tensor is always read in place (and whatever torch queued on it is waited for)."""
    from . import _lib

    if _is_torch(samples) and not samples.is_cuda:
        samples = samples.numpy()
    if _is_torch(samples):
        import torch
        if samples.dtype != torch.float64:
            raise ValueError(f"samples must be float64; got {samples.dtype}")
        C, T, P = _check_shape(tuple(samples.shape), burn)
        t = samples if samples.dim() == 3 else samples.unsqueeze(0)
        ld = t.stride(1)
        if t.stride(2) != 1 or ld < P or (C > 1 and t.stride(0) != T * ld):
            raise ValueError("a device tensor must have a contiguous last dimension and chains "
                             "T * row-stride elements apart")
        ctx = _lib.default_context(t.device.index if t.device.index is not None else device)
        # the library reads on its own stream: whatever torch queued that writes `t` (a sampler
        # run, an RCCL gather, a matmul) must be done first (cf. chains.pool_samples)
        torch.cuda.current_stream(t.device).synchronize()
        return ctx, True, t, C, T, P, ld

    a = np.asarray(samples)
    if a.dtype != np.float64:
        raise ValueError(f"samples must be float64; got {a.dtype}")
    C, T, P = _check_shape(a.shape, burn)
    a = a if a.ndim == 3 else a[None]
    st = a.strides
    if st[2] == 8 and st[1] % 8 == 0 and st[1] >= 8 * P and (C == 1 or st[0] == T * st[1]):
        ld = st[1] // 8   # a column subset of a wider array: read in place
    else:
        a = np.ascontiguousarray(a)
        ld = P
    return _lib.default_context(device), False, a, C, T, P, ld


def chain_diagnostics(samples, burn=0, device=0):
    """Split R-hat, ESS and Monte-Carlo standard error of every column of ``samples``.

    ``samples`` is a float64 array ``(T, P)`` (one chain) or ``(C, T, P)``: a numpy array, or a
    CUDA torch tensor whose last dimension is contiguous (read in place, row stride passed as
    ``ld``: the route for ``chains.run_chains`` output; ``device`` is then the tensor's).
    Returns a dict of ``[P]`` arrays: ``mean``, ``sd``, ``mcse_mean``, ``ess``, ``r_hat``,
    ``max_lag``.  The estimator is the module docstring's."""
    ctx, on_device, a, C, T, P, ld = _prepare(samples, burn, device)
    with ctx.lock:
        if on_device:
            return _order(ctx.chain_diagnostics_device(a.data_ptr(), C, T, P, ld, int(burn)))
        return _order(ctx.chain_diagnostics(a, C, T, P, ld, int(burn)))


def _order(d):
    return {k: d[k] for k in KEYS}


MAX_LAGS = 1 << 20     # of one chain_autocovariance call (the C ABI's limit)


def chain_autocovariance(samples, burn=0, cols=None, first_lag=0, n_lags=64, device=0):
    """The raw quantities behind ``chain_diagnostics``, e.g. for autocorrelation plots: the moments
    of every split half-chain and one block of autocovariance lags, straight from the kernels.

    ``samples``, ``burn`` and ``device`` follow ``chain_diagnostics``.  ``cols`` selects columns
    (any order, repeats allowed; ``None``: all).  With ``M = 2C`` halves of ``n`` draws, returns a dict:

    * ``seq_mean``, ``seq_m2``: ``(n_seq, P)``; sequence ``2c + h`` is half ``h`` of chain ``c``:
      the mean of ``x - shift`` and the centred sum of squares.  When ``T - burn`` is odd, sequences
      ``2C + c`` are the chains' middle draws (``n_seq = 3C``; their ``seq_m2`` is 0).
    * ``shift``: ``(P,)``, the column's first kept draw of chain 0.
    * ``acov``: ``(len(cols), n_lags)``, ``a(t) = mean_m acov_m(t)`` of the module docstring for
      ``t = first_lag .. first_lag + n_lags - 1``; a lag ``t >= n`` is 0.

    ``rho(t)`` of a column follows as ``1 - (W - a(t)) / var_plus`` with
    ``W = mean_m seq_m2[m] / (n - 1)`` and ``var_plus = (n - 1) / n * W + var(seq_mean[:M], ddof=1)``."""
    for name, v, lo in (("first_lag", first_lag, 0), ("n_lags", n_lags, 1)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo:
            raise ValueError(f"{name} must be an integer >= {lo}")
    if n_lags > MAX_LAGS:
        raise ValueError(f"n_lags must be at most {MAX_LAGS}")
    ctx, on_device, a, C, T, P, ld = _prepare(samples, burn, device)
    if cols is not None:
        cols = np.asarray(cols)
        if cols.ndim != 1 or cols.size < 1 or cols.dtype.kind not in "iu":
            raise ValueError("cols must be a non-empty 1-d integer array (n_active >= 1)")
        if cols.min() < 0 or cols.max() >= P:
            raise ValueError(f"cols must lie in [0, {P}): got {int(cols.min())} .. {int(cols.max())}")
    with ctx.lock:
        if on_device:
            return ctx.chain_autocov_device(a.data_ptr(), C, T, P, ld, int(burn), cols, int(first_lag),
                                            int(n_lags))
        return ctx.chain_autocov(a, C, T, P, ld, int(burn), cols, int(first_lag), int(n_lags))


def lag_blocks(max_lag, n):
    """Lag blocks a call launched, from its ``max_lag`` output and the half-chain length ``n``:
    blocks cover lags [0, 64), [64, 192), [192, 448), ... (clipped at n); one more block is
    computed while a column's scan reads a lag at or past the end of the lags so far."""
    need = int(np.max(np.asarray(max_lag))) if np.size(max_lag) else 0
    have, L, blocks = 0, FIRST_BLOCK, 0
    while have < n:
        have = min(n, have + L)
        L *= 2
        blocks += 1
        if need < have:
            break
    return blocks
