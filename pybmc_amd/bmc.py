"""``BayesianModelCombination`` with the reference's method surface
(reference pybmc/bmc.py:11-376), backed by the MI355X Gibbs core.

Host-side pandas/numpy bookkeeping is restated here; the sampling
(``train`` -> ``gibbs_sampler``) and the posterior predictive
(``predict*``/``evaluate`` -> ``rndm_m_random_calculator``) run on the GPU.
"""
from __future__ import annotations

import numpy as np
import pandas as pd

from .data import apply_domain_filters
from .inference_utils import (USVt_hat_extraction, gibbs_sampler, gibbs_sampler_robust,
                              gibbs_sampler_simplex, robust_nu_prior)
from .sampling_utils import predictive_coverage, rndm_m_random_calculator


class BayesianModelCombination:
    """Bayesian model combination of several models' predictions.

    Constructor arguments, attributes and methods follow reference bmc.py:46-77.
    Unlike the reference, ``samples`` and the SVD attributes start as ``None`` so the
    "call orthogonalize()/train() first" guards raise the intended ``ValueError``
    (the reference raises ``AttributeError`` there).
    """

    def __init__(self, models_list, data_dict, truth_column_name, weights=None, device=0):
        if not isinstance(models_list, list) or any(not isinstance(m, str) for m in models_list):
            raise ValueError(
                "The 'models' should be a list of model names (strings) for Bayesian Combination.")
        if not isinstance(data_dict, dict) or any(
                not isinstance(df, pd.DataFrame) for df in data_dict.values()):
            raise ValueError(
                "The 'data_dict' should be a dictionary of pandas DataFrames, one per property.")
        self.data_dict = data_dict
        self.models_list = models_list
        # only the literal "truth" is dropped (reference bmc.py:75, quirk Q9)
        self.models = [m for m in models_list if m != "truth"]
        self.weights = weights
        self.truth_column_name = truth_column_name
        self.device = device
        self.samples = None
        self.n_chains = None
        self.current_property = None
        self.centered_experiment_train = None
        self.U_hat = self.S_hat = self.Vt_hat = self.Vt_hat_normalized = None
        self._predictions_mean_train = None
        self._train_df = None
        self.last_stats = None
        self._device_problem = None
        self._trained_with = None   # (sampler, [b0, C0, nu0, sigma20][, nu]) of the last train()
        self.row_weights = None     # (N,) mean latent weight per training row ("student_t" only)
        self.nu_samples = None      # draws of nu, one per row of samples ("nu": "estimate" only)
        self._nu_prior = None       # (grid, weights) of the prior nu had ("nu": "estimate" only)

    # ------------------------------------------------------------------ set-up
    def orthogonalize(self, property, train_df, components_kept, method="auto"):
        """Centre the model predictions and keep ``components_kept`` SVD components
        (reference bmc.py:79-130).

        ``method="svd"``: host thin SVD -- its leading columns equal the reference's
        full-matrices ones (same LAPACK, same signs) without the O(N^2) memory.
        ``method="device"``: centring, Gram (f64 MFMA), K x K eigen-decomposition and
        U_hat = Fc V S^-1 on the GPU (``bmc_orthogonalize``); works at sizes where the
        reference's full SVD cannot run (N = 200000 needs a 320 GB U).  Singular vectors are
        then signed by their largest entry; the model weights do not depend on the signs.
        ``"auto"`` picks the device route from 20000 rows on."""
        self.current_property = property
        self.selected_models_dataset = self.data_dict[property].copy()
        F = train_df[self.models].values
        k = int(components_kept)
        if k < 1 or k > min(F.shape):
            raise ValueError("components_kept must be between 1 and min(n_rows, n_models)")
        if method not in ("auto", "svd", "device"):
            raise ValueError("method must be 'auto', 'svd' or 'device'")
        if method == "auto":
            method = "device" if F.shape[0] >= 20000 else "svd"
        self._device_problem = None
        if method == "device":
            from . import _lib
            ctx = _lib.default_context(self.device)
            try:
                with ctx.lock:
                    mu, y_c, U_hat, S_hat, Vt_norm = ctx.orthogonalize(
                        F, train_df[self.truth_column_name].values, k)
            except np.linalg.LinAlgError as e:
                raise ValueError(str(e)) from None
            U_hat = np.asfortranarray(U_hat)
            Vt_hat = Vt_norm / S_hat[:, None]
            # the context already holds (y_c, U_hat) -- for as long as nobody else (another
            # BayesianModelCombination, a functional gibbs_sampler call: the per-device context
            # is shared) puts a different problem there: remember its generation
            self._device_problem = (ctx, U_hat, y_c, ctx.problem_generation)
        else:
            mu = np.mean(F, axis=1)
            y_c = train_df[self.truth_column_name].values - mu
            Fc = F - mu[:, None]
            U, S, Vt = np.linalg.svd(Fc, full_matrices=False)
            if S[k - 1] <= S[0] * 1e-13 * max(F.shape):
                raise ValueError(
                    "components_kept reaches the null space of the centred model matrix "
                    "(rows sum to zero, so at most n_models - 1 components carry signal)")
            U_hat, S_hat, Vt_hat, Vt_norm = USVt_hat_extraction(U, S, Vt, k)
        self.centered_experiment_train = y_c
        self.U_hat, self.S_hat = U_hat, S_hat
        self.Vt_hat, self.Vt_hat_normalized = Vt_hat, Vt_norm
        self._predictions_mean_train = mu
        self._train_df = train_df

    # ------------------------------------------------------------------- train
    def train(self, training_options=None):
        """Sample the posterior (reference bmc.py:132-193).  Options and their defaults
        are the reference's; any sampler string other than ``"simplex"`` and ``"student_t"``
        selects the Gibbs sampler (quirk Q6).  ``{"sampler": "student_t", "nu": 4.0}`` (not in the
        reference) runs the outlier-robust sampler ``gibbs_sampler_robust``: Student-t likelihood
        with ``nu`` degrees of freedom, ``n_chains`` and ``seeds`` honoured, ``burn`` sweeps dropped
        per chain only when the caller gives ``burn`` (default 0), ``devices`` other than this GPU a
        ``ValueError``; afterwards ``row_weights`` holds the mean latent weight of every training
        row, averaged over chains (far below 1: an outlier), and the predictive noise of
        ``predict``, ``predict2`` and ``evaluate`` is ``sigma t_nu``.  ``"nu": "estimate"`` (with the
        optional ``nu_grid``, ``nu_prior``, ``nu_init`` of ``gibbs_sampler_robust``) draws ``nu`` from
        a discrete prior in every sweep: ``nu_samples`` then holds its draws, pooled in chain order
        like ``samples``, ``diagnostics()`` and ``summary()`` gain a row ``nu`` after ``sigma``, and
        the predictive noise of draw s is ``sigma_s t_{nu_s}``.  Extra optional keys (defaults
        keep the reference behaviour):
        ``n_chains`` (pooled along the sample axis), ``seeds``, ``dtype`` (``"float32"`` stores
        U_hat and y in float32 on the device, sums stay float64 -- BASELINE configs[3]),
        ``devices`` (list of GPU ids: the chains are split over them, one host thread and one
        context per device, and pooled in chain order; Gibbs sampler only -- with the simplex
        sampler it raises ``ValueError``).  The simplex sampler honours ``n_chains`` and ``seeds``
        the same way: its chains run side by side on this GPU, each from beta = 0 with its own
        ``burn`` steps dropped, and are pooled in chain order."""
        if self.U_hat is None:
            raise ValueError("Must call `orthogonalize()` before training.")
        opts = training_options if training_options is not None else {}

        def get_option(key, default):
            if key not in opts:
                print(f"[INFO] Using default value for '{key}': {default}")
            return opts.get(key, default)

        iterations = get_option("iterations", 50000)
        sampler = get_option("sampler", "gibbs_sampling")
        burn = get_option("burn", 10000)
        stepsize = get_option("stepsize", 0.001)
        kc = self.U_hat.shape[1]
        b_mean_prior = get_option("b_mean_prior", np.zeros(kc))
        b_mean_cov = get_option("b_mean_cov", np.diag(self.S_hat ** 2))
        nu0 = get_option("nu0_chosen", 1.0)
        sigma20 = get_option("sigma20_chosen", 0.02)

        self._trained_with = ("simplex" if sampler == "simplex" else "gibbs",
                              [b_mean_prior, b_mean_cov, nu0, sigma20])
        self.row_weights = None
        self.nu_samples = None
        self._nu_prior = None
        if sampler == "student_t":
            devices = opts.get("devices")
            if devices is not None and list(devices) != [self.device]:
                raise ValueError('"devices" is for the Gibbs sampler: Student-t chains run on one '
                                 'GPU (use n_chains for several chains on this device)')
            nu = opts.get("nu", 4.0)
            estimate = isinstance(nu, str)
            nu = nu if estimate else float(nu)
            n_chains = int(opts.get("n_chains", 1))
            prior = [b_mean_prior, b_mean_cov, nu0, sigma20]
            self._trained_with = ("student_t", prior, nu)
            self._device_problem = None   # this path sets its own problem
            extra = {key: opts.get(key) for key in ("nu_grid", "nu_prior", "nu_init") if key in opts}
            got = gibbs_sampler_robust(
                self.centered_experiment_train, self.U_hat, iterations, prior, nu,
                burn=int(opts.get("burn", 0)), n_chains=n_chains, seeds=opts.get("seeds"),
                device=self.device, return_row_weights=True, return_stats=True,
                return_nu=estimate, **extra)
            res, w, stats = got[0], got[1], got[-1]
            if estimate:
                self.nu_samples = np.ascontiguousarray(got[2]).reshape(-1)   # pooled in chain order
                self._nu_prior = robust_nu_prior(extra.get("nu_grid"), extra.get("nu_prior"))[:2]
            self.last_stats = stats
            self.samples = res if res.ndim == 2 else res.reshape(-1, res.shape[-1])
            self.row_weights = w if w.ndim == 1 else w.mean(axis=0)
            self.n_chains = n_chains
        elif sampler == "simplex":
            devices = opts.get("devices")
            if devices is not None and list(devices) != [self.device]:
                raise ValueError('"devices" is for the Gibbs sampler: simplex chains run on one '
                                 'GPU (use n_chains for several chains on this device)')
            n_chains = int(opts.get("n_chains", 1))
            self._device_problem = None   # the simplex path sets its own problem
            res, stats = gibbs_sampler_simplex(
                self.centered_experiment_train, self.U_hat, self.Vt_hat, self.S_hat,
                iterations, [nu0, sigma20], burn=burn, stepsize=stepsize, device=self.device,
                n_chains=n_chains, seeds=opts.get("seeds"), return_stats=True)
            self.last_stats = stats
            # several chains are pooled along the sample axis, in chain order
            self.samples = res if res.ndim == 2 else res.reshape(-1, res.shape[-1])
            self.n_chains = n_chains
        else:
            dtype = opts.get("dtype")
            if dtype is not None and np.dtype(dtype) not in (np.dtype(np.float32),
                                                             np.dtype(np.float64)):
                raise ValueError("dtype must be float32 or float64")
            devices = opts.get("devices")
            n_chains = int(opts.get("n_chains", 1))
            prior = [b_mean_prior, b_mean_cov, nu0, sigma20]
            if devices is not None and list(devices) != [self.device]:
                from .chains import run_on_devices
                res, stats = run_on_devices(self.centered_experiment_train, self.U_hat, iterations,
                                            prior, n_chains, opts.get("seeds"), list(devices), dtype)
            else:
                dp = self._device_problem
                # the resident problem is reusable only if it is still THIS object's: same
                # arrays, same context generation, and float64 storage was asked for
                on_device = (dp is not None and dp[1] is self.U_hat
                             and dp[2] is self.centered_experiment_train
                             and dp[0].problem_generation == dp[3]
                             and (dtype is None or np.dtype(dtype) == np.float64))
                res, stats = gibbs_sampler(
                    self.centered_experiment_train, self.U_hat, iterations, prior,
                    n_chains=n_chains, seeds=opts.get("seeds"), dtype=dtype,
                    device=self.device, return_stats=True, _problem_on_device=on_device)
            self.last_stats = stats
            # several chains are pooled along the sample axis
            self.samples = res if res.ndim == 2 else res.reshape(-1, res.shape[-1])
            self.n_chains = n_chains

    # ------------------------------------------------------------- diagnostics
    def diagnostics(self, burn=0):
        """Convergence diagnostics of the last ``train()`` (not in the reference): split R-hat,
        ESS, Monte-Carlo standard error, mean and sd of every coefficient ``beta_i``, of
        ``sigma`` and of every model weight ``beta Vt_hat + 1/K`` (the numbers a BMC user reads),
        computed on the GPU (``pybmc_amd.diagnostics``).  The pooled ``samples`` are split back
        into their ``n_chains`` chains; ``burn`` more draws are dropped from the start of each.
        Returns a DataFrame indexed by ``beta_0 .. beta_{k-1}``, ``sigma`` and the model names,
        with columns ``mean``, ``sd``, ``mcse_mean``, ``ess``, ``r_hat``, ``max_lag``."""
        if self.samples is None or self.Vt_hat is None:
            raise ValueError("Must call `orthogonalize()` and `train()` before computing diagnostics.")
        s = np.asarray(self.samples)
        k1 = s.shape[-1]
        chains = int(self.n_chains or 1)
        s = s.reshape(chains, -1, k1)
        d = _series_diagnostics(s, self.Vt_hat, burn, self.device, **self._nu_series())
        index = [f"beta_{i}" for i in range(k1 - 1)] + ["sigma"] + self._nu_row() + list(self.models)
        from .diagnostics import KEYS
        return pd.DataFrame({key: np.asarray(d[key]) for key in KEYS}, index=index)

    def summary(self, burn=0, probs=(0.05, 0.5, 0.95)):
        """Posterior summary of the last ``train()`` with the rank-normalised diagnostics (not in
        the reference; ``pybmc_amd.rankdiag``): over ``beta_i``, ``sigma`` and the model weights,
        the rows of ``diagnostics()`` formed the same way, the columns ``mean``, ``sd``, one
        quantile per entry of ``probs`` (``q5``, ``q50``, ``q95``), ``mcse_mean``, ``ess_bulk``,
        ``ess_tail`` and ``r_hat`` (folded, rank-normalised), computed on the GPU."""
        if self.samples is None or self.Vt_hat is None:
            raise ValueError("Must call `orthogonalize()` and `train()` before computing a summary.")
        from .rankdiag import quantile_names, rank_diagnostics
        s = self._chains()
        d = rank_diagnostics(_series_tensor(s, self.Vt_hat, self.device, **self._nu_series()), burn=burn,
                             probs=probs, device=self.device)
        index = [f"beta_{i}" for i in range(s.shape[-1] - 1)] + ["sigma"] + self._nu_row() + list(self.models)
        cols = {"mean": d["mean"], "sd": d["sd"]}
        for name, row in zip(quantile_names(probs), d["quantiles"]):
            cols[name] = row
        for key in ("mcse_mean", "ess_bulk", "ess_tail", "r_hat"):
            cols[key] = d[key]
        return pd.DataFrame({k: np.asarray(v) for k, v in cols.items()}, index=index)

    def _require_gaussian(self, what, training_options=None):
        """The checking and cross-validation kernels hard-code the Gaussian density, and the scoring
        methods that call this one keep to it (``score()`` takes the fit's own likelihood)."""
        opts = training_options if training_options is not None else {}
        trained = self._trained_with[0] if self._trained_with is not None else None
        if opts.get("sampler", trained) == "student_t":
            raise ValueError(f'{what} supports the Gaussian Gibbs sampler only (sampler == "student_t")')

    def _noise_df(self):
        """Degrees of freedom of the predictive noise: None (normal) unless the fit was Student-t;
        the draws ``nu_samples`` (one per row of ``samples``) when ``nu`` was estimated."""
        tw = self._trained_with
        if tw is None or tw[0] != "student_t":
            return None
        return self.nu_samples if self._nu_estimated() else tw[2]

    def _nu_estimated(self):
        tw = self._trained_with
        return (tw is not None and tw[0] == "student_t" and isinstance(tw[2], str)
                and getattr(self, "nu_samples", None) is not None)

    def _nu_chains(self):
        """(n_chains, T) draws of nu of a fit that estimated it, else None."""
        if not self._nu_estimated():
            return None
        return np.asarray(self.nu_samples, dtype=np.float64).reshape(int(self.n_chains or 1), -1)

    def _nu_series(self):
        """The extra keyword of the series helpers: the nu column of a fit that estimated it."""
        return {"nu": self._nu_chains()} if self._nu_estimated() else {}

    def _nu_row(self):
        return ["nu"] if self._nu_estimated() else []

    # ----------------------------------------------------------------- scoring
    def _chains(self):
        s = np.asarray(self.samples)
        return s.reshape(int(self.n_chains or 1), -1, s.shape[-1])

    def waic(self, burn=0):
        """WAIC of the last ``train()`` on its training data (not in the reference;
        ``pybmc_amd.scoring``): the likelihood of ``centered_experiment_train`` given ``U_hat`` under
        every draw, reduced on the GPU.  The pooled ``samples`` are split back into their
        ``n_chains`` chains and ``burn`` more draws dropped from the start of each.  Returns a dict:
        ``elpd_waic``, ``p_waic``, ``waic``, ``se``, ``n_high_p``, ``n_points`` and the pointwise
        ``lppd``, ``p_waic_i``, ``mean_ll``, ``elpd_waic_i``."""
        if self.samples is None or self.U_hat is None:
            raise ValueError("Must call `orthogonalize()` and `train()` before computing WAIC.")
        self._require_gaussian("waic")
        from .scoring import waic
        return waic(self.U_hat, np.asarray(self.centered_experiment_train, dtype=np.float64),
                    self._chains(), burn=burn, device=self.device)

    def loo(self, burn=0):
        """PSIS-LOO cross-validation of the last ``train()`` on its training data (not in the
        reference; ``pybmc_amd.scoring.psis_loo``), on the same data as ``waic()``: ``U_hat``,
        ``centered_experiment_train`` and the chains, ``burn`` more draws dropped from the start of
        each.  Returns a dict: ``elpd_loo``, ``p_loo``, ``looic``, ``se``, ``n_high_k``,
        ``k_threshold``, ``n_above_threshold``, ``n_points``, ``n_draws`` and the pointwise
        ``elpd_loo_i``, ``p_loo_i``, ``pareto_k``, ``lppd``."""
        if self.samples is None or self.U_hat is None:
            raise ValueError("Must call `orthogonalize()` and `train()` before computing LOO.")
        self._require_gaussian("loo")
        from .scoring import psis_loo
        return psis_loo(self.U_hat, np.asarray(self.centered_experiment_train, dtype=np.float64),
                        self._chains(), burn=burn, device=self.device)

    def score(self, method="loo", X=None, burn=0):
        """Score the last ``train()`` under the likelihood it sampled from (not in the reference;
        ``pybmc_amd.scoring``): Gaussian, or after ``{"sampler": "student_t"}`` the Student-t
        density with that fit's ``nu`` -- the one scoring method that accepts a Student-t fit.
        ``method`` is ``"loo"`` (``psis_loo``) or ``"waic"`` (``waic``) on the training data of
        ``loo()`` and ``waic()``.  With a DataFrame ``X`` (model columns and the truth column) it is
        the log predictive density of held-out data instead, built as ``log_predictive_density``
        builds it (``elpd``, ``se``, ``n_points``, ``lppd``; ``method`` is not used).  ``burn`` more
        draws are dropped from the start of each chain.  The result also carries ``likelihood``
        (``"gaussian"`` or ``"student_t"``) and ``nu`` (None for the Gaussian one; after
        ``"nu": "estimate"`` every draw is scored with its own ``nu``, ``nu`` is the mean over the
        scored draws and ``nu_estimated`` is True); the results of
        two fits of the same data feed ``pybmc_amd.compare_elpd`` directly."""
        if method not in ("loo", "waic"):
            raise ValueError(f'method must be "loo" or "waic"; got {method!r}')
        nu = self._noise_df()
        estimated = self._nu_estimated()
        lik = {"nu_draws": self._nu_chains()} if estimated else {"nu": nu}
        from . import scoring
        if X is not None:
            if self.samples is None or self.Vt_hat is None:
                raise ValueError("Must call `orthogonalize()` and `train()` before scoring.")
            if not isinstance(X, pd.DataFrame):
                raise ValueError(
                    "X must be a pandas DataFrame containing model predictions and the truth column.")
            if self.truth_column_name not in X.columns:
                raise ValueError(f"X must contain the truth column '{self.truth_column_name}'.")
            preds = np.asarray(X[self.models].values, dtype=np.float64)
            truth = np.asarray(X[self.truth_column_name].values, dtype=np.float64)
            A = preds @ np.asarray(self.Vt_hat, dtype=np.float64).T
            pw = scoring.pointwise_log_likelihood(A, truth - preds.mean(axis=1), self._chains(),
                                                  burn=burn, device=self.device, **lik)
            out = scoring.elpd_summary(pw["lppd"])
            out["lppd"] = pw["lppd"]
        else:
            if self.samples is None or self.U_hat is None:
                raise ValueError("Must call `orthogonalize()` and `train()` before scoring.")
            fn = scoring.psis_loo if method == "loo" else scoring.waic
            out = fn(self.U_hat, np.asarray(self.centered_experiment_train, dtype=np.float64),
                     self._chains(), burn=burn, device=self.device, **lik)
        out["likelihood"] = "gaussian" if nu is None else "student_t"
        if estimated:    # the mean over the scored draws
            out["nu"] = float(np.mean(lik["nu_draws"][:, int(burn):]))
            out["nu_estimated"] = True
        else:
            out["nu"] = nu
        return out

    def loo_predict(self, burn=0):
        """What the combination would have predicted for every training point had that point not
        been in the fit (not in the reference; ``pybmc_amd.scoring.psis_loo_predict``), from the
        data of ``loo()``.  Returns that function's dict (``loo_mean`` is the prediction of the
        centred target) and, in the truth's units, ``predicted = loo_mean +`` the row mean of the
        model predictions, ``truth`` and ``residual = truth - predicted``."""
        if self.samples is None or self.U_hat is None:
            raise ValueError("Must call `orthogonalize()` and `train()` before computing LOO.")
        self._require_gaussian("loo_predict")
        from .scoring import psis_loo_predict
        y = np.asarray(self.centered_experiment_train, dtype=np.float64)
        out = psis_loo_predict(self.U_hat, y, self._chains(), burn=burn, device=self.device)
        mu = np.asarray(self._predictions_mean_train, dtype=np.float64)
        out["predicted"] = out["loo_mean"] + mu
        out["truth"] = y + mu
        out["residual"] = y - out["loo_mean"]
        return out

    def loo_predictions(self, burn=0):
        """The leave-one-out predictions of the last ``train()`` under the likelihood it sampled
        from (not in the reference; ``pybmc_amd.scoring.psis_loo_predict``): what ``loo_predict()``
        returns for a Gaussian fit, and after ``{"sampler": "student_t"}`` the same under the
        Student-t density with that fit's ``nu`` (every draw's own after ``"nu": "estimate"``) --
        the leave-one-out method that accepts a Student-t fit, as ``score()`` is the scoring one.
        Under the t likelihood ``loo_mean`` is the location of the predictive distribution (its mean
        where ``nu > 1``), ``loo_sd`` carries the t variance and is ``+inf`` when a scored ``nu`` is
        at most 2, ``loo_pit`` uses the t distribution function, and ``nu`` must lie in 0.06 .. 1000.
        The rows the robust fit down-weights are the ones to look at first: large ``|residual|``,
        ``|2 loo_pit - 1|`` near 1.  ``burn`` more draws are dropped from the start of each chain.
        The result also carries ``likelihood``, ``nu`` and ``nu_estimated`` as ``score()`` sets
        them."""
        if self.samples is None or self.U_hat is None:
            raise ValueError("Must call `orthogonalize()` and `train()` before computing LOO.")
        nu = self._noise_df()
        estimated = self._nu_estimated()
        lik = {"nu_draws": self._nu_chains()} if estimated else {"nu": nu}
        from .scoring import psis_loo_predict
        y = np.asarray(self.centered_experiment_train, dtype=np.float64)
        out = psis_loo_predict(self.U_hat, y, self._chains(), burn=burn, device=self.device, **lik)
        mu = np.asarray(self._predictions_mean_train, dtype=np.float64)
        out["predicted"] = out["loo_mean"] + mu
        out["truth"] = y + mu
        out["residual"] = y - out["loo_mean"]
        out["likelihood"] = "gaussian" if nu is None else "student_t"
        if estimated:    # the mean over the scored draws
            out["nu"] = float(np.mean(lik["nu_draws"][:, int(burn):]))
            out["nu_estimated"] = True
        else:
            out["nu"] = nu
        return out

    def prior_sensitivity(self, burn=0, alphas=None, training_options=None):
        """Power-scaling sensitivity of the last ``train()`` to its prior and its likelihood (not in
        the reference; ``pybmc_amd.sensitivity.power_scale_sensitivity``): for every coefficient,
        ``sigma`` and every model weight ``beta Vt_hat + 1/K``, how far the posterior marginal moves
        when the prior, or the likelihood, is raised to a power near 1 -- from the draws already
        taken.  The priors are those ``train()`` used; ``training_options`` (the keys
        ``b_mean_prior``, ``b_mean_cov``, ``nu0_chosen``, ``sigma20_chosen``) overrides them.
        ``burn`` more draws are dropped from the start of each chain.  Gibbs sampler only: after
        ``sampler == "simplex"`` it raises ``ValueError`` (that sampler's target is not this
        posterior).  Returns that function's dict; ``sensitivity.sensitivity_summary`` makes the
        table."""
        if self.samples is None or self.U_hat is None or self._trained_with is None:
            raise ValueError("Must call `orthogonalize()` and `train()` before the prior sensitivity.")
        self._require_gaussian("prior_sensitivity", training_options)
        sampler, prior = self._trained_with[:2]
        opts = training_options if training_options is not None else {}
        if sampler == "simplex" or opts.get("sampler", "gibbs_sampling") == "simplex":
            raise ValueError('prior_sensitivity supports the Gibbs sampler only (sampler == "simplex")')
        prior = [opts.get("b_mean_prior", prior[0]), opts.get("b_mean_cov", prior[1]),
                 opts.get("nu0_chosen", prior[2]), opts.get("sigma20_chosen", prior[3])]
        from .sensitivity import power_scale_sensitivity
        return power_scale_sensitivity(
            self.U_hat, np.asarray(self.centered_experiment_train, dtype=np.float64), self._chains(),
            prior, Vt_hat=self.Vt_hat, burn=burn, alphas=alphas, device=self.device,
            models=self.models)

    def sensitivity(self, burn=0, alphas=None, training_options=None):
        """``prior_sensitivity`` under the likelihood the last ``train()`` sampled from, as
        ``score()`` and ``check()`` read a fit: the plain call after a Gaussian fit, the Student-t
        likelihood with that fit's ``nu`` after ``{"sampler": "student_t"}`` and, after
        ``"nu": "estimate"``, every draw with its own ``nu`` and the prior that fit gave ``nu``: the
        columns then end in ``nu``, and ``prior_nu`` is a third component beside ``prior`` and
        ``likelihood`` -- does the posterior of ``nu`` only restate its prior?  Arguments and result as
        ``prior_sensitivity`` (the result's ``likelihood`` and ``nu`` say which call it was); after
        ``sampler == "simplex"`` it raises ``ValueError``."""
        if self.samples is None or self.U_hat is None or self._trained_with is None:
            raise ValueError("Must call `orthogonalize()` and `train()` before the prior sensitivity.")
        sampler, prior = self._trained_with[:2]
        opts = training_options if training_options is not None else {}
        if sampler == "simplex" or opts.get("sampler", "gibbs_sampling") == "simplex":
            raise ValueError('sensitivity supports the Gibbs samplers only (sampler == "simplex")')
        prior = [opts.get("b_mean_prior", prior[0]), opts.get("b_mean_cov", prior[1]),
                 opts.get("nu0_chosen", prior[2]), opts.get("sigma20_chosen", prior[3])]
        lik, components = {}, ("prior", "likelihood")
        if self._nu_estimated():
            lik = {"nu_draws": self._nu_chains()}
            if self._nu_prior is not None:
                lik.update(nu_grid=self._nu_prior[0], nu_prior=self._nu_prior[1])
                components += ("prior_nu",)
        elif sampler == "student_t":
            lik = {"nu": self._trained_with[2]}
        from .sensitivity import power_scale_sensitivity
        return power_scale_sensitivity(
            self.U_hat, np.asarray(self.centered_experiment_train, dtype=np.float64), self._chains(),
            prior, Vt_hat=self.Vt_hat, burn=burn, alphas=alphas, components=components,
            device=self.device, models=self.models, **lik)

    def _cv_arguments(self, what, n_folds, groups, training_options, seed, gaussian_only=True):
        """(options, y, fold labels, group values or None, prior) of ``cross_validate``,
        ``component_path`` and ``validate``; ValueError for what they do not accept."""
        if self.U_hat is None:
            raise ValueError("Must call `orthogonalize()` before cross-validating.")
        opts = training_options if training_options is not None else {}
        if gaussian_only:
            self._require_gaussian(what, training_options)
        if opts.get("sampler", "gibbs_sampling") == "simplex":
            raise ValueError(f'{what} supports the Gibbs sampler only (sampler == "simplex")')
        from .cv import fold_labels, group_labels
        y = np.asarray(self.centered_experiment_train, dtype=np.float64)
        n, kc = self.U_hat.shape
        values = None
        if groups is not None:
            if isinstance(groups, str):
                if self._train_df is None or groups not in self._train_df.columns:
                    raise ValueError(f"groups: the training frame has no column '{groups}'")
                groups = self._train_df[groups].values
            groups = np.asarray(groups)
            if groups.shape != (n,):
                raise ValueError(f"groups must have one entry per training row ({n},); got {groups.shape}")
            folds, values = group_labels(groups)
        else:
            folds = fold_labels(n, n_folds, seed)
        prior = [opts.get("b_mean_prior", np.zeros(kc)), opts.get("b_mean_cov", np.diag(self.S_hat ** 2)),
                 opts.get("nu0_chosen", 1.0), opts.get("sigma20_chosen", 0.02)]
        return opts, y, folds, values, prior

    def cross_validate(self, n_folds=10, groups=None, training_options=None, seed=None):
        """Exact K-fold or leave-group-out cross-validation of the combination (not in the
        reference; ``pybmc_amd.cv.kfold_cv``): for every fold the Gibbs sampler is run on
        ``U_hat`` and ``centered_experiment_train`` WITHOUT that fold's rows and the held-out rows
        are scored against it -- all folds in one call on the GPU, no ``train()`` needed.

        ``n_folds`` balanced random folds (``cv.fold_labels(n, n_folds, seed)``), or, with
        ``groups``, one fold per distinct value: ``groups`` is a column name of the training frame
        given to ``orthogonalize()`` or an array with one entry per training row (leave-group-out:
        "what if this isotopic chain had not been measured?").  ``training_options`` are those of
        ``train()`` with the same defaults (``iterations``, ``burn``, ``b_mean_prior``,
        ``b_mean_cov``, ``nu0_chosen``, ``sigma20_chosen``, ``n_chains``) plus ``thin``; ``seed``
        fixes the fold labels and the chains' seeds.  Gibbs sampler only: ``sampler == "simplex"``
        raises ``ValueError``.

        The SVD basis is held fixed: ``U_hat`` is the basis ``orthogonalize()`` made from ALL
        training rows and is not recomputed per fold.  That basis depends on the model predictions
        only, never on the truth, so no held-out truth reaches a fold's fit; it is the same
        conditioning as ``loo()``, whose ``elpd_loo`` is therefore comparable with ``elpd_cv``.

        Returns the dict of ``kfold_cv`` (``elpd_cv``, ``se``, ``cv_rmse``, ``elpd_fold``,
        ``n_fold``, ``n_points``, ``n_folds``, ``n_draws``, ``elpd_cv_i``, ``cv_mean_i``, ``seeds``),
        ``folds`` (the labels), ``groups`` (the distinct values, with ``groups``) and, in the
        truth's units as ``loo_predict()``, ``predicted = cv_mean_i +`` the row mean of the model
        predictions, ``truth`` and ``residual = truth - predicted``."""
        from .cv import kfold_cv
        opts, y, folds, values, prior = self._cv_arguments("cross_validate", n_folds, groups,
                                                          training_options, seed)
        out = kfold_cv(np.asarray(self.U_hat, dtype=np.float64), y, prior, folds,
                       opts.get("iterations", 50000), burn=opts.get("burn", 10000),
                       thin=opts.get("thin", 1), n_chains=int(opts.get("n_chains", 1)), seed=seed,
                       device=self.device)
        return self._cv_extras(out, y, folds, values)

    def _cv_extras(self, out, y, folds, values):
        """The extras of ``cross_validate()`` on a ``kfold_cv`` result."""
        mu = np.asarray(self._predictions_mean_train, dtype=np.float64)
        out["folds"] = folds
        if values is not None:
            out["groups"] = values
        out["predicted"] = out["cv_mean_i"] + mu
        out["truth"] = y + mu
        out["residual"] = y - out["cv_mean_i"]
        return out

    def validate(self, n_folds=10, groups=None, training_options=None, seed=None):
        """``cross_validate()`` under the likelihood the options name: the plain call for the
        Gaussian Gibbs sampler, and for ``{"sampler": "student_t", "nu": ...}`` exact
        cross-validation of the Student-t fit (``pybmc_amd.cv.kfold_cv(nu=...)``: every fold's
        chains are ``gibbs_sampler_robust``'s on its training rows, all in one launch, the held-out
        rows scored under the t density).  Options that name no sampler take the likelihood of the
        last ``train()``, as ``score()``, ``check()`` and ``sensitivity()`` read a fit: its ``nu``, or
        ``"estimate"`` with that fit's grid and prior.  ``"nu": "estimate"`` takes the optional
        ``nu_grid``, ``nu_prior`` and ``nu_init`` of ``train()``.  Arguments, defaults and the returned
        extras (``folds``, ``groups``, ``predicted``, ``truth``, ``residual``) are
        ``cross_validate()``'s; a Student-t result also carries ``likelihood`` and ``nu``.
        ``sampler == "simplex"`` raises ``ValueError``."""
        opts = training_options if training_options is not None else {}
        trained = self._trained_with
        sampler = opts.get("sampler", trained[0] if trained is not None else None)
        if sampler != "student_t":
            return self.cross_validate(n_folds, groups, training_options, seed)
        opts, y, folds, values, prior = self._cv_arguments("validate", n_folds, groups, training_options,
                                                          seed, gaussian_only=False)
        extra = {key: opts[key] for key in ("nu_grid", "nu_prior", "nu_init") if key in opts}
        if "nu" in opts or opts.get("sampler") == "student_t":
            nu = opts.get("nu", 4.0)
        else:                               # the last train()'s own likelihood
            nu = trained[2]
            if isinstance(nu, str) and self._nu_prior is not None and not extra:
                extra = {"nu_grid": self._nu_prior[0], "nu_prior": self._nu_prior[1]}
        from .cv import kfold_cv
        out = kfold_cv(np.asarray(self.U_hat, dtype=np.float64), y, prior, folds,
                       opts.get("iterations", 50000), burn=opts.get("burn", 10000),
                       thin=opts.get("thin", 1), n_chains=int(opts.get("n_chains", 1)), seed=seed,
                       device=self.device, nu=nu if isinstance(nu, str) else float(nu), **extra)
        return self._cv_extras(out, y, folds, values)

    def component_path(self, n_folds=10, groups=None, components=None, training_options=None, seed=None):
        """Choose ``components_kept`` by cross-validation (not in the reference;
        ``pybmc_amd.cv.cv_component_path``): ``cross_validate()`` for every candidate number of
        components in one call on the GPU.  Call it after ``orthogonalize(..., components_kept=k_max)``
        with the largest count worth considering; no ``train()`` is needed.  Candidate k is the model
        on the leading k columns of ``U_hat`` -- what ``orthogonalize(..., components_kept=k)`` would
        keep -- under the leading block of the prior (the default ``diag(S_hat ** 2)`` is the one
        ``train()`` would use).  ``components`` is a strictly increasing sequence in ``1 .. k_max``
        (default: all); ``n_folds``, ``groups``, ``training_options`` and ``seed`` as in
        ``cross_validate()``, Gibbs sampler only (``sampler == "simplex"`` raises ``ValueError``).

        The SVD basis is held fixed: ``U_hat`` is the basis ``orthogonalize()`` made from ALL
        training rows and is not recomputed per fold.  That basis depends on the model predictions
        only, never on the truth, so no held-out truth reaches a fold's fit; it is the same
        conditioning as ``loo()``, whose ``elpd_loo`` is therefore comparable with ``elpd_cv``.

        Returns the dict of ``cv_component_path`` (per candidate ``elpd_cv``, ``se``, ``cv_rmse``,
        ``elpd_fold``, ``elpd_cv_i``, ``cv_mean_i``; ``k_best``, ``k_1se``, ``elpd_diff``,
        ``se_diff``; ...), ``folds`` (the labels), ``groups`` (the distinct values, with ``groups``)
        and ``table``: a DataFrame indexed by ``components`` with the columns ``elpd_cv``, ``se``,
        ``elpd_diff``, ``se_diff`` and ``cv_rmse``.  Then call
        ``orthogonalize(..., components_kept=out["k_1se"])`` (the most parsimonious count
        indistinguishable from the best; or ``out["k_best"]``) followed by ``train()``."""
        from .cv import cv_component_path
        opts, y, folds, values, prior = self._cv_arguments("component_path", n_folds, groups,
                                                          training_options, seed)
        out = cv_component_path(np.asarray(self.U_hat, dtype=np.float64), y, prior, folds,
                                opts.get("iterations", 50000), components=components,
                                burn=opts.get("burn", 10000), thin=opts.get("thin", 1),
                                n_chains=int(opts.get("n_chains", 1)), seed=seed, device=self.device)
        out["folds"] = folds
        if values is not None:
            out["groups"] = values
        out["table"] = pd.DataFrame({key: out[key] for key in ("elpd_cv", "se", "elpd_diff", "se_diff",
                                                               "cv_rmse")},
                                    index=pd.Index(out["components"], name="components"))
        return out

    def log_predictive_density(self, X, burn=0):
        """Log predictive density of held-out data (a validation or test split): ``X`` is a
        DataFrame with the model columns and the truth column.  The predictive mean of point p
        under draw s is ``preds_p . (beta_s Vt_hat + 1/K)`` (reference sampling_utils.py:60-72),
        so the design row is ``preds_p Vt_hat'`` and the target ``truth_p - mean(preds_p)``.
        Returns ``elpd`` (the sum of the pointwise ``lppd``; no penalty on held-out data), its
        ``se``, ``n_points`` and ``lppd``."""
        if self.samples is None or self.Vt_hat is None:
            raise ValueError(
                "Must call `orthogonalize()` and `train()` before computing predictive densities.")
        if not isinstance(X, pd.DataFrame):
            raise ValueError(
                "X must be a pandas DataFrame containing model predictions and the truth column.")
        if self.truth_column_name not in X.columns:
            raise ValueError(f"X must contain the truth column '{self.truth_column_name}'.")
        self._require_gaussian("log_predictive_density")
        from .scoring import elpd_summary, pointwise_log_likelihood
        preds = np.asarray(X[self.models].values, dtype=np.float64)
        truth = np.asarray(X[self.truth_column_name].values, dtype=np.float64)
        A = preds @ np.asarray(self.Vt_hat, dtype=np.float64).T
        pw = pointwise_log_likelihood(A, truth - preds.mean(axis=1), self._chains(), burn=burn,
                                      device=self.device)
        out = elpd_summary(pw["lppd"])
        out["lppd"] = pw["lppd"]
        return out

    def posterior_predictive_check(self, X=None, burn=0, seed=None):
        """Posterior predictive check of the last ``train()`` (not in the reference;
        ``pybmc_amd.ppc.posterior_predictive_check``): Bayesian p-values of eight test quantities
        of data replicated from every draw against the observed data.  Without ``X`` on the
        training data of ``loo()`` (``U_hat``, ``centered_experiment_train``), with the row mean of
        the model predictions as the offset, so that ``min``, ``max``, ``mean``, ``sd``, ``skew`` and
        ``kurt`` are in the truth's units.  With a DataFrame ``X`` (model columns and the truth
        column) on held-out data, built as ``log_predictive_density`` builds it: design
        ``preds Vt_hat'``, target ``truth - mean(preds)``, offset ``mean(preds)``.  ``burn`` more
        draws are dropped from the start of each chain; ``seed`` fixes the replicated noise (None:
        drawn from numpy's global stream and returned).  Returns that function's dict."""
        from .ppc import posterior_predictive_check
        self._require_gaussian("posterior_predictive_check")
        A, y, offset = self._check_data(X)
        return posterior_predictive_check(A, y, self._chains(), burn=burn, offset=offset, seed=seed,
                                          device=self.device)

    def _check_data(self, X):
        """(A, y, offset) of a posterior predictive check: the training data without ``X``, else the
        held-out frame (see ``posterior_predictive_check``)."""
        if X is None:
            if self.samples is None or self.U_hat is None:
                raise ValueError("Must call `orthogonalize()` and `train()` before a posterior "
                                 "predictive check.")
            A = self.U_hat
            y = np.asarray(self.centered_experiment_train, dtype=np.float64)
            offset = np.asarray(self._predictions_mean_train, dtype=np.float64)
        else:
            if self.samples is None or self.Vt_hat is None:
                raise ValueError("Must call `orthogonalize()` and `train()` before a posterior "
                                 "predictive check.")
            if not isinstance(X, pd.DataFrame):
                raise ValueError(
                    "X must be a pandas DataFrame containing model predictions and the truth column.")
            if self.truth_column_name not in X.columns:
                raise ValueError(f"X must contain the truth column '{self.truth_column_name}'.")
            preds = np.asarray(X[self.models].values, dtype=np.float64)
            truth = np.asarray(X[self.truth_column_name].values, dtype=np.float64)
            A = preds @ np.asarray(self.Vt_hat, dtype=np.float64).T
            offset = preds.mean(axis=1)
            y = truth - offset
        return A, y, offset

    def check(self, X=None, burn=0, seed=None):
        """Posterior predictive check of the last ``train()`` under the likelihood it sampled from,
        as ``score()`` scores it (not in the reference): for a Gaussian or simplex fit exactly
        ``posterior_predictive_check()``; after ``{"sampler": "student_t"}`` the replicated noise
        is Student-t with that fit's ``nu``, and after ``"nu": "estimate"`` every draw replicates
        with its own ``nu`` -- the one predictive check that accepts a Student-t fit.  ``X``,
        ``burn`` and ``seed`` as ``posterior_predictive_check()``.  Returns the dict of
        ``pybmc_amd.ppc.posterior_predictive_check`` (``likelihood`` and ``nu_estimated``
        included) and ``nu``: None for the Gaussian likelihood, the fit's value, or the mean over
        the checked draws when it was estimated."""
        from .ppc import posterior_predictive_check
        nu = self._noise_df()
        estimated = self._nu_estimated()
        lik = {"nu_draws": self._nu_chains()} if estimated else {"nu": nu}
        A, y, offset = self._check_data(X)
        out = posterior_predictive_check(A, y, self._chains(), burn=burn, offset=offset, seed=seed,
                                         device=self.device, **lik)
        out["nu"] = float(np.mean(lik["nu_draws"][:, int(burn):])) if estimated else nu
        return out

    # ----------------------------------------------------------------- predict
    def _require_trained(self):
        if self.samples is None or self.Vt_hat is None:
            raise ValueError("Must call `orthogonalize()` and `train()` before predicting.")

    @staticmethod
    def _band_frames(domain_df, lower, median, upper):
        frames = []
        for name, vals in (("Predicted_Lower", lower), ("Predicted_Median", median),
                           ("Predicted_Upper", upper)):
            f = domain_df.copy()
            f[name] = vals
            frames.append(f)
        return frames

    def predict(self, X, noise_source="host"):
        """Posterior predictive for a DataFrame of model predictions
        (reference bmc.py:195-242).  ``noise_source``: where the t noise of a Student-t fit is made,
        ``"host"`` or ``"device"`` (``rndm_m_random_calculator``); a Gaussian fit ignores it."""
        self._require_trained()
        if not isinstance(X, pd.DataFrame):
            raise ValueError(
                "X must be a pandas DataFrame containing model predictions and domain info.")
        domain_keys = [c for c in X.columns if c not in self.models]
        rndm_m, (lo, med, up) = rndm_m_random_calculator(
            X[self.models].values, self.samples, self.Vt_hat, device=self.device,
            noise_df=self._noise_df(), noise_source=noise_source)
        lo_df, med_df, up_df = self._band_frames(X[domain_keys].reset_index(drop=True),
                                                 lo, med, up)
        return rndm_m, lo_df, med_df, up_df

    def predict2(self, property, noise_source="host"):
        """Posterior predictive for a property of ``data_dict``
        (reference bmc.py:244-337), including its model-set checks and prints.  ``noise_source``
        as in ``predict``."""
        self._require_trained()
        if property not in self.data_dict:
            raise KeyError(f"Property '{property}' not found in data_dict.")
        df = self.data_dict[property].copy()
        domain_keys = [c for c in df.columns
                       if c not in self.models and c != self.truth_column_name]
        available = [c for c in df.columns if c in self.models]
        trained_set, available_set = set(self.models), set(available)
        print(f"Available models: {available_set}")
        print(f"Trained models: {trained_set}")
        extra = available_set - trained_set
        if extra:
            raise ValueError(
                f"ERROR: Property '{property}' contains extra models not present during "
                f"training: {list(extra)}. You must retrain if using a larger model space.")
        missing = trained_set - available_set
        if missing:
            print(f"WARNING: Predicting on property '{property}' with missing models: "
                  f"{list(missing)}")
            print("         The trained model weights include these models — prediction will "
                  "proceed, but results may not be statistically accurate.")
        if not available:
            raise ValueError("No available trained models are present in prediction DataFrame.")
        idx = [self.models.index(m) for m in available]
        rndm_m, (lo, med, up) = rndm_m_random_calculator(
            df[available].values, self.samples, self.Vt_hat[:, idx], device=self.device,
            noise_df=self._noise_df(), noise_source=noise_source)
        lo_df, med_df, up_df = self._band_frames(df[domain_keys].reset_index(drop=True),
                                                 lo, med, up)
        return rndm_m, lo_df, med_df, up_df

    # ---------------------------------------------------------------- evaluate
    def evaluate(self, domain_filter=None, noise_source="host"):
        """Coverage of the credible intervals at 0,5,...,100 %
        (reference bmc.py:339-376; same filter semantics).  ``noise_source`` as in ``predict``."""
        self._require_trained()
        # tuple ranges use Series.between in the reference (bmc.py:360): inclusive, like the
        # explicit comparisons of the shared helper
        df = apply_domain_filters(self.data_dict[self.current_property], domain_filter)
        return predictive_coverage(np.arange(0, 101, 5), df[self.models].to_numpy(), self.samples,
                                   self.Vt_hat, df[self.truth_column_name].to_numpy(),
                                   device=self.device, noise_df=self._noise_df(),
                                   noise_source=noise_source)


def _series_tensor(samples, Vt_hat, device, nu=None):
    """[beta, sigma, weights] per draw as one device tensor (C, T, k+1+K): ONE upload of the
    (C, T, k+1) samples, the weights beta Vt_hat + 1/K formed next to them (torch matmul).  With
    ``nu`` (C, T) its column stands between sigma and the weights."""
    import torch

    dev = torch.device("cuda", device)
    s = torch.as_tensor(np.ascontiguousarray(samples, dtype=np.float64), device=dev)
    V = torch.as_tensor(np.ascontiguousarray(Vt_hat, dtype=np.float64), device=dev)
    w = torch.matmul(s[..., :-1], V) + 1.0 / V.shape[1]
    if nu is not None:
        col = torch.as_tensor(np.ascontiguousarray(nu, dtype=np.float64), device=dev)
        return torch.cat([s, col.reshape(s.shape[0], s.shape[1], 1), w], dim=-1)
    return torch.cat([s, w], dim=-1)


def _series_diagnostics(samples, Vt_hat, burn, device, nu=None):
    """Diagnostics of [beta, sigma, weights] per draw: the ``chain_diagnostics`` kernels on the
    concatenated tensor of ``_series_tensor``."""
    from .diagnostics import chain_diagnostics

    return chain_diagnostics(_series_tensor(samples, Vt_hat, device, nu), burn=burn, device=device)
