"""pybmc_amd: MI355X-native Gibbs-sampling core for Bayesian model combination.

Public names follow the reference package (pybmc/__init__.py:11-24); the
nonexistent ``Model`` of its ``__all__`` is dropped.
"""
from .bmc import BayesianModelCombination
from .cv import cv_component_path, fold_labels, kfold_cv, path_summary
from .data import Dataset
from .diagnostics import chain_autocovariance, chain_diagnostics
from .inference_utils import (gibbs_sampler, gibbs_sampler_robust, gibbs_sampler_simplex,
                              USVt_hat_extraction)
from .ppc import PPC_STATS, posterior_predictive_check, ppc_summary
from .rankdiag import rank_diagnostics, rank_normalize
from .sampling_utils import coverage, rndm_m_random_calculator
from .scoring import compare_elpd, pointwise_log_likelihood, psis_loo, psis_loo_predict, waic
from .sensitivity import (T_COMPONENTS, power_scale_sensitivity, power_scale_weights,
                          sensitivity_summary)

__all__ = [
    "Dataset",
    "BayesianModelCombination",
    "gibbs_sampler",
    "gibbs_sampler_robust",
    "gibbs_sampler_simplex",
    "USVt_hat_extraction",
    "coverage",
    "rndm_m_random_calculator",
    "chain_autocovariance",
    "chain_diagnostics",
    "rank_diagnostics",
    "rank_normalize",
    "pointwise_log_likelihood",
    "waic",
    "psis_loo",
    "psis_loo_predict",
    "compare_elpd",
    "kfold_cv",
    "fold_labels",
    "cv_component_path",
    "path_summary",
    "posterior_predictive_check",
    "ppc_summary",
    "PPC_STATS",
    "power_scale_sensitivity",
    "power_scale_weights",
    "sensitivity_summary",
    "T_COMPONENTS",
]
