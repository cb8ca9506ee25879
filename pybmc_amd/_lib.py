"""ctypes binding of libpybmc_amd.so (the C ABI declared in include/pybmc_amd.h).

There is no CPU fallback: if the shared library is missing, or no gfx950 GPU is
usable, the calls raise.  Status codes are mapped back to the exception types the
reference raises at the same places (numpy ``LinAlgError`` for singular matrices,
``ValueError`` for bad arguments).
"""
from __future__ import annotations

import ctypes as C
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libpybmc_amd.so")

ABI_VERSION = 4   # PYBMC_AMD_ABI_VERSION of include/pybmc_amd.h this binding was written for
BMC_OK, BMC_EINVAL, BMC_ESINGULAR, BMC_EHIP, BMC_ENOMEM, BMC_ETIMEOUT, BMC_ESTATE = range(7)
BMC_F64, BMC_F32 = 0, 1
BMC_ROW_MAJOR, BMC_COL_MAJOR = 0, 1
BMC_RNG_DEVICE, BMC_RNG_REPLAY = 0, 1
# smallest nu of device-made predictive t noise (bmc_predict_t): below about 0.052 the largest
# |t| = sqrt(nu) 2^(53/nu) is no double
MIN_PREDICT_NU = 0.06


class Tuning(C.Structure):
    _fields_ = [("groups_per_chain", C.c_int32), ("waves_per_group", C.c_int32),
                ("residency", C.c_int32), ("panels_per_wave", C.c_int32),
                ("force_agent_scope", C.c_int32), ("chains_per_pass", C.c_int32),
                ("rss_mode", C.c_int32), ("cu_limit", C.c_int32)]


class Stats(C.Structure):
    _fields_ = [("loop_ms", C.c_double), ("rng_ms", C.c_double), ("post_ms", C.c_double),
                ("total_ms", C.c_double), ("iterations", C.c_int64), ("n_chains", C.c_int32),
                ("launches", C.c_int32), ("groups_per_chain", C.c_int32),
                ("waves_per_group", C.c_int32), ("chains_per_pass", C.c_int32),
                ("residency", C.c_int32), ("xcd_local_chains", C.c_int32),
                ("bytes_per_pass", C.c_int64),
                ("passes", C.c_int64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


# name -> (restype, argtypes); every symbol include/pybmc_amd.h declares
_P = C.c_void_p
_D = C.POINTER(C.c_double)
PROTOTYPES = {
    "bmc_abi_version": (C.c_int, []),
    "bmc_create": (C.c_int, [C.c_int, C.POINTER(_P)]),
    "bmc_destroy": (None, [_P]),
    "bmc_last_error": (C.c_char_p, [_P]),
    "bmc_set_stream": (C.c_int, [_P, _P]),
    "bmc_set_tuning": (C.c_int, [_P, C.POINTER(Tuning)]),
    "bmc_set_problem": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int64, C.c_int, _P, C.c_int]),
    "bmc_set_problem_device": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int64, C.c_int, _P,
                                         C.c_int]),
    "bmc_orthogonalize": (C.c_int, [_P, _D, C.c_int64, C.c_int32, C.c_int64, _D, C.c_int32, _D, _D, _D,
                                    _D, _D]),
    "bmc_set_prior": (C.c_int, [_P, _D, _D, C.c_double, C.c_double]),
    "bmc_get_gram": (C.c_int, [_P, _D]),
    "bmc_get_basis": (C.c_int, [_P, _D, _D, _D]),
    "bmc_conditional_moments": (C.c_int, [_P, C.c_double, _D, _D]),
    "bmc_last_kernels": (C.c_int, [_P, C.c_char_p, C.c_int64, C.POINTER(C.c_int32),
                                   C.POINTER(C.c_int64)]),
    "bmc_residual_rss": (C.c_int, [_P, _D, C.c_int32, _D]),
    "bmc_residual_rss_bench": (C.c_int, [_P, C.c_int32, C.c_int32, _D]),
    "bmc_gram_bench": (C.c_int, [_P, C.c_int32, _D]),
    "bmc_predict_timing": (C.c_int, [_P, _D, _D, _D, _D]),
    "bmc_predict_draws": (C.c_int, [_P, _D, C.c_int]),
    "bmc_comm_unique_id": (C.c_int, [C.c_char_p]),
    "bmc_comm_init": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_char_p]),
    "bmc_allgather": (C.c_int, [_P, _P, _P, C.c_int64]),
    "bmc_comm_destroy": (C.c_int, [_P]),
    "bmc_gibbs_run": (C.c_int, [_P, C.c_int32, C.c_int64, C.POINTER(C.c_uint64), C.c_int, _D, _D,
                                _D, C.POINTER(Stats)]),
    "bmc_gibbs_run_device": (C.c_int, [_P, C.c_int32, C.c_int64, C.POINTER(C.c_uint64), _P,
                                       C.POINTER(Stats)]),
    "bmc_simplex_run": (C.c_int, [_P, _D, C.c_int32, _D, C.c_int64, C.c_int64, C.c_double, C.c_double,
                                  C.c_double, C.c_int, C.c_uint64, _D, _D, C.c_int64, _D, _D,
                                  C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(Stats)]),
    "bmc_simplex_run_chains": (C.c_int, [_P, _D, C.c_int32, _D, C.c_int32, C.c_int64, C.c_int64,
                                         C.c_double, C.c_double, C.c_double, C.c_int,
                                         C.POINTER(C.c_uint64), _D, _D, C.c_int64,
                                         C.POINTER(C.c_int64), _D, _D, C.POINTER(C.c_int64),
                                         C.POINTER(C.c_int64), C.POINTER(Stats)]),
    "bmc_predict": (C.c_int, [_P, _D, C.c_int64, C.c_int32, _D, C.c_int32, C.c_int32, _D, C.c_int,
                              C.c_uint64, _D, C.POINTER(C.c_int32), _D, C.c_int32, _D,
                              C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32, _D, _D,
                              C.POINTER(C.c_int64)]),
    "bmc_predict_t": (C.c_int, [_P, _D, C.c_int64, C.c_int32, _D, C.c_int32, C.c_int32, _D,
                                C.c_uint64, C.POINTER(C.c_int32), _D, C.c_int32, _D,
                                C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32, _D, _D,
                                C.POINTER(C.c_int64), C.c_double]),
    "bmc_predict_tv": (C.c_int, [_P, _D, C.c_int64, C.c_int32, _D, C.c_int32, C.c_int32, _D,
                                 C.c_uint64, C.POINTER(C.c_int32), _D, C.c_int32, _D,
                                 C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32, _D, _D,
                                 C.POINTER(C.c_int64), _D]),
    "bmc_chain_diagnostics": (C.c_int, [_P, _D, C.c_int32, C.c_int64, C.c_int32, C.c_int64,
                                        C.c_int64, _D, _D, _D, _D, _D, C.POINTER(C.c_int64)]),
    "bmc_chain_diagnostics_device": (C.c_int, [_P, _P, C.c_int32, C.c_int64, C.c_int32, C.c_int64,
                                               C.c_int64, _D, _D, _D, _D, _D,
                                               C.POINTER(C.c_int64)]),
    "bmc_chain_autocov": (C.c_int, [_P, _D, C.c_int32, C.c_int64, C.c_int32, C.c_int64, C.c_int64,
                                    C.POINTER(C.c_int32), C.c_int32, C.c_int64, C.c_int64, _D, _D, _D,
                                    _D]),
    "bmc_chain_autocov_device": (C.c_int, [_P, _P, C.c_int32, C.c_int64, C.c_int32, C.c_int64,
                                           C.c_int64, C.POINTER(C.c_int32), C.c_int32, C.c_int64,
                                           C.c_int64, _D, _D, _D, _D]),
    "bmc_rank_diagnostics": (C.c_int, [_P, _D, C.c_int32, C.c_int64, C.c_int32, C.c_int64, C.c_int64,
                                       _D, C.c_int32, C.c_int32, _D, _D, _D, _D, _D, _D, _D]),
    "bmc_rank_diagnostics_device": (C.c_int, [_P, _P, C.c_int32, C.c_int64, C.c_int32, C.c_int64,
                                              C.c_int64, _D, C.c_int32, C.c_int32, _D, _D, _D, _D, _D,
                                              _D, _D]),
    "bmc_rank_normalize": (C.c_int, [_P, _D, C.c_int32, C.c_int64, C.c_int32, C.c_int64, C.c_int64,
                                     C.c_int, _D]),
    "bmc_rank_normalize_device": (C.c_int, [_P, _P, C.c_int32, C.c_int64, C.c_int32, C.c_int64,
                                            C.c_int64, C.c_int, _D]),
    "bmc_rank_last_timing": (C.c_int, [_P, _D]),
    "bmc_pointwise_loglik": (C.c_int, [_P, _D, C.c_int64, C.c_int32, C.c_int64, C.c_int, _D, _D,
                                       C.c_int64, C.c_int64, _D, _D, _D]),
    "bmc_pointwise_loglik_device": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int64, C.c_int, _P,
                                              _P, C.c_int64, C.c_int64, _D, _D, _D]),
    "bmc_psis_loo": (C.c_int, [_P, _D, C.c_int64, C.c_int32, C.c_int64, C.c_int, _D, _D, C.c_int64,
                               C.c_int64, _D, _D, _D]),
    "bmc_psis_loo_device": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int64, C.c_int, _P, _P,
                                      C.c_int64, C.c_int64, _D, _D, _D]),
    "bmc_pointwise_loglik_t": (C.c_int, [_P, _D, C.c_int64, C.c_int32, C.c_int64, C.c_int, _D, _D,
                                         C.c_int64, C.c_int64, C.c_double, _D, _D, _D]),
    "bmc_pointwise_loglik_t_device": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int64, C.c_int, _P,
                                                _P, C.c_int64, C.c_int64, C.c_double, _D, _D, _D]),
    "bmc_psis_loo_t": (C.c_int, [_P, _D, C.c_int64, C.c_int32, C.c_int64, C.c_int, _D, _D, C.c_int64,
                                 C.c_int64, C.c_double, _D, _D, _D]),
    "bmc_psis_loo_t_device": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int64, C.c_int, _P, _P,
                                        C.c_int64, C.c_int64, C.c_double, _D, _D, _D]),
    "bmc_pointwise_loglik_tv": (C.c_int, [_P, _D, C.c_int64, C.c_int32, C.c_int64, C.c_int, _D, _D,
                                          C.c_int64, C.c_int64, _D, C.c_int32, C.POINTER(C.c_int32),
                                          _D, _D, _D]),
    "bmc_pointwise_loglik_tv_device": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int64, C.c_int, _P,
                                                 _P, C.c_int64, C.c_int64, _D, C.c_int32, _P, _D, _D,
                                                 _D]),
    "bmc_psis_loo_tv": (C.c_int, [_P, _D, C.c_int64, C.c_int32, C.c_int64, C.c_int, _D, _D, C.c_int64,
                                  C.c_int64, _D, C.c_int32, C.POINTER(C.c_int32), _D, _D, _D]),
    "bmc_psis_loo_tv_device": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int64, C.c_int, _P, _P,
                                         C.c_int64, C.c_int64, _D, C.c_int32, _P, _D, _D, _D]),
    "bmc_psis_loo_predict": (C.c_int, [_P, _D, C.c_int64, C.c_int32, C.c_int64, C.c_int, _D, _D,
                                       C.c_int64, C.c_int64, _D, _D, _D, _D, _D, _D, _D]),
    "bmc_psis_loo_predict_device": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int64, C.c_int, _P,
                                              _P, C.c_int64, C.c_int64, _D, _D, _D, _D, _D, _D, _D]),
    "bmc_psis_loo_predict_t": (C.c_int, [_P, _D, C.c_int64, C.c_int32, C.c_int64, C.c_int, _D, _D,
                                         C.c_int64, C.c_int64, C.c_double, _D, _D, _D, _D, _D, _D, _D]),
    "bmc_psis_loo_predict_t_device": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int64, C.c_int, _P,
                                                _P, C.c_int64, C.c_int64, C.c_double, _D, _D, _D, _D,
                                                _D, _D, _D]),
    "bmc_psis_loo_predict_tv": (C.c_int, [_P, _D, C.c_int64, C.c_int32, C.c_int64, C.c_int, _D, _D,
                                          C.c_int64, C.c_int64, _D, C.c_int32, C.POINTER(C.c_int32),
                                          _D, _D, _D, _D, _D, _D, _D]),
    "bmc_psis_loo_predict_tv_device": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int64, C.c_int, _P,
                                                 _P, C.c_int64, C.c_int64, _D, C.c_int32, _P, _D, _D,
                                                 _D, _D, _D, _D, _D]),
    "bmc_kfold_cv": (C.c_int, [_P, _D, C.c_int64, C.c_int32, C.c_int64, C.c_int, _D,
                               C.POINTER(C.c_int64), C.c_int32, _D, _D, C.c_double, C.c_double,
                               C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_uint64), _D,
                               _D, _D]),
    "bmc_kfold_cv_t": (C.c_int, [_P, _D, C.c_int64, C.c_int32, C.c_int64, C.c_int, _D,
                                 C.POINTER(C.c_int64), C.c_int32, _D, _D, C.c_double, C.c_double,
                                 C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_uint64),
                                 C.c_double, _D, _D, _D, _D]),
    "bmc_kfold_cv_tv": (C.c_int, [_P, _D, C.c_int64, C.c_int32, C.c_int64, C.c_int, _D,
                                  C.POINTER(C.c_int64), C.c_int32, _D, _D, C.c_double, C.c_double,
                                  C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_uint64),
                                  _D, _D, C.c_int32, C.c_int32, _D, _D, _D, _D, C.POINTER(C.c_int32)]),
    "bmc_cv_path": (C.c_int, [_P, _D, C.c_int64, C.c_int32, C.c_int64, C.c_int, _D,
                              C.POINTER(C.c_int64), C.c_int32, _D, _D, C.c_double, C.c_double,
                              C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_uint64),
                              C.POINTER(C.c_int32), C.c_int32, _D, _D, _D]),
    "bmc_ppc": (C.c_int, [_P, _D, C.c_int64, C.c_int32, C.c_int64, C.c_int, _D, _D, _D, C.c_int64,
                          C.c_int64, C.c_uint64, C.c_double, _D, _D]),
    "bmc_ppc_device": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int64, C.c_int, _P, _P, _P,
                                 C.c_int64, C.c_int64, C.c_uint64, C.c_double, _D, _D]),
    "bmc_ppc_t": (C.c_int, [_P, _D, C.c_int64, C.c_int32, C.c_int64, C.c_int, _D, _D, _D, C.c_int64,
                            C.c_int64, C.c_uint64, C.c_double, _D, _D]),
    "bmc_ppc_t_device": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int64, C.c_int, _P, _P, _P,
                                   C.c_int64, C.c_int64, C.c_uint64, C.c_double, _D, _D]),
    "bmc_ppc_tv": (C.c_int, [_P, _D, C.c_int64, C.c_int32, C.c_int64, C.c_int, _D, _D, _D, C.c_int64,
                             C.c_int64, C.c_uint64, _D, C.c_int32, C.POINTER(C.c_int32), _D, _D]),
    "bmc_ppc_tv_device": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int64, C.c_int, _P, _P, _P,
                                    C.c_int64, C.c_int64, C.c_uint64, _D, C.c_int32, _P, _D, _D]),
    "bmc_power_sensitivity": (C.c_int, [_P, _D, C.c_int64, C.c_int32, C.c_int64, C.c_int, _D, _D,
                                        C.c_int64, C.c_int64, _D, _D, C.c_double, C.c_double, _D,
                                        C.c_int32, _D, C.c_int32, C.c_uint32, C.c_int32, _D, _D, _D,
                                        _D, _D, _D, C.POINTER(C.c_uint32)]),
    "bmc_power_sensitivity_device": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int64, C.c_int, _P,
                                               _P, C.c_int64, C.c_int64, _D, _D, C.c_double,
                                               C.c_double, _D, C.c_int32, _D, C.c_int32, C.c_uint32,
                                               C.c_int32, _D, _D, _D, _D, _D, _D,
                                               C.POINTER(C.c_uint32)]),
    "bmc_power_sensitivity_t": (C.c_int, [_P, _D, C.c_int64, C.c_int32, C.c_int64, C.c_int, _D, _D,
                                          C.c_int64, C.c_int64, _D, _D, C.c_double, C.c_double, _D,
                                          C.c_int32, _D, C.c_int32, C.c_uint32, C.c_int32, C.c_double,
                                          _D, _D, _D, _D, _D, _D, C.POINTER(C.c_uint32)]),
    "bmc_power_sensitivity_t_device": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int64, C.c_int, _P,
                                                 _P, C.c_int64, C.c_int64, _D, _D, C.c_double,
                                                 C.c_double, _D, C.c_int32, _D, C.c_int32, C.c_uint32,
                                                 C.c_int32, C.c_double, _D, _D, _D, _D, _D, _D,
                                                 C.POINTER(C.c_uint32)]),
    "bmc_power_sensitivity_tv": (C.c_int, [_P, _D, C.c_int64, C.c_int32, C.c_int64, C.c_int, _D, _D,
                                           C.c_int64, C.c_int64, _D, _D, C.c_double, C.c_double, _D,
                                           C.c_int32, _D, C.c_int32, C.c_uint32, C.c_int32, _D,
                                           C.c_int32, C.POINTER(C.c_int32), _D, _D, _D, _D, _D, _D, _D,
                                           C.POINTER(C.c_uint32)]),
    "bmc_power_sensitivity_tv_device": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int64, C.c_int, _P,
                                                  _P, C.c_int64, C.c_int64, _D, _D, C.c_double,
                                                  C.c_double, _D, C.c_int32, _D, C.c_int32, C.c_uint32,
                                                  C.c_int32, _D, C.c_int32, _P, _D, _D, _D, _D, _D, _D,
                                                  _D, C.POINTER(C.c_uint32)]),
    "bmc_sens_last_timing": (C.c_int, [_P, _D]),
    "bmc_robust_run": (C.c_int, [_P, C.c_double, C.c_int32, C.c_int64, C.c_int64, C.c_int,
                                 C.POINTER(C.c_uint64), _D, _D, _D, _D, _D, C.POINTER(Stats)]),
    "bmc_robust_run_device": (C.c_int, [_P, C.c_double, C.c_int32, C.c_int64, C.c_int64,
                                        C.POINTER(C.c_uint64), _P, _P, C.POINTER(Stats)]),
    "bmc_robust_run_nu": (C.c_int, [_P, _D, _D, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64,
                                    C.c_int, C.POINTER(C.c_uint64), _D, _D, _D, _D,
                                    C.POINTER(C.c_int32), _D, _D, C.POINTER(C.c_int32), _D,
                                    C.POINTER(Stats)]),
    "bmc_robust_run_nu_device": (C.c_int, [_P, _D, _D, C.c_int32, C.c_int32, C.c_int32, C.c_int64,
                                           C.c_int64, C.POINTER(C.c_uint64), _P, _P, _P, _P,
                                           C.POINTER(Stats)]),
    "bmc_rng_fill": (C.c_int, [_P, C.c_uint64, C.c_int64, _D, C.c_double, C.c_int64, _D]),
    "bmc_philox_raw": (C.c_int, [_P, C.c_uint64, C.c_uint32, C.c_int64, C.POINTER(C.c_uint32)]),
}

_lib = None
_lib_lock = threading.Lock()


def _share_hip_runtime_with_torch():
    """One HIP runtime per process.  torch's wheel bundles its own libamdhip64.so (same
    soname as /opt/rocm's); if torch is imported AFTER this library bound the system copy, the
    process would hold two runtimes and device pointers could not be shared (bench.py and
    pybmc_amd.chains hand torch tensors to the C ABI).  So when torch is installed but not yet
    imported, its copy is loaded first; the dynamic loader then resolves our NEEDED entry and
    torch's own to that one object.  Set PYBMC_AMD_SYSTEM_HIP=1 to skip this."""
    import importlib.util
    import sys
    if "torch" in sys.modules or os.environ.get("PYBMC_AMD_SYSTEM_HIP") == "1":
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def bind(path, mode=C.RTLD_GLOBAL):
    """dlopen one build of the library and bind every prototype."""
    lib = C.CDLL(path, mode=mode)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.bmc_abi_version() != ABI_VERSION:
        raise RuntimeError(f"{path}: ABI version mismatch")
    return lib


def load_library():
    """dlopen the in-tree library and bind every prototype.  Raises if absent."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `make -C pybmc_amd/csrc` "
                "(or __graft_entry__.build()).  pybmc_amd has no CPU fallback.")
        _share_hip_runtime_with_torch()
        _lib = bind(LIB_PATH)
        return _lib


def _dptr(a):
    return a.ctypes.data_as(_D) if a is not None else None


class BmcError(RuntimeError):
    pass


class SingularFoldError(BmcError, np.linalg.LinAlgError):
    """A fold of ``kfold_cv``, or a (candidate, fold) of ``cv_component_path``, whose training Gram is
    numerically singular (BMC_ESINGULAR): the library's error, and the ``LinAlgError`` a refit of
    that fold would raise."""


class Context:
    """One bmc_ctx: one GPU, one host thread at a time."""

    def __init__(self, device=0, lib=None):
        # `lib`: another build of the same ABI (scripts/ab.py compares builds in one process)
        self._lib = lib if lib is not None else load_library()
        h = _P()
        rc = self._lib.bmc_create(int(device), C.byref(h))
        if rc != BMC_OK:
            raise BmcError(
                f"bmc_create(device={device}) failed with status {rc}: no usable gfx950 "
                "(MI355X) device.  pybmc_amd has no CPU fallback.")
        self._h = h
        self.device = int(device)
        self.n = self.k = 0
        # bumped whenever the resident (y, X) changes: lets a caller that left a problem on the
        # device (BayesianModelCombination.orthogonalize(method="device")) find out whether it
        # is still there before sampling from it
        self.problem_generation = 0
        self._last_predict = None     # (n_points, n_draws) of the last predict()
        # a bmc_ctx is driven by one host thread at a time: the functional API
        # (gibbs_sampler, rndm_m_random_calculator, ...) holds this lock for the whole
        # set_problem -> set_prior -> run sequence, so that two threads sharing the
        # per-device context serialise instead of sampling each other's problem
        self.lock = threading.RLock()

    # -- plumbing --------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._lib.bmc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc == BMC_OK:
            return
        msg = (self._lib.bmc_last_error(self._h) or b"").decode("utf-8", "replace")
        if rc == BMC_ESINGULAR:
            raise np.linalg.LinAlgError(msg or "Singular matrix")
        if rc == BMC_EINVAL:
            raise ValueError(msg)
        if rc == BMC_ENOMEM:
            raise MemoryError(msg)
        raise BmcError(f"status {rc}: {msg}")

    def set_stream(self, hip_stream_ptr):
        self._check(self._lib.bmc_set_stream(self._h, _P(hip_stream_ptr or 0)))

    def set_tuning(self, groups_per_chain=0, waves_per_group=0, residency=0, panels_per_wave=0,
                   force_agent_scope=0, chains_per_pass=0, rss_mode=0, cu_limit=0):
        """residency: 0 auto, 1 registers, 2 LDS, 3 stream from HBM; chains_per_pass: 0 auto,
        1 off, 2/4/8 cap (chains served per pass over X, or per bundle of an XCD's resident panels); rss_mode: 0 a pass over the data every iteration (the reference's
        computation, default), 1 the same number from sufficient statistics (opt-in, K <= 64);
        cu_limit: plan persistent launches for at most this many CUs (0 = the device's)."""
        t = Tuning(groups_per_chain, waves_per_group, residency, panels_per_wave,
                   force_agent_scope, chains_per_pass, rss_mode, cu_limit)
        self._check(self._lib.bmc_set_tuning(self._h, C.byref(t)))

    # -- problem / prior ---------------------------------------------------------
    def set_problem(self, y, X, dtype=None):
        """y (n,), X (n,k).  Keeps X's own memory order when it is C- or F-contiguous."""
        X = np.asarray(X)
        y = np.asarray(y)
        if X.ndim != 2 or y.ndim != 1 or X.shape[0] != y.shape[0]:
            raise ValueError("X must be (n, k) and y (n,)")
        if dtype is None:
            dtype = np.float32 if (X.dtype == np.float32 and y.dtype == np.float32) else np.float64
        dtype = np.dtype(dtype)
        if dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError("dtype must be float32 or float64")
        if X.flags.f_contiguous and not X.flags.c_contiguous:
            Xc = np.asfortranarray(X, dtype=dtype)
            layout, ldx = BMC_COL_MAJOR, X.shape[0]
        else:
            Xc = np.ascontiguousarray(X, dtype=dtype)
            layout, ldx = BMC_ROW_MAJOR, X.shape[1]
        yc = np.ascontiguousarray(y, dtype=dtype)
        n, k = X.shape
        self.problem_generation += 1   # (before the call: a failed call leaves no problem)
        self._check(self._lib.bmc_set_problem(
            self._h, Xc.ctypes.data_as(_P), n, k, max(ldx, 1), layout, yc.ctypes.data_as(_P),
            BMC_F32 if dtype == np.float32 else BMC_F64))
        self.n, self.k = n, k

    def set_problem_device(self, x_ptr, n, k, ldx, layout, y_ptr, f32=False):
        self.problem_generation += 1
        self._check(self._lib.bmc_set_problem_device(
            self._h, _P(x_ptr), n, k, ldx, layout, _P(y_ptr), BMC_F32 if f32 else BMC_F64))
        self.n, self.k = n, k

    def orthogonalize(self, F, truth, k, want_U=True):
        """Centre + thin SVD through the Gram on the device.  Returns
        (mu, y_c, U_hat or None, S_hat, Vt_rows); the context then holds (y_c, U_hat)."""
        F = np.ascontiguousarray(F, dtype=np.float64)
        truth = np.ascontiguousarray(truth, dtype=np.float64).reshape(-1)
        n, km = F.shape
        if truth.shape[0] != n:
            raise ValueError("truth must have one value per row of F")
        mu, yc = np.empty(n), np.empty(n)
        U = np.empty((k, n)) if want_U else None
        S, Vt = np.empty(k), np.empty((k, km))
        self.problem_generation += 1
        self._check(self._lib.bmc_orthogonalize(self._h, _dptr(F), n, km, km, _dptr(truth), int(k),
                                                _dptr(mu), _dptr(yc), _dptr(U), _dptr(S), _dptr(Vt)))
        self.n, self.k = n, int(k)
        return mu, yc, (U.T if U is not None else None), S, Vt

    def set_prior(self, b0, C0, nu0, sigma20):
        b0 = np.ascontiguousarray(b0, dtype=np.float64).reshape(-1)
        C0 = np.ascontiguousarray(C0, dtype=np.float64)
        if b0.shape[0] != self.k or C0.shape != (self.k, self.k):
            raise ValueError("prior shapes do not match the design matrix")
        self._check(self._lib.bmc_set_prior(self._h, _dptr(b0), _dptr(C0), float(nu0),
                                            float(sigma20)))

    # -- introspection -------------------------------------------------------------
    def gram(self):
        out = np.empty((self.k + 1, self.k + 1))
        self._check(self._lib.bmc_get_gram(self._h, _dptr(out)))
        return out

    def basis(self):
        W = np.empty((self.k, self.k))
        lam = np.empty(self.k)
        s2 = C.c_double()
        self._check(self._lib.bmc_get_basis(self._h, _dptr(W), _dptr(lam), C.byref(s2)))
        return W, lam, s2.value

    def conditional_moments(self, sigma2):
        mean = np.empty(self.k)
        cov = np.empty((self.k, self.k))
        self._check(self._lib.bmc_conditional_moments(self._h, float(sigma2), _dptr(mean),
                                                      _dptr(cov)))
        return mean, cov

    def last_kernels(self):
        """Demangled names of the persistent loop kernels the last gibbs_run* / simplex_run on
        this context launched, one per launch, in launch order ([] for rss_mode 1)."""
        need = C.c_int64()
        self._check(self._lib.bmc_last_kernels(self._h, None, 0, None, C.byref(need)))
        buf = C.create_string_buffer(need.value)
        self._check(self._lib.bmc_last_kernels(self._h, buf, need.value, None, None))
        return buf.value.decode().splitlines()

    def residual_rss(self, beta):
        beta = np.ascontiguousarray(np.atleast_2d(beta), dtype=np.float64)
        if beta.shape[1] != self.k:
            raise ValueError("beta must have k columns")
        out = np.empty(beta.shape[0])
        self._check(self._lib.bmc_residual_rss(self._h, _dptr(beta), beta.shape[0], _dptr(out)))
        return out

    def residual_rss_bench(self, nb=1, reps=20):
        ms = C.c_double()
        self._check(self._lib.bmc_residual_rss_bench(self._h, nb, reps, C.byref(ms)))
        return ms.value

    def gram_bench(self, reps=20):
        ms = C.c_double()
        self._check(self._lib.bmc_gram_bench(self._h, reps, C.byref(ms)))
        return ms.value

    def predict_timing(self):
        """HIP-event times (ms) of the last predict() on this context."""
        v = [C.c_double() for _ in range(4)]
        self._check(self._lib.bmc_predict_timing(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("h2d_ms", "gemm_ms", "select_ms", "device_ms"), (x.value for x in v)))

    # -- pooling over GPUs without torch (RCCL through the C ABI) ------------------------
    @staticmethod
    def comm_unique_id():
        """128-byte RCCL id made by rank 0; hand it to the other ranks by any transport."""
        buf = C.create_string_buffer(128)
        rc = load_library().bmc_comm_unique_id(buf)
        if rc != BMC_OK:
            raise BmcError(f"bmc_comm_unique_id failed with status {rc}: RCCL could not be loaded")
        return buf.raw

    def comm_init(self, world, rank, unique_id):
        if len(unique_id) != 128:
            raise ValueError("unique_id must be the 128 bytes of comm_unique_id()")
        self._check(self._lib.bmc_comm_init(self._h, int(world), int(rank), bytes(unique_id)))

    def allgather(self, send_ptr, recv_ptr, count_per_rank):
        """f64 all-gather of DEVICE buffers on the context's stream; blocks until done."""
        self._check(self._lib.bmc_allgather(self._h, _P(send_ptr), _P(recv_ptr),
                                            int(count_per_rank)))

    def comm_destroy(self):
        self._check(self._lib.bmc_comm_destroy(self._h))

    # -- the loop --------------------------------------------------------------------
    def gibbs_run(self, n_chains, iters, seeds=None, xi=None, g=None):
        """Returns (samples [n_chains, iters, k+1], stats dict)."""
        out = np.empty((n_chains, iters, self.k + 1))
        st = Stats()
        if xi is not None or g is not None:
            xi = np.ascontiguousarray(xi, dtype=np.float64).reshape(n_chains, iters, self.k)
            g = np.ascontiguousarray(g, dtype=np.float64).reshape(n_chains, iters)
            rc = self._lib.bmc_gibbs_run(self._h, n_chains, iters, None, BMC_RNG_REPLAY,
                                         _dptr(xi), _dptr(g), _dptr(out), C.byref(st))
        else:
            sd = np.ascontiguousarray(seeds, dtype=np.uint64).reshape(n_chains)
            rc = self._lib.bmc_gibbs_run(self._h, n_chains, iters,
                                         sd.ctypes.data_as(C.POINTER(C.c_uint64)),
                                         BMC_RNG_DEVICE, None, None, _dptr(out), C.byref(st))
        self._check(rc)
        return out, st.as_dict()

    def gibbs_run_device(self, n_chains, iters, seeds, out_ptr):
        sd = np.ascontiguousarray(seeds, dtype=np.uint64).reshape(n_chains)
        st = Stats()
        self._check(self._lib.bmc_gibbs_run_device(
            self._h, n_chains, iters, sd.ctypes.data_as(C.POINTER(C.c_uint64)), _P(out_ptr),
            C.byref(st)))
        return st.as_dict()

    # -- Student-t (outlier-robust) sampler ------------------------------------------------------
    def robust_run(self, nu, n_chains, iters, burn=0, seeds=None, xi=None, g=None, gl=None,
                   want_weights=True, nu_grid=None, nu_weight=None, nu_init=None, u_nu=None,
                   nu_path=None, want_tstat=False):
        """``n_chains`` Student-t chains on the resident problem and prior (bmc_robust_run).
        Device mode: ``seeds`` (n_chains,).  Replay mode: ``xi`` (n_chains, burn+iters, k), ``g``
        (n_chains, burn+iters), ``gl`` (n_chains, burn+iters, n).  Returns (samples (n_chains,
        iters, k+1), mean row weights (n_chains, n) or None, stats dict).

        With ``nu_grid`` (``nu`` is ignored) the degrees of freedom are drawn from the grid every
        sweep (bmc_robust_run_nu): ``nu_weight`` the prior weights, ``nu_init`` the starting index;
        replay mode also takes ``u_nu`` (n_chains, burn+iters) and the forced path ``nu_path``
        (n_chains, burn+iters) of grid indices.  Returns (samples, weights or None, grid indices
        (n_chains, iters) int32, T_t (n_chains, iters) or None, stats dict)."""
        n_chains, iters, burn = int(n_chains), int(iters), int(burn)
        if n_chains < 1 or iters < 0:
            raise ValueError("need n_chains >= 1 and iters >= 0")
        if nu_grid is not None:
            return self._robust_run_nu(nu_grid, nu_weight, nu_init, n_chains, iters, burn, seeds, xi, g,
                                       gl, u_nu, nu_path, want_weights, want_tstat)
        out = np.empty((n_chains, iters, self.k + 1))
        w = np.empty((n_chains, self.n)) if want_weights else None
        st = Stats()
        if xi is not None or g is not None or gl is not None:
            tt = burn + iters
            xi = np.ascontiguousarray(xi, dtype=np.float64).reshape(n_chains, tt, self.k)
            g = np.ascontiguousarray(g, dtype=np.float64).reshape(n_chains, tt)
            gl = np.ascontiguousarray(gl, dtype=np.float64).reshape(n_chains, tt, self.n)
            rc = self._lib.bmc_robust_run(self._h, float(nu), n_chains, iters, burn, BMC_RNG_REPLAY,
                                          None, _dptr(xi), _dptr(g), _dptr(gl), _dptr(out), _dptr(w),
                                          C.byref(st))
        else:
            sd = np.ascontiguousarray(seeds, dtype=np.uint64).reshape(n_chains)
            rc = self._lib.bmc_robust_run(self._h, float(nu), n_chains, iters, burn, BMC_RNG_DEVICE,
                                          sd.ctypes.data_as(C.POINTER(C.c_uint64)), None, None, None,
                                          _dptr(out), _dptr(w), C.byref(st))
        self._check(rc)
        return out, w, st.as_dict()

    def _robust_run_nu(self, nu_grid, nu_weight, nu_init, n_chains, iters, burn, seeds, xi, g, gl, u_nu,
                       nu_path, want_weights, want_tstat):
        grid = np.ascontiguousarray(nu_grid, dtype=np.float64).reshape(-1)
        wt = np.ascontiguousarray(nu_weight, dtype=np.float64).reshape(-1)
        if wt.shape != grid.shape:
            raise ValueError("nu_weight must have one entry per grid value")
        if nu_init is None:
            raise ValueError("nu_init (an index of nu_grid) is required with nu_grid")
        out = np.empty((n_chains, iters, self.k + 1))
        w = np.empty((n_chains, self.n)) if want_weights else None
        idx = np.empty((n_chains, iters), dtype=np.int32)
        ts = np.empty((n_chains, iters)) if want_tstat else None
        st = Stats()
        i32p = C.POINTER(C.c_int32)
        head = (self._h, _dptr(grid), _dptr(wt), grid.shape[0], int(nu_init), n_chains, iters, burn)
        tail = (_dptr(out), _dptr(w), idx.ctypes.data_as(i32p), _dptr(ts), C.byref(st))
        if xi is not None or g is not None or gl is not None:
            tt = burn + iters
            xi = np.ascontiguousarray(xi, dtype=np.float64).reshape(n_chains, tt, self.k)
            g = np.ascontiguousarray(g, dtype=np.float64).reshape(n_chains, tt)
            gl = np.ascontiguousarray(gl, dtype=np.float64).reshape(n_chains, tt, self.n)
            u_nu = np.ascontiguousarray(u_nu, dtype=np.float64).reshape(n_chains, tt)
            nu_path = np.ascontiguousarray(nu_path, dtype=np.int32).reshape(n_chains, tt)
            rc = self._lib.bmc_robust_run_nu(*head, BMC_RNG_REPLAY, None, _dptr(xi), _dptr(g), _dptr(gl),
                                             _dptr(u_nu), nu_path.ctypes.data_as(i32p), *tail)
        else:
            sd = np.ascontiguousarray(seeds, dtype=np.uint64).reshape(n_chains)
            rc = self._lib.bmc_robust_run_nu(*head, BMC_RNG_DEVICE,
                                             sd.ctypes.data_as(C.POINTER(C.c_uint64)), None, None, None,
                                             None, None, *tail)
        self._check(rc)
        return out, w, idx, ts, st.as_dict()

    def robust_run_nu_device(self, nu_grid, nu_weight, nu_init, n_chains, iters, burn, seeds, out_ptr,
                             idx_ptr, weight_ptr=None, tstat_ptr=None):
        grid = np.ascontiguousarray(nu_grid, dtype=np.float64).reshape(-1)
        wt = np.ascontiguousarray(nu_weight, dtype=np.float64).reshape(-1)
        if wt.shape != grid.shape:
            raise ValueError("nu_weight must have one entry per grid value")
        sd = np.ascontiguousarray(seeds, dtype=np.uint64).reshape(n_chains)
        st = Stats()
        self._check(self._lib.bmc_robust_run_nu_device(
            self._h, _dptr(grid), _dptr(wt), grid.shape[0], int(nu_init), int(n_chains), int(iters),
            int(burn), sd.ctypes.data_as(C.POINTER(C.c_uint64)), _P(out_ptr), _P(weight_ptr or 0),
            _P(idx_ptr), _P(tstat_ptr or 0), C.byref(st)))
        return st.as_dict()

    def robust_run_device(self, nu, n_chains, iters, burn, seeds, out_ptr, weight_ptr=None):
        sd = np.ascontiguousarray(seeds, dtype=np.uint64).reshape(n_chains)
        st = Stats()
        self._check(self._lib.bmc_robust_run_device(
            self._h, float(nu), int(n_chains), int(iters), int(burn),
            sd.ctypes.data_as(C.POINTER(C.c_uint64)), _P(out_ptr), _P(weight_ptr or 0), C.byref(st)))
        return st.as_dict()

    # -- simplex sampler --------------------------------------------------------------------
    def simplex_run(self, Vt_hat, S_hat, iters, nu0, sigma20, burn, stepsize, seed=0, xi=None,
                    unif=None, g=None, return_stats=False):
        """Returns (samples (iters, k+1), accepted) [+ (uniforms used, stats)]."""
        Vt_hat = np.ascontiguousarray(Vt_hat, dtype=np.float64)
        S_hat = np.ascontiguousarray(S_hat, dtype=np.float64).reshape(-1)
        if Vt_hat.ndim != 2 or Vt_hat.shape[0] != self.k or S_hat.shape[0] != self.k:
            raise ValueError("Vt_hat must be (k, n_models) and S_hat (k,)")
        out = np.empty((iters, self.k + 1))
        acc, used, st = C.c_int64(), C.c_int64(), Stats()
        if xi is not None:
            tt = burn + iters
            xi = np.ascontiguousarray(xi, dtype=np.float64).reshape(tt, self.k)
            g = np.ascontiguousarray(g, dtype=np.float64).reshape(tt)
            unif = np.ascontiguousarray(unif, dtype=np.float64).reshape(-1)
            rc = self._lib.bmc_simplex_run(
                self._h, _dptr(Vt_hat), Vt_hat.shape[1], _dptr(S_hat), iters, burn, stepsize, nu0,
                sigma20, BMC_RNG_REPLAY, 0, _dptr(xi), _dptr(unif), unif.shape[0], _dptr(g),
                _dptr(out), C.byref(acc), C.byref(used), C.byref(st))
        else:
            rc = self._lib.bmc_simplex_run(
                self._h, _dptr(Vt_hat), Vt_hat.shape[1], _dptr(S_hat), iters, burn, stepsize, nu0,
                sigma20, BMC_RNG_DEVICE, int(seed) & (2 ** 64 - 1), None, None, 0, None,
                _dptr(out), C.byref(acc), C.byref(used), C.byref(st))
        self._check(rc)
        if return_stats:
            return out, acc.value, used.value, st.as_dict()
        return out, acc.value

    def simplex_run_chains(self, Vt_hat, S_hat, n_chains, iters, nu0, sigma20, burn, stepsize,
                           seeds=None, xi=None, unif=None, n_unif=None, g=None, return_stats=False):
        """``n_chains`` independent simplex chains side by side on the device.  Device mode:
        ``seeds`` (n_chains,); chain c is bit for bit ``simplex_run(seed=seeds[c])``.  Replay mode:
        ``xi`` (n_chains, burn+iters, k), ``g`` (n_chains, burn+iters), ``unif`` (n_chains, ld) of
        which chain c may consume the first ``n_unif[c]`` (default: all ld).  Every chain starts
        at beta = 0 and burn-in is per chain.  Returns (samples (n_chains, iters, k+1), accepted
        (n_chains,), uniforms used (n_chains,)) [+ stats]."""
        Vt_hat = np.ascontiguousarray(Vt_hat, dtype=np.float64)
        S_hat = np.ascontiguousarray(S_hat, dtype=np.float64).reshape(-1)
        if Vt_hat.ndim != 2 or Vt_hat.shape[0] != self.k or S_hat.shape[0] != self.k:
            raise ValueError("Vt_hat must be (k, n_models) and S_hat (k,)")
        n_chains = int(n_chains)
        if n_chains < 1:
            raise ValueError("n_chains must be >= 1")
        out = np.empty((n_chains, iters, self.k + 1))
        acc = np.zeros(n_chains, dtype=np.int64)
        used = np.zeros(n_chains, dtype=np.int64)
        st = Stats()
        i64 = C.POINTER(C.c_int64)
        if xi is not None:
            tt = burn + iters
            xi = np.ascontiguousarray(xi, dtype=np.float64).reshape(n_chains, tt, self.k)
            g = np.ascontiguousarray(g, dtype=np.float64).reshape(n_chains, tt)
            unif = np.ascontiguousarray(unif, dtype=np.float64).reshape(n_chains, -1)
            ld = unif.shape[1]
            nu = (np.full(n_chains, ld, dtype=np.int64) if n_unif is None
                  else np.ascontiguousarray(n_unif, dtype=np.int64).reshape(n_chains))
            rc = self._lib.bmc_simplex_run_chains(
                self._h, _dptr(Vt_hat), Vt_hat.shape[1], _dptr(S_hat), n_chains, iters, burn,
                stepsize, nu0, sigma20, BMC_RNG_REPLAY, None, _dptr(xi), _dptr(unif), ld,
                nu.ctypes.data_as(i64), _dptr(g), _dptr(out), acc.ctypes.data_as(i64),
                used.ctypes.data_as(i64), C.byref(st))
        else:
            sd = np.ascontiguousarray(seeds, dtype=np.uint64).reshape(n_chains)
            rc = self._lib.bmc_simplex_run_chains(
                self._h, _dptr(Vt_hat), Vt_hat.shape[1], _dptr(S_hat), n_chains, iters, burn,
                stepsize, nu0, sigma20, BMC_RNG_DEVICE, sd.ctypes.data_as(C.POINTER(C.c_uint64)),
                None, None, 0, None, None, _dptr(out), acc.ctypes.data_as(i64),
                used.ctypes.data_as(i64), C.byref(st))
        self._check(rc)
        if return_stats:
            return out, acc, used, st.as_dict()
        return out, acc, used

    # -- posterior predictive --------------------------------------------------------------
    def predict_draws(self, order="C"):
        """The draws of the last predict() as an (n_draws, n_points) array: order "C" is the
        reference's layout (sampling_utils.py:77; transposed on the device), order "F" a
        Fortran-ordered array of the same shape (the device layout, no transpose)."""
        if self._last_predict is None:
            raise BmcError("no predict() has run on this context")
        M, S = self._last_predict
        if order == "C":
            out = np.empty((S, M))
            self._check(self._lib.bmc_predict_draws(self._h, _dptr(out), 1))
            return out
        out = np.empty((M, S))
        self._check(self._lib.bmc_predict_draws(self._h, _dptr(out), 0))
        return out.T

    def predict(self, preds, theta, Vt_hat, seed=0, noise=None, q=(2.5, 50, 97.5), truth=None,
                cov_percentiles=None, want_draws=True, draws_order="C", nu=None, nu_draws=None):
        """preds (M, Km), theta (S, k+1) selected posterior rows, Vt_hat (k, Km).
        Returns (rndm_m (S, M) or None, bands (len(q), M), coverage or None).  rndm_m is
        C-ordered like the reference's (draws_order="C", default) or Fortran-ordered
        (draws_order="F": the device layout, a point's draws contiguous).

        The noise: standard normals made on the device from ``seed`` (default); ``noise`` (S, M),
        replayed; Student-t variates made on the device from ``seed`` with ``nu`` degrees of freedom
        (bmc_predict_t) or ``nu_draws`` (S,) or (S, 1), one value per draw (bmc_predict_tv), every
        value finite and at least ``MIN_PREDICT_NU``.  At most one of the three may be given."""
        preds = np.ascontiguousarray(preds, dtype=np.float64)
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        Vt_hat = np.ascontiguousarray(Vt_hat, dtype=np.float64)
        M, Km = preds.shape
        S, k1 = theta.shape
        if Vt_hat.shape != (k1 - 1, Km):
            raise ValueError("Vt_hat must be (k, n_models) with k = theta.shape[1] - 1")
        if sum(x is not None for x in (noise, nu, nu_draws)) > 1:
            raise ValueError("at most one of noise, nu and nu_draws may be given")
        if nu is not None:
            if np.ndim(nu) != 0:
                raise ValueError("nu must be one number (nu_draws takes one per draw)")
            nu = float(nu)
            if not (np.isfinite(nu) and nu >= MIN_PREDICT_NU):
                raise ValueError(f"nu must be finite and at least {MIN_PREDICT_NU}")
        if nu_draws is not None:
            nu_draws = np.asarray(nu_draws, dtype=np.float64)
            if nu_draws.shape not in ((S,), (S, 1)):
                raise ValueError("nu_draws must be (n_draws,) or (n_draws, 1)")
            nu_draws = np.ascontiguousarray(nu_draws.reshape(S))
            if not (np.isfinite(nu_draws).all() and (nu_draws >= MIN_PREDICT_NU).all()):
                raise ValueError(f"every nu_draws must be finite and at least {MIN_PREDICT_NU}")
        qi, qg = order_stat_plan(S, q)
        bands = np.empty((len(q), M))
        lo = hi = hits = None
        tr = None
        n_cov = 0
        if truth is not None:
            tr = np.ascontiguousarray(truth, dtype=np.float64).reshape(M)
            lo, hi = coverage_plan(S, cov_percentiles)
            n_cov = len(lo)
            hits = np.zeros(n_cov, dtype=np.int64)
        nz = None
        if noise is not None:
            nz = np.ascontiguousarray(noise, dtype=np.float64)
            if nz.shape != (S, M):
                raise ValueError("noise must be (n_draws, n_points)")
        i32p = C.POINTER(C.c_int32)
        problem = (self._h, _dptr(preds), M, Km, _dptr(theta), S, k1 - 1, _dptr(Vt_hat))
        seed = int(seed) & (2 ** 64 - 1)
        asked = (qi.ctypes.data_as(i32p), _dptr(qg), len(q), _dptr(tr),
                 lo.ctypes.data_as(i32p) if lo is not None else None,
                 hi.ctypes.data_as(i32p) if hi is not None else None, n_cov, None,
                 _dptr(bands), hits.ctypes.data_as(C.POINTER(C.c_int64)) if hits is not None else None)
        if nu is not None:
            self._check(self._lib.bmc_predict_t(*problem, seed, *asked, nu))
        elif nu_draws is not None:
            self._check(self._lib.bmc_predict_tv(*problem, seed, *asked, _dptr(nu_draws)))
        else:
            self._check(self._lib.bmc_predict(
                *problem, BMC_RNG_REPLAY if nz is not None else BMC_RNG_DEVICE, seed, _dptr(nz),
                *asked))
        self._last_predict = (M, S)
        cov = None if hits is None else [int(h) / M * 100 for h in hits]
        return (self.predict_draws(draws_order) if want_draws else None), bands, cov

    # -- convergence diagnostics ------------------------------------------------------------
    def _diag_call(self, fn, ptr, n_chains, iters, n_cols, ld, burn):
        out = {k: np.empty(n_cols) for k in ("mean", "sd", "r_hat", "ess", "mcse_mean")}
        lag = np.empty(n_cols, dtype=np.int64)
        self._check(fn(self._h, ptr, int(n_chains), int(iters), int(n_cols), int(ld), int(burn),
                       _dptr(out["mean"]), _dptr(out["sd"]), _dptr(out["r_hat"]),
                       _dptr(out["ess"]), _dptr(out["mcse_mean"]),
                       lag.ctypes.data_as(C.POINTER(C.c_int64))))
        out["max_lag"] = lag
        return out

    def chain_diagnostics(self, samples, n_chains, iters, n_cols, ld, burn=0):
        """Split R-hat / ESS of a HOST f64 array whose element (c, t, j) is at
        c*iters*ld + t*ld + j (bmc_chain_diagnostics).  Returns a dict of [n_cols] arrays."""
        return self._diag_call(self._lib.bmc_chain_diagnostics, samples.ctypes.data_as(_D),
                               n_chains, iters, n_cols, ld, burn)

    def chain_diagnostics_device(self, d_ptr, n_chains, iters, n_cols, ld, burn=0):
        """The same on DEVICE memory (bmc_chain_diagnostics_device), read on the context's
        stream: the caller orders its producer before the call."""
        return self._diag_call(self._lib.bmc_chain_diagnostics_device, _P(d_ptr), n_chains, iters,
                               n_cols, ld, burn)

    def _autocov_call(self, fn, ptr, n_chains, iters, n_cols, ld, burn, cols, first_lag, n_lags):
        n_seq = 2 * n_chains + (n_chains if (iters - burn) % 2 else 0)
        if cols is None:
            n_active, cp = n_cols, None
        else:
            cols = np.ascontiguousarray(cols, dtype=np.int32).reshape(-1)
            n_active, cp = len(cols), cols.ctypes.data_as(C.POINTER(C.c_int32))
        out = {"seq_mean": np.empty((n_seq, n_cols)), "seq_m2": np.empty((n_seq, n_cols)),
               "shift": np.empty(n_cols), "acov": np.empty((max(n_active, 0), max(int(n_lags), 0)))}
        self._check(fn(self._h, ptr, int(n_chains), int(iters), int(n_cols), int(ld), int(burn), cp,
                       n_active, int(first_lag), int(n_lags), _dptr(out["seq_mean"]),
                       _dptr(out["seq_m2"]), _dptr(out["shift"]), _dptr(out["acov"])))
        return out

    def chain_autocov(self, samples, n_chains, iters, n_cols, ld, burn=0, cols=None, first_lag=0,
                      n_lags=64):
        """Per-sequence moments and the autocovariances a(first_lag .. first_lag + n_lags) of the
        columns `cols` (None: all) of a HOST f64 array laid out as for chain_diagnostics
        (bmc_chain_autocov).  Returns seq_mean, seq_m2 [n_seq, n_cols], shift [n_cols] and acov
        [len(cols), n_lags]."""
        return self._autocov_call(self._lib.bmc_chain_autocov, samples.ctypes.data_as(_D), n_chains,
                                  iters, n_cols, ld, burn, cols, first_lag, n_lags)

    def chain_autocov_device(self, d_ptr, n_chains, iters, n_cols, ld, burn=0, cols=None, first_lag=0,
                             n_lags=64):
        """The same on DEVICE memory (bmc_chain_autocov_device), read on the context's stream."""
        return self._autocov_call(self._lib.bmc_chain_autocov_device, _P(d_ptr), n_chains, iters,
                                  n_cols, ld, burn, cols, first_lag, n_lags)

    # -- rank-normalised diagnostics -------------------------------------------------------------
    RANK_KEYS = ("mean", "sd", "mcse_mean", "ess_bulk", "ess_tail", "r_hat")

    def _rank_call(self, fn, ptr, n_chains, iters, n_cols, ld, burn, probs, cols_per_batch):
        probs = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
        out = {k: np.empty(n_cols) for k in self.RANK_KEYS}
        quant = np.empty((len(probs), n_cols))
        self._check(fn(self._h, ptr, int(n_chains), int(iters), int(n_cols), int(ld), int(burn),
                       _dptr(probs), len(probs), int(cols_per_batch), _dptr(out["mean"]),
                       _dptr(out["sd"]), _dptr(quant), _dptr(out["r_hat"]), _dptr(out["ess_bulk"]),
                       _dptr(out["ess_tail"]), _dptr(out["mcse_mean"])))
        out["quantiles"] = quant
        return out

    def rank_diagnostics(self, samples, n_chains, iters, n_cols, ld, burn=0, probs=(0.05, 0.5, 0.95),
                         cols_per_batch=0):
        """Rank-normalised R-hat, bulk / tail ESS and quantiles of a HOST f64 array laid out as
        for chain_diagnostics (bmc_rank_diagnostics).  Returns a dict of [n_cols] arrays and
        ``quantiles`` [len(probs), n_cols]."""
        return self._rank_call(self._lib.bmc_rank_diagnostics, samples.ctypes.data_as(_D), n_chains,
                               iters, n_cols, ld, burn, probs, cols_per_batch)

    def rank_diagnostics_device(self, d_ptr, n_chains, iters, n_cols, ld, burn=0,
                                probs=(0.05, 0.5, 0.95), cols_per_batch=0):
        """The same on DEVICE memory (bmc_rank_diagnostics_device), read on the context's stream."""
        return self._rank_call(self._lib.bmc_rank_diagnostics_device, _P(d_ptr), n_chains, iters,
                               n_cols, ld, burn, probs, cols_per_batch)

    def _rank_normalize(self, fn, ptr, n_chains, iters, n_cols, ld, burn, folded):
        z = np.empty((2 * n_chains, (iters - burn) // 2, n_cols))
        self._check(fn(self._h, ptr, int(n_chains), int(iters), int(n_cols), int(ld), int(burn),
                       1 if folded else 0, _dptr(z)))
        return z

    def rank_normalize(self, samples, n_chains, iters, n_cols, ld, burn=0, folded=False):
        """z-scores of the exact ranks of a HOST f64 array's split draws (bmc_rank_normalize):
        (2 n_chains, n, n_cols)."""
        return self._rank_normalize(self._lib.bmc_rank_normalize, samples.ctypes.data_as(_D), n_chains,
                                    iters, n_cols, ld, burn, folded)

    def rank_normalize_device(self, d_ptr, n_chains, iters, n_cols, ld, burn=0, folded=False):
        return self._rank_normalize(self._lib.bmc_rank_normalize_device, _P(d_ptr), n_chains, iters,
                                    n_cols, ld, burn, folded)

    def rank_last_timing(self):
        """Device milliseconds of the last rank_diagnostics* call: sort, rank, classic, moments."""
        ms = np.zeros(4)
        self._check(self._lib.bmc_rank_last_timing(self._h, _dptr(ms)))
        return dict(zip(("sort_ms", "rank_ms", "classic_ms", "moments_ms"), ms.tolist()))

    # -- scoring: pointwise log predictive density, PSIS-LOO and its predictive moments -----------
    SCORE_KEYS = ("lppd", "p_waic", "mean_ll")
    LOO_KEYS = ("elpd_loo", "pareto_k", "lppd")
    LOO_PREDICT_KEYS = LOO_KEYS + ("loo_mean", "loo_sd", "loo_pit", "ess")

    def _score_call(self, fn, keys, ptr, A, n, k, lda, layout, y, theta, n_draws, ldt, nu=None):
        """One scoring entry point: `ptr` turns A, y and theta into what it takes (_dptr: host
        arrays, _P: device addresses), one [n] output vector per key.  `nu`: the degrees of
        freedom the Student-t (_t) entry points take behind ldt."""
        out = {key: np.empty(n) for key in keys}
        lik = () if nu is None else (float(nu),)
        self._check(fn(self._h, ptr(A), int(n), int(k), int(lda), int(layout), ptr(y), ptr(theta),
                       int(n_draws), int(ldt), *lik, *(_dptr(out[key]) for key in keys)))
        return out

    def pointwise_loglik(self, A, n, k, lda, layout, y, theta, n_draws, ldt):
        """lppd_i, p_waic_i and mean_ll_i of HOST f64 arrays (bmc_pointwise_loglik): A's element
        (i, j) at i*lda + j (BMC_ROW_MAJOR) or j*lda + i (BMC_COL_MAJOR), draw s at theta + s*ldt.
        Returns a dict of [n] arrays."""
        return self._score_call(self._lib.bmc_pointwise_loglik, self.SCORE_KEYS, _dptr,
                                A, n, k, lda, layout, y, theta, n_draws, ldt)

    def pointwise_loglik_device(self, dA, n, k, lda, layout, dy, dtheta, n_draws, ldt):
        """The same on DEVICE memory (bmc_pointwise_loglik_device), read on the context's stream:
        the caller orders its producers before the call."""
        return self._score_call(self._lib.bmc_pointwise_loglik_device, self.SCORE_KEYS, _P,
                                dA, n, k, lda, layout, dy, dtheta, n_draws, ldt)

    def psis_loo(self, A, n, k, lda, layout, y, theta, n_draws, ldt):
        """elpd_loo_i, pareto_k_i and lppd_i of HOST f64 arrays (bmc_psis_loo); arguments as
        pointwise_loglik.  Returns a dict of [n] arrays."""
        return self._score_call(self._lib.bmc_psis_loo, self.LOO_KEYS, _dptr,
                                A, n, k, lda, layout, y, theta, n_draws, ldt)

    def psis_loo_device(self, dA, n, k, lda, layout, dy, dtheta, n_draws, ldt):
        """The same on DEVICE memory (bmc_psis_loo_device), read on the context's stream: the
        caller orders its producers before the call."""
        return self._score_call(self._lib.bmc_psis_loo_device, self.LOO_KEYS, _P,
                                dA, n, k, lda, layout, dy, dtheta, n_draws, ldt)

    def pointwise_loglik_t(self, A, n, k, lda, layout, y, theta, n_draws, ldt, nu):
        """pointwise_loglik under the Student-t likelihood with `nu` degrees of freedom
        (bmc_pointwise_loglik_t)."""
        return self._score_call(self._lib.bmc_pointwise_loglik_t, self.SCORE_KEYS, _dptr,
                                A, n, k, lda, layout, y, theta, n_draws, ldt, nu)

    def pointwise_loglik_t_device(self, dA, n, k, lda, layout, dy, dtheta, n_draws, ldt, nu):
        """The same on DEVICE memory (bmc_pointwise_loglik_t_device)."""
        return self._score_call(self._lib.bmc_pointwise_loglik_t_device, self.SCORE_KEYS, _P,
                                dA, n, k, lda, layout, dy, dtheta, n_draws, ldt, nu)

    def psis_loo_t(self, A, n, k, lda, layout, y, theta, n_draws, ldt, nu):
        """psis_loo under the Student-t likelihood with `nu` degrees of freedom (bmc_psis_loo_t)."""
        return self._score_call(self._lib.bmc_psis_loo_t, self.LOO_KEYS, _dptr,
                                A, n, k, lda, layout, y, theta, n_draws, ldt, nu)

    def psis_loo_t_device(self, dA, n, k, lda, layout, dy, dtheta, n_draws, ldt, nu):
        """The same on DEVICE memory (bmc_psis_loo_t_device)."""
        return self._score_call(self._lib.bmc_psis_loo_t_device, self.LOO_KEYS, _P,
                                dA, n, k, lda, layout, dy, dtheta, n_draws, ldt, nu)

    def _score_call_tv(self, fn, keys, ptr, A, n, k, lda, layout, y, theta, n_draws, ldt, nu_values,
                       nu_index):
        """A _tv entry point: `nu_values` and `nu_index` as `_nu_args` takes them."""
        out = {key: np.empty(n) for key in keys}
        table, held = self._nu_args(ptr, nu_values, nu_index, n_draws)
        self._check(fn(self._h, ptr(A), int(n), int(k), int(lda), int(layout), ptr(y), ptr(theta),
                       int(n_draws), int(ldt), *table, *(_dptr(out[key]) for key in keys)))
        del held
        return out

    def pointwise_loglik_tv(self, A, n, k, lda, layout, y, theta, n_draws, ldt, nu_values, nu_index):
        """pointwise_loglik under the Student-t likelihood with nu_values[nu_index[s]] degrees of
        freedom for draw s (bmc_pointwise_loglik_tv)."""
        return self._score_call_tv(self._lib.bmc_pointwise_loglik_tv, self.SCORE_KEYS, _dptr, A, n, k,
                                   lda, layout, y, theta, n_draws, ldt, nu_values, nu_index)

    def pointwise_loglik_tv_device(self, dA, n, k, lda, layout, dy, dtheta, n_draws, ldt, nu_values,
                                   d_nu_index):
        """The same on DEVICE memory, the int32 index included (bmc_pointwise_loglik_tv_device)."""
        return self._score_call_tv(self._lib.bmc_pointwise_loglik_tv_device, self.SCORE_KEYS, _P, dA, n,
                                   k, lda, layout, dy, dtheta, n_draws, ldt, nu_values, d_nu_index)

    def psis_loo_tv(self, A, n, k, lda, layout, y, theta, n_draws, ldt, nu_values, nu_index):
        """psis_loo under the Student-t likelihood with a nu per draw (bmc_psis_loo_tv)."""
        return self._score_call_tv(self._lib.bmc_psis_loo_tv, self.LOO_KEYS, _dptr, A, n, k, lda, layout,
                                   y, theta, n_draws, ldt, nu_values, nu_index)

    def psis_loo_tv_device(self, dA, n, k, lda, layout, dy, dtheta, n_draws, ldt, nu_values, d_nu_index):
        """The same on DEVICE memory, the int32 index included (bmc_psis_loo_tv_device)."""
        return self._score_call_tv(self._lib.bmc_psis_loo_tv_device, self.LOO_KEYS, _P, dA, n, k, lda,
                                   layout, dy, dtheta, n_draws, ldt, nu_values, d_nu_index)

    def psis_loo_predict(self, A, n, k, lda, layout, y, theta, n_draws, ldt):
        """What psis_loo returns and the leave-one-out predictive loo_mean_i, loo_sd_i, loo_pit_i
        and the PSIS effective sample size ess_i of HOST f64 arrays (bmc_psis_loo_predict);
        arguments as pointwise_loglik.  Returns a dict of [n] arrays."""
        return self._score_call(self._lib.bmc_psis_loo_predict, self.LOO_PREDICT_KEYS, _dptr,
                                A, n, k, lda, layout, y, theta, n_draws, ldt)

    def psis_loo_predict_device(self, dA, n, k, lda, layout, dy, dtheta, n_draws, ldt):
        """The same on DEVICE memory (bmc_psis_loo_predict_device), read on the context's stream:
        the caller orders its producers before the call."""
        return self._score_call(self._lib.bmc_psis_loo_predict_device, self.LOO_PREDICT_KEYS, _P,
                                dA, n, k, lda, layout, dy, dtheta, n_draws, ldt)

    def psis_loo_predict_t(self, A, n, k, lda, layout, y, theta, n_draws, ldt, nu):
        """psis_loo_predict under the Student-t likelihood with `nu` degrees of freedom, 0.06 to 1000
        (bmc_psis_loo_predict_t)."""
        return self._score_call(self._lib.bmc_psis_loo_predict_t, self.LOO_PREDICT_KEYS, _dptr,
                                A, n, k, lda, layout, y, theta, n_draws, ldt, nu)

    def psis_loo_predict_t_device(self, dA, n, k, lda, layout, dy, dtheta, n_draws, ldt, nu):
        """The same on DEVICE memory (bmc_psis_loo_predict_t_device)."""
        return self._score_call(self._lib.bmc_psis_loo_predict_t_device, self.LOO_PREDICT_KEYS, _P,
                                dA, n, k, lda, layout, dy, dtheta, n_draws, ldt, nu)

    def psis_loo_predict_tv(self, A, n, k, lda, layout, y, theta, n_draws, ldt, nu_values, nu_index):
        """psis_loo_predict under the Student-t likelihood with a nu per draw
        (bmc_psis_loo_predict_tv)."""
        return self._score_call_tv(self._lib.bmc_psis_loo_predict_tv, self.LOO_PREDICT_KEYS, _dptr, A,
                                   n, k, lda, layout, y, theta, n_draws, ldt, nu_values, nu_index)

    def psis_loo_predict_tv_device(self, dA, n, k, lda, layout, dy, dtheta, n_draws, ldt, nu_values,
                                   d_nu_index):
        """The same on DEVICE memory, the int32 index included (bmc_psis_loo_predict_tv_device)."""
        return self._score_call_tv(self._lib.bmc_psis_loo_predict_tv_device, self.LOO_PREDICT_KEYS, _P,
                                   dA, n, k, lda, layout, dy, dtheta, n_draws, ldt, nu_values,
                                   d_nu_index)

    # -- posterior predictive check ---------------------------------------------------------------
    def _ppc_call(self, fn, ptr, A, n, k, lda, layout, y, theta, n_draws, ldt, offset, seed, *noise):
        """One predictive-check entry point; `noise` is what it takes between the seed and the
        outputs: `center`, `nu`, or the table of `_nu_args`."""
        t_rep = np.empty((int(n_draws), 8))
        t_obs2 = np.empty((int(n_draws), 2))
        self._check(fn(self._h, ptr(A), int(n), int(k), int(lda), int(layout), ptr(y),
                       ptr(offset) if offset is not None else None, ptr(theta), int(n_draws),
                       int(ldt), int(seed) & (2 ** 64 - 1), *noise, _dptr(t_rep), _dptr(t_obs2)))
        return {"t_rep": t_rep, "t_obs2": t_obs2}

    @staticmethod
    def _nu_args(ptr, nu_values, nu_index, n_draws):
        """(values, count, index) as a _tv entry point takes them, and what must outlive the call:
        `nu_values` the distinct degrees of freedom (host), `nu_index` every draw's index into
        them, a host int32 array (ptr is _dptr) or a device address (_P)."""
        vals = np.ascontiguousarray(nu_values, dtype=np.float64).reshape(-1)
        if ptr is _dptr:
            nu_index = np.ascontiguousarray(nu_index, dtype=np.int32).reshape(-1)
            if nu_index.shape[0] != int(n_draws):
                raise ValueError("nu_index must have one entry per draw")
            idx = nu_index.ctypes.data_as(C.POINTER(C.c_int32))
        else:
            idx = _P(nu_index)
        return (_dptr(vals), vals.shape[0], idx), (vals, nu_index)

    def ppc(self, A, n, k, lda, layout, y, theta, n_draws, ldt, offset, seed, center):
        """The per-draw statistics of replicated data, t_rep (n_draws, 8), and the observed chi2
        and max_abs_z, t_obs2 (n_draws, 2), of HOST f64 arrays (bmc_ppc); A, y and theta as
        pointwise_loglik, offset [n] or None; center is kept by the ABI and no longer read."""
        return self._ppc_call(self._lib.bmc_ppc, _dptr, A, n, k, lda, layout, y, theta, n_draws,
                              ldt, offset, seed, float(center))

    def ppc_device(self, dA, n, k, lda, layout, dy, dtheta, n_draws, ldt, doffset, seed, center):
        """The same on DEVICE memory (bmc_ppc_device; doffset an address or None), read on the
        context's stream: the caller orders its producers before the call."""
        return self._ppc_call(self._lib.bmc_ppc_device, _P, dA, n, k, lda, layout, dy, dtheta,
                              n_draws, ldt, doffset, seed, float(center))

    def ppc_t(self, A, n, k, lda, layout, y, theta, n_draws, ldt, offset, seed, nu):
        """ppc with Student-t replicated noise of `nu` degrees of freedom (bmc_ppc_t)."""
        return self._ppc_call(self._lib.bmc_ppc_t, _dptr, A, n, k, lda, layout, y, theta, n_draws,
                              ldt, offset, seed, float(nu))

    def ppc_t_device(self, dA, n, k, lda, layout, dy, dtheta, n_draws, ldt, doffset, seed, nu):
        """The same on DEVICE memory (bmc_ppc_t_device)."""
        return self._ppc_call(self._lib.bmc_ppc_t_device, _P, dA, n, k, lda, layout, dy, dtheta,
                              n_draws, ldt, doffset, seed, float(nu))

    def ppc_tv(self, A, n, k, lda, layout, y, theta, n_draws, ldt, offset, seed, nu_values, nu_index):
        """ppc with Student-t replicated noise of nu_values[nu_index[s]] degrees of freedom for draw
        s (bmc_ppc_tv)."""
        noise, held = self._nu_args(_dptr, nu_values, nu_index, n_draws)
        out = self._ppc_call(self._lib.bmc_ppc_tv, _dptr, A, n, k, lda, layout, y, theta, n_draws,
                             ldt, offset, seed, *noise)
        del held
        return out

    def ppc_tv_device(self, dA, n, k, lda, layout, dy, dtheta, n_draws, ldt, doffset, seed, nu_values,
                      d_nu_index):
        """The same on DEVICE memory, the int32 index included (bmc_ppc_tv_device)."""
        noise, held = self._nu_args(_P, nu_values, d_nu_index, n_draws)
        out = self._ppc_call(self._lib.bmc_ppc_tv_device, _P, dA, n, k, lda, layout, dy, dtheta,
                             n_draws, ldt, doffset, seed, *noise)
        del held
        return out

    # -- power-scaling sensitivity ----------------------------------------------------------------
    SENS_COMPONENTS = ("prior", "likelihood", "prior_beta", "prior_sigma2")   # bit order of the mask

    SENS_T_COMPONENTS = SENS_COMPONENTS + ("prior_nu",)   # the mask of the Student-t forms

    def _sens_call(self, fn, ptr, A, n, k, lda, layout, y, theta, n_draws, ldt, prior, Vt, alphas,
                   components, cols_per_batch, want_weights, likelihood=(), logdens_rows=3,
                   nu_column=False):
        """One sensitivity entry point; `likelihood` is what a Student-t form takes between
        cols_per_batch and the outputs (`nu`, or the table of `_nu_args` and the log prior)."""
        b0, C0, nu0, sigma20 = prior
        b0 = np.ascontiguousarray(b0, dtype=np.float64).reshape(-1)
        C0 = np.ascontiguousarray(C0, dtype=np.float64)
        if b0.shape != (k,) or C0.shape != (k, k):
            raise ValueError(f"the prior must hold b0 ({k},) and C0 ({k}, {k})")
        if Vt is not None and (np.ndim(Vt) != 2 or np.shape(Vt)[0] != k):
            raise ValueError(f"Vt must be ({k}, n_models)")
        alphas = np.ascontiguousarray(alphas, dtype=np.float64).reshape(-1)
        n_models = 0
        if Vt is not None:
            Vt = np.ascontiguousarray(Vt, dtype=np.float64)
            n_models = int(Vt.shape[1])
        S, mask = int(n_draws), int(components)
        n_comp = bin(mask).count("1")
        W, Q = n_comp * len(alphas), int(k) + 1 + n_models + (1 if nu_column else 0)
        out = {"logdens": np.empty((logdens_rows, S)), "pareto_k": np.empty((n_comp, len(alphas))),
               "mean": np.empty((n_comp, len(alphas), Q)), "sd": np.empty((n_comp, len(alphas), Q)),
               "cjs": np.empty((n_comp, len(alphas), Q)),
               "weights": np.empty((S, W)) if want_weights else None}
        flags = np.zeros(n_comp + Q, dtype=np.uint32)
        self._check(fn(self._h, ptr(A), int(n), int(k), int(lda), int(layout), ptr(y), ptr(theta), S,
                       int(ldt), _dptr(b0), _dptr(C0), float(nu0), float(sigma20), _dptr(Vt), n_models,
                       _dptr(alphas), len(alphas), mask, int(cols_per_batch), *likelihood,
                       _dptr(out["logdens"]),
                       _dptr(out["pareto_k"]), _dptr(out["mean"]), _dptr(out["sd"]), _dptr(out["cjs"]),
                       _dptr(out["weights"]), flags.ctypes.data_as(C.POINTER(C.c_uint32))))
        out["component_flags"] = flags[:n_comp].astype(bool)
        out["column_flags"] = flags[n_comp:].astype(bool)
        return out

    def power_sensitivity(self, A, n, k, lda, layout, y, theta, n_draws, ldt, prior, Vt, alphas,
                          components, cols_per_batch=0, want_weights=False):
        """bmc_power_sensitivity of HOST f64 arrays: A, y and theta as pointwise_loglik, prior =
        (b0, C0, nu0, sigma20), Vt (k, n_models) or None, alphas, components a bit mask in the
        order of SENS_COMPONENTS.  Returns a dict: ``logdens`` (3, S), ``pareto_k`` (c, a),
        ``mean`` / ``sd`` / ``cjs`` (c, a, Q), ``weights`` (S, c * a) or None, and the boolean
        ``component_flags`` (c,) and ``column_flags`` (Q,)."""
        return self._sens_call(self._lib.bmc_power_sensitivity, _dptr, A, n, k, lda, layout, y, theta,
                               n_draws, ldt, prior, Vt, alphas, components, cols_per_batch, want_weights)

    def power_sensitivity_device(self, dA, n, k, lda, layout, dy, dtheta, n_draws, ldt, prior, Vt,
                                 alphas, components, cols_per_batch=0, want_weights=False):
        """The same on DEVICE memory for A, y and theta (bmc_power_sensitivity_device), read on the
        context's stream: the caller orders its producers before the call."""
        return self._sens_call(self._lib.bmc_power_sensitivity_device, _P, dA, n, k, lda, layout, dy,
                               dtheta, n_draws, ldt, prior, Vt, alphas, components, cols_per_batch,
                               want_weights)

    def power_sensitivity_t(self, A, n, k, lda, layout, y, theta, n_draws, ldt, prior, Vt, alphas,
                            components, cols_per_batch, want_weights, nu):
        """power_sensitivity under the Student-t likelihood with `nu` degrees of freedom
        (bmc_power_sensitivity_t): components a mask in the order of SENS_T_COMPONENTS (prior_nu is
        not valid here), ``logdens`` (4, S) with a last row of zeros, the log prior of nu."""
        return self._sens_call(self._lib.bmc_power_sensitivity_t, _dptr, A, n, k, lda, layout, y, theta,
                               n_draws, ldt, prior, Vt, alphas, components, cols_per_batch, want_weights,
                               likelihood=(float(nu),), logdens_rows=4)

    def power_sensitivity_t_device(self, dA, n, k, lda, layout, dy, dtheta, n_draws, ldt, prior, Vt,
                                   alphas, components, cols_per_batch, want_weights, nu):
        """The same on DEVICE memory (bmc_power_sensitivity_t_device)."""
        return self._sens_call(self._lib.bmc_power_sensitivity_t_device, _P, dA, n, k, lda, layout, dy,
                               dtheta, n_draws, ldt, prior, Vt, alphas, components, cols_per_batch,
                               want_weights, likelihood=(float(nu),), logdens_rows=4)

    def _sens_call_tv(self, fn, ptr, args, nu_values, nu_index, nu_log_prior):
        table, held = self._nu_args(ptr, nu_values, nu_index, args[7])   # (args[7]: n_draws)
        if nu_log_prior is not None:
            nu_log_prior = np.ascontiguousarray(nu_log_prior, dtype=np.float64).reshape(-1)
            if nu_log_prior.shape[0] != table[1]:
                raise ValueError("nu_log_prior must have one entry per value of nu_values")
        out = self._sens_call(fn, ptr, *args, likelihood=(*table, _dptr(nu_log_prior)), logdens_rows=4,
                              nu_column=True)
        del held
        return out

    def power_sensitivity_tv(self, A, n, k, lda, layout, y, theta, n_draws, ldt, prior, Vt, alphas,
                             components, cols_per_batch, want_weights, nu_values, nu_index,
                             nu_log_prior=None):
        """power_sensitivity under the Student-t likelihood with nu_values[nu_index[s]] degrees of
        freedom for draw s (bmc_power_sensitivity_tv); nu_log_prior, one entry per value or None,
        is the log of the normalised prior weight of every value (with it, prior_nu is a
        component).  ``logdens`` is (4, S); the quantity columns end in one more, nu."""
        return self._sens_call_tv(self._lib.bmc_power_sensitivity_tv, _dptr,
                                  (A, n, k, lda, layout, y, theta, n_draws, ldt, prior, Vt, alphas,
                                   components, cols_per_batch, want_weights),
                                  nu_values, nu_index, nu_log_prior)

    def power_sensitivity_tv_device(self, dA, n, k, lda, layout, dy, dtheta, n_draws, ldt, prior, Vt,
                                    alphas, components, cols_per_batch, want_weights, nu_values,
                                    d_nu_index, nu_log_prior=None):
        """The same on DEVICE memory, the int32 index included (bmc_power_sensitivity_tv_device)."""
        return self._sens_call_tv(self._lib.bmc_power_sensitivity_tv_device, _P,
                                  (dA, n, k, lda, layout, dy, dtheta, n_draws, ldt, prior, Vt, alphas,
                                   components, cols_per_batch, want_weights),
                                  nu_values, d_nu_index, nu_log_prior)

    def sens_last_timing(self):
        """Device milliseconds of the last power_sensitivity* call: log densities, sorts, Pareto
        smoothing, distances."""
        ms = np.zeros(4)
        self._check(self._lib.bmc_sens_last_timing(self._h, _dptr(ms)))
        return dict(zip(("logdens_ms", "sort_ms", "psis_ms", "cjs_ms"), ms.tolist()))

    # -- exact K-fold / leave-group-out cross-validation --------------------------------------------
    def kfold_cv(self, A, n, k, lda, layout, y, fold, n_folds, b0, C0, nu0, sigma20, n_chains, iters,
                 burn, thin, seeds, return_draws=False):
        """bmc_kfold_cv of HOST arrays: A's element (i, j) as in pointwise_loglik, y [n] f64, fold
        [n] int64 labels, seeds [n_folds * n_chains] uint64.  Returns (elpd_cv_i [n], cv_mean_i [n],
        draws (n_folds, n_chains, kept, k+1) or None).  A singular fold raises SingularFoldError."""
        kept = max(0, -(-(int(iters) - int(burn)) // int(thin)))
        elpd, mean = np.empty(n), np.empty(n)
        draws = np.empty((n_folds, n_chains, kept, k + 1)) if return_draws else None
        b0 = np.ascontiguousarray(b0, dtype=np.float64)
        C0 = np.ascontiguousarray(C0, dtype=np.float64)
        fold = np.ascontiguousarray(fold, dtype=np.int64)
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
        rc = self._lib.bmc_kfold_cv(
            self._h, _dptr(A), int(n), int(k), int(lda), int(layout), _dptr(y),
            fold.ctypes.data_as(C.POINTER(C.c_int64)), int(n_folds), _dptr(b0), _dptr(C0),
            float(nu0), float(sigma20), int(n_chains), int(iters), int(burn), int(thin),
            seeds.ctypes.data_as(C.POINTER(C.c_uint64)), _dptr(elpd), _dptr(mean), _dptr(draws))
        if rc == BMC_ESINGULAR:
            raise SingularFoldError(
                (self._lib.bmc_last_error(self._h) or b"").decode("utf-8", "replace"))
        self._check(rc)
        return elpd, mean, draws

    def kfold_cv_t(self, A, n, k, lda, layout, y, fold, n_folds, b0, C0, nu0, sigma20, n_chains, iters,
                   burn, thin, seeds, nu=None, nu_grid=None, nu_weight=None, nu_init=None,
                   return_draws=False, return_row_weights=False):
        """bmc_kfold_cv_t (``nu`` a number) or bmc_kfold_cv_tv (``nu_grid``, ``nu_weight`` and the
        index ``nu_init``) of HOST arrays, the arguments of ``kfold_cv``.  Returns (elpd_cv_i [n],
        cv_mean_i [n], draws (n_folds, n_chains, kept, k+1) or None, row weights (n_folds, n_chains,
        n) or None, grid indices (n_folds, n_chains, kept) int32 or None).  A singular fold or a
        failed Cholesky pivot raises SingularFoldError."""
        kept = max(0, -(-(int(iters) - int(burn)) // int(thin)))
        elpd, mean = np.empty(n), np.empty(n)
        draws = np.empty((n_folds, n_chains, kept, k + 1)) if return_draws else None
        w = np.empty((n_folds, n_chains, n)) if return_row_weights else None
        b0 = np.ascontiguousarray(b0, dtype=np.float64)
        C0 = np.ascontiguousarray(C0, dtype=np.float64)
        fold = np.ascontiguousarray(fold, dtype=np.int64)
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
        head = (self._h, _dptr(A), int(n), int(k), int(lda), int(layout), _dptr(y),
                fold.ctypes.data_as(C.POINTER(C.c_int64)), int(n_folds), _dptr(b0), _dptr(C0),
                float(nu0), float(sigma20), int(n_chains), int(iters), int(burn), int(thin),
                seeds.ctypes.data_as(C.POINTER(C.c_uint64)))
        idx = None
        if nu_grid is None:
            rc = self._lib.bmc_kfold_cv_t(*head, float(nu), _dptr(elpd), _dptr(mean), _dptr(draws), _dptr(w))
        else:
            grid = np.ascontiguousarray(nu_grid, dtype=np.float64).reshape(-1)
            wt = np.ascontiguousarray(nu_weight, dtype=np.float64).reshape(-1)
            if wt.shape != grid.shape:
                raise ValueError("nu_weight must have one entry per grid value")
            idx = np.empty((n_folds, n_chains, kept), dtype=np.int32)
            rc = self._lib.bmc_kfold_cv_tv(*head, _dptr(grid), _dptr(wt), grid.shape[0], int(nu_init),
                                           _dptr(elpd), _dptr(mean), _dptr(draws), _dptr(w),
                                           idx.ctypes.data_as(C.POINTER(C.c_int32)))
        if rc == BMC_ESINGULAR:
            raise SingularFoldError(
                (self._lib.bmc_last_error(self._h) or b"").decode("utf-8", "replace"))
        self._check(rc)
        return elpd, mean, draws, w, idx

    def cv_path(self, A, n, k, lda, layout, y, fold, n_folds, b0, C0, nu0, sigma20, n_chains, iters,
                burn, thin, seeds, comps, return_draws=False):
        """bmc_cv_path of HOST arrays: the arguments of ``kfold_cv`` and comps [m] int32 candidate
        component counts.  Returns (elpd_cv_i [m, n], cv_mean_i [m, n], draws: a list of m arrays
        (n_folds, n_chains, kept, k_j + 1), or None).  A singular (candidate, fold) raises
        SingularFoldError."""
        kept = max(0, -(-(int(iters) - int(burn)) // int(thin)))
        comps = np.ascontiguousarray(comps, dtype=np.int32)
        m = int(comps.shape[0])
        elpd, mean = np.empty((m, n)), np.empty((m, n))
        sizes = [n_folds * n_chains * kept * (int(kj) + 1) for kj in comps]
        flat = np.empty(sum(sizes)) if return_draws else None
        b0 = np.ascontiguousarray(b0, dtype=np.float64)
        C0 = np.ascontiguousarray(C0, dtype=np.float64)
        fold = np.ascontiguousarray(fold, dtype=np.int64)
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
        rc = self._lib.bmc_cv_path(
            self._h, _dptr(A), int(n), int(k), int(lda), int(layout), _dptr(y),
            fold.ctypes.data_as(C.POINTER(C.c_int64)), int(n_folds), _dptr(b0), _dptr(C0),
            float(nu0), float(sigma20), int(n_chains), int(iters), int(burn), int(thin),
            seeds.ctypes.data_as(C.POINTER(C.c_uint64)), comps.ctypes.data_as(C.POINTER(C.c_int32)), m,
            _dptr(elpd), _dptr(mean), _dptr(flat))
        if rc == BMC_ESINGULAR:
            raise SingularFoldError(
                (self._lib.bmc_last_error(self._h) or b"").decode("utf-8", "replace"))
        self._check(rc)
        draws = None
        if return_draws:
            draws, at = [], 0
            for kj, size in zip(comps, sizes):
                draws.append(flat[at:at + size].reshape(n_folds, n_chains, kept, int(kj) + 1).copy())
                at += size
        return elpd, mean, draws

    # -- variates -----------------------------------------------------------------------
    def rng_fill(self, seed, n_normal=0, shape=1.0, n_gamma=0):
        z = np.empty(n_normal)
        g = np.empty(n_gamma)
        self._check(self._lib.bmc_rng_fill(self._h, int(seed), n_normal, _dptr(z), float(shape),
                                           n_gamma, _dptr(g)))
        return z, g

    def philox_raw(self, seed, stream_id, nblocks4):
        out = np.empty(4 * nblocks4, dtype=np.uint32)
        self._check(self._lib.bmc_philox_raw(self._h, int(seed), int(stream_id), nblocks4,
                                             out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out.reshape(nblocks4, 4)


def order_stat_plan(n, percentiles):
    """(index, weight) of numpy.percentile's default linear method for each percentile:
    virtual index (n - 1) * q in float64, as numpy does (reference sampling_utils.py:80-82
    calls np.percentile)."""
    idx, gam = [], []
    for p in percentiles:
        qq = np.true_divide(np.float64(p), 100)
        vi = (n - 1) * qq
        lo = np.floor(vi)
        g = vi - lo
        lo = int(lo)
        if lo >= n - 1:
            lo, g = n - 1, 0.0
        if lo < 0:
            lo, g = 0, 0.0
        idx.append(lo)
        gam.append(float(g))
    return np.array(idx, dtype=np.int32), np.array(gam, dtype=np.float64)


def coverage_plan(n, percentiles):
    """Index pairs of reference sampling_utils.py:30-31 (truncating int())."""
    lo = [int((0.5 - p / 200) * n) for p in percentiles]
    hi = [int((0.5 + p / 200) * n) - 1 for p in percentiles]
    hi = [h if h >= 0 else n + h for h in hi]   # python negative index
    return np.array(lo, dtype=np.int32), np.array(hi, dtype=np.int32)


_default_ctx = {}
_ctx_lock = threading.Lock()


def default_context(device=0):
    """A cached per-device context for the functional API (creation is thread-safe; use
    ``with ctx.lock:`` around a sequence of calls that belongs together)."""
    ctx = _default_ctx.get(device)
    if ctx is None:
        with _ctx_lock:
            ctx = _default_ctx.get(device)
            if ctx is None:
                ctx = _default_ctx[device] = Context(device)
    return ctx
