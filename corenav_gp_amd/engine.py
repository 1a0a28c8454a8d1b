"""ctypes binding of include/corenav_gp.h (libcorenav_gp.so).  This is the reference-side stub
INTEGRATION.md shows for gp_slip_node.py; there is no CPU fallback -- a missing library or a
missing GPU raises."""
from __future__ import annotations

import ctypes
import os

import numpy as np

KERNEL_SE_ISO, KERNEL_SE_ARD, KERNEL_RBF_BROWNIAN = 0, 1, 2
KERNEL_MATERN32_ARD, KERNEL_MATERN52_ARD = 3, 4   # theta layout of SE_ARD; fp64 contexts only (include/corenav_gp.h)
F64, F32 = 0, 1
MAX_D = 8
MAX_THETA = MAX_D + 2
PROF_KERNELS = 5
PROF_NAMES = ("update", "potf2", "trmm", "finalize", "alpha")


def ntheta(kernel_id, d):
    """Entries of theta for `kernel_id` at d input dimensions (the layouts of include/corenav_gp.h)."""
    if kernel_id == KERNEL_SE_ISO:
        return 3
    return 4 if kernel_id == KERNEL_RBF_BROWNIAN else d + 2


_HERE = os.path.dirname(os.path.abspath(__file__))
# CGP_LIB selects another build of the same ABI for measurements (the -DCGP_AB -DCGP_ABLATION library
# `make ab` writes next to the shipped one); there is still no CPU fallback.
LIB_PATH = os.environ.get("CGP_LIB") or os.path.join(_HERE, "libcorenav_gp.so")
DEBUG_SLOTS = 512
ABI_VERSION = 3   # include/corenav_gp.h CGP_ABI_VERSION: load() refuses a library of another revision
BUILD_ABLATION, BUILD_AB, BUILD_F32_NATIVE = 1, 2, 4
STREAM_CTX = ctypes.c_void_p(-1).value   # CGP_STREAM_CTX: the context's private stream
PLAN_TICKS, PLAN_PAIRS, PLAN_MULTI = 0, 1, 2   # CGP_PLAN_*: the kinds of launch cgp_debug_window_plan reports

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int)
_vp = ctypes.c_void_p
OBJECTIVE_FN = ctypes.CFUNCTYPE(ctypes.c_double, _dp, _dp, ctypes.c_int, ctypes.c_void_p)   # cgp_objective_fn

_SIGS = {
    "cgp_create": (_vp, [ctypes.c_int] * 6),
    "cgp_create_ex": (_vp, [ctypes.c_int] * 6 + [_ip]),
    "cgp_destroy": (None, [_vp]),
    "cgp_strerror": (ctypes.c_char_p, [ctypes.c_int]),
    "cgp_last_error": (ctypes.c_char_p, [_vp]),
    "cgp_abi_version": (ctypes.c_int, []),
    "cgp_build_flags": (ctypes.c_int, []),
    "cgp_synchronize": (ctypes.c_int, [_vp]),
    "cgp_sweep_create": (_vp, [_ip, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "cgp_sweep_destroy": (None, [_vp]),
    "cgp_sweep_ndev": (ctypes.c_int, [_vp]),
    "cgp_sweep_shard": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _ip, _ip]),
    "cgp_sweep_fit_predict": (ctypes.c_int, [_vp] + [ctypes.c_int] * 5 + [_dp, _dp, _dp, _dp, ctypes.c_int,
                                                                          ctypes.c_int, _dp, _dp, _dp, _ip, _dp]),
    "cgp_sweep_fit_predict_device": (ctypes.c_int, [_vp] + [ctypes.c_int] * 5 + [_vp] * 5 + [ctypes.c_int] + [_vp] * 5),
    "cgp_sweep_synchronize": (ctypes.c_int, [_vp]),
    "cgp_sweep_context": (_vp, [_vp, ctypes.c_int]),
    "cgp_fit": (ctypes.c_int, [_vp, _dp, _dp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _dp, _dp]),
    "cgp_predict": (ctypes.c_int, [_vp, _dp, ctypes.c_int, ctypes.c_int, _dp, _dp]),
    "cgp_get_alpha": (ctypes.c_int, [_vp, _dp]),
    "cgp_get_factor": (ctypes.c_int, [_vp, _dp]),
    "cgp_last_jitter": (ctypes.c_double, [_vp]),
    "cgp_nll_grad": (ctypes.c_int, [_vp, _dp, _dp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _dp, _dp, _dp]),
    "cgp_optimize": (ctypes.c_int, [_vp, _dp, _dp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _dp, ctypes.c_int, _dp, _ip]),
    "cgp_loo": (ctypes.c_int, [_vp, _dp, _dp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _dp, _dp, _dp, _dp, _dp]),
    "cgp_loo_batch": (ctypes.c_int, [_vp] + [ctypes.c_int] * 4 + [_dp, _dp, _dp, ctypes.c_int, _dp, _dp, _dp, _dp, _dp, _ip]),
    "cgp_loo_batch_device": (ctypes.c_int, [_vp] + [ctypes.c_int] * 4 + [_vp] * 11),
    "cgp_loo_grad_reserve": (ctypes.c_int, [_vp, ctypes.c_int]),
    "cgp_loo_nll_grad": (ctypes.c_int, [_vp, _dp, _dp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _dp, _dp, _dp]),
    "cgp_loo_nll_grad_batch": (ctypes.c_int, [_vp] + [ctypes.c_int] * 4 + [_dp, _dp, _dp, ctypes.c_int, _dp, _dp, ctypes.c_int,
                                                                           _dp, _ip]),
    "cgp_loo_nll_grad_batch_device": (ctypes.c_int, [_vp] + [ctypes.c_int] * 4 + [_vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_int,
                                                                                  _vp, _vp, _vp]),
    "cgp_optimize_loo_batch": (ctypes.c_int, [_vp] + [ctypes.c_int] * 4 + [_dp, _dp, _dp, ctypes.c_int, ctypes.c_int, _dp, _dp, _ip]),
    "cgp_slip_node_callback_opt": (ctypes.c_int, [_vp, _dp, _dp, ctypes.c_int, ctypes.c_int, _dp, ctypes.c_int, _dp, _dp,
                                                  ctypes.c_int, _ip]),
    "cgp_slip_node_callback": (ctypes.c_int, [_vp, _dp, _dp, ctypes.c_int, ctypes.c_int, _dp, _dp, _dp,
                                              ctypes.c_int, _ip]),
    "cgp_fit_predict_batch": (ctypes.c_int, [_vp] + [ctypes.c_int] * 5 + [_dp, _dp, _dp, _dp, ctypes.c_int,
                                                                          ctypes.c_int, _dp, _dp, _dp, _ip]),
    "cgp_fit_predict_batch_device": (ctypes.c_int, [_vp] + [ctypes.c_int] * 5 + [_vp, _vp, _vp, _vp, _vp,
                                                                                 ctypes.c_int, _vp, _vp, _vp, _vp, _vp]),
    "cgp_joint_reserve": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int]),
    "cgp_fit_predict_cov_batch": (ctypes.c_int, [_vp] + [ctypes.c_int] * 5 + [_dp, _dp, _dp, _dp, ctypes.c_int,
                                                                              ctypes.c_int, _dp, _dp, _dp, _ip]),
    "cgp_fit_predict_cov_batch_device": (ctypes.c_int, [_vp] + [ctypes.c_int] * 5 + [_vp, _vp, _vp, _vp, _vp,
                                                                                     ctypes.c_int, _vp, _vp, _vp, _vp, _vp]),
    "cgp_fit_sample_batch": (ctypes.c_int, [_vp] + [ctypes.c_int] * 5 + [_dp, _dp, _dp, _dp, ctypes.c_int, ctypes.c_int,
                                                                         ctypes.c_int, _dp, ctypes.c_double, _dp, _dp, _ip, _ip]),
    "cgp_fit_sample_batch_device": (ctypes.c_int, [_vp] + [ctypes.c_int] * 5 + [_vp, _vp, _vp, _vp, _vp, ctypes.c_int,
                                                                                ctypes.c_int, _vp, ctypes.c_double, _vp, _vp, _vp,
                                                                                _vp, _vp]),
    "cgp_pgrad_reserve": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int]),
    "cgp_fit_predict_grad_batch": (ctypes.c_int, [_vp] + [ctypes.c_int] * 5 + [_dp, _dp, _dp, _dp, ctypes.c_int,
                                                                               ctypes.c_int, _dp, _dp, _dp, _ip, _dp, _dp]),
    "cgp_fit_predict_grad_batch_device": (ctypes.c_int, [_vp] + [ctypes.c_int] * 5 + [_vp, _vp, _vp, _vp, _vp,
                                                                                      ctypes.c_int, _vp, _vp, _vp, _vp, _vp, _vp,
                                                                                      _vp]),
    "cgp_predict_gradients": (ctypes.c_int, [_vp, _dp, ctypes.c_int, _dp, _dp, _dp, _dp]),
    "cgp_multi_reserve": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int]),
    "cgp_multi_set_form": (ctypes.c_int, [_vp, ctypes.c_int]),
    "cgp_fit_predict_multi_batch": (ctypes.c_int, [_vp] + [ctypes.c_int] * 6 + [_dp, _dp, _dp, _dp, ctypes.c_int,
                                                                                ctypes.c_int, _dp, _dp, _dp, _ip]),
    "cgp_fit_predict_multi_batch_device": (ctypes.c_int, [_vp] + [ctypes.c_int] * 6 + [_vp, _vp, _vp, _vp, _vp,
                                                                                       ctypes.c_int, _vp, _vp, _vp, _vp, _vp]),
    "cgp_trend_reserve": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "cgp_sparse_chunk": (ctypes.c_int, []),
    "cgp_sparse_reserve": (ctypes.c_int, [_vp] + [ctypes.c_int] * 4),
    "cgp_fit_predict_sparse_batch": (ctypes.c_int, [_vp] + [ctypes.c_int] * 6 + [_dp] * 5 + [ctypes.c_int, ctypes.c_int,
                                                                                             _dp, _dp, _dp, _ip]),
    "cgp_fit_predict_sparse_batch_device": (ctypes.c_int, [_vp] + [ctypes.c_int] * 6 + [_vp] * 6 + [ctypes.c_int] + [_vp] * 5),
    "cgp_sparse_grad_reserve": (ctypes.c_int, [_vp, ctypes.c_int]),
    "cgp_sparse_nll_grad_batch": (ctypes.c_int, [_vp] + [ctypes.c_int] * 5 + [_dp] * 4 + [ctypes.c_int, _dp, _dp, ctypes.c_int,
                                                                              _dp, _ip]),
    "cgp_sparse_nll_grad_batch_device": (ctypes.c_int, [_vp] + [ctypes.c_int] * 5 + [_vp] * 7 + [ctypes.c_int, _vp, _vp, _vp]),
    "cgp_optimize_sparse_batch": (ctypes.c_int, [_vp] + [ctypes.c_int] * 5 + [_dp] * 4 + [ctypes.c_int] * 3 + [_dp, _ip]),
    "cgp_sparse_multi_reserve": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int]),
    "cgp_fit_predict_sparse_multi_batch": (ctypes.c_int, [_vp] + [ctypes.c_int] * 7 + [_dp] * 5 + [ctypes.c_int, ctypes.c_int,
                                                                                                   _dp, _dp, _dp, _ip]),
    "cgp_fit_predict_sparse_multi_batch_device": (ctypes.c_int, [_vp] + [ctypes.c_int] * 7 + [_vp] * 6 + [ctypes.c_int] + [_vp] * 5),
    "cgp_sparse_multi_grad_reserve": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int]),
    "cgp_sparse_multi_nll_grad_batch": (ctypes.c_int, [_vp] + [ctypes.c_int] * 6 + [_dp] * 4 + [ctypes.c_int, _dp, _dp, ctypes.c_int,
                                                                                    _dp, _dp, _ip]),
    "cgp_sparse_multi_nll_grad_batch_device": (ctypes.c_int, [_vp] + [ctypes.c_int] * 6 + [_vp] * 7 + [ctypes.c_int, _vp, _vp, _vp, _vp]),
    "cgp_optimize_sparse_multi_batch": (ctypes.c_int, [_vp] + [ctypes.c_int] * 6 + [_dp] * 4 + [ctypes.c_int] * 3 + [_dp, _ip]),
    "cgp_fit_predict_trend_batch": (ctypes.c_int, [_vp] + [ctypes.c_int] * 7 + [_dp] * 6 + [ctypes.c_int, ctypes.c_int,
                                                                                          _dp, _dp, _dp, _dp, _ip, _ip]),
    "cgp_fit_predict_trend_batch_device": (ctypes.c_int, [_vp] + [ctypes.c_int] * 7 + [_vp] * 7 + [ctypes.c_int] + [_vp] * 7),
    "cgp_multi_grad_reserve": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int]),
    "cgp_multi_nll_grad_batch": (ctypes.c_int, [_vp] + [ctypes.c_int] * 5 + [_dp, _dp, _dp, ctypes.c_int, _dp, _dp, ctypes.c_int,
                                                                             _dp, _ip]),
    "cgp_multi_nll_grad_batch_device": (ctypes.c_int, [_vp] + [ctypes.c_int] * 5 + [_vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_int,
                                                                                    _vp, _vp, _vp]),
    "cgp_optimize_multi_batch": (ctypes.c_int, [_vp] + [ctypes.c_int] * 5 + [_dp, _dp, _dp, ctypes.c_int, ctypes.c_int, _dp, _ip]),
    "cgp_predict_cov": (ctypes.c_int, [_vp, _dp, ctypes.c_int, ctypes.c_int, _dp, _dp]),
    "cgp_sample": (ctypes.c_int, [_vp, _dp, ctypes.c_int, ctypes.c_int, _dp, ctypes.c_int, ctypes.c_double, _dp, _ip]),
    "cgp_window_init": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _dp, ctypes.c_int]),
    "cgp_window_push": (ctypes.c_int, [_vp, ctypes.c_int, _dp, _dp, ctypes.c_int, _dp, _dp, _dp]),
    "cgp_window_push_device": (ctypes.c_int, [_vp, ctypes.c_int, _vp, _vp, ctypes.c_int, _vp, _vp, _vp, _vp]),
    "cgp_window_state": (ctypes.c_int, [_vp, ctypes.c_int, _ip, _ip]),
    "cgp_window_predict": (ctypes.c_int, [_vp, ctypes.c_int, _dp, ctypes.c_int, _dp, _dp]),
    "cgp_window_predict_device": (ctypes.c_int, [_vp, ctypes.c_int, _vp, ctypes.c_int, _vp, _vp, _vp]),
    "cgp_window_predict_gradients": (ctypes.c_int, [_vp, ctypes.c_int, _dp, ctypes.c_int, _dp, _dp, _dp, _dp]),
    "cgp_window_predict_gradients_device": (ctypes.c_int, [_vp, ctypes.c_int, _vp, ctypes.c_int, _vp, _vp, _vp, _vp, _vp]),
    "cgp_window_multi_reserve": (ctypes.c_int, [_vp, ctypes.c_int]),
    "cgp_window_push_multi": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _dp, _dp, ctypes.c_int, _dp, _dp, _dp]),
    "cgp_window_push_multi_device": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _vp, _vp, ctypes.c_int, _vp, _vp, _vp, _vp]),
    "cgp_window_predict_multi": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _dp, ctypes.c_int, _dp, _dp, _dp]),
    "cgp_window_predict_multi_device": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _vp, ctypes.c_int, _vp, _vp, _vp, _vp]),
    "cgp_window_joint_reserve": (ctypes.c_int, [_vp, ctypes.c_int]),
    "cgp_window_predict_cov": (ctypes.c_int, [_vp, ctypes.c_int, _dp, ctypes.c_int, _dp, _dp]),
    "cgp_window_predict_cov_device": (ctypes.c_int, [_vp, ctypes.c_int, _vp, ctypes.c_int, _vp, _vp, _vp]),
    "cgp_window_sample": (ctypes.c_int, [_vp, ctypes.c_int, _dp, ctypes.c_int, _dp, ctypes.c_int, ctypes.c_double, _dp, _ip]),
    "cgp_window_sample_device": (ctypes.c_int, [_vp, ctypes.c_int, _vp, ctypes.c_int, _vp, ctypes.c_int, ctypes.c_double, _vp, _vp,
                                                _vp]),
    "cgp_window_set_theta": (ctypes.c_int, [_vp, _dp, ctypes.c_int, _vp, _dp, _ip]),
    "cgp_window_set_theta_device": (ctypes.c_int, [_vp, _vp, ctypes.c_int, _vp, _vp, _vp, _vp]),
    "cgp_window_nll_grad": (ctypes.c_int, [_vp, _dp, _dp, ctypes.c_int]),
    "cgp_window_nll_grad_device": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _vp]),
    "cgp_window_loo": (ctypes.c_int, [_vp, _dp, _dp, _dp, _dp]),
    "cgp_window_loo_device": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "cgp_window_optimize": (ctypes.c_int, [_vp, ctypes.c_int, _vp, _dp, ctypes.c_int, _dp, _ip]),
    "cgp_window_trend_reserve": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int]),
    "cgp_window_predict_trend": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _dp, _dp, ctypes.c_int,
                                                _dp, _dp, _dp, _dp, _ip]),
    "cgp_window_predict_trend_device": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, ctypes.c_int]
                                        + [_vp] * 6),
    "cgp_window_multi_grad_reserve": (ctypes.c_int, [_vp]),
    "cgp_window_multi_nll_grad": (ctypes.c_int, [_vp, ctypes.c_int, _dp, _dp, ctypes.c_int, _dp]),
    "cgp_window_multi_nll_grad_device": (ctypes.c_int, [_vp, ctypes.c_int, _vp, _vp, ctypes.c_int, _vp, _vp]),
    "cgp_window_optimize_multi": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _vp, _dp, ctypes.c_int, _dp, _ip]),
    "cgp_window_loo_grad_reserve": (ctypes.c_int, [_vp]),
    "cgp_window_loo_nll_grad": (ctypes.c_int, [_vp, _dp, _dp, ctypes.c_int, _dp]),
    "cgp_window_loo_nll_grad_device": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _vp, _vp]),
    "cgp_window_optimize_loo": (ctypes.c_int, [_vp, ctypes.c_int, _vp, _dp, ctypes.c_int, _dp, _ip]),
    "cgp_set_streams": (ctypes.c_int, [_vp, ctypes.c_int]),
    "cgp_set_refine": (ctypes.c_int, [_vp, ctypes.c_int]),
    "cgp_debug_read": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_longlong)]),
    "cgp_debug_buffers": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_ulonglong)]),
    "cgp_debug_small": (ctypes.c_int, [_vp, _dp]),
    "cgp_debug_window_plan": (ctypes.c_int, [_vp, ctypes.c_int, _ip, ctypes.c_int]),
    "cgp_profile_enable": (ctypes.c_int, [_vp, ctypes.c_int]),
    "cgp_profile_read": (ctypes.c_int, [_vp, _dp, _dp, ctypes.POINTER(ctypes.c_longlong)]),
    "cgp_llh_to_enu": (ctypes.c_int, [ctypes.c_double] * 3 + [_dp, _dp, _dp]),
    "cgp_predict_stop": (ctypes.c_int, [_dp, _dp, ctypes.c_int, _dp, _dp, _dp, _dp, _dp, ctypes.c_double,
                                        ctypes.c_double, ctypes.c_double, ctypes.c_int, _dp, _dp, _ip, _dp, _ip, _dp]),
    "cgp_predict_stop_batch": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int] + [_dp] * 9 + [ctypes.c_double, ctypes.c_int,
                                                                                            _dp, _dp, _ip, _dp, _ip, _dp]),
    "cgp_optimize_batch": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _dp, _dp, _dp,
                                          ctypes.c_int, ctypes.c_int, _dp, _ip]),
    "cgp_selftest_lbfgs": (ctypes.c_int, [_dp, ctypes.c_int, ctypes.c_int, _dp]),
    "cgp_lbfgs_minimize": (ctypes.c_int, [_vp, _vp, _dp, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double,
                                          _dp, _ip, _ip, _ip]),
    "cgp_recorder_create": (_vp, []),
    "cgp_recorder_destroy": (None, [_vp]),
    "cgp_recorder_update": (ctypes.c_int, [_vp, _dp, ctypes.c_double, ctypes.c_double, _dp, _dp, _dp, ctypes.c_int, _ip]),
    "cgp_recorder_stop_cmd": (None, [_vp, ctypes.c_double]),
    "cgp_recorder_cmd": (None, [_vp, ctypes.c_double]),
    "cgp_recorder_state": (None, [_vp, _dp]),
    "cgp_gppredictor_callback": (ctypes.c_int, [_dp, _dp, ctypes.c_int, _dp, _dp, _dp, _dp, _dp, ctypes.c_double,
                                                ctypes.c_double, ctypes.c_int, _ip, _dp]),
}
EXPORTS = tuple(_SIGS)

_lib = None


def load():
    """Loads libcorenav_gp.so and binds every symbol of include/corenav_gp.h (raises if missing).
    Load order in a process that also uses torch.cuda: `import torch` FIRST -- torch bundles its own libamdhip64,
    and if this library has already pulled in /opt/rocm's copy, torch.cuda later reports "No HIP GPUs"."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        if lib.cgp_abi_version() != ABI_VERSION:
            raise ImportError(f"{LIB_PATH} has ABI revision {lib.cgp_abi_version()}, this binding is for {ABI_VERSION}: rebuild it")
        _lib = lib
    return _lib


def lbfgs_minimize(fg, x0, max_evals=1000, pgtol=1e-5, factr=1e7):
    """cgp_lbfgs_minimize (host only): the engine's optimiser state machine on a Python objective fg(x) -> (f, grad).
    Returns (x, f, n_evals, n_iters, status)."""
    x = _d(x0).copy()
    n = len(x)

    def cb(xp, gp, nn, _user):
        f, g = fg(np.array([xp[i] for i in range(nn)]))
        for i in range(nn):
            gp[i] = g[i]
        return float(f)

    fn = OBJECTIVE_FN(cb)
    f = ctypes.c_double()
    nev, nit, st = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    rc = load().cgp_lbfgs_minimize(ctypes.cast(fn, _vp), None, _p(x), n, max_evals, pgtol, factr, ctypes.byref(f),
                                   ctypes.byref(nev), ctypes.byref(nit), ctypes.byref(st))
    if rc != 0:
        raise CgpError(rc)
    return x, f.value, nev.value, nit.value, st.value


class CgpError(RuntimeError):
    def __init__(self, code, detail=""):
        self.code = code
        msg = load().cgp_strerror(code).decode()
        super().__init__(f"cgp error {code}: {msg}" + (f" [{detail}]" if detail else ""))


def _d(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a):
    return a.ctypes.data_as(_dp)


class Context:
    """One engine context (= one GPU, one stream).  Not thread-safe."""

    def __init__(self, device=0, max_n=2048, max_m=640, max_d=MAX_D, max_batch=1, dtype=F64):
        self.lib = load()
        self.dtype = dtype
        st = ctypes.c_int(0)
        self.h = self.lib.cgp_create_ex(device, max_n, max_m, max_d, max_batch, dtype, ctypes.byref(st))
        if not self.h:
            raise RuntimeError(f"cgp_create failed ({st.value}: {self.lib.cgp_strerror(st.value).decode()}): no usable gfx950 "
                               "device, an argument out of range, or out of device memory (the engine has no CPU fallback)")

    def close(self):
        if getattr(self, "h", None):
            self.lib.cgp_destroy(self.h)
            self.h = None

    __del__ = close

    def _chk(self, rc):
        if rc < 0:
            raise CgpError(rc, self.lib.cgp_last_error(self.h).decode())
        return rc

    # -- single window -------------------------------------------------------------------------
    def fit(self, X, y, kernel_id, theta):
        X = _d(X)
        if X.ndim == 1:
            X = X[:, None]
        y, theta = _d(y).reshape(-1), _d(theta)
        logml = ctypes.c_double(0.0)
        rc = self._chk(self.lib.cgp_fit(self.h, _p(X), _p(y), X.shape[0], X.shape[1], kernel_id, _p(theta),
                                        ctypes.byref(logml)))
        self._n = X.shape[0]
        return rc, logml.value

    def predict(self, Xs, include_noise=True):
        Xs = _d(Xs)
        if Xs.ndim == 1:
            Xs = Xs[:, None]
        M = Xs.shape[0]
        mean, var = np.empty(M), np.empty(M)
        self._chk(self.lib.cgp_predict(self.h, _p(Xs), M, int(include_noise), _p(mean), _p(var)))
        return mean, var

    def alpha(self):
        a = np.empty(self._n)
        self._chk(self.lib.cgp_get_alpha(self.h, _p(a)))
        return a

    def factor(self):
        L = np.empty((self._n, self._n))
        self._chk(self.lib.cgp_get_factor(self.h, _p(L)))
        return L

    def last_jitter(self):
        return self.lib.cgp_last_jitter(self.h)

    def nll_grad(self, X, y, kernel_id, theta):
        """Negative log marginal likelihood and its gradient wrt the natural parameters."""
        X = _d(X)
        if X.ndim == 1:
            X = X[:, None]
        y, theta = _d(y).reshape(-1), _d(theta)
        nll, grad = ctypes.c_double(0.0), np.empty(len(theta))
        rc = self._chk(self.lib.cgp_nll_grad(self.h, _p(X), _p(y), X.shape[0], X.shape[1], kernel_id, _p(theta),
                                             ctypes.byref(nll), _p(grad)))
        if rc > 0:
            raise CgpError(rc)
        self._n = X.shape[0]
        return nll.value, grad

    def loo(self, X, y, kernel_id, theta):
        """Leave-one-out cross-validation of one window in closed form (fp64 contexts): (loo_mean, loo_var, loo_lpd), each
        (N,), and lpd_sum.  Leaves the context fitted at theta, like nll_grad."""
        X = _d(X)
        if X.ndim == 1:
            X = X[:, None]
        y, theta = _d(y).reshape(-1), _d(theta)
        N = X.shape[0]
        mean, var, lpd, tot = np.empty(N), np.empty(N), np.empty(N), ctypes.c_double(0.0)
        rc = self._chk(self.lib.cgp_loo(self.h, _p(X), _p(y), N, X.shape[1], kernel_id, _p(theta), _p(mean), _p(var), _p(lpd),
                                        ctypes.byref(tot)))
        if rc > 0:
            raise CgpError(rc)
        self._n = N
        return mean, var, lpd, tot.value

    def loo_batch(self, X, y, theta, kernel_id):
        """Batched LOO: X (B, N, d), y (B, N), theta (B, nth) -> (rc, loo_mean, loo_var, loo_lpd (B, N), lpd_sum, logml, info
        (B,)); a fit that stays not positive definite through the jitter ladder has NaN rows and a non-zero info."""
        X, y, theta = _d(X), _d(y), _d(theta)
        B, N, d = X.shape
        mean, var, lpd = np.empty((B, N)), np.empty((B, N)), np.empty((B, N))
        tot, logml, info = np.empty(B), np.empty(B), np.zeros(B, dtype=np.int32)
        rc = self._chk(self.lib.cgp_loo_batch(self.h, B, N, d, kernel_id, _p(X), _p(y), _p(theta), theta.shape[1], _p(mean),
                                              _p(var), _p(lpd), _p(tot), _p(logml), info.ctypes.data_as(_ip)))
        return rc, mean, var, lpd, tot, logml, info

    def loo_batch_device(self, B, N, d, kernel_id, dX, dy, dtheta, djitter, dloo_mean, dloo_var, dloo_lpd, dlpd_sum, dlogml,
                         dinfo, stream=0):
        """Device pointers (ints, fit_predict_batch_device's layout, fp64) on a caller stream; 0 for an output not wanted."""
        return self._chk(self.lib.cgp_loo_batch_device(self.h, B, N, d, kernel_id, dX, dy, dtheta, djitter or None,
                                                       dloo_mean or None, dloo_var or None, dloo_lpd or None, dlpd_sum or None,
                                                       dlogml, dinfo, ctypes.c_void_p(stream)))

    # -- the leave-one-out objective nlpd = -lpd_sum: gradient and optimiser (fp64 contexts) -------------------
    def loo_grad_reserve(self, max_batch):
        """Scratch for the four calls below: max_batch x (max_n rounded up to 128)^2 doubles."""
        return self._chk(self.lib.cgp_loo_grad_reserve(self.h, int(max_batch)))

    def loo_nll_grad(self, X, y, kernel_id, theta):
        """(nlpd, grad) of one window: nlpd = -lpd_sum of loo() and its gradient with respect to theta.  Leaves the context
        fitted at theta, like loo()."""
        X = _d(X)
        if X.ndim == 1:
            X = X[:, None]
        y, theta = _d(y).reshape(-1), _d(theta)
        nlpd, grad = ctypes.c_double(0.0), np.empty(len(theta))
        rc = self._chk(self.lib.cgp_loo_nll_grad(self.h, _p(X), _p(y), X.shape[0], X.shape[1], kernel_id, _p(theta),
                                                 ctypes.byref(nlpd), _p(grad)))
        if rc > 0:
            raise CgpError(rc)
        self._n = X.shape[0]
        return nlpd.value, grad

    def loo_nll_grad_batch(self, X, y, theta, kernel_id, want_logml=True):
        """X (B, N, d), y (B, N), theta (B, nth) -> (rc, nlpd (B,), grad (B, nth), logml (B,) or None, info (B,))."""
        X, y, theta = _d(X), _d(y), _d(theta)
        B, N, d = X.shape
        nth = theta.shape[1]
        nlpd, grad = np.empty(B), np.empty((B, nth))
        logml, info = (np.empty(B) if want_logml else None), np.zeros(B, dtype=np.int32)
        rc = self._chk(self.lib.cgp_loo_nll_grad_batch(self.h, B, N, d, kernel_id, _p(X), _p(y), _p(theta), nth, _p(nlpd),
                                                       _p(grad), nth, _p(logml) if want_logml else None,
                                                       info.ctypes.data_as(_ip)))
        return rc, nlpd, grad, logml, info

    def loo_nll_grad_batch_device(self, B, N, d, kernel_id, dX, dy, dtheta, djitter, dnlpd, dgrad, grad_stride, dlogml, dinfo,
                                  stream=0):
        """Device pointers as loo_batch_device; dnlpd (B,), dgrad (B, grad_stride), dlogml (B,) or 0."""
        return self._chk(self.lib.cgp_loo_nll_grad_batch_device(self.h, B, N, d, kernel_id, dX, dy, dtheta, djitter or None,
                                                                dnlpd, dgrad, int(grad_stride), dlogml or None, dinfo,
                                                                ctypes.c_void_p(stream)))

    def optimize_loo_batch(self, X, y, kernel_id, theta0, max_evals=1000):
        """theta chosen by the leave-one-out pseudo-likelihood: X (B, N, d), y (B, N), theta0 (B, nth) or (nth,) ->
        (theta_opt (B, nth), lpd_sum (B,), logml (B,), n_evals (B,)), both objectives at theta_opt."""
        X, y = _d(X), _d(y)
        B, N, d = X.shape
        theta = np.array(theta0, dtype=np.float64)
        if theta.ndim == 1:
            theta = np.tile(theta, (B, 1))
        theta = np.ascontiguousarray(theta)
        lpd, logml, nev = np.empty(B), np.empty(B), np.zeros(B, dtype=np.int32)
        rc = self._chk(self.lib.cgp_optimize_loo_batch(self.h, B, N, d, kernel_id, _p(X), _p(y), _p(theta), theta.shape[1],
                                                       max_evals, _p(lpd), _p(logml), nev.ctypes.data_as(_ip)))
        if rc > 0:
            raise CgpError(rc)
        return theta, lpd, logml, nev

    def optimize(self, X, y, kernel_id, theta0, max_evals=1000):
        """GPy m.optimize() equivalent; returns (theta_opt, logml, n_evals)."""
        X = _d(X)
        if X.ndim == 1:
            X = X[:, None]
        y = _d(y).reshape(-1)
        theta = np.array(theta0, dtype=np.float64)
        logml, nev = ctypes.c_double(0.0), ctypes.c_int(0)
        rc = self._chk(self.lib.cgp_optimize(self.h, _p(X), _p(y), X.shape[0], X.shape[1], kernel_id, _p(theta),
                                             max_evals, ctypes.byref(logml), ctypes.byref(nev)))
        if rc > 0:
            raise CgpError(rc)
        self._n = X.shape[0]
        return theta, logml.value, nev.value

    def optimize_batch(self, X, y, kernel_id, theta0, max_evals=1000):
        """Batched m.optimize(): X (B, N, d), y (B, N), theta0 (B, nth) -> (theta_opt, logml, n_evals)."""
        X, y = _d(X), _d(y)
        B, N, d = X.shape
        theta = np.array(theta0, dtype=np.float64)
        if theta.ndim == 1:
            theta = np.tile(theta, (B, 1))
        theta = np.ascontiguousarray(theta)
        logml, nev = np.empty(B), np.zeros(B, dtype=np.int32)
        rc = self._chk(self.lib.cgp_optimize_batch(self.h, B, N, d, kernel_id, _p(X), _p(y), _p(theta), theta.shape[1],
                                                   max_evals, _p(logml), nev.ctypes.data_as(_ip)))
        if rc > 0:
            raise CgpError(rc)
        return theta, logml, nev

    def slip_node_callback_opt(self, time_array, slip_array, theta0, kernel_id=KERNEL_RBF_BROWNIAN, max_evals=1000,
                               cap=4096):
        t, s = _d(time_array).reshape(-1), _d(slip_array).reshape(-1)
        theta = np.array(theta0, dtype=np.float64)
        mean, sigma = np.empty(cap), np.empty(cap)
        m_out = ctypes.c_int(0)
        rc = self._chk(self.lib.cgp_slip_node_callback_opt(self.h, _p(t), _p(s), len(t), kernel_id, _p(theta), max_evals,
                                                           _p(mean), _p(sigma), cap, ctypes.byref(m_out)))
        if rc > 0:
            raise CgpError(rc)
        m = min(m_out.value, cap)
        return mean[:m].copy(), sigma[:m].copy(), theta

    def slip_node_callback(self, time_array, slip_array, theta, kernel_id=KERNEL_RBF_BROWNIAN, cap=4096):
        t, s, theta = _d(time_array).reshape(-1), _d(slip_array).reshape(-1), _d(theta)
        mean, sigma = np.empty(cap), np.empty(cap)
        m_out = ctypes.c_int(0)
        rc = self._chk(self.lib.cgp_slip_node_callback(self.h, _p(t), _p(s), len(t), kernel_id, _p(theta), _p(mean),
                                                       _p(sigma), cap, ctypes.byref(m_out)))
        if rc > 0:
            raise CgpError(rc)
        m = min(m_out.value, cap)
        return mean[:m].copy(), sigma[:m].copy()

    # -- batch, host buffers -------------------------------------------------------------------
    def fit_predict_batch(self, X, y, Xs, theta, kernel_id, include_noise=True):
        X, y, Xs, theta = _d(X), _d(y), _d(Xs), _d(theta)
        B, N, d = X.shape
        M = Xs.shape[1]
        mean, var = np.empty((B, M)), np.empty((B, M))
        logml, info = np.empty(B), np.zeros(B, dtype=np.int32)
        rc = self._chk(self.lib.cgp_fit_predict_batch(self.h, B, N, d, M, kernel_id, _p(X), _p(y), _p(Xs), _p(theta),
                                                      theta.shape[1], int(include_noise), _p(mean), _p(var),
                                                      _p(logml), info.ctypes.data_as(_ip)))
        return rc, mean, var, logml, info

    # -- batch, device pointers (ints) on a caller stream ------------------------------------------
    def fit_predict_batch_device(self, B, N, d, M, kernel_id, dX, dy, dXs, dtheta, djitter, include_noise, dmean,
                                 dvar, dlogml, dinfo, stream=0):
        """stream: a hipStream_t handle as an int.  0 is the legacy default stream itself (what
        torch.cuda.current_stream().cuda_stream returns for the default stream), so the work is ordered
        with the caller's default-stream kernels; engine.STREAM_CTX = the context's private stream."""
        return self._chk(self.lib.cgp_fit_predict_batch_device(self.h, B, N, d, M, kernel_id, dX, dy, dXs, dtheta,
                                                               djitter or None, int(include_noise), dmean, dvar,
                                                               dlogml, dinfo, ctypes.c_void_p(stream)))

    def synchronize(self):
        self._chk(self.lib.cgp_synchronize(self.h))

    # -- joint forecast after batch / single fits (fp64 contexts) ---------------------------------------
    def joint_reserve(self, max_batch, max_m):
        """Scratch for the joint calls below (posterior covariance / its factor of up to max_batch fits at up to max_m test
        points: max_batch x max_m^2 doubles, max_m rounded up to 16)."""
        return self._chk(self.lib.cgp_joint_reserve(self.h, int(max_batch), int(max_m)))

    def fit_predict_cov_batch(self, X, y, Xs, theta, kernel_id, include_noise=True):
        """fit_predict_batch with the full posterior covariance (B, M, M) in place of the variance; include_noise adds the
        noise variance to the diagonal only.  A fit whose info stays non-zero after the jitter ladder has NaN in its covariance."""
        X, y, Xs, theta = _d(X), _d(y), _d(Xs), _d(theta)
        B, N, d = X.shape
        M = Xs.shape[1]
        mean, cov = np.empty((B, M)), np.empty((B, M, M))
        logml, info = np.empty(B), np.zeros(B, dtype=np.int32)
        rc = self._chk(self.lib.cgp_fit_predict_cov_batch(self.h, B, N, d, M, kernel_id, _p(X), _p(y), _p(Xs), _p(theta),
                                                          theta.shape[1], int(include_noise), _p(mean), _p(cov),
                                                          _p(logml), info.ctypes.data_as(_ip)))
        return rc, mean, cov, logml, info

    def fit_predict_cov_batch_device(self, B, N, d, M, kernel_id, dX, dy, dXs, dtheta, djitter, include_noise, dmean,
                                     dcov, dlogml, dinfo, stream=0):
        """Device pointers as fit_predict_batch_device, dcov (B, M, M) in place of dvar."""
        return self._chk(self.lib.cgp_fit_predict_cov_batch_device(self.h, B, N, d, M, kernel_id, dX, dy, dXs, dtheta,
                                                                   djitter or None, int(include_noise), dmean, dcov,
                                                                   dlogml, dinfo, ctypes.c_void_p(stream)))

    # -- predictive gradients after batch / single fits (fp64 contexts) ----------------------------------
    def pgrad_reserve(self, max_batch, max_m):
        """Scratch for the predictive-gradient calls below (B^T = (Ky^-1 K*)^T and alpha of up to max_batch fits at up to max_m
        test points: max_batch x max_n x (max_m + 1) doubles, both rounded up to 128)."""
        return self._chk(self.lib.cgp_pgrad_reserve(self.h, int(max_batch), int(max_m)))

    def fit_predict_grad_batch(self, X, y, Xs, theta, kernel_id, include_noise=True):
        """fit_predict_batch plus d mean / d x* and d var / d x*, each (B, M, d): (code, mean, var, logml, info, dmean, dvar).
        A fit whose info stays non-zero after the jitter ladder has NaN in its gradients."""
        X, y, Xs, theta = _d(X), _d(y), _d(Xs), _d(theta)
        B, N, d = X.shape
        M = Xs.shape[1]
        mean, var = np.empty((B, M)), np.empty((B, M))
        dmean, dvar = np.empty((B, M, d)), np.empty((B, M, d))
        logml, info = np.empty(B), np.zeros(B, dtype=np.int32)
        rc = self._chk(self.lib.cgp_fit_predict_grad_batch(self.h, B, N, d, M, kernel_id, _p(X), _p(y), _p(Xs), _p(theta),
                                                           theta.shape[1], int(include_noise), _p(mean), _p(var),
                                                           _p(logml), info.ctypes.data_as(_ip), _p(dmean), _p(dvar)))
        return rc, mean, var, logml, info, dmean, dvar

    def fit_predict_grad_batch_device(self, B, N, d, M, kernel_id, dX, dy, dXs, dtheta, djitter, include_noise, dmean,
                                      dvar, dlogml, dinfo, ddmean, ddvar, stream=0):
        """Device pointers as fit_predict_batch_device, plus ddmean / ddvar (B, M, d); either may be 0, not both."""
        return self._chk(self.lib.cgp_fit_predict_grad_batch_device(self.h, B, N, d, M, kernel_id, dX, dy, dXs, dtheta,
                                                                    djitter or None, int(include_noise), dmean, dvar,
                                                                    dlogml, dinfo, ddmean or None, ddvar or None,
                                                                    ctypes.c_void_p(stream)))

    def predict_gradients(self, Xs):
        """After fit / optimize: m.predictive_gradients(Xs) with the marginals -> (mean (M,), var (M,) without the noise
        variance, dmean (M, d), dvar (M, d))."""
        Xs = _d(Xs)
        if Xs.ndim == 1:
            Xs = Xs[:, None]
        M, d = Xs.shape
        mean, var = np.empty(M), np.empty(M)
        dmean, dvar = np.empty((M, d)), np.empty((M, d))
        self._chk(self.lib.cgp_predict_gradients(self.h, _p(Xs), M, _p(mean), _p(var), _p(dmean), _p(dvar)))
        return mean, var, dmean, dvar

    def fit_sample_batch(self, X, y, Xs, theta, kernel_id, xi, include_noise=False, jitter_rel=1e-6):
        """Fits and sample paths of their joint posterior: xi (B, S, M) standard normals drawn by the caller -> (code, paths
        (B, S, M) = mean + C xi, logml, info, sinfo); C the Cholesky factor of the posterior covariance (+ noise) + jitter_rel x
        its mean diagonal.  A fit whose matrix is not positive definite gets NaN paths and its 1-based pivot in sinfo; code is
        the 1-based index of the first such fit."""
        X, y, Xs, theta = _d(X), _d(y), _d(Xs), _d(theta)
        B, N, d = X.shape
        M = Xs.shape[1]
        xi = _d(xi).reshape(B, -1, M)
        S = xi.shape[1]
        out, logml = np.empty((B, S, M)), np.empty(B)
        info, sinfo = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
        rc = self._chk(self.lib.cgp_fit_sample_batch(self.h, B, N, d, M, kernel_id, _p(X), _p(y), _p(Xs), _p(theta),
                                                     theta.shape[1], int(include_noise), S, _p(xi), float(jitter_rel), _p(out),
                                                     _p(logml), info.ctypes.data_as(_ip), sinfo.ctypes.data_as(_ip)))
        return rc, out, logml, info, sinfo

    def fit_sample_batch_device(self, B, N, d, M, kernel_id, dX, dy, dXs, dtheta, djitter, include_noise, S, dxi, jitter_rel,
                                dout, dlogml, dinfo, dsinfo, stream=0):
        return self._chk(self.lib.cgp_fit_sample_batch_device(self.h, B, N, d, M, kernel_id, dX, dy, dXs, dtheta,
                                                              djitter or None, int(include_noise), S, dxi, float(jitter_rel),
                                                              dout, dlogml, dinfo, dsinfo or None, ctypes.c_void_p(stream)))

    # -- multi-target fits: P target columns share one factor (fp64 contexts) ------------------------------
    def multi_reserve(self, max_batch, max_p):
        """Scratch for the multi-target calls below (Z = L^-1 Y of up to max_batch fits x max_p targets)."""
        return self._chk(self.lib.cgp_multi_reserve(self.h, int(max_batch), int(max_p)))

    def multi_set_form(self, rows):
        """Debug: 64 / 128 forces the tile height of the multi-target solve, 0 gives the choice back to the engine."""
        return self._chk(self.lib.cgp_multi_set_form(self.h, int(rows)))

    def fit_predict_multi_batch(self, X, Y, Xs, theta, kernel_id, include_noise=True):
        """X (B, N, d), Y (B, P, N) -- P targets per fit sharing inputs and theta -- Xs (B, M, d), theta (B, nth) ->
        (rc, mean (B, P, M), var (B, M), logml (B, P), info (B,)).  One factorisation per fit; a fit whose info stays
        non-zero after the jitter ladder has NaN in all of its outputs."""
        X, Y, Xs, theta = _d(X), _d(Y), _d(Xs), _d(theta)
        B, N, d = X.shape
        P, M = Y.shape[1], Xs.shape[1]
        mean, var = np.empty((B, P, M)), np.empty((B, M))
        logml, info = np.empty((B, P)), np.zeros(B, dtype=np.int32)
        rc = self._chk(self.lib.cgp_fit_predict_multi_batch(self.h, B, N, d, M, P, kernel_id, _p(X), _p(Y), _p(Xs), _p(theta),
                                                            theta.shape[1], int(include_noise), _p(mean), _p(var),
                                                            _p(logml), info.ctypes.data_as(_ip)))
        return rc, mean, var, logml, info

    def fit_predict_multi_batch_device(self, B, N, d, M, P, kernel_id, dX, dY, dXs, dtheta, djitter, include_noise, dmean,
                                       dvar, dlogml, dinfo, stream=0):
        """Device pointers as fit_predict_batch_device; dY (B, P, N), dmean (B, P, M), dvar (B, M), dlogml (B, P)."""
        return self._chk(self.lib.cgp_fit_predict_multi_batch_device(self.h, B, N, d, M, P, kernel_id, dX, dY, dXs, dtheta,
                                                                     djitter or None, int(include_noise), dmean, dvar,
                                                                     dlogml, dinfo, ctypes.c_void_p(stream)))

    # -- explicit basis functions (a trend with a vague prior) after the multi-target fits (fp64 contexts) -----
    def trend_reserve(self, max_batch, max_p, max_m):
        """Scratch for the two calls below; needs a multi_reserve that covers (max_batch, max_p + 16)."""
        return self._chk(self.lib.cgp_trend_reserve(self.h, int(max_batch), int(max_p), int(max_m)))

    def fit_predict_trend_batch(self, X, Y, H, Xs, Hs, theta, kernel_id, include_noise=True):
        """X (B, N, d), Y (B, P, N), H (B, q, N) -- the basis at the samples --, Xs (B, M, d), Hs (B, q, M), theta (B, nth) ->
        (rc, mean (B, P, M), var (B, M), beta (B, P, q), logml (B, P), info (B,), tinfo (B,)).  A fit whose info stays
        non-zero, or whose q x q normal equations fail the rank rule (tinfo = the 1-based pivot), has NaN outputs."""
        X, Y, H, Xs, Hs, theta = _d(X), _d(Y), _d(H), _d(Xs), _d(Hs), _d(theta)
        B, N, d = X.shape
        P, M, q = Y.shape[1], Xs.shape[1], H.shape[1]
        assert Y.shape == (B, P, N) and H.shape == (B, q, N) and Hs.shape == (B, q, M)
        mean, var, beta = np.empty((B, P, M)), np.empty((B, M)), np.empty((B, P, q))
        logml, info, tinfo = np.empty((B, P)), np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
        rc = self._chk(self.lib.cgp_fit_predict_trend_batch(self.h, B, N, d, M, P, q, kernel_id, _p(X), _p(Y), _p(H), _p(Xs),
                                                            _p(Hs), _p(theta), theta.shape[1], int(include_noise), _p(mean),
                                                            _p(var), _p(beta), _p(logml), info.ctypes.data_as(_ip),
                                                            tinfo.ctypes.data_as(_ip)))
        return rc, mean, var, beta, logml, info, tinfo

    def fit_predict_trend_batch_device(self, B, N, d, M, P, q, kernel_id, dX, dY, dH, dXs, dHs, dtheta, djitter,
                                       include_noise, dmean, dvar, dbeta, dlogml, dinfo, dtinfo, stream=0):
        """Device pointers as fit_predict_multi_batch_device; dH (B, q, N), dHs (B, q, M), dbeta (B, P, q), dtinfo (B,) int32."""
        return self._chk(self.lib.cgp_fit_predict_trend_batch_device(self.h, B, N, d, M, P, q, kernel_id, dX, dY, dH, dXs, dHs,
                                                                     dtheta, djitter or None, int(include_noise), dmean, dvar,
                                                                     dbeta, dlogml, dinfo, dtinfo, ctypes.c_void_p(stream)))

    # -- sparse (inducing-point) fits: the collapsed variational bound and its forecast (fp64 contexts) -----------
    def sparse_reserve(self, max_batch, max_n, max_m_ind, max_m):
        """Scratch for the two calls below: up to max_batch fits of max_n samples -- NOT bounded by the context's max_n --
        max_m_ind <= 512 inducing inputs and max_m test points."""
        return self._chk(self.lib.cgp_sparse_reserve(self.h, int(max_batch), int(max_n), int(max_m_ind), int(max_m)))

    def fit_predict_sparse_batch(self, X, y, Z, Xs, theta, kernel_id, include_noise=True):
        """X (B, N, d), y (B, N), Z (B, m, d) -- every fit's own inducing inputs --, Xs (B, M, d) or None (M = 0: the bound
        only), theta (B, nth) -> (rc, mean (B, M), var (B, M), bound (B,), info (B,)).  info: 0, the failing pivot k of K_uu
        (after the jitter ladder) or m + k for a pivot of B; such a fit has NaN outputs."""
        X, y, Z, theta = _d(X), _d(y), _d(Z), _d(theta)
        B, N, d = X.shape
        m = Z.shape[1]
        assert y.shape == (B, N) and Z.shape == (B, m, d)
        M = 0 if Xs is None else np.shape(Xs)[1]
        Xs = _d(Xs) if M > 0 else None
        mean, var = np.empty((B, M)), np.empty((B, M))
        logml, info = np.empty(B), np.zeros(B, dtype=np.int32)
        rc = self._chk(self.lib.cgp_fit_predict_sparse_batch(self.h, B, N, d, M, m, kernel_id, _p(X), _p(y), _p(Z),
                                                             _p(Xs) if M > 0 else None, _p(theta), theta.shape[1],
                                                             int(include_noise), _p(mean) if M > 0 else None,
                                                             _p(var) if M > 0 else None, _p(logml), info.ctypes.data_as(_ip)))
        return rc, mean, var, logml, info

    def fit_predict_sparse_batch_device(self, B, N, d, M, m, kernel_id, dX, dy, dZ, dXs, dtheta, djitter, include_noise,
                                        dmean, dvar, dlogml, dinfo, stream=0):
        """Device pointers as fit_predict_batch_device (fp64, SoA): dX (B, d, N), dy (B, N), dZ (B, d, m), dXs (B, d, M),
        dtheta (B, MAX_THETA), djitter (B) or 0; dmean / dvar (B, M) -- may be 0 when M = 0 --, dlogml (B), dinfo (B) int32."""
        return self._chk(self.lib.cgp_fit_predict_sparse_batch_device(self.h, B, N, d, M, m, kernel_id, dX, dy, dZ, dXs or None,
                                                                      dtheta, djitter or None, int(include_noise), dmean or None,
                                                                      dvar or None, dlogml, dinfo, ctypes.c_void_p(stream)))

    # -- sparse fits: gradient of the bound in theta and Z, and optimiser (fp64 contexts) -----------------------------
    def sparse_grad_reserve(self, max_batch):
        """Scratch for the three calls below; needs a sparse_reserve that covers it and is sized by it."""
        return self._chk(self.lib.cgp_sparse_grad_reserve(self.h, int(max_batch)))

    def sparse_nll_grad_batch(self, X, y, Z, theta, kernel_id, want_grad_z=True):
        """X (B, N, d), y (B, N), Z (B, m, d), theta (B, nth) -> (rc, nll (B,), grad (B, nth), gradZ (B, m, d) or None, info (B,)):
        nll = -bound of each fit, its gradient in theta (natural parameters) and in the inducing inputs.  A fit whose info stays
        non-zero after the jitter ladder on K_uu has NaN outputs."""
        X, y, Z, theta = _d(X), _d(y), _d(Z), _d(theta)
        B, N, d = X.shape
        m, nth = Z.shape[1], theta.shape[1]
        assert y.shape == (B, N) and Z.shape == (B, m, d)
        nll, grad = np.empty(B), np.empty((B, nth))
        gz, info = (np.empty((B, m, d)) if want_grad_z else None), np.zeros(B, dtype=np.int32)
        rc = self._chk(self.lib.cgp_sparse_nll_grad_batch(self.h, B, N, d, m, kernel_id, _p(X), _p(y), _p(Z), _p(theta), nth,
                                                          _p(nll), _p(grad), nth, _p(gz) if want_grad_z else None,
                                                          info.ctypes.data_as(_ip)))
        return rc, nll, grad, gz, info

    def sparse_nll_grad_batch_device(self, B, N, d, m, kernel_id, dX, dy, dZ, dtheta, djitter, dnll, dgrad, grad_stride, dgradZ,
                                     dinfo, stream=0):
        """Device pointers as fit_predict_sparse_batch_device; dnll (B,), dgrad (B, grad_stride), dgradZ (B, d, m) or 0."""
        return self._chk(self.lib.cgp_sparse_nll_grad_batch_device(self.h, B, N, d, m, kernel_id, dX, dy, dZ, dtheta,
                                                                   djitter or None, dnll, dgrad, int(grad_stride),
                                                                   dgradZ or None, dinfo, ctypes.c_void_p(stream)))

    def optimize_sparse_batch(self, X, y, Z0, theta0, kernel_id, optimize_z=True, max_evals=1000):
        """SparseGPRegression(...).optimize(): X (B, N, d), y (B, N), Z0 (B, m, d), theta0 (B, nth) or (nth,) ->
        (theta_opt (B, nth), Z_opt (B, m, d), bound (B,), n_evals (B,)); optimize_z=False keeps Z0."""
        X, y = _d(X), _d(y)
        B, N, d = X.shape
        Z = np.array(Z0, dtype=np.float64, order="C")
        m = Z.shape[1]
        theta = np.array(theta0, dtype=np.float64)
        if theta.ndim == 1:
            theta = np.tile(theta, (B, 1))
        theta = np.ascontiguousarray(theta)
        bound, nev = np.empty(B), np.zeros(B, dtype=np.int32)
        rc = self._chk(self.lib.cgp_optimize_sparse_batch(self.h, B, N, d, m, kernel_id, _p(X), _p(y), _p(Z), _p(theta),
                                                          theta.shape[1], int(bool(optimize_z)), int(max_evals), _p(bound),
                                                          nev.ctypes.data_as(_ip)))
        if rc > 0:
            raise CgpError(rc)
        return theta, Z, bound, nev

    # -- sparse fits: P target columns share one inducing-point fit (fp64 contexts) -----------------------------------
    def sparse_multi_reserve(self, max_batch, max_p):
        """What up to max_p <= 64 target columns add to the sparse scratch; needs a sparse_reserve that covers max_batch and is
        sized by it."""
        return self._chk(self.lib.cgp_sparse_multi_reserve(self.h, int(max_batch), int(max_p)))

    def fit_predict_sparse_multi_batch(self, X, Y, Z, Xs, theta, kernel_id, include_noise=True):
        """X (B, N, d), Y (B, P, N), Z (B, m, d), Xs (B, M, d) or None (M = 0: the bounds only), theta (B, nth) ->
        (rc, mean (B, P, M), var (B, M), bound (B, P), info (B,)): one Phi, one pair of factors and one variance per fit;
        bound[b, p] is what fit_predict_sparse_batch returns for y = Y[b, p].  A failed fit has NaN in all its outputs."""
        X, Y, Z, theta = _d(X), _d(Y), _d(Z), _d(theta)
        B, N, d = X.shape
        m, P = Z.shape[1], Y.shape[1]
        assert Y.shape == (B, P, N) and Z.shape == (B, m, d)
        M = 0 if Xs is None else np.shape(Xs)[1]
        Xs = _d(Xs) if M > 0 else None
        mean, var = np.empty((B, P, M)), np.empty((B, M))
        logml, info = np.empty((B, P)), np.zeros(B, dtype=np.int32)
        rc = self._chk(self.lib.cgp_fit_predict_sparse_multi_batch(self.h, B, N, d, M, P, m, kernel_id, _p(X), _p(Y), _p(Z),
                                                                   _p(Xs) if M > 0 else None, _p(theta), theta.shape[1],
                                                                   int(include_noise), _p(mean) if M > 0 else None,
                                                                   _p(var) if M > 0 else None, _p(logml), info.ctypes.data_as(_ip)))
        return rc, mean, var, logml, info

    def fit_predict_sparse_multi_batch_device(self, B, N, d, M, P, m, kernel_id, dX, dY, dZ, dXs, dtheta, djitter, include_noise,
                                              dmean, dvar, dlogml, dinfo, stream=0):
        """Device pointers as fit_predict_sparse_batch_device with dY (B, P, N), dmean (B, P, M), dvar (B, M), dlogml (B, P)."""
        return self._chk(self.lib.cgp_fit_predict_sparse_multi_batch_device(self.h, B, N, d, M, P, m, kernel_id, dX, dY, dZ,
                                                                            dXs or None, dtheta, djitter or None,
                                                                            int(include_noise), dmean or None, dvar or None,
                                                                            dlogml, dinfo, ctypes.c_void_p(stream)))

    # -- sparse fits: gradient and optimiser of the P columns' summed bound (fp64 contexts) --------------------------------
    def sparse_multi_grad_reserve(self, max_batch, max_p):
        """What up to max_p columns add to the gradient scratch; needs a sparse_reserve, a sparse_grad_reserve and a
        sparse_multi_reserve that cover it."""
        return self._chk(self.lib.cgp_sparse_multi_grad_reserve(self.h, int(max_batch), int(max_p)))

    def sparse_multi_nll_grad_batch(self, X, Y, Z, theta, kernel_id, want_grad_z=True, want_logml=True):
        """X (B, N, d), Y (B, P, N), Z (B, m, d), theta (B, nth) -> (rc, nll (B,), grad (B, nth), gradZ (B, m, d) or None, logml (B, P)
        or None, info (B,)): nll = -sum_p bound[p] of each fit (summed in column order), its gradient in theta (natural parameters)
        and in the inducing inputs, and the columns' bounds.  A fit whose info stays non-zero after the jitter ladder on K_uu has
        NaN outputs."""
        X, Y, Z, theta = _d(X), _d(Y), _d(Z), _d(theta)
        B, N, d = X.shape
        m, nth, P = Z.shape[1], theta.shape[1], Y.shape[1]
        assert Y.shape == (B, P, N) and Z.shape == (B, m, d)
        nll, grad = np.empty(B), np.empty((B, nth))
        gz, info = (np.empty((B, m, d)) if want_grad_z else None), np.zeros(B, dtype=np.int32)
        logml = np.empty((B, P)) if want_logml else None
        rc = self._chk(self.lib.cgp_sparse_multi_nll_grad_batch(self.h, B, N, d, P, m, kernel_id, _p(X), _p(Y), _p(Z), _p(theta), nth,
                                                                _p(nll), _p(grad), nth, _p(gz) if want_grad_z else None,
                                                                _p(logml) if want_logml else None, info.ctypes.data_as(_ip)))
        return rc, nll, grad, gz, logml, info

    def sparse_multi_nll_grad_batch_device(self, B, N, d, P, m, kernel_id, dX, dY, dZ, dtheta, djitter, dnll, dgrad, grad_stride,
                                           dgradZ, dlogml, dinfo, stream=0):
        """Device pointers as sparse_nll_grad_batch_device with dY (B, P, N); dgradZ (B, d, m) or 0, dlogml (B, P) or 0."""
        return self._chk(self.lib.cgp_sparse_multi_nll_grad_batch_device(self.h, B, N, d, P, m, kernel_id, dX, dY, dZ, dtheta,
                                                                         djitter or None, dnll, dgrad, int(grad_stride),
                                                                         dgradZ or None, dlogml or None, dinfo,
                                                                         ctypes.c_void_p(stream)))

    def optimize_sparse_multi_batch(self, X, Y, Z0, theta0, kernel_id, optimize_z=True, max_evals=1000):
        """SparseGPRegression(X, Y, Z=Z).optimize() with Y (N, P): X (B, N, d), Y (B, P, N), Z0 (B, m, d), theta0 (B, nth) or (nth,)
        -> (theta_opt (B, nth), Z_opt (B, m, d), bound_sum (B,), n_evals (B,)); optimize_z=False keeps Z0."""
        X, Y = _d(X), _d(Y)
        B, N, d = X.shape
        P = Y.shape[1]
        Z = np.array(Z0, dtype=np.float64, order="C")
        m = Z.shape[1]
        theta = np.array(theta0, dtype=np.float64)
        if theta.ndim == 1:
            theta = np.tile(theta, (B, 1))
        theta = np.ascontiguousarray(theta)
        bound, nev = np.empty(B), np.zeros(B, dtype=np.int32)
        rc = self._chk(self.lib.cgp_optimize_sparse_multi_batch(self.h, B, N, d, P, m, kernel_id, _p(X), _p(Y), _p(Z), _p(theta),
                                                                theta.shape[1], int(bool(optimize_z)), int(max_evals), _p(bound),
                                                                nev.ctypes.data_as(_ip)))
        if rc > 0:
            raise CgpError(rc)
        return theta, Z, bound, nev

    # -- multi-target fits: gradient and optimiser of the summed logML (fp64 contexts) ------------------------
    def multi_grad_reserve(self, max_batch, max_p):
        """Scratch for the three calls below (A = Ky^-1 Y); needs a multi_reserve that covers it."""
        return self._chk(self.lib.cgp_multi_grad_reserve(self.h, int(max_batch), int(max_p)))

    def multi_nll_grad_batch(self, X, Y, theta, kernel_id, want_logml=True):
        """X (B, N, d), Y (B, P, N), theta (B, nth) -> (rc, nll (B,), grad (B, nth), logml (B, P) or None, info (B,)):
        nll = -sum_p logml[p] of each fit and its gradient with respect to the shared theta, from ONE factorisation per fit."""
        X, Y, theta = _d(X), _d(Y), _d(theta)
        B, N, d = X.shape
        P, nth = Y.shape[1], theta.shape[1]
        nll, grad = np.empty(B), np.empty((B, nth))
        logml, info = (np.empty((B, P)) if want_logml else None), np.zeros(B, dtype=np.int32)
        rc = self._chk(self.lib.cgp_multi_nll_grad_batch(self.h, B, N, d, P, kernel_id, _p(X), _p(Y), _p(theta), nth, _p(nll),
                                                         _p(grad), nth, _p(logml) if want_logml else None,
                                                         info.ctypes.data_as(_ip)))
        return rc, nll, grad, logml, info

    def multi_nll_grad_batch_device(self, B, N, d, P, kernel_id, dX, dY, dtheta, djitter, dnll, dgrad, grad_stride, dlogml,
                                    dinfo, stream=0):
        """Device pointers as fit_predict_multi_batch_device; dnll (B,), dgrad (B, grad_stride), dlogml (B, P) or 0."""
        return self._chk(self.lib.cgp_multi_nll_grad_batch_device(self.h, B, N, d, P, kernel_id, dX, dY, dtheta, djitter or None,
                                                                  dnll, dgrad, int(grad_stride), dlogml or None, dinfo,
                                                                  ctypes.c_void_p(stream)))

    def optimize_multi_batch(self, X, Y, kernel_id, theta0, max_evals=1000):
        """m.optimize() of the multi-column model: X (B, N, d), Y (B, P, N), theta0 (B, nth) or (nth,) ->
        (theta_opt (B, nth), sum_p logml (B,), n_evals (B,))."""
        X, Y = _d(X), _d(Y)
        B, N, d = X.shape
        theta = np.array(theta0, dtype=np.float64)
        if theta.ndim == 1:
            theta = np.tile(theta, (B, 1))
        theta = np.ascontiguousarray(theta)
        logml, nev = np.empty(B), np.zeros(B, dtype=np.int32)
        rc = self._chk(self.lib.cgp_optimize_multi_batch(self.h, B, N, d, Y.shape[1], kernel_id, _p(X), _p(Y), _p(theta),
                                                         theta.shape[1], max_evals, _p(logml), nev.ctypes.data_as(_ip)))
        if rc > 0:
            raise CgpError(rc)
        return theta, logml, nev

    def predict_cov(self, Xs, include_noise=True):
        """After fit / optimize: mean (M,) and the full posterior covariance (M, M), m.predict(Xs, full_cov=True)."""
        Xs = _d(Xs)
        if Xs.ndim == 1:
            Xs = Xs[:, None]
        M = Xs.shape[0]
        mean, cov = np.empty(M), np.empty((M, M))
        self._chk(self.lib.cgp_predict_cov(self.h, _p(Xs), M, int(include_noise), _p(mean), _p(cov)))
        return mean, cov

    def sample(self, Xs, xi, include_noise=False, jitter_rel=1e-6):
        """After fit / optimize: sample paths (S, M) = mean + C xi, m.posterior_samples_f with the caller's normals xi (S, M);
        returns (paths, pivot): pivot != 0 (and NaN paths) when the matrix is not positive definite."""
        Xs = _d(Xs)
        if Xs.ndim == 1:
            Xs = Xs[:, None]
        M = Xs.shape[0]
        xi = _d(xi).reshape(-1, M)
        S = xi.shape[0]
        out, info = np.empty((S, M)), np.zeros(1, dtype=np.int32)
        self._chk(self.lib.cgp_sample(self.h, _p(Xs), M, S, _p(xi), int(include_noise), float(jitter_rel), _p(out),
                                      info.ctypes.data_as(_ip)))
        return out, int(info[0])

    # -- sliding windows (BASELINE configs[3]) ----------------------------------------------------
    def window_init(self, nwin, N, d, kernel_id, theta):
        theta = _d(theta)
        if theta.ndim == 1:
            theta = np.tile(theta, (nwin, 1))
        self._win = (nwin, d)
        self._win_nth = ntheta(kernel_id, d)
        self._win_n = N
        self._win_p = 0   # (a multi-target reservation goes with the windows it was made for)
        self._win_q = 0
        self._chk(self.lib.cgp_window_init(self.h, nwin, N, d, kernel_id, _p(theta), theta.shape[1]))

    def window_push(self, xs, ys, include_noise=True, check=True):
        """xs (nwin, T, d), ys (nwin, T) -> one-step-ahead mean, variance and logML per tick, each (nwin, T).  A window that
        lost positive definiteness, in this push or an earlier one, raises CgpError with the 1-based tick of the push it failed
        in (check=False: returns (mean, var, logml, code); the other windows' outputs are valid)."""
        nwin, d = self._win
        xs, ys = _d(xs).reshape(nwin, -1, d), _d(ys).reshape(nwin, -1)
        T = ys.shape[1]
        pm, pv, lm = np.empty((nwin, T)), np.empty((nwin, T)), np.empty((nwin, T))
        rc = self._chk(self.lib.cgp_window_push(self.h, T, _p(xs), _p(ys), int(include_noise), _p(pm), _p(pv), _p(lm)))
        if not check:
            return pm, pv, lm, rc
        if rc > 0:
            raise CgpError(rc)
        return pm, pv, lm

    def window_push_device(self, T, dxs, dys, include_noise, dpm, dpv, dlm, stream=0):
        return self._chk(self.lib.cgp_window_push_device(self.h, T, dxs, dys, int(include_noise), dpm, dpv, dlm,
                                                         ctypes.c_void_p(stream)))

    def window_predict(self, xs, include_noise=True, check=True):
        """Forecast from the windows as they stand: xs (nwin, M, d) (or (M, d) for one window) -> mean, variance, each
        (nwin, M).  A window that failed in an earlier push raises CgpError (check=False: returns (mean, var, code), that
        window's outputs NaN)."""
        nwin, d = self._win
        xs = _d(xs).reshape(nwin, -1, d)
        M = xs.shape[1]
        mean, var = np.empty((nwin, M)), np.empty((nwin, M))
        rc = self._chk(self.lib.cgp_window_predict(self.h, M, _p(xs), int(include_noise), _p(mean), _p(var)))
        if not check:
            return mean, var, rc
        if rc > 0:
            raise CgpError(rc)
        return mean, var

    def window_predict_device(self, M, dxs, include_noise, dmean, dvar, stream=0):
        return self._chk(self.lib.cgp_window_predict_device(self.h, M, dxs, int(include_noise), dmean, dvar,
                                                            ctypes.c_void_p(stream)))

    def window_predict_gradients(self, xs, include_noise=True, check=True, want=("dmean", "dvar"), moments=("mean", "var")):
        """m.predictive_gradients(Xnew) from the windows as they stand: xs (nwin, M, d) (or (M, d) for one window) ->
        (mean, var, dmean, dvar): mean / var (nwin, M) as window_predict returns them, dmean / dvar (nwin, M, d) the
        derivatives of the mean and of the unclipped latent variance with respect to the test inputs.  `want` names the
        gradients and `moments` the moments to compute (the others come back as None; at least one gradient).  A window that
        failed in an earlier push raises CgpError (check=False: returns (mean, var, dmean, dvar, code), that window's outputs
        NaN)."""
        nwin, d = self._win
        xs = _d(xs).reshape(nwin, -1, d)
        M = xs.shape[1]
        mean = np.empty((nwin, M)) if "mean" in moments else None
        var = np.empty((nwin, M)) if "var" in moments else None
        dmean = np.empty((nwin, M, d)) if "dmean" in want else None
        dvar = np.empty((nwin, M, d)) if "dvar" in want else None
        opt = lambda a: _p(a) if a is not None else None
        rc = self._chk(self.lib.cgp_window_predict_gradients(self.h, M, _p(xs), int(include_noise), opt(mean), opt(var),
                                                             opt(dmean), opt(dvar)))
        if not check:
            return mean, var, dmean, dvar, rc
        if rc > 0:
            raise CgpError(rc)
        return mean, var, dmean, dvar

    def window_predict_gradients_device(self, M, dxs, include_noise, dmean, dvar, ddmean, ddvar, stream=0):
        """Device pointers (ints; 0 / None = not wanted, for dmean / dvar -- the moments -- and for one of ddmean / ddvar)."""
        return self._chk(self.lib.cgp_window_predict_gradients_device(self.h, M, dxs, int(include_noise), dmean or None,
                                                                      dvar or None, ddmean or None, ddvar or None,
                                                                      ctypes.c_void_p(stream)))

    def window_multi_reserve(self, P):
        """Multi-target windows: target store and Z scratch for P target columns per tick (1 <= P <= 64); once after
        window_init, while the windows are empty.  From here on the windows are fed with window_push_multi."""
        rc = self._chk(self.lib.cgp_window_multi_reserve(self.h, int(P)))
        self._win_p = int(P)
        self._win_q = 0   # (a trend reservation goes with the multi-target one)
        return rc

    def window_push_multi(self, xs, Ys, include_noise=True, check=True):
        """xs (nwin, T, d), Ys (nwin, T, P) -> column 0's one-step-ahead mean, variance and logML per tick, each (nwin, T):
        bitwise window_push's for that column.  Failure reporting as window_push."""
        nwin, d = self._win
        P = self._win_p
        xs, Ys = _d(xs).reshape(nwin, -1, d), _d(Ys).reshape(nwin, -1, P)
        T = Ys.shape[1]
        pm, pv, lm = np.empty((nwin, T)), np.empty((nwin, T)), np.empty((nwin, T))
        rc = self._chk(self.lib.cgp_window_push_multi(self.h, T, P, _p(xs), _p(Ys), int(include_noise), _p(pm), _p(pv), _p(lm)))
        if not check:
            return pm, pv, lm, rc
        if rc > 0:
            raise CgpError(rc)
        return pm, pv, lm

    def window_push_multi_device(self, T, P, dxs, dYs, include_noise, dpm, dpv, dlm, stream=0):
        return self._chk(self.lib.cgp_window_push_multi_device(self.h, T, P, dxs, dYs, int(include_noise), dpm, dpv, dlm,
                                                               ctypes.c_void_p(stream)))

    def window_predict_multi(self, xs, include_noise=True, check=True, want_logml=True):
        """Forecast of all P target columns from the windows as they stand: xs (nwin, M, d) -> mean (nwin, P, M), var
        (nwin, M) (shared by the columns), logml (nwin, P) (None with want_logml=False).  A failed window raises CgpError
        (check=False: returns (mean, var, logml, code), that window's outputs NaN)."""
        nwin, d = self._win
        P = self._win_p
        xs = _d(xs).reshape(nwin, -1, d)
        M = xs.shape[1]
        mean, var = np.empty((nwin, P, M)), np.empty((nwin, M))
        logml = np.empty((nwin, P)) if want_logml else None
        rc = self._chk(self.lib.cgp_window_predict_multi(self.h, M, P, _p(xs), int(include_noise), _p(mean), _p(var),
                                                         _p(logml) if want_logml else None))
        if not check:
            return mean, var, logml, rc
        if rc > 0:
            raise CgpError(rc)
        return mean, var, logml

    def window_predict_multi_device(self, M, P, dxs, include_noise, dmean, dvar, dlogml, stream=0):
        """Device pointers (ints; dlogml 0 / None = not wanted)."""
        return self._chk(self.lib.cgp_window_predict_multi_device(self.h, M, P, dxs, int(include_noise), dmean, dvar,
                                                                  dlogml or None, ctypes.c_void_p(stream)))

    def window_trend_reserve(self, q, max_m):
        """Explicit basis functions on the multi-target windows: the last q of the P pushed columns are the basis at the
        samples (1 <= q < P, q <= 16); scratch for forecasts of up to max_m test points.  After window_multi_reserve."""
        rc = self._chk(self.lib.cgp_window_trend_reserve(self.h, int(q), int(max_m)))
        self._win_q = int(q)
        return rc

    def window_predict_trend(self, xs, Hs, include_noise=True, check=True):
        """xs (nwin, M, d), Hs (nwin, q, M) -> mean (nwin, P - q, M), var (nwin, M), beta (nwin, P - q, q), logml (nwin, P - q),
        tinfo (nwin,).  A failed window raises CgpError (check=False: the code is returned last); a window whose normal
        equations fail the rank rule has NaN outputs and its 1-based pivot in tinfo."""
        nwin, d = self._win
        P, q = self._win_p, self._win_q
        xs = _d(xs).reshape(nwin, -1, d)
        M = xs.shape[1]
        Hs = _d(Hs).reshape(nwin, q, M)
        mean, var = np.empty((nwin, P - q, M)), np.empty((nwin, M))
        beta, logml, tinfo = np.empty((nwin, P - q, q)), np.empty((nwin, P - q)), np.zeros(nwin, dtype=np.int32)
        rc = self._chk(self.lib.cgp_window_predict_trend(self.h, M, P, q, _p(xs), _p(Hs), int(include_noise), _p(mean), _p(var),
                                                         _p(beta), _p(logml), tinfo.ctypes.data_as(_ip)))
        if not check:
            return mean, var, beta, logml, tinfo, rc
        if rc > 0:
            raise CgpError(rc)
        return mean, var, beta, logml, tinfo

    def window_predict_trend_device(self, M, P, q, dxs, dHs, include_noise, dmean, dvar, dbeta, dlogml, dtinfo, stream=0):
        """Device pointers (ints), all required."""
        return self._chk(self.lib.cgp_window_predict_trend_device(self.h, M, P, q, dxs, dHs, int(include_noise), dmean, dvar,
                                                                  dbeta, dlogml, dtinfo, ctypes.c_void_p(stream)))

    def window_joint_reserve(self, max_m):
        """Scratch for joint forecasts (window_predict_cov / window_sample) of up to max_m test points per window; once
        after window_init."""
        return self._chk(self.lib.cgp_window_joint_reserve(self.h, int(max_m)))

    def window_predict_cov(self, xs, include_noise=True, check=True):
        """Joint forecast from the windows as they stand: xs (nwin, M, d) (or (M, d) for one window) -> mean (nwin, M) and the
        full posterior covariance (nwin, M, M); include_noise adds the noise variance to the diagonal only.  A window that
        failed in an earlier push raises CgpError (check=False: returns (mean, cov, code), that window's outputs NaN)."""
        nwin, d = self._win
        xs = _d(xs).reshape(nwin, -1, d)
        M = xs.shape[1]
        mean, cov = np.empty((nwin, M)), np.empty((nwin, M, M))
        rc = self._chk(self.lib.cgp_window_predict_cov(self.h, M, _p(xs), int(include_noise), _p(mean), _p(cov)))
        if not check:
            return mean, cov, rc
        if rc > 0:
            raise CgpError(rc)
        return mean, cov

    def window_predict_cov_device(self, M, dxs, include_noise, dmean, dcov, stream=0):
        return self._chk(self.lib.cgp_window_predict_cov_device(self.h, M, dxs, int(include_noise), dmean, dcov,
                                                                ctypes.c_void_p(stream)))

    def window_sample(self, xs, xi, include_noise=False, jitter_rel=1e-6, check=True):
        """Sample paths of the joint forecast: xs (nwin, M, d), xi (nwin, S, M) standard normals drawn by the caller ->
        paths (nwin, S, M) = mean + C xi and info (nwin,), C the Cholesky factor of the posterior covariance (+ noise) +
        jitter_rel x its mean diagonal.  A window whose matrix is not positive definite gets NaN paths and its 1-based pivot
        in info, and raises CgpError with the window's 1-based index (check=False: returns (paths, info, code))."""
        nwin, d = self._win
        xs = _d(xs).reshape(nwin, -1, d)
        M = xs.shape[1]
        xi = _d(xi).reshape(nwin, -1, M)
        S = xi.shape[1]
        out, info = np.empty((nwin, S, M)), np.zeros(nwin, dtype=np.int32)
        rc = self._chk(self.lib.cgp_window_sample(self.h, M, _p(xs), S, _p(xi), int(include_noise), float(jitter_rel), _p(out),
                                                  info.ctypes.data_as(_ip)))
        if not check:
            return out, info, rc
        if rc > 0:
            raise CgpError(rc)
        return out, info

    def window_sample_device(self, M, dxs, S, dxi, include_noise, jitter_rel, dout, dinfo, stream=0):
        return self._chk(self.lib.cgp_window_sample_device(self.h, M, dxs, S, dxi, int(include_noise), float(jitter_rel), dout,
                                                           dinfo, ctypes.c_void_p(stream)))

    def _select(self, select):
        if select is None:
            return None, None
        sel = np.ascontiguousarray(np.asarray(select).astype(bool).astype(np.uint8).reshape(self._win[0]))
        return sel, sel.ctypes.data_as(ctypes.c_void_p)

    def window_set_theta(self, theta, select=None, check=True):
        """Replaces theta of the selected windows (all when select is None) and rebuilds their factors from the resident
        samples: theta (nwin, nth) or (nth,) -> (logml, info), each (nwin,).  A window whose matrix is not positive definite
        under the new theta raises CgpError with that window's 1-based index (check=False: returns (logml, info, code))."""
        nwin, _ = self._win
        theta = _d(theta)
        if theta.ndim == 1:
            theta = np.ascontiguousarray(np.tile(theta, (nwin, 1)))
        sel, selp = self._select(select)
        logml, info = np.empty(nwin), np.zeros(nwin, dtype=np.int32)
        rc = self._chk(self.lib.cgp_window_set_theta(self.h, _p(theta), theta.shape[1], selp, _p(logml), info.ctypes.data_as(_ip)))
        if not check:
            return logml, info, rc
        if rc > 0:
            raise CgpError(rc)
        return logml, info

    def window_set_theta_device(self, dtheta, theta_stride, dselect, dlogml, dinfo, stream=0):
        return self._chk(self.lib.cgp_window_set_theta_device(self.h, dtheta, theta_stride, dselect, dlogml, dinfo,
                                                              ctypes.c_void_p(stream)))

    def window_nll_grad(self, nth=None):
        """Negative log marginal likelihood and its gradient wrt the natural parameters of every window at the theta it
        holds: (nll (nwin,), grad (nwin, nth))."""
        nwin, _ = self._win
        stride = self._win_nth if nth is None else nth
        nll, grad = np.empty(nwin), np.zeros((nwin, stride))
        self._chk(self.lib.cgp_window_nll_grad(self.h, _p(nll), _p(grad), stride))
        return nll, grad

    def window_nll_grad_device(self, dnll, dgrad, grad_stride, stream=0):
        return self._chk(self.lib.cgp_window_nll_grad_device(self.h, dnll, dgrad, grad_stride, ctypes.c_void_p(stream)))

    def window_loo(self):
        """Leave-one-out cross-validation of every window as it stands: (loo_mean, loo_var, loo_lpd (nwin, N), lpd_sum (nwin,)),
        rows in the window's own order (oldest sample first), NaN past the samples a window holds."""
        nwin, N = self._win[0], self._win_n
        mean, var, lpd, tot = np.empty((nwin, N)), np.empty((nwin, N)), np.empty((nwin, N)), np.empty(nwin)
        self._chk(self.lib.cgp_window_loo(self.h, _p(mean), _p(var), _p(lpd), _p(tot)))
        return mean, var, lpd, tot

    def window_loo_device(self, dloo_mean, dloo_var, dloo_lpd, dlpd_sum, stream=0):
        return self._chk(self.lib.cgp_window_loo_device(self.h, dloo_mean or None, dloo_var or None, dloo_lpd or None,
                                                        dlpd_sum or None, ctypes.c_void_p(stream)))

    def window_optimize(self, max_evals=1000, select=None, nth=None):
        """m.optimize() on the resident windows, started at the theta each holds: (theta (nwin, nth), logml, n_evals);
        rows of unselected windows are NaN / 0."""
        nwin, _ = self._win
        stride = self._win_nth if nth is None else nth
        sel, selp = self._select(select)
        theta, logml, nev = np.full((nwin, stride), np.nan), np.full(nwin, np.nan), np.zeros(nwin, dtype=np.int32)
        self._chk(self.lib.cgp_window_optimize(self.h, max_evals, selp, _p(theta), stride, _p(logml), nev.ctypes.data_as(_ip)))
        return theta, logml, nev

    def window_multi_grad_reserve(self):
        """Scratch for window_multi_nll_grad / window_optimize_multi; after window_multi_reserve, at any fill state."""
        return self._chk(self.lib.cgp_window_multi_grad_reserve(self.h))

    def window_multi_nll_grad(self, want_logml=True, nth=None):
        """Negative summed log marginal likelihood of the P target columns and its gradient wrt the natural parameters of
        every window at the theta it holds: (nll (nwin,), grad (nwin, nth), logml (nwin, P)) (logml None with
        want_logml=False); nll = -logml.sum(axis=1)."""
        nwin, _ = self._win
        P = self._win_p
        stride = self._win_nth if nth is None else nth
        nll, grad = np.empty(nwin), np.zeros((nwin, stride))
        logml = np.empty((nwin, P)) if want_logml else None
        self._chk(self.lib.cgp_window_multi_nll_grad(self.h, P, _p(nll), _p(grad), stride, _p(logml) if want_logml else None))
        return nll, grad, logml

    def window_multi_nll_grad_device(self, P, dnll, dgrad, grad_stride, dlogml, stream=0):
        """Device pointers (ints; dlogml 0 / None = not wanted)."""
        return self._chk(self.lib.cgp_window_multi_nll_grad_device(self.h, P, dnll, dgrad, grad_stride, dlogml or None,
                                                                   ctypes.c_void_p(stream)))

    def window_optimize_multi(self, max_evals=1000, select=None, nth=None):
        """m.optimize() with Y (n, P) on the resident windows: the P columns' summed logML maximised over one theta per
        window, started at the theta each holds: (theta (nwin, nth), logml_sum, n_evals); rows of unselected windows are
        NaN / 0."""
        nwin, _ = self._win
        stride = self._win_nth if nth is None else nth
        sel, selp = self._select(select)
        theta, logml, nev = np.full((nwin, stride), np.nan), np.full(nwin, np.nan), np.zeros(nwin, dtype=np.int32)
        self._chk(self.lib.cgp_window_optimize_multi(self.h, self._win_p, max_evals, selp, _p(theta), stride, _p(logml),
                                                     nev.ctypes.data_as(_ip)))
        return theta, logml, nev

    def window_loo_grad_reserve(self):
        """Scratch for window_loo_nll_grad / window_optimize_loo; after window_init, at any fill state."""
        return self._chk(self.lib.cgp_window_loo_grad_reserve(self.h))

    def window_loo_nll_grad(self, want_logml=True, nth=None):
        """Leave-one-out objective nlpd = -lpd_sum and its gradient wrt the natural parameters of every window at the theta
        it holds: (nlpd (nwin,), grad (nwin, nth), logml (nwin,)) (logml None with want_logml=False)."""
        nwin, _ = self._win
        stride = self._win_nth if nth is None else nth
        nlpd, grad = np.empty(nwin), np.zeros((nwin, stride))
        logml = np.empty(nwin) if want_logml else None
        self._chk(self.lib.cgp_window_loo_nll_grad(self.h, _p(nlpd), _p(grad), stride, _p(logml) if want_logml else None))
        return nlpd, grad, logml

    def window_loo_nll_grad_device(self, dnlpd, dgrad, grad_stride, dlogml, stream=0):
        """Device pointers (ints; dlogml 0 / None = not wanted)."""
        return self._chk(self.lib.cgp_window_loo_nll_grad_device(self.h, dnlpd, dgrad, grad_stride, dlogml or None,
                                                                 ctypes.c_void_p(stream)))

    def window_optimize_loo(self, max_evals=1000, select=None, nth=None):
        """L-BFGS on the leave-one-out objective of the resident windows, started at the theta each holds:
        (theta (nwin, nth), lpd_sum, n_evals); rows of unselected windows are NaN / 0."""
        nwin, _ = self._win
        stride = self._win_nth if nth is None else nth
        sel, selp = self._select(select)
        theta, lpd, nev = np.full((nwin, stride), np.nan), np.full(nwin, np.nan), np.zeros(nwin, dtype=np.int32)
        self._chk(self.lib.cgp_window_optimize_loo(self.h, max_evals, selp, _p(theta), stride, _p(lpd), nev.ctypes.data_as(_ip)))
        return theta, lpd, nev

    def window_state(self, w=0):
        n, info = ctypes.c_int(0), ctypes.c_int(0)
        self._chk(self.lib.cgp_window_state(self.h, w, ctypes.byref(n), ctypes.byref(info)))
        return n.value, info.value

    def predict_stop_batch(self, mean, sigma, P, Q, STM, Hvec, pos, arrival, now, threshold=3.0, h_bug_compatible=True,
                           init_llh=None, init_ecef=None):
        """Batched GPU look-ahead (one wave per trajectory); returns (fired, stop_cmd, i, xy_err) arrays."""
        mean, sigma = _d(mean), _d(sigma)
        T, M = mean.shape
        P, Q, STM, Hvec, pos = (_d(a).reshape(T, -1) for a in (P, Q, STM, Hvec, pos))
        arrival, now = _d(np.broadcast_to(arrival, (T,))), _d(np.broadcast_to(now, (T,)))
        fired, iout = np.zeros(T, dtype=np.int32), np.zeros(T, dtype=np.int32)
        cmd, xy = np.zeros(T), np.zeros(T)
        illh, iecef = _d(init_llh if init_llh is not None else INIT_LLH), _d(init_ecef if init_ecef is not None else INIT_ECEF)
        self._chk(self.lib.cgp_predict_stop_batch(self.h, T, M, _p(mean), _p(sigma), _p(P), _p(Q), _p(STM), _p(Hvec),
                                                  _p(pos), _p(arrival), _p(now), threshold, int(h_bug_compatible),
                                                  _p(illh), _p(iecef), fired.ctypes.data_as(_ip), _p(cmd),
                                                  iout.ctypes.data_as(_ip), _p(xy)))
        return fired.astype(bool), cmd, iout, xy

    def debug_read(self):
        out = np.zeros(DEBUG_SLOTS, dtype=np.int64)
        self._chk(self.lib.cgp_debug_read(self.h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))))
        return out

    def debug_buffers(self):
        """[(address, bytes)] of the context's large device buffers (include/corenav_gp.h: cgp_debug_buffers)."""
        out = np.zeros(16, dtype=np.uint64)
        self._chk(self.lib.cgp_debug_buffers(self.h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong))))
        return [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(8)]

    def debug_small(self):
        """Raw result record of the last short-window launch (include/corenav_gp.h: cgp_debug_small)."""
        out = np.zeros(48)
        self._chk(self.lib.cgp_debug_small(self.h, _p(out)))
        return out

    def window_plan(self, T, cap=64):
        """[(kind, arg, t0, nt)] of the launches a window_push of T ticks would make now (include/corenav_gp.h:
        cgp_debug_window_plan; kind is PLAN_TICKS / PLAN_PAIRS / PLAN_MULTI)."""
        out = np.zeros(4 * cap, dtype=np.int32)
        n = self._chk(self.lib.cgp_debug_window_plan(self.h, int(T), out.ctypes.data_as(_ip), cap))
        if n > cap:
            return self.window_plan(T, n)
        return [tuple(int(v) for v in out[4 * i:4 * i + 4]) for i in range(n)]

    def set_streams(self, n):
        self._chk(self.lib.cgp_set_streams(self.h, int(n)))

    def set_refine(self, steps=-1):
        """fp32 contexts: correction steps of alpha / the mean against a double-precision residual (cgp_set_refine): -1 the
        engine decides (one step: every fit at d <= 3, the dense fits beyond), 0 never, 1..3 always."""
        self._chk(self.lib.cgp_set_refine(self.h, int(steps)))

    def profile_enable(self, on=True):
        self._chk(self.lib.cgp_profile_enable(self.h, int(on)))

    def profile_read(self):
        ms, fl = np.zeros(PROF_KERNELS), np.zeros(PROF_KERNELS)
        n = np.zeros(PROF_KERNELS, dtype=np.int64)
        self._chk(self.lib.cgp_profile_read(self.h, _p(ms), _p(fl), n.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))))
        return {PROF_NAMES[i]: {"ms": float(ms[i]), "flops": float(fl[i]), "launches": int(n[i])}
                for i in range(PROF_KERNELS)}


class Sweep:
    """Multi-device sweep of independent fits through the C ABI (cgp_sweep_*): one context and one host
    thread per listed device, contiguous block partition, summaries gathered on the host."""

    def __init__(self, devices, max_n, max_m, max_d, max_batch_total, dtype=F64):
        self.lib = load()
        dv = np.ascontiguousarray(devices, dtype=np.int32)
        self.h = self.lib.cgp_sweep_create(dv.ctypes.data_as(_ip), len(dv), max_n, max_m, max_d, max_batch_total, dtype)
        if not self.h:
            raise RuntimeError("cgp_sweep_create failed: a listed device is not a usable gfx950 GPU or out of memory")
        self.ndev = self.lib.cgp_sweep_ndev(self.h)

    def close(self):
        if getattr(self, "h", None):
            self.lib.cgp_sweep_destroy(self.h)
            self.h = None

    __del__ = close

    def shard(self, batch, i):
        a, b = ctypes.c_int(0), ctypes.c_int(0)
        rc = self.lib.cgp_sweep_shard(self.h, batch, i, ctypes.byref(a), ctypes.byref(b))
        if rc:
            raise CgpError(rc)
        return a.value, b.value

    def fit_predict(self, X, y, Xs, theta, kernel_id, include_noise=True):
        X, y, Xs, theta = _d(X), _d(y), _d(Xs), _d(theta)
        B, N, d = X.shape
        M = Xs.shape[1]
        mean, var = np.empty((B, M)), np.empty((B, M))
        logml, info, summ = np.empty(B), np.zeros(B, dtype=np.int32), np.empty((B, 3))
        rc = self.lib.cgp_sweep_fit_predict(self.h, B, N, d, M, kernel_id, _p(X), _p(y), _p(Xs), _p(theta), theta.shape[1],
                                            int(include_noise), _p(mean), _p(var), _p(logml), info.ctypes.data_as(_ip),
                                            _p(summ))
        if rc < 0:
            raise CgpError(rc)
        return rc, mean, var, logml, info, summ

    def fit_predict_device(self, B, N, d, M, kernel_id, dX, dy, dXs, dtheta, djitter, include_noise, dmean, dvar, dlogml,
                           dinfo, streams=None):
        """cgp_sweep_fit_predict_device: every argument a list of ndev per-shard device pointers (ints), shard i's fits
        only; `streams` a list of hipStream_t handles (ints; None = the contexts' own streams).  Enqueues and returns."""
        def arr(ptrs):
            if ptrs is None:
                return None
            a = (ctypes.c_void_p * self.ndev)(*[ctypes.c_void_p(int(p) if p else 0) for p in ptrs])
            return ctypes.cast(a, _vp)
        keep = [arr(x) for x in (dX, dy, dXs, dtheta, djitter, dmean, dvar, dlogml, dinfo, streams)]
        rc = self.lib.cgp_sweep_fit_predict_device(self.h, B, N, d, M, kernel_id, keep[0], keep[1], keep[2], keep[3], keep[4],
                                                   int(include_noise), keep[5], keep[6], keep[7], keep[8], keep[9])
        if rc < 0:
            raise CgpError(rc)
        return rc

    def synchronize(self):
        rc = self.lib.cgp_sweep_synchronize(self.h)
        if rc:
            raise CgpError(rc)

    def set_streams(self, n):
        """cgp_set_streams on every shard's context."""
        for i in range(self.ndev):
            rc = self.lib.cgp_set_streams(self.lib.cgp_sweep_context(self.h, i), n)
            if rc:
                raise CgpError(rc)

    def set_refine(self, steps=-1):
        """cgp_set_refine on every shard's context."""
        for i in range(self.ndev):
            rc = self.lib.cgp_set_refine(self.lib.cgp_sweep_context(self.h, i), int(steps))
            if rc:
                raise CgpError(rc)


INIT_LLH = (0.693457963620326, -1.39498384275845, 334.993517334743)   # init_params.yaml:13-16
INIT_ECEF = (859153.0153, -4836303.7266, 4055378.501)                  # init_params.yaml:9-12


def llh_to_enu(lat, lon, h, init_llh=INIT_LLH, init_ecef=INIT_ECEF):
    out = np.empty(3)
    rc = load().cgp_llh_to_enu(lat, lon, h, _p(_d(init_llh)), _p(_d(init_ecef)), _p(out))
    if rc:
        raise CgpError(rc)
    return out


def predict_stop(mean, sigma, PvecData, QvecData, STMvecData, HvecData, pos_llh, arrival_time=0.0, now=0.0,
                 threshold=3.0, h_bug_compatible=True, init_llh=INIT_LLH, init_ecef=INIT_ECEF):
    mean, sigma = _d(mean), _d(sigma)
    fired, i = ctypes.c_int(0), ctypes.c_int(0)
    cmd, xy = ctypes.c_double(0.0), ctypes.c_double(0.0)
    rc = load().cgp_predict_stop(_p(mean), _p(sigma), len(mean), _p(_d(PvecData)), _p(_d(QvecData)),
                                 _p(_d(STMvecData)), _p(_d(HvecData)), _p(_d(pos_llh)), arrival_time, now, threshold,
                                 int(h_bug_compatible), _p(_d(init_llh)), _p(_d(init_ecef)), ctypes.byref(fired),
                                 ctypes.byref(cmd), ctypes.byref(i), ctypes.byref(xy))
    if rc:
        raise CgpError(rc)
    return bool(fired.value), cmd.value, i.value, xy.value


def gppredictor_callback(mean, sigma, PvecData, QvecData, STMvecData, HvecData, pos_llh, arrival_time, now,
                         h_bug_compatible=True):
    """One GpPredictor::GPCallBack through the C++ class; returns (n_published, stop_cmd)."""
    mean, sigma = _d(mean), _d(sigma)
    npub, cmd = ctypes.c_int(0), ctypes.c_double(0.0)
    rc = load().cgp_gppredictor_callback(_p(mean), _p(sigma), len(mean), _p(_d(PvecData)), _p(_d(QvecData)),
                                         _p(_d(STMvecData)), _p(_d(HvecData)), _p(_d(pos_llh)), arrival_time, now,
                                         int(h_bug_compatible), ctypes.byref(npub), ctypes.byref(cmd))
    if rc:
        raise CgpError(rc)
    return npub.value, cmd.value


class SlipRecorder:
    """CoreNav's slip computation + recording-window state machine (C++ class behind the C ABI)."""
    STATE_FIELDS = ("odomUptCount", "startRecording", "stopRecording", "gp_flag", "first_driving_flag",
                    "new_stop_data_arrived_", "skipped_windows", "cmd_stop_")

    def __init__(self):
        self.lib = load()
        self.h = self.lib.cgp_recorder_create()
        self.slip = 0.0

    def close(self):
        if getattr(self, "h", None):
            self.lib.cgp_recorder_destroy(self.h)
            self.h = None

    __del__ = close

    def update(self, vfl, vfr, vbl, vbr, vlin, cmd_x, cap=256):
        wv = _d([vfl, vfr, vbl, vbr])
        slip, n = ctypes.c_double(0.0), ctypes.c_int(0)
        t, s = np.empty(cap), np.empty(cap)
        pub = self.lib.cgp_recorder_update(self.h, _p(wv), vlin, cmd_x, ctypes.byref(slip), _p(t), _p(s), cap,
                                           ctypes.byref(n))
        self.slip = slip.value
        if pub < 0:
            raise CgpError(pub)
        return (t[:n.value].copy(), s[:n.value].copy()) if pub == 1 else None

    def stop_callback(self, cmd_stop):
        self.lib.cgp_recorder_stop_cmd(self.h, float(cmd_stop))

    def cmd_callback(self, cmd_x):
        self.lib.cgp_recorder_cmd(self.h, float(cmd_x))

    def state(self):
        st = np.zeros(8)
        self.lib.cgp_recorder_state(self.h, _p(st))
        return dict(zip(self.STATE_FIELDS, st))
