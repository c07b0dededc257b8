"""ctypes binding of the C ABI in include/ebm_hip.h (libebm_hip.so, built in-tree by
``csrc/Makefile`` / ``__graft_entry__.build()``).

This is the only compute path of the package: if the shared library is missing or no GPU is
present the calls fail loudly — there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# EBM_LIB: alternative build of the same library (A/B benchmarking of kernel variants)
LIB_PATH = os.environ.get("EBM_LIB") or os.path.join(_HERE, "libebm_hip.so")

# enum ebm_model / ebm_grid / ebm_field / ebm_param (include/ebm_hip.h)
MODEL = {"MIZ": 0, "Classic": 1, "MIZ_IMEX": 2}     # MIZ_IMEX: extension, see include/ebm_hip.h
GRID = {"identity": 0, "nonuniform": 1}
FIELD = {"Ei": 0, "Ew": 1, "h": 2, "D": 3, "phi": 4, "T0": 5, "Tw": 6, "Ti": 7, "n": 8,
         "E": 9, "T": 10, "Tg": 11}
SCALAR_KIND = {"integral": 0, "mean": 1, "edge_ge": 2, "edge_le": 3}     # enum ebm_scalar_kind
PARAM_ORDER = ("D", "A", "B", "cw", "S0", "S1", "S2", "a0", "a2", "ai", "Fb", "k", "Lf", "F",
               "cg", "tau", "Tm", "m1", "m2", "alpha", "rl", "Dmin", "Dmax", "hmin", "kappa")
_lib = None

STATUS = {0: "EBM_OK", -1: "EBM_ERR_ARG", -2: "EBM_ERR_HIP", -3: "EBM_ERR_UNSUPPORTED", -4: "EBM_ERR_NO_DEVICE",
          -5: "EBM_ERR_STALE"}


class Options(C.Structure):
    """struct ebm_options (include/ebm_hip.h)."""
    _fields_ = [("struct_bytes", C.c_int), ("cells_per_thread", C.c_int), ("use_graph", C.c_int),
                ("prefetch_cols", C.c_int), ("launch_chains", C.c_int), ("integrate_steps_per_launch", C.c_int),
                ("fused_state_in_lds", C.c_int), ("elide_zero_lines", C.c_int)]


# The C ABI, one row per prototype of include/ebm_hip.h, in its parameter order (tests/test_host.py holds every row against
# the header).  _h: an ebm_handle_t; _dev: a device address (the header's double *dev_...); every function returns int
# (an ebm_status) but those of RESTYPES.
_i, _ll, _u, _ull, _d, _h, _dev = C.c_int, C.c_longlong, C.c_uint, C.c_ulonglong, C.c_double, C.c_void_p, C.c_void_p
_ip, _llp, _up, _dp = C.POINTER(_i), C.POINTER(_ll), C.POINTER(_u), C.POINTER(_d)
_create = [C.POINTER(_h), _i, _i, _i, _i, _dp, _dp, _d, _i]
SIGNATURES = {
    "ebm_create": _create,
    "ebm_create_ex": _create + [C.POINTER(Options)],
    "ebm_options_default": [C.POINTER(Options)],
    "ebm_field_step": [_h, _i, _llp, _llp, _ip],
    "ebm_get_field_as_of": [_h, _i, _ll, _dp],
    "ebm_destroy": [_h],
    "ebm_last_error": [],
    "ebm_version": [],
    "ebm_set_field": [_h, _i, _dp],
    "ebm_get_field": [_h, _i, _dp],
    "ebm_hemispheric_mean": [_h, _i, _dp],
    "ebm_hemispheric_mean_device": [_h, _i, _dev],
    "ebm_get_field_device": [_h, _i, _dev],
    "ebm_field_device_ptr": [_h, _i, C.POINTER(_dev), _llp],
    "ebm_diffusion": [_h, _dp, _dp, _dp],
    "ebm_zonal_diffusion": [_h, _i, _dp, _dp, _dp],
    "ebm_set_column_forcing": [_h, _dp],
    "ebm_set_column_schedule": [_h, _dp],
    "ebm_set_column_params": [_h, _dp],
    "ebm_set_column_noise": [_h, _dp, _dp, C.POINTER(_ull), _ull],
    "ebm_get_noise_state": [_h, _dp],
    "ebm_set_noise_state": [_h, _dp],
    "ebm_noise_innovations": [_h, _ll, _i, _dp],
    "ebm_set_step_clock": [_h, _ll],
    "ebm_set_time_table": [_h, _i, _dp],
    "ebm_step": [_h, _d, _d, _d, _i],
    "ebm_run": [_h, _ll, _i, _dp, _i],
    "ebm_run_fused": [_h, _ll, _i, _dp, _i, _i],
    "ebm_run_series": [_h, _ll, _i, _dp, _i, _i, _i, _ip, _dp],
    "ebm_integrate": [_h, _i, _i, _dp, _i, _i, _i, _i, _ip, _dp, _dp, _dp, _dp],
    "ebm_integrate_hemispheric": [_h, _i, _i, _dp, _i, _i, _i, _ip, _dp, _dp, _dp],
    "ebm_equilibrate": [_h, _i, _i, _i, _dp, _i, _ip, _dp, _ip, _ip, _dp],
    "ebm_run_until": [_h, _ll, _i, _i, _dp, _i, _i, _dp, _ip, _ip, _ip, _dp],
    "ebm_resample_columns": [_h, _ip],
    "ebm_column_record": [_h, _llp, _up],
    "ebm_export_columns": [_h, _i, _ip, _dev, _up],
    "ebm_import_columns": [_h, _i, _ip, _ip, _dev, _u],
    "ebm_ensemble_sums": [_h, _i, _ip, _dp, _dp, _dp],
    "ebm_ensemble_sums_device": [_h, _i, _ip, _dp, _dp, _dev],
    "ebm_ensemble_range": [_h, _i, _ip, _dp, _dp],
    "ebm_ensemble_range_device": [_h, _i, _ip, _dp, _dev],
    "ebm_ensemble_histogram": [_h, _i, _ip, _dp, _i, _dp, _dp, _dp],
    "ebm_ensemble_histogram_device": [_h, _i, _ip, _dp, _i, _dp, _dp, _dev],
    "ebm_ensemble_covariance": [_h, _i, _i, _dp, _dp, _dp, _dp],
    "ebm_ensemble_covariance_device": [_h, _i, _i, _dp, _dp, _dp, _dev],
    "ebm_column_misfits": [_h, _i, _ip, _i, _dp, _dp, _dp],
    "ebm_column_misfits_device": [_h, _i, _ip, _i, _dp, _dp, _dev],
    "ebm_update_columns": [_h, _i, _ip, _i, _dp, _dp, _d, _dev, _dp, _dp],
    "ebm_update_columns_device": [_h, _i, _ip, _i, _dev, _dp, _d, _dev, _dp, _dp],
    "ebm_spd_solve_device": [_h, _i, _ll, _dev, _ll, _dev, _ll, _ip],
    "ebm_kalman_gain_device": [_h, _i, _dp, _dp, _d, _d, _dev, C.POINTER(C.c_void_p), _dev, _ip],
    "ebm_kalman_gain_phases": [_h, C.POINTER(C.c_float)],
    "ebm_column_scalars": [_h, _i, _ip, _dp, _dp],
    "ebm_column_scalars_device": [_h, _i, _ip, _dp, _dev],
    "ebm_run_series_scalars": [_h, _ll, _i, _dp, _i, _i, _i, _ip, _dp, _dp],
    "ebm_run_until_scalar": [_h, _ll, _i, _i, _dp, _i, _ip, _d, _dp, _ip, _ip, _ip, _dp],
    "ebm_sync": [_h],
    "ebm_get_counters": [_h, _llp],
    "ebm_reset_counters": [_h],
    "ebm_state_conversions": [_h, _llp],
    "ebm_zero_line_flags": [_h, _up, _ip],
    "ebm_timer_start": [_h],
    "ebm_timer_stop": [_h, C.POINTER(C.c_float)],
    "ebm_launch_info": [_h, _ip],
    "ebm_selftest_divide": [_i, _i, _dp, _dp, _dp],
    "ebm_selftest_permute": [_i, _i, _i, _dp, _dp, _dp],
}
RESTYPES = {"ebm_last_error": C.c_char_p, "ebm_version": C.c_char_p}
EXPORTS = tuple(SIGNATURES)


class EBMError(RuntimeError):
    """A C-ABI call returned a negative ebm_status (``.status``)."""
    status = 0


class StaleFieldError(EBMError):
    """EBM_ERR_STALE: a diagnostic field (or the fp64 T0) older than the state was asked for."""


def load():
    """Load libebm_hip.so (once).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EBMError(
            f"{LIB_PATH} not found: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()' or make -C csrc); "
            "this package has no CPU fallback")
    # One HIP runtime per process: PyTorch ships its own libamdhip64 and the system has another.  If this
    # library pulls in the system's first, a later `import torch` finds a runtime it did not expect
    # ("No HIP GPUs are available").  Importing torch first makes the dynamic loader resolve this
    # library's libamdhip64 dependency to the copy torch has already loaded.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = argtypes, RESTYPES.get(name, C.c_int)
    _lib = lib
    return lib


def check(rc: int, what: str):
    if rc != 0:
        msg = load().ebm_last_error().decode()
        err = (StaleFieldError if rc == -5 else EBMError)(f"{what} failed (status {rc} {STATUS.get(rc, '?')}): {msg}")
        err.status = rc
        raise err


def dptr(a):
    return None if a is None else a.ctypes.data_as(_dp)


def iptr(a):
    """``dptr`` for an int32 array."""
    return None if a is None else a.ctypes.data_as(_ip)


def field_ids(ids):
    """The ``const int *fields`` argument: the field ids as a C int array."""
    return (C.c_int * len(ids))(*ids)


def as_f64(a, shape=None):
    out = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and out.shape != tuple(shape):
        raise ValueError(f"expected array of shape {tuple(shape)}, got {out.shape}")
    return out
