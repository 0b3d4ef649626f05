"""ctypes binding of the C-ABI in include/ntm_mpc.h (lib/libntm_mpc.so).

The product path has no fallback: if the HIP library is missing or fails to
load, every call raises ``NtmLibraryError``.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

PKG_ROOT = Path(__file__).resolve().parent.parent          # mpc-ntm-control_amd/
LIB_PATH = Path(os.environ.get("NTM_MPC_LIB", PKG_ROOT / "lib" / "libntm_mpc.so"))

MAX_N = 64
MODE_NONE, MODE_BOX, MODE_FULL, MODE_FULL_DU = 0, 1, 2, 3
ABI_VERSION = 7          # include/ntm_mpc.h NTM_MPC_ABI_VERSION
LITERAL_PHI_RIGHTMUL, LITERAL_GAMMA_INDEX, LITERAL_PLANT_NO_C, RHO1_SQUARED = 1, 2, 4, 8
EXIT_OPTIMAL, EXIT_MAXITER, EXIT_INFEASIBLE, EXIT_NONFINITE = 1, 0, -2, -7
NTM_OK = 0

PHYSICS_FIELDS = ("j_BS w_dep w_marg w_sat tau_r rs a eta_CD tau_E0 tau_E mu0 Lq B_pol m Cw "
                  "tau_A0 tau_w omega0").split()


class NtmLibraryError(RuntimeError):
    pass


class NtmPhysics(C.Structure):
    """ntm_physics — NTM_MPC_Sim.m:5-22."""
    _fields_ = [(n, C.c_double) for n in PHYSICS_FIELDS]


class NtmConfig(C.Structure):
    """ntm_config — NTM_MPC_Sim.m:30-60, 80-88."""
    _fields_ = [("N", C.c_int32), ("i_sim", C.c_int32), ("mode", C.c_int32), ("flags", C.c_int32),
                ("Ts", C.c_double), ("xmin", C.c_double * 2), ("xmax", C.c_double * 2),
                ("umin", C.c_double), ("umax", C.c_double), ("Q", C.c_double * 4),
                ("r", C.c_double * 2), ("epsilon", C.c_double), ("du_max", C.c_double),
                ("Ru", C.c_double)]


class NtmScenarioGen(C.Structure):
    """ntm_scenario_gen — plasma scenarios and disturbance realisations (include/ntm_mpc.h)."""
    _fields_ = [("seed", C.c_uint64), ("first_id", C.c_int64), ("k0", C.c_int32), ("reserved", C.c_int32),
                ("sigma_w", C.c_double), ("sigma_omega", C.c_double), ("jbs_spread", C.c_double),
                ("wdep_spread", C.c_double)]


class NtmObserver(C.Structure):
    """ntm_observer — plant-model mismatch and the disturbance estimate (include/ntm_mpc.h)."""
    _fields_ = [("nominal_model", C.c_int32), ("reserved", C.c_int32), ("gain", C.c_double)]


class NtmEstimator(C.Structure):
    """ntm_estimator — measurement noise and the filtered state estimate (include/ntm_mpc.h)."""
    _fields_ = [("nominal_model", C.c_int32), ("reserved", C.c_int32), ("gain", C.c_double * 2),
                ("kappa", C.c_double * 2), ("sigma_y", C.c_double * 2)]


class NtmDelay(C.Structure):
    """ntm_delay — actuator dead time and the delay-compensating plan (include/ntm_mpc.h)."""
    _fields_ = [("steps", C.c_int32), ("predict", C.c_int32)]


MAX_DELAY = 8            # include/ntm_mpc.h NTM_MAX_DELAY

_DP = C.POINTER(C.c_double)
_IP = C.POINTER(C.c_int32)
_V = C.c_void_p
_PHY = C.POINTER(NtmPhysics)
_CFG = C.POINTER(NtmConfig)
_OBS = C.POINTER(NtmObserver)
_EST = C.POINTER(NtmEstimator)
_DLY = C.POINTER(NtmDelay)


def _both(name, head, arrays):
    """The host entry point ``name`` and its ``_device`` twin, both returning int: context,
    physics and ``head`` (config, option structs, dimensions), then ``arrays``, a string of
    "d" (double*) and "i" (int32_t*).  The device form takes every array as void* (device
    memory) and a trailing void*, the stream."""
    lead = [C.c_void_p, _PHY] + head
    return {name: (C.c_int, lead + [_DP if a == "d" else _IP for a in arrays]),
            name + "_device": (C.c_int, lead + [_V] * (len(arrays) + 1))}


_B, _K = C.c_int64, C.c_int32          # the batch size; the number of closed-loop steps

# name -> (restype, argtypes); tests/test_host_signatures.py checks every entry against the header's prototype
EXPORTS = {
    "ntm_physics_default": (None, [_PHY]),
    "ntm_config_default": (None, [_CFG, C.c_int32]),
    "ntm_abi_version": (C.c_int32, []),
    "ntm_ctx_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32]),
    "ntm_ctx_destroy": (None, [C.c_void_p]),
    "ntm_last_error": (C.c_char_p, [C.c_void_p]),
    "ntm_ctx_set_stats": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ntm_ctx_set_small_batch": (C.c_int, [C.c_void_p, C.c_int64]),
    "ntm_ctx_set_one_wave_batch": (C.c_int, [C.c_void_p, C.c_int64]),
    "ntm_ctx_step_build": (C.c_int, [C.c_void_p, _CFG, C.c_int64, C.POINTER(C.c_int32)]),
    "ntm_ctx_step_layout": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.POINTER(C.c_int32)]),
    "ntm_ctx_step_layout_cfg": (C.c_int, [C.c_void_p, _CFG, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                          C.POINTER(C.c_int32)]),
    "ntm_debug_stamps": (C.c_int, [C.POINTER(C.c_ulonglong), C.c_int]),
    "ntm_step_launch_info": (C.c_int, [C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    **_both("ntm_mpc_init", [_CFG, _B], "ddd"),
    **_both("ntm_mpc_step", [_CFG, _B], "dddddd" "ii"),
    **_both("ntm_mpc_step_ws", [_CFG, _B], "dddddd" "iii"),
    **_both("ntm_mpc_run", [_CFG, _B, _K], "ddddd" "ii"),
    "ntm_rho_device": (C.c_int, [C.c_void_p, _PHY, _CFG, C.c_int64, _V, _V, _V]),
    "ntm_AB_device": (C.c_int, [C.c_void_p, _PHY, _CFG, C.c_int64, _V, _V, _V, _V]),
    "ntm_lift_device": (C.c_int, [C.c_void_p, _PHY, _CFG, C.c_int64, _V, _V, _V, _V, _V]),
    "ntm_cost_device": (C.c_int, [C.c_void_p, _PHY, _CFG, C.c_int64, _V, _V, _V, _V, _V]),
    "ntm_getwlc_device": (C.c_int, [C.c_void_p, _PHY, _CFG, C.c_int64, _V, _V, _V, _V, _V]),
    "ntm_qp_device": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, _V, _V, _V, _V, _V, _V, _V, _V]),
    "ntm_qp_mixed_device": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, _V, _V, _V, _V, _V, _V, _V,
                                      _V, _V, _V]),
    "ntm_qp_dual_device": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, _V, _V, _V, _V, _V, _V, _V, _V, _V,
                                     _V]),
    **_both("ntm_mpc_step_dual", [_CFG, _B], "dddddd" "iii" "dd"),
    **_both("ntm_mpc_step_obs", [_CFG, _OBS, _B], "ddddddd" "iii"),
    **_both("ntm_mpc_run_obs", [_CFG, _OBS, _B, _K], "ddddddd" "ii"),
    **_both("ntm_mpc_step_est", [_CFG, _EST, _B], "ddddddddd" "iii"),
    **_both("ntm_mpc_run_est", [_CFG, _EST, _B, _K], "dddddddddd" "ii"),
    **_both("ntm_mpc_run_from", [_CFG, _B, _K], "ddd" "i" "dddd" "ii"),
    **_both("ntm_mpc_run_est_from", [_CFG, _EST, _B, _K], "ddd" "i" "ddddddddd" "ii"),
    **_both("ntm_mpc_step_dly", [_CFG, _EST, _DLY, _B], "d" * 12 + "iii"),
    **_both("ntm_mpc_run_dly", [_CFG, _EST, _DLY, _B, _K], "d" * 13 + "ii"),
    **_both("ntm_mpc_run_dly_from", [_CFG, _EST, _DLY, _B, _K], "ddd" "i" + "d" * 12 + "ii"),
    "ntm_qp_kkt_device": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, _V, _V, _V, _V, _V, _V, _V, _V]),
    "ntm_mpc_kkt_device": (C.c_int, [C.c_void_p, _PHY, _CFG, C.c_int64, _V, _V, _V, _V, _V, _V]),
    "ntm_scenarios_x0": (None, [C.c_uint64, C.c_int64, C.c_int64, _DP]),
    "ntm_ctx_set_scenarios": (C.c_int, [C.c_void_p, C.POINTER(NtmScenarioGen)]),
    "ntm_scenario_sample": (None, [C.POINTER(NtmScenarioGen), C.c_int64, C.c_int32, _DP]),
    "ntm_meas_sample": (None, [C.POINTER(NtmScenarioGen), C.c_int64, C.c_int32, _DP]),
}

# additive entry points an older build of the library (one loaded through NTM_MPC_LIB, an
# A/B against a parent commit) may lack: bound when present, see has_run_from()
OPTIONAL = ("ntm_mpc_run_from", "ntm_mpc_run_from_device", "ntm_mpc_run_est_from", "ntm_mpc_run_est_from_device")
# the actuator dead time's (NTM_MPC_HAS_INPUT_DELAY), a set of its own: see has_input_delay()
OPTIONAL_DELAY = ("ntm_mpc_step_dly", "ntm_mpc_step_dly_device", "ntm_mpc_run_dly", "ntm_mpc_run_dly_device",
                  "ntm_mpc_run_dly_from", "ntm_mpc_run_dly_from_device")

_lib = None


def load(path: Path | str | None = None):
    """Load libntm_mpc.so (once) and bind every exported symbol."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = Path(path) if path is not None else LIB_PATH
    if not p.exists():
        raise NtmLibraryError(f"HIP library not built: {p} (run `make -C mpc-ntm-control_amd` "
                              "or __graft_entry__.build())")
    try:
        lib = C.CDLL(str(p))
    except OSError as e:  # pragma: no cover - depends on the loader
        raise NtmLibraryError(f"cannot load {p}: {e}") from e
    for name, (res, args) in EXPORTS.items():
        if name in OPTIONAL + OPTIONAL_DELAY and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.ntm_abi_version() != ABI_VERSION:
        raise NtmLibraryError("ABI version mismatch")
    if path is None:
        _lib = lib
    return lib


def has_run_from(lib=None) -> bool:
    """The loaded library has the resumable closed loops (NTM_MPC_HAS_RUN_FROM in the
    header): ntm_mpc_run_from* / ntm_mpc_run_est_from*, detected by symbol."""
    lib = lib or load()
    return all(hasattr(lib, n) for n in OPTIONAL)


def has_input_delay(lib=None) -> bool:
    """The loaded library has the actuator dead time (NTM_MPC_HAS_INPUT_DELAY in the
    header): ntm_mpc_step_dly* / ntm_mpc_run_dly* / ntm_mpc_run_dly_from*, detected by symbol."""
    lib = lib or load()
    return all(hasattr(lib, n) for n in OPTIONAL_DELAY)


def default_physics() -> NtmPhysics:
    p = NtmPhysics()
    load().ntm_physics_default(C.byref(p))
    return p


def default_config(N: int) -> NtmConfig:
    c = NtmConfig()
    load().ntm_config_default(C.byref(c), N)
    return c
