"""Host-side mirror of the reference's MATLAB interface over the HIP C-ABI.

The reference (IsaacSavona/MPC-NTM-Control) is a MATLAB script whose hot path
is a handful of functions resolved by name.  MATLAB is not available in this
image, so the host side is Python; it keeps the reference's names, argument
meaning and error behaviour, batched over scenarios:

    rho1 / rho2 / rho3          rho1.m, rho2.m, rho3.m
    A / B                       A.m, B.m
    Rho_to_PhiGammaLambda       Rho_to_PhiGammaLambda.m
    cost (G, F)                 NTM_MPC_Sim.m:120-121
    getWLc                      getWLc.m
    quadprog                    NTM_MPC_Sim.m:97 (exitflag semantics :98-103)
    NtmMpc.step                 NTM_MPC_Sim.m:94-130  (one time step, drop-in)
    NtmMpc.run / NTM_MPC_Sim    NTM_MPC_Sim.m:80-131  (closed loop)

All batched arrays have shape (E, B) — element e of scenario s at [e, s] —
and their storage is the C-ABI's scenario-major layout: each scenario's
E-record is contiguous, [s*E + e], i.e. the transpose of a contiguous (B, E)
array (MATLAB's E-by-B arrays, one column per scenario).  Arrays this module
returns are laid out that way, so passing them back costs nothing; any other
(E, B) array is accepted too, through a staged copy (in/out arguments are
copied back).  ``device_tensor`` builds a device tensor in the ABI layout from
host data.  PyTorch is only plumbing (device memory, streams); every
computation runs in the HIP kernels of lib/libntm_mpc.so.  There is no CPU
fallback: without the library or a GPU, calls raise.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib as L
from ._lib import NtmConfig, NtmLibraryError, NtmPhysics, NtmScenarioGen


STATS_ROWS = 6   # include/ntm_mpc.h NTM_STATS_ROWS


@dataclass
class Physics:
    """Physics constants, NTM_MPC_Sim.m:5-22."""
    j_BS: float = 73e3
    w_dep: float = 0.024
    w_marg: float = 0.02
    w_sat: float = 0.32
    tau_r: float = 293.0
    rs: float = 1.55
    a: float = 2.0
    eta_CD: float = 0.9
    tau_E0: float = 3.7
    tau_E: float = 3.7
    mu0: float = 4e-7 * math.pi
    Lq: float = 0.87
    B_pol: float = 0.97
    m: float = 2.0
    Cw: float = 1.0
    tau_A0: float = 3e-6
    tau_w: float = 0.188
    omega0: float = 2 * math.pi * 420

    def to_c(self) -> NtmPhysics:
        return NtmPhysics(*[float(getattr(self, n)) for n in L.PHYSICS_FIELDS])


@dataclass
class Config:
    """Controller configuration, NTM_MPC_Sim.m:30-60, 80-88 (mode/flags: SURVEY.md §2.1)."""
    N: int = 20
    Ts: float = 0.1
    xmin: tuple = (0.06, 100 * 2 * math.pi)
    xmax: tuple = (0.15, 5000 * 2 * math.pi)
    umin: float = 0.0
    umax: float = 2e6
    Q: tuple = (1.0, 0.0, 0.0, 1.0)
    r: tuple = (0.0, 1000 * 2 * math.pi)
    i_sim: int = 10
    epsilon: float = 1e-14
    mode: int = L.MODE_FULL
    flags: int = 0
    du_max: float = 5e5      # NTM_MODE_FULL_DU (config 5, extension): |U_i - U_{i-1}| <= du_max
    Ru: float = 0.0          # input weight (ABI v5): G = 2 Gamma' Om Gamma + 2 Ru I; the reference: 0

    def to_c(self) -> NtmConfig:
        return NtmConfig(int(self.N), int(self.i_sim), int(self.mode), int(self.flags), float(self.Ts),
                         (C.c_double * 2)(*self.xmin), (C.c_double * 2)(*self.xmax), float(self.umin),
                         float(self.umax), (C.c_double * 4)(*self.Q), (C.c_double * 2)(*self.r),
                         float(self.epsilon), float(self.du_max), float(self.Ru))

    @property
    def m(self) -> int:
        if self.mode == L.MODE_NONE:
            return 0
        if self.mode == L.MODE_BOX:
            return 2 * self.N
        return 6 * self.N + 4 + (2 * (self.N - 1) if self.mode == L.MODE_FULL_DU else 0)


@dataclass
class ScenarioGen:
    """ntm_scenario_gen: independent plasma scenarios (j_BS, w_dep of NTM_MPC_Sim.m:5-6,
    each scaled by 1 + spread (2u - 1)) and additive plant disturbances (on
    NTM_MPC_Sim.m:130, unit-variance Irwin-Hall samples times sigma), all
    counter-based on (seed, global scenario id, time index)."""
    seed: int = 20241220
    first_id: int = 0          # global id of the batch's scenario 0 (a shard's offset)
    k0: int = 0                # time index of the next launch's first plant step
    sigma_w: float = 0.0       # [m]
    sigma_omega: float = 0.0   # [rad/s]
    jbs_spread: float = 0.0
    wdep_spread: float = 0.0

    def to_c(self) -> NtmScenarioGen:
        return NtmScenarioGen(int(self.seed) & 0xFFFFFFFFFFFFFFFF, int(self.first_id), int(self.k0), 0,
                              float(self.sigma_w), float(self.sigma_omega), float(self.jbs_spread),
                              float(self.wdep_spread))


@dataclass
class Observer:
    """ntm_observer: plant-model mismatch and the offset-free disturbance estimate.
    ``nominal_model``: the controller's model is this controller's Physics and the
    generator's j_BS / w_dep spreads are the plant's alone (False: model = the
    scenario's plasma, as step / run).  ``gain`` in [0, 1]: d_hat <- d_hat +
    gain (e - d_hat) from the one-step prediction error e; 0 freezes d_hat."""
    nominal_model: bool = False
    gain: float = 0.0

    def to_c(self) -> L.NtmObserver:
        return L.NtmObserver(1 if self.nominal_model else 0, 0, float(self.gain))


def _pair(v) -> tuple:
    """A scalar (both components) or a (w, omega) pair as two floats."""
    a = np.broadcast_to(np.asarray(v, dtype=float), (2,))
    return float(a[0]), float(a[1])


@dataclass
class Estimator:
    """ntm_estimator: output feedback, a noisy measurement and a fixed-gain state filter
    next to the disturbance estimate.  ``nominal_model`` as Observer.  ``gain``, ``kappa``
    and ``sigma_y`` are (w, omega) pairs (a scalar sets both): d_hat's gain in [0, 1];
    the trust in the model in [0, 1] (0: x_hat is the measurement); the measurement
    noise's standard deviation in m and rad/s (non-zero needs an attached ScenarioGen)."""
    nominal_model: bool = False
    gain: tuple = (0.0, 0.0)
    kappa: tuple = (0.0, 0.0)
    sigma_y: tuple = (0.0, 0.0)

    def to_c(self) -> L.NtmEstimator:
        d2 = C.c_double * 2
        return L.NtmEstimator(1 if self.nominal_model else 0, 0, d2(*_pair(self.gain)), d2(*_pair(self.kappa)),
                              d2(*_pair(self.sigma_y)))


@dataclass
class Delay:
    """ntm_delay: actuator dead time.  The plant applies the input commanded ``steps``
    sampling periods ago (0 .. MAX_DELAY = 8); the pending inputs travel in a queue
    ``u_queue`` (steps, B), oldest first.  ``predict``: the controller plans from the
    state its model predicts for the moment the command arrives (x_hat carried over the
    queued inputs); False plans from x_hat, a controller that does not know the delay."""
    steps: int = 0
    predict: bool = True

    def to_c(self) -> L.NtmDelay:
        return L.NtmDelay(int(self.steps), 1 if self.predict else 0)


def meas_sample(gen: ScenarioGen, B: int, k: int = 0) -> np.ndarray:
    """(B, 2) host-side unit samples of the measurement noise for scenarios
    gen.first_id + s at time index k: the generator's normal channels 2 (w) and 3
    (omega) (ntm_meas_sample; no GPU needed)."""
    out = np.zeros((B, 2))
    L.load().ntm_meas_sample(C.byref(gen.to_c()), B, k, out.ctypes.data_as(C.POINTER(C.c_double)))
    return out


def scenario_sample(gen: ScenarioGen, B: int, k: int = 0) -> np.ndarray:
    """(B, 4) host-side samples of the generator for scenarios gen.first_id + s: j_BS
    factor, w_dep factor, n_w(k), n_omega(k) (ntm_scenario_sample; no GPU needed)."""
    out = np.zeros((B, 4))
    L.load().ntm_scenario_sample(C.byref(gen.to_c()), B, k, out.ctypes.data_as(C.POINTER(C.c_double)))
    return out


def _ptr(t: torch.Tensor | None):
    if t is None:
        return None
    return C.c_void_p(t.data_ptr())


def _host_ptr(a: np.ndarray | None):
    """Host pointer typed by the array's dtype (int32 or double); None stays None."""
    if a is None:
        return None
    return a.ctypes.data_as(L._IP if a.dtype == np.int32 else L._DP)


def _dev_checked(t, shape, dtype, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name} must be a CUDA tensor")
    if t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype}, got {t.dtype}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")


def _check_dev(t: torch.Tensor, shape, dtype=torch.float64, name="tensor"):
    """Plain contiguous CUDA array (instrumentation counters, SoA)."""
    _dev_checked(t, shape, dtype, name)
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def is_scenario_major(a) -> bool:
    """(E, B) array whose storage is scenario-major ([s*E + e]); 1-D arrays trivially."""
    if isinstance(a, np.ndarray):
        return a.ndim < 2 or a.T.flags.c_contiguous
    return a.dim() < 2 or a.T.is_contiguous()


def _dev_arg(t, shape, dtype=torch.float64, name="tensor"):
    """Validate an (E, B) CUDA argument; return (array in the ABI layout, staged?)."""
    _dev_checked(t, shape, dtype, name)
    if is_scenario_major(t):
        return t, False
    return t.T.contiguous().T, True


def _host_arg(a, shape, dtype=np.float64, name="array"):
    """Validate an (E, B) host argument; return (array in the ABI layout, staged?)."""
    if not isinstance(a, np.ndarray) or a.shape != tuple(shape) or a.dtype != dtype:
        raise ValueError(f"{name}: expected {np.dtype(dtype).name} {tuple(shape)}")
    if is_scenario_major(a):
        return a, False
    return np.asfortranarray(a), True


def _host_empty(*shape, dtype=np.float64):
    return np.empty(shape[::-1], dtype).T if len(shape) == 2 else np.empty(shape, dtype)


def device_tensor(a, device=None, dtype=torch.float64) -> torch.Tensor:
    """(E, B) host data -> (E, B) CUDA tensor in the ABI's scenario-major layout."""
    a = np.asarray(a)
    if device is None:
        device = torch.cuda.current_device()
    dev = device if isinstance(device, (str, torch.device)) else torch.device("cuda", int(device))
    return torch.tensor(np.ascontiguousarray(a.T), dtype=dtype, device=dev).T


class _Device:
    """What the ``_device`` form of an entry point needs: CUDA tensors in and out, the
    launch on the controller's current stream.  ``arg`` validates an argument into the ABI
    layout, ``empty`` allocates, ``ptr`` makes a pointer (None: NULL), ``copy_back`` returns
    a staged in/out argument; ``suffix`` ends the symbol, ``tail`` the argument list."""
    suffix, i32 = "_device", torch.int32
    arg, ptr = staticmethod(_dev_arg), staticmethod(_ptr)

    def __init__(self, device: int):
        self.device = device

    def empty(self, *shape, dtype=torch.float64):
        """(E, B) output in the ABI's scenario-major layout (1-D: plain)."""
        dev = f"cuda:{self.device}"
        if len(shape) == 2:
            return torch.empty(shape[1], shape[0], dtype=dtype, device=dev).T
        return torch.empty(*shape, dtype=dtype, device=dev)

    def stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def tail(self):
        return (self.stream(),)

    @staticmethod
    def copy_back(dst, src):
        dst.copy_(src)


class _Host:
    """The host form (the MEX path): NumPy arrays, which the library stages itself."""
    suffix, i32 = "", np.int32
    arg, empty, ptr = staticmethod(_host_arg), staticmethod(_host_empty), staticmethod(_host_ptr)

    @staticmethod
    def tail():
        return ()

    @staticmethod
    def copy_back(dst, src):
        dst[...] = src


_HOST = _Host()
_NONE = {}          # no carried arrays (a default argument; never written to)


def _optional(arg, a, *spec, **kw):
    """``arg`` for an argument that may be None: (None, False) then."""
    return (None, False) if a is None else arg(a, *spec, **kw)


def _queue_arg(be, q, opts, Bn, name):
    """The dead time's queue (steps, B) as (array, staged?); None where there is none.  The
    delay is the last of the option structs."""
    if q is None:
        return None, False
    return be.arg(q, (int(opts[-1].steps), Bn), name=name)


class NtmMpc:
    """Batched LPV-MPC controller on one MI355X (one ``ntm_ctx`` per device)."""

    def __init__(self, physics: Physics | None = None, config: Config | None = None, device: int | None = None):
        self.lib = L.load()
        if not torch.cuda.is_available():
            raise NtmLibraryError("no GPU visible: the HIP path has no CPU fallback")
        self.device = torch.cuda.current_device() if device is None else int(device)
        self.physics = physics or Physics()
        self.config = config or Config()
        self.gen = None
        self._dev = _Device(self.device)
        self._ctx = C.c_void_p()
        rc = self.lib.ntm_ctx_create(C.byref(self._ctx), self.device)
        if rc != L.NTM_OK:
            raise NtmLibraryError(f"ntm_ctx_create failed ({rc})")

    def close(self):
        if self._ctx:
            self.lib.ntm_ctx_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------ helpers
    def _cfg(self, cfg: Config | None):
        return (cfg or self.config).to_c()

    def _stream(self):
        return self._dev.stream()

    def _raise(self, rc, what):
        if rc != L.NTM_OK:
            raise NtmLibraryError(f"{what} failed ({rc}): {self.lib.ntm_last_error(self._ctx).decode()}")

    def _empty(self, *shape, dtype=torch.float64):
        """(E, B) output in the ABI's scenario-major layout (1-D: plain)."""
        return self._dev.empty(*shape, dtype=dtype)

    def tensor(self, a, dtype=torch.float64) -> torch.Tensor:
        """(E, B) host data -> device tensor in the ABI layout on this controller's GPU."""
        return device_tensor(a, self.device, dtype)

    def set_stats(self, stats: torch.Tensor | None):
        """Accumulate per-scenario counters (NTM_STATS_ROWS=6, B) int32 (plain
        contiguous rows) into ``stats`` during subsequent step/run launches: QP
        solves, GI iterations, final active rows, state rows in the final active
        set, warm-start candidate verifications, full GI solves; None disables."""
        if stats is not None:
            if stats.dim() != 2 or stats.shape[0] != STATS_ROWS:
                raise ValueError(f"stats must be ({STATS_ROWS}, B) int32")
            _check_dev(stats, tuple(stats.shape), dtype=torch.int32, name="stats")
        self._raise(self.lib.ntm_ctx_set_stats(self._ctx, _ptr(stats)), "ntm_ctx_set_stats")

    def set_small_batch(self, max_scenarios: int = -1):
        """ntm_ctx_set_small_batch: N = 20 batches of at most ``max_scenarios``
        run on the all-LDS build, larger ones on the far-workspace 4-wave build;
        -1 restores the default (8 x the compute units), 0 always uses the far
        build."""
        self._raise(self.lib.ntm_ctx_set_small_batch(self._ctx, int(max_scenarios)), "ntm_ctx_set_small_batch")

    def set_one_wave_batch(self, max_scenarios: int = -1):
        """ntm_ctx_set_one_wave_batch: all-LDS N = 20 batches of at most
        ``max_scenarios`` use the one-wave register budget (bit-identical results);
        -1 restores the default (4 x the compute units), 0 never."""
        self._raise(self.lib.ntm_ctx_set_one_wave_batch(self._ctx, int(max_scenarios)), "ntm_ctx_set_one_wave_batch")

    def step_build(self, B: int, cfg: Config | None = None) -> str:
        """The build a launch of B scenarios takes: "far", "lds" or "lds1" (the
        all-LDS build with the one-wave register budget; ntm_ctx_step_build)."""
        b = C.c_int32()
        self._raise(self.lib.ntm_ctx_step_build(self._ctx, C.byref((cfg or self.config).to_c()), int(B), C.byref(b)),
                    "ntm_ctx_step_build")
        return ("far", "lds", "lds1")[b.value]

    def set_scenarios(self, gen: ScenarioGen | None):
        """Attach a scenario generator (ntm_ctx_set_scenarios): subsequent
        initial_state / step / run launches use each scenario's own plasma and
        add its disturbance realisation to the plant step; None restores the
        nominal, disturbance-free loop of the reference."""
        self.gen = gen
        self._raise(self.lib.ntm_ctx_set_scenarios(self._ctx, None if gen is None else C.byref(gen.to_c())),
                    "ntm_ctx_set_scenarios")

    def _layout(self, B: int, cfg: Config):
        far, lanes, nn = C.c_int32(), C.c_int32(), C.c_int32()
        self._raise(self.lib.ntm_ctx_step_layout_cfg(self._ctx, C.byref(cfg.to_c()), int(B), C.byref(far),
                                                     C.byref(lanes), C.byref(nn)), "ntm_ctx_step_layout_cfg")
        return ("far" if far.value else "lds"), lanes.value, nn.value

    def step_layout(self, B: int, cfg: Config | None = None) -> str:
        """Workspace layout of the build a launch of B scenarios with ``cfg``
        (flags included) takes: "far" (J/R in a per-scenario HBM block) or "lds"
        (ntm_ctx_step_layout_cfg)."""
        return self._layout(B, cfg or self.config)[0]

    def step_kernel_name(self, B: int, cfg: Config | None = None) -> str:
        """Name of the fused step kernel specialisation a launch uses (reporting)."""
        layout, lanes, nn = self._layout(B, cfg or self.config)
        build = self.step_build(B, cfg)
        return f"k_mpc_step<P={lanes},NN={nn},{layout}>" + (" (one-wave budget)" if build == "lds1" else "")

    # ------------------------------------------------------------ closed-loop entry points: one body per family
    # Every public method below forwards here with its backend (self._dev or _HOST); the
    # argument list of each entry point is marshalled in one place, in the ABI's order.
    def _call(self, be, entry, cfg, opts, dims, arrays):
        """ntm_mpc_<entry> in the backend's form: context, physics, cfg, the option structs,
        the dimensions, every array (None: NULL), then the backend's trailing arguments."""
        what = "ntm_mpc_" + entry + be.suffix
        rc = getattr(self.lib, what)(self._ctx, C.byref(self.physics.to_c()), C.byref(cfg.to_c()),
                                     *[C.byref(o.to_c()) for o in opts], *dims, *[be.ptr(a) for a in arrays],
                                     *be.tail())
        self._raise(rc, what)

    def _need_run_from(self):
        if not L.has_run_from(self.lib):
            raise NtmLibraryError("this build of the library has no ntm_mpc_run_from (NTM_MPC_HAS_RUN_FROM)")

    def _need_input_delay(self, entry):
        if not L.has_input_delay(self.lib):
            raise NtmLibraryError(f"this build of the library has no {entry} (NTM_MPC_HAS_INPUT_DELAY)")

    @staticmethod
    def _carried_args(be, carried, opts, Bn):
        """The estimator's carried d_hat / x_hat (2, B) and the dead time's u_queue (steps, B;
        None where there is none), by name and in the ABI's order, as [(array, staged?)]."""
        return [_queue_arg(be, a, opts, Bn, n) if n == "u_queue" else be.arg(a, (2, Bn), name=n)
                for n, a in carried.items()]

    def _initial_state(self, be, x0, cfg):
        cfg = cfg or self.config
        Bn = x0.shape[1]
        x0, _ = be.arg(x0, (2, Bn), name="x0")
        rho, U_old = be.empty(3 * cfg.N, Bn), be.empty(cfg.N, Bn)
        self._call(be, "init", cfg, (), (Bn,), (x0, rho, U_old))
        return rho, U_old

    def _step(self, be, entry, x_k, rho, U_old, cfg, active_ws, opts=(), carried=_NONE, dual=False, out=None):
        """The step* family.  ABI order: x_k, the in/out state (rho, U_old, then ``carried``),
        the outputs (U, x_pred, x_next, y with x_hat, x_plan and u_applied with u_queue,
        exitflag, inner_iters), active_ws, and step_dual's lambda and rho_qp.  In/out arguments
        not in the ABI layout are staged and copied back; ``carried`` is echoed into the dict."""
        cfg = cfg or self.config
        N, Bn = cfg.N, x_k.shape[1]
        xk, _ = be.arg(x_k, (2, Bn), name="x_k")
        state = [be.arg(rho, (3 * N, Bn), name="rho"), be.arg(U_old, (N, Bn), name="U_old")]
        if carried:
            state += self._carried_args(be, carried, opts, Bn)
        state.append(_optional(be.arg, active_ws, (2 * (N + 1), Bn), be.i32, "active_ws"))
        spec = [("U", (N, Bn)), ("x_pred", (2 * (N + 1), Bn)), ("x_next", (2, Bn))]
        if "x_hat" in carried:
            spec.append(("y", (2, Bn)))
        if "u_queue" in carried:
            spec += [("x_plan", (2, Bn)), ("u_applied", (Bn,))]
        if out is None:
            out = {k: be.empty(*shp) for k, shp in spec}
            out["exitflag"], out["inner_iters"] = be.empty(Bn, dtype=be.i32), be.empty(Bn, dtype=be.i32)
            if dual:
                out["lambda"], out["rho_qp"] = be.empty(cfg.m, Bn), be.empty(3 * N, Bn)
        else:
            for k, shp in spec:
                if tuple(out[k].shape) != shp or not is_scenario_major(out[k]):
                    raise ValueError(f"out[{k!r}] must be a {shp} array from an earlier step()")
        arrays = [xk, *[a for a, _ in state[:-1]], *[out[k] for k, _ in spec], out["exitflag"], out["inner_iters"],
                  state[-1][0]]
        if dual:
            arrays += [out["lambda"] if cfg.m else None, out["rho_qp"]]
        self._call(be, entry, cfg, opts, (Bn,), arrays)
        for dst, (src, staged) in zip((rho, U_old, *carried.values(), active_ws), state):
            if staged:
                be.copy_back(dst, src)
        if carried:
            out.update(carried)
        return out

    def _run_out(self, be, k_sim, N, Bn, dk=False, est=False, dly=False):
        """The closed loops' histories in the ABI's order (which is the dict's): xk, uk, Uk,
        wpred, the observer's dk, the estimator's xhk and yk, the dead time's uak and xpk,
        exitflag, inner_iters."""
        mk = be.empty
        out = {"xk": mk(2 * (k_sim + 1), Bn), "uk": mk(k_sim, Bn), "Uk": mk(N * k_sim, Bn),
               "wpred": mk((N + 1) * k_sim, Bn)}
        if dk:
            out["dk"] = mk(2 * (k_sim + 1), Bn)
        if est:
            out.update(xhk=mk(2 * (k_sim + 1), Bn), yk=mk(2 * k_sim, Bn))
        if dly:
            out.update(uak=mk(k_sim, Bn), xpk=mk(2 * k_sim, Bn))
        out.update(exitflag=mk(k_sim, Bn, dtype=be.i32), inner_iters=mk(k_sim, Bn, dtype=be.i32))
        return out

    def _run(self, be, entry, x0, k_sim, cfg, opts=(), init=_NONE):
        """The run* family from x0.  ``init``: the optional initial d0, xhat0 (2, B) and uq0
        (steps, B) by name, in the ABI's order; each brings its histories."""
        cfg = cfg or self.config
        N, Bn = cfg.N, x0.shape[1]
        ins = [be.arg(x0, (2, Bn), name="x0")[0]]
        for n, a in init.items():
            ins.append((_queue_arg(be, a, opts, Bn, n) if n == "uq0" else _optional(be.arg, a, (2, Bn), name=n))[0])
        if "uq0" in init:
            self._need_run_from()
            self._need_input_delay("ntm_mpc_run_dly")
        out = self._run_out(be, k_sim, N, Bn, dk="d0" in init, est="xhat0" in init, dly="uq0" in init)
        self._call(be, entry, cfg, opts, (Bn, k_sim), (*ins, *out.values()))
        return out

    def _run_from(self, be, entry, x, rho, U_old, active_ws, k_sim, cfg, opts=(), carried=_NONE):
        """The run*_from family: the carried state (x, rho, U_old, active_ws, then ``carried``)
        goes in and out, staged and copied back where it is not in the ABI layout."""
        cfg = cfg or self.config
        N, Bn = cfg.N, x.shape[1]
        state = [be.arg(x, (2, Bn), name="x"), be.arg(rho, (3 * N, Bn), name="rho"),
                 be.arg(U_old, (N, Bn), name="U_old"), be.arg(active_ws, (2 * (N + 1), Bn), be.i32, "active_ws")]
        state += self._carried_args(be, carried, opts, Bn)
        self._need_run_from()
        if "u_queue" in carried:
            self._need_input_delay("ntm_mpc_run_dly")
        out = self._run_out(be, k_sim, N, Bn, dk="d_hat" in carried, est="x_hat" in carried, dly="u_queue" in carried)
        self._call(be, entry, cfg, opts, (Bn, k_sim), (*[a for a, _ in state], *out.values()))
        for dst, (src, staged) in zip((x, rho, U_old, active_ws, *carried.values()), state):
            if staged:
                be.copy_back(dst, src)
        return out

    # ------------------------------------------------------------ hot path
    def initial_state(self, x0: torch.Tensor, cfg: Config | None = None):
        """Rho = repmat(rho(x0), 1, N) (NTM_MPC_Sim.m:63-65); U_old = +inf (D14)."""
        return self._initial_state(self._dev, x0, cfg)

    def initial_state_host(self, x0: np.ndarray, cfg: Config | None = None):
        """ntm_mpc_init with host arrays (the MEX path)."""
        return self._initial_state(_HOST, x0, cfg)

    def new_active_ws(self, B: int, cfg: Config | None = None) -> torch.Tensor:
        """Empty warm-start workspace for step(..., active_ws=): (2(N+1), B) int32 of -1."""
        cfg = cfg or self.config
        return self._empty(2 * (cfg.N + 1), B, dtype=torch.int32).fill_(-1)

    def step(self, x_k: torch.Tensor, rho: torch.Tensor, U_old: torch.Tensor, cfg: Config | None = None,
             out: dict | None = None, active_ws: torch.Tensor | None = None):
        """One MPC time step for a batch (NTM_MPC_Sim.m:94-130).  ``rho`` (3N, B) and
        ``U_old`` (N, B) are updated in place.  ``active_ws`` (see new_active_ws)
        carries the last two active sets from step to step as verified warm
        starts (ntm_mpc_step_ws_device).  Returns dict U, x_pred, x_next,
        exitflag, inner_iters (all CUDA tensors); ``out`` (a dict this method
        returned earlier) is reused."""
        return self._step(self._dev, "step_ws", x_k, rho, U_old, cfg, active_ws, out=out)

    def run(self, x0: torch.Tensor, k_sim: int = 20, cfg: Config | None = None):
        """Closed loop NTM_MPC_Sim.m:80-131 on device.  Returns the workspace
        variables xk (2(k_sim+1), B), uk (k_sim, B), Uk (N k_sim, B), wpred
        ((N+1) k_sim, B), exitflag / inner_iters (k_sim, B)."""
        return self._run(self._dev, "run", x0, k_sim, cfg)

    # ------------------------------------------------------------ host-buffer entry points (the MEX path)
    def step_host(self, x_k: np.ndarray, rho: np.ndarray, U_old: np.ndarray, cfg: Config | None = None,
                  active_ws: np.ndarray | None = None):
        """ntm_mpc_step with host (NumPy fp64) arrays, as a MEX gateway calls it:
        the library stages through its own device buffers.  ``rho`` and
        ``U_old`` (and ``active_ws``) are updated in place."""
        return self._step(_HOST, "step_ws", x_k, rho, U_old, cfg, active_ws)

    def run_host(self, x0: np.ndarray, k_sim: int = 20, cfg: Config | None = None):
        """ntm_mpc_run with host arrays (NTM_MPC_Sim.m:80-131 for a batch)."""
        return self._run(_HOST, "run", x0, k_sim, cfg)

    # ------------------------------------------------------------ function level
    def rho(self, x: torch.Tensor, cfg: Config | None = None, physics: Physics | None = None):
        """rho1.m / rho2.m / rho3.m at x (2, B) -> (3, B) (``physics`` overrides w_marg / w_dep)."""
        Bn = x.shape[1]
        x, _ = _dev_arg(x, (2, Bn), name="x")
        out = self._empty(3, Bn)
        ph = physics or self.physics
        self._raise(self.lib.ntm_rho_device(self._ctx, C.byref(ph.to_c()), C.byref(self._cfg(cfg)), Bn,
                                            _ptr(x), _ptr(out), self._stream()), "ntm_rho_device")
        return out

    def AB(self, rho: torch.Tensor, cfg: Config | None = None):
        """A.m / B.m at rho (3, B) -> A (4, B) col-major 2x2, B (2, B) column (D5)."""
        Bn = rho.shape[1]
        rho, _ = _dev_arg(rho, (3, Bn), name="rho")
        A, Bv = self._empty(4, Bn), self._empty(2, Bn)
        self._raise(self.lib.ntm_AB_device(self._ctx, C.byref(self.physics.to_c()), C.byref(self._cfg(cfg)), Bn,
                                           _ptr(rho), _ptr(A), _ptr(Bv), self._stream()), "ntm_AB_device")
        return A, Bv

    def lift(self, rho: torch.Tensor, cfg: Config | None = None):
        """Rho_to_PhiGammaLambda.m: rho (3N, B) -> Phi (4N, B), Gamma (2N*N, B), Lambda (2N, B)."""
        cfg = cfg or self.config
        N, Bn = cfg.N, rho.shape[1]
        rho, _ = _dev_arg(rho, (3 * N, Bn), name="rho")
        Phi, Gam, Lam = self._empty(4 * N, Bn), self._empty(2 * N * N, Bn), self._empty(2 * N, Bn)
        self._raise(self.lib.ntm_lift_device(self._ctx, C.byref(self.physics.to_c()), C.byref(cfg.to_c()), Bn,
                                             _ptr(rho), _ptr(Phi), _ptr(Gam), _ptr(Lam), self._stream()),
                    "ntm_lift_device")
        return Phi, Gam, Lam

    def cost(self, rho: torch.Tensor, x_k: torch.Tensor, cfg: Config | None = None):
        """NTM_MPC_Sim.m:120-121 -> G (N*N, B), F (N, B)."""
        cfg = cfg or self.config
        N, Bn = cfg.N, rho.shape[1]
        rho, _ = _dev_arg(rho, (3 * N, Bn), name="rho")
        x_k, _ = _dev_arg(x_k, (2, Bn), name="x_k")
        G, F = self._empty(N * N, Bn), self._empty(N, Bn)
        self._raise(self.lib.ntm_cost_device(self._ctx, C.byref(self.physics.to_c()), C.byref(cfg.to_c()), Bn,
                                             _ptr(rho), _ptr(x_k), _ptr(G), _ptr(F), self._stream()),
                    "ntm_cost_device")
        return G, F

    def getWLc(self, rho: torch.Tensor, cfg: Config | None = None):
        """getWLc.m -> W (2m, B), L (m*N, B), c (m, B), m = 6N+4 (column-major per scenario)."""
        cfg = cfg or self.config
        N, Bn = cfg.N, rho.shape[1]
        m = 6 * N + 4
        rho, _ = _dev_arg(rho, (3 * N, Bn), name="rho")
        W, Lm, c = self._empty(2 * m, Bn), self._empty(m * N, Bn), self._empty(m, Bn)
        self._raise(self.lib.ntm_getwlc_device(self._ctx, C.byref(self.physics.to_c()), C.byref(cfg.to_c()), Bn,
                                               _ptr(rho), _ptr(W), _ptr(Lm), _ptr(c), self._stream()),
                    "ntm_getwlc_device")
        return W, Lm, c

    def _qp_args(self, H, f, Lin, b):
        N, Bn = f.shape
        m = 0 if Lin is None else b.shape[0]
        H, _ = _dev_arg(H, (N * N, Bn), name="H")
        f, _ = _dev_arg(f, (N, Bn), name="f")
        if m:
            Lin, _ = _dev_arg(Lin, (m * N, Bn), name="A")
            b, _ = _dev_arg(b, (m, Bn), name="b")
        return N, Bn, m, H, f, (Lin if m else None), (b if m else None)

    def quadprog(self, H: torch.Tensor, f: torch.Tensor, Lin: torch.Tensor | None, b: torch.Tensor | None):
        """quadprog(H, f, A, b) for a batch: min 1/2 U'HU + f'U s.t. Lin U <= b.
        H (N*N, B), f (N, B), Lin (m*N, B) column-major per scenario, b (m, B).
        Returns (U (N, B), exitflag (B,), iterations (B,)); exitflag as quadprog
        (1 optimal, 0 max iterations, -2 infeasible -> U = 0, -7 non-finite)."""
        N, Bn, m, H, f, Lin, b = self._qp_args(H, f, Lin, b)
        U = self._empty(N, Bn)
        flag = self._empty(Bn, dtype=torch.int32)
        its = self._empty(Bn, dtype=torch.int32)
        self._raise(self.lib.ntm_qp_device(self._ctx, Bn, N, m, _ptr(H), _ptr(f), _ptr(Lin), _ptr(b), _ptr(U),
                                           _ptr(flag), _ptr(its), self._stream()), "ntm_qp_device")
        return U, flag, its

    def quadprog_mixed(self, H: torch.Tensor, f: torch.Tensor, Lin: torch.Tensor | None, b: torch.Tensor | None):
        """Config 5's fp32 leg (ntm_qp_mixed_device; not the fp64 product path): the QP
        solved in fp32 on fp32-rounded data, its active set then re-solved exactly in
        fp64 and certified (fp64 fallback otherwise).  Returns (U refined (N, B),
        U32 fp32 solution (N, B), exitflag (B,), info (B,) bit 0 certified / bit 1
        fp64 fallback / bit 2 fp32 not optimal, fp32 GI iterations (B,))."""
        N, Bn, m, H, f, Lin, b = self._qp_args(H, f, Lin, b)
        U, U32 = self._empty(N, Bn), self._empty(N, Bn)
        flag, info, its = (self._empty(Bn, dtype=torch.int32) for _ in range(3))
        self._raise(self.lib.ntm_qp_mixed_device(self._ctx, Bn, N, m, _ptr(H), _ptr(f), _ptr(Lin), _ptr(b), _ptr(U),
                                                 _ptr(U32), _ptr(flag), _ptr(info), _ptr(its), self._stream()),
                    "ntm_qp_mixed_device")
        return U, U32, flag, info, its

    # ------------------------------------------------------------ multipliers and the KKT audit
    def quadprog_dual(self, H: torch.Tensor, f: torch.Tensor, Lin: torch.Tensor | None, b: torch.Tensor | None):
        """[x, fval, exitflag, output, lambda] = quadprog(H, f, A, b) for a batch
        (ntm_qp_dual_device).  Returns (U (N, B), fval (B,), exitflag (B,),
        iterations (B,), lambda (m, B)): U, exitflag and iterations are quadprog()'s
        bit for bit; lambda is quadprog's lambda.ineqlin (>= 0, one entry per row
        of A, zero on inactive rows and wherever exitflag != 1); fval =
        1/2 U'HU + f'U at the returned U."""
        N, Bn, m, H, f, Lin, b = self._qp_args(H, f, Lin, b)
        U, lam, fval = self._empty(N, Bn), self._empty(m, Bn), self._empty(Bn)
        flag = self._empty(Bn, dtype=torch.int32)
        its = self._empty(Bn, dtype=torch.int32)
        self._raise(self.lib.ntm_qp_dual_device(self._ctx, Bn, N, m, _ptr(H), _ptr(f), _ptr(Lin), _ptr(b), _ptr(U),
                                                _ptr(flag), _ptr(its), _ptr(lam) if m else None, _ptr(fval),
                                                self._stream()), "ntm_qp_dual_device")
        return U, fval, flag, its, lam

    def kkt(self, H: torch.Tensor, f: torch.Tensor, Lin: torch.Tensor | None, b: torch.Tensor | None,
            U: torch.Tensor, lam: torch.Tensor | None):
        """The KKT audit of (U, lambda) on explicit QP data (ntm_qp_kkt_device):
        (4, B) = stationarity, primal, dual, complementarity in the solver's scaled
        units (include/ntm_mpc.h); NaN for a scenario with non-finite input."""
        N, Bn, m, H, f, Lin, b = self._qp_args(H, f, Lin, b)
        U, _ = _dev_arg(U, (N, Bn), name="U")
        if m:
            lam, _ = _dev_arg(lam, (m, Bn), name="lam")
        out = self._empty(4, Bn)
        self._raise(self.lib.ntm_qp_kkt_device(self._ctx, Bn, N, m, _ptr(H), _ptr(f), _ptr(Lin), _ptr(b), _ptr(U),
                                               _ptr(lam) if m else None, _ptr(out), self._stream()),
                    "ntm_qp_kkt_device")
        return out

    def step_dual(self, x_k: torch.Tensor, rho: torch.Tensor, U_old: torch.Tensor, cfg: Config | None = None,
                  active_ws: torch.Tensor | None = None):
        """step() plus, in the returned dict, ``lambda`` (cfg.m, B): the multipliers of
        the step's last QP by row id (zero where its exit flag is not 1), and
        ``rho_qp`` (3N, B): the scheduling rho that QP was built from
        (ntm_mpc_step_dual_device).  Every horizon runs on the runtime-N kernels
        here, so U agrees with step() to the parity tolerances, not bit for bit."""
        return self._step(self._dev, "step_dual", x_k, rho, U_old, cfg, active_ws, dual=True)

    def step_dual_host(self, x_k: np.ndarray, rho: np.ndarray, U_old: np.ndarray, cfg: Config | None = None,
                       active_ws: np.ndarray | None = None):
        """ntm_mpc_step_dual with host arrays (the MEX path): step_host plus ``lambda``
        and ``rho_qp``."""
        return self._step(_HOST, "step_dual", x_k, rho, U_old, cfg, active_ws, dual=True)

    # ------------------------------------------------------------ plant-model mismatch, disturbance estimate
    def step_obs(self, x_k: torch.Tensor, rho: torch.Tensor, U_old: torch.Tensor, d_hat: torch.Tensor,
                 obs: Observer, cfg: Config | None = None, active_ws: torch.Tensor | None = None):
        """step() with the observer (ntm_mpc_step_obs_device): the model is the nominal
        plasma under ``obs.nominal_model`` and carries the disturbance estimate
        ``d_hat`` (2, B), which is updated in place like ``rho`` and ``U_old`` and
        also returned as ``d_hat`` in the dict.  Every horizon runs on the runtime-N
        kernels here, as for step_dual."""
        return self._step(self._dev, "step_obs", x_k, rho, U_old, cfg, active_ws, (obs,), {"d_hat": d_hat})

    def step_obs_host(self, x_k: np.ndarray, rho: np.ndarray, U_old: np.ndarray, d_hat: np.ndarray, obs: Observer,
                      cfg: Config | None = None, active_ws: np.ndarray | None = None):
        """ntm_mpc_step_obs with host arrays (the MEX path): step_host with the observer;
        ``d_hat`` (2, B) is updated in place and returned as ``d_hat``."""
        return self._step(_HOST, "step_obs", x_k, rho, U_old, cfg, active_ws, (obs,), {"d_hat": d_hat})

    def run_obs(self, x0: torch.Tensor, obs: Observer, k_sim: int = 20, cfg: Config | None = None,
                d0: torch.Tensor | None = None):
        """run() with the observer (ntm_mpc_run_obs_device), d_hat kept on chip.  ``d0``
        (2, B) is the initial estimate (None: zeros).  Returns run()'s dict plus ``dk``
        (2(k_sim+1), B): column 0 is d0, column k+1 the estimate after step k."""
        return self._run(self._dev, "run_obs", x0, k_sim, cfg, (obs,), {"d0": d0})

    def run_obs_host(self, x0: np.ndarray, obs: Observer, k_sim: int = 20, cfg: Config | None = None,
                     d0: np.ndarray | None = None):
        """ntm_mpc_run_obs with host arrays: run_host with the observer, plus ``dk``."""
        return self._run(_HOST, "run_obs", x0, k_sim, cfg, (obs,), {"d0": d0})

    # ------------------------------------------------------------ measurement noise, filtered state estimate
    def step_est(self, x_k: torch.Tensor, rho: torch.Tensor, U_old: torch.Tensor, d_hat: torch.Tensor,
                 x_hat: torch.Tensor, est: Estimator, cfg: Config | None = None,
                 active_ws: torch.Tensor | None = None):
        """step_obs() with output feedback (ntm_mpc_step_est_device): the controller plans
        from the estimate ``x_hat`` (2, B) while the plant steps from its true state
        ``x_k``; ``x_hat`` and ``d_hat`` are updated in place from the noisy measurement
        ``y`` of ``x_next`` and are also returned in the dict, with ``y``."""
        return self._step(self._dev, "step_est", x_k, rho, U_old, cfg, active_ws, (est,),
                          {"d_hat": d_hat, "x_hat": x_hat})

    def step_est_host(self, x_k: np.ndarray, rho: np.ndarray, U_old: np.ndarray, d_hat: np.ndarray,
                      x_hat: np.ndarray, est: Estimator, cfg: Config | None = None,
                      active_ws: np.ndarray | None = None):
        """ntm_mpc_step_est with host arrays (the MEX path): ``d_hat`` and ``x_hat`` (2, B)
        are updated in place and returned in the dict, with the measurement ``y``."""
        return self._step(_HOST, "step_est", x_k, rho, U_old, cfg, active_ws, (est,),
                          {"d_hat": d_hat, "x_hat": x_hat})

    def run_est(self, x0: torch.Tensor, est: Estimator, k_sim: int = 20, cfg: Config | None = None,
                d0: torch.Tensor | None = None, xhat0: torch.Tensor | None = None):
        """run_obs() with output feedback (ntm_mpc_run_est_device): x, x_hat and d_hat stay
        on chip.  ``xhat0`` (2, B) is the initial estimate (None: x0).  Returns run_obs()'s
        dict plus ``xhk`` (2(k_sim+1), B), column 0 the initial estimate, and ``yk``
        (2 k_sim, B), the measurements."""
        return self._run(self._dev, "run_est", x0, k_sim, cfg, (est,), {"d0": d0, "xhat0": xhat0})

    def run_est_host(self, x0: np.ndarray, est: Estimator, k_sim: int = 20, cfg: Config | None = None,
                     d0: np.ndarray | None = None, xhat0: np.ndarray | None = None):
        """ntm_mpc_run_est with host arrays: run_obs_host with the estimator, plus ``xhk``
        and ``yk``."""
        return self._run(_HOST, "run_est", x0, k_sim, cfg, (est,), {"d0": d0, "xhat0": xhat0})

    # ------------------------------------------------------------ resumable closed loops
    def run_from(self, x: torch.Tensor, rho: torch.Tensor, U_old: torch.Tensor, active_ws: torch.Tensor,
                 k_sim: int = 20, cfg: Config | None = None):
        """run() from a carried state (ntm_mpc_run_from_device): ``x`` (2, B), ``rho``
        (3N, B), ``U_old`` (N, B) and ``active_ws`` (2(N+1), B) int32 are updated in
        place to the state after the last step, so the next call (or step()) continues
        the loop; one call of k steps and any split of them give the same bits.  The
        first call takes initial_state() and new_active_ws().  An attached generator's
        ``k0`` is the caller's to advance between calls.  Returns run()'s dict; xk's
        column 0 is the input ``x``."""
        return self._run_from(self._dev, "run_from", x, rho, U_old, active_ws, k_sim, cfg)

    def run_from_host(self, x: np.ndarray, rho: np.ndarray, U_old: np.ndarray, active_ws: np.ndarray,
                      k_sim: int = 20, cfg: Config | None = None):
        """ntm_mpc_run_from with host arrays (the MEX path); the state arrays are
        updated in place."""
        return self._run_from(_HOST, "run_from", x, rho, U_old, active_ws, k_sim, cfg)

    def run_est_from(self, x: torch.Tensor, rho: torch.Tensor, U_old: torch.Tensor, active_ws: torch.Tensor,
                     d_hat: torch.Tensor, x_hat: torch.Tensor, est: Estimator, k_sim: int = 20,
                     cfg: Config | None = None):
        """run_est() from a carried state (ntm_mpc_run_est_from_device): run_from() with
        the estimator's ``d_hat`` and ``x_hat`` (2, B) carried too, all updated in place.
        With sigma_y = 0, kappa = 0, equal gains and x_hat == x it continues run_obs()
        bit for bit.  Returns run_est()'s dict."""
        return self._run_from(self._dev, "run_est_from", x, rho, U_old, active_ws, k_sim, cfg, (est,),
                              {"d_hat": d_hat, "x_hat": x_hat})

    def run_est_from_host(self, x: np.ndarray, rho: np.ndarray, U_old: np.ndarray, active_ws: np.ndarray,
                          d_hat: np.ndarray, x_hat: np.ndarray, est: Estimator, k_sim: int = 20,
                          cfg: Config | None = None):
        """ntm_mpc_run_est_from with host arrays; the state arrays are updated in place."""
        return self._run_from(_HOST, "run_est_from", x, rho, U_old, active_ws, k_sim, cfg, (est,),
                              {"d_hat": d_hat, "x_hat": x_hat})

    # ------------------------------------------------------------ actuator dead time
    def step_dly(self, x_k: torch.Tensor, rho: torch.Tensor, U_old: torch.Tensor, d_hat: torch.Tensor,
                 x_hat: torch.Tensor, u_queue: torch.Tensor | None, est: Estimator, dly: Delay,
                 cfg: Config | None = None, active_ws: torch.Tensor | None = None):
        """step_est() with an actuator dead time (ntm_mpc_step_dly_device): the plant applies
        ``u_queue[0]`` (the input commanded dly.steps steps ago) and the controller plans from
        ``x_plan``, x_hat carried over the queued inputs by its model (dly.predict; else
        x_hat).  ``u_queue`` (steps, B) is shifted in place and takes the new command
        ``U[0]`` at its end (None is allowed when steps == 0).  Returns step_est()'s dict
        plus ``x_plan`` (2, B), ``u_applied`` (B,) and ``u_queue``.  With steps == 0 it is
        step_est() bit for bit."""
        self._need_input_delay("ntm_mpc_step_dly")
        return self._step(self._dev, "step_dly", x_k, rho, U_old, cfg, active_ws, (est, dly),
                          {"d_hat": d_hat, "x_hat": x_hat, "u_queue": u_queue})

    def step_dly_host(self, x_k: np.ndarray, rho: np.ndarray, U_old: np.ndarray, d_hat: np.ndarray,
                      x_hat: np.ndarray, u_queue: np.ndarray | None, est: Estimator, dly: Delay,
                      cfg: Config | None = None, active_ws: np.ndarray | None = None):
        """ntm_mpc_step_dly with host arrays (the MEX path): ``d_hat``, ``x_hat`` and
        ``u_queue`` are updated in place and returned in the dict."""
        self._need_input_delay("ntm_mpc_step_dly")
        return self._step(_HOST, "step_dly", x_k, rho, U_old, cfg, active_ws, (est, dly),
                          {"d_hat": d_hat, "x_hat": x_hat, "u_queue": u_queue})

    def run_dly(self, x0: torch.Tensor, est: Estimator, dly: Delay, k_sim: int = 20, cfg: Config | None = None,
                d0: torch.Tensor | None = None, xhat0: torch.Tensor | None = None, uq0: torch.Tensor | None = None):
        """run_est() with an actuator dead time (ntm_mpc_run_dly_device): the queue of
        pending inputs stays on chip with x, x_hat and d_hat.  ``uq0`` (steps, B) is the
        initial queue (None: zeros, power off until the first command arrives).  Returns
        run_est()'s dict plus ``uak`` (k_sim, B), the applied input (``uk`` stays the
        commanded U[0]: uak[k + steps] == uk[k]), and ``xpk`` (2 k_sim, B), the plan state."""
        return self._run(self._dev, "run_dly", x0, k_sim, cfg, (est, dly), {"d0": d0, "xhat0": xhat0, "uq0": uq0})

    def run_dly_host(self, x0: np.ndarray, est: Estimator, dly: Delay, k_sim: int = 20, cfg: Config | None = None,
                     d0: np.ndarray | None = None, xhat0: np.ndarray | None = None, uq0: np.ndarray | None = None):
        """ntm_mpc_run_dly with host arrays: run_est_host with the dead time, plus ``uak``
        and ``xpk``."""
        return self._run(_HOST, "run_dly", x0, k_sim, cfg, (est, dly), {"d0": d0, "xhat0": xhat0, "uq0": uq0})

    def run_dly_from(self, x: torch.Tensor, rho: torch.Tensor, U_old: torch.Tensor, active_ws: torch.Tensor,
                     d_hat: torch.Tensor, x_hat: torch.Tensor, u_queue: torch.Tensor | None, est: Estimator,
                     dly: Delay, k_sim: int = 20, cfg: Config | None = None):
        """run_dly() from a carried state (ntm_mpc_run_dly_from_device): run_est_from() with
        the queue ``u_queue`` (steps, B) carried too, all updated in place; one call of k
        steps and any split of them give the same bits.  ``dly.steps`` must not change
        between the chunks of one loop.  Returns run_dly()'s dict."""
        return self._run_from(self._dev, "run_dly_from", x, rho, U_old, active_ws, k_sim, cfg, (est, dly),
                              {"d_hat": d_hat, "x_hat": x_hat, "u_queue": u_queue})

    def run_dly_from_host(self, x: np.ndarray, rho: np.ndarray, U_old: np.ndarray, active_ws: np.ndarray,
                          d_hat: np.ndarray, x_hat: np.ndarray, u_queue: np.ndarray | None, est: Estimator,
                          dly: Delay, k_sim: int = 20, cfg: Config | None = None):
        """ntm_mpc_run_dly_from with host arrays; the state arrays are updated in place."""
        return self._run_from(_HOST, "run_dly_from", x, rho, U_old, active_ws, k_sim, cfg, (est, dly),
                              {"d_hat": d_hat, "x_hat": x_hat, "u_queue": u_queue})

    def step_kkt(self, x_k: torch.Tensor, rho_qp: torch.Tensor, U: torch.Tensor, lam: torch.Tensor | None,
                 cfg: Config | None = None):
        """The KKT audit of an MPC step's own QP (ntm_mpc_kkt_device), rebuilt in the
        kernel from x_k (2, B) and rho_qp (3N, B) and never materialised: (4, B) as
        kkt().  ``lam`` (cfg.m, B) in the step's row order (step_dual)."""
        cfg = cfg or self.config
        N, Bn = cfg.N, x_k.shape[1]
        xk, _ = _dev_arg(x_k, (2, Bn), name="x_k")
        rq, _ = _dev_arg(rho_qp, (3 * N, Bn), name="rho_qp")
        U, _ = _dev_arg(U, (N, Bn), name="U")
        if cfg.m:
            lam, _ = _dev_arg(lam, (cfg.m, Bn), name="lam")
        out = self._empty(4, Bn)
        self._raise(self.lib.ntm_mpc_kkt_device(self._ctx, C.byref(self.physics.to_c()), C.byref(cfg.to_c()), Bn,
                                                _ptr(xk), _ptr(rq), _ptr(U), _ptr(lam) if cfg.m else None, _ptr(out),
                                                self._stream()), "ntm_mpc_kkt_device")
        return out


def scenarios_x0(first_id: int, B: int, seed: int = 20241220):
    """Synthetic initial states for global ids first_id..first_id+B-1:
    (2, B) float64 numpy array in the ABI layout (each scenario's [w, omega] contiguous)."""
    x0 = _host_empty(2, B)
    L.load().ntm_scenarios_x0(C.c_uint64(seed), first_id, B, x0.ctypes.data_as(C.POINTER(C.c_double)))
    return x0


# ---- MATLAB-named thin wrappers (reference function names) ----------------

_default = None


def _ctl():
    global _default
    if _default is None:
        _default = NtmMpc()
    return _default


def _phys_with(**kw):
    ph = _ctl().physics
    kw = {k: float(v) for k, v in kw.items() if v is not None}
    return dataclasses.replace(ph, **kw) if kw else ph


def rho1(x, wmarg=None):
    """rho1.m (batched): rho1(x, wmarg) = 1/(x(1) + wmarg^2), x (2, B) CUDA -> (B,).
    ``wmarg`` defaults to the controller's physics (NTM_MPC_Sim.m:7)."""
    return _ctl().rho(x, physics=_phys_with(w_marg=wmarg))[0]


def rho2(x):
    """rho2.m (batched): x(1)^2 / x(2)."""
    return _ctl().rho(x)[1]


def rho3(x, w_dep=None):
    """rho3.m (batched): rho3(x, w_dep); ``w_dep`` defaults to the controller's physics (:6)."""
    return _ctl().rho(x, physics=_phys_with(w_dep=w_dep))[2]


def Rho_to_PhiGammaLambda(Rho1, Rho2, Rho3, cfg: Config | None = None):
    """Rho_to_PhiGammaLambda.m (batched): Rho1/2/3 (N, B) -> Phi, Gamma, Lambda."""
    rho = torch.stack([Rho1, Rho2, Rho3], dim=1).reshape(-1, Rho1.shape[1])
    return _ctl().lift(rho, cfg)


def quadprog(H, f, A=None, b=None):
    """quadprog stand-in (NTM_MPC_Sim.m:97)."""
    return _ctl().quadprog(H, f, A, b)


def NTM_MPC_Sim(x0, k_sim: int = 20, cfg: Config | None = None):
    """The driver NTM_MPC_Sim.m:80-131 for a batch of initial states x0 (2, B)."""
    return _ctl().run(x0, k_sim, cfg)
