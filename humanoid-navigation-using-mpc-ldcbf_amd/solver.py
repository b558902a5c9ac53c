"""Batched step solver: the Python face of the C ABI.  Tensors live on the GPU (torch is used
only to own device memory and streams); every call is asynchronous on torch's current stream."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib

STATUS_SOLVED, STATUS_MAX_ITER, STATUS_INFEASIBLE, STATUS_DEGENERATE, STATUS_UNCERTIFIED = 0, 1, 2, 3, 4
STATUS_SENSOR_OVERFLOW = 5     # a scan's clusters did not fit the obstacle slots: not solved (sense_plan_step, plan_step_batch_c_eta(overflow=)), robot stopped (fleet loop)
FLAG_INTERIOR = 1
FLAG_WARM_START = 2      # start every step from the previous step's shifted interior-point result (rollout; steps: set_warm_start)
FLAG_NO_PRESOLVE = 4     # keep the LDCBF rows the leg-reach rows make redundant in the solve (include/lipmpc.h)
_LIPMPC_E_UNSUPPORTED = -2


@dataclass
class LipMpcParams:
    """Constants of the step problem; defaults are the reference's config.yml:2-17 and
    HumanoidMpc.py:20-22,:200."""
    N: int = 3
    n_obs_max: int = 0
    v_max: int = 5
    max_iter: int = 60
    finish_rounds: int = 0      # 0 = library default (8 active-set rounds for N <= 8, else 16)
    flags: int = 0
    dt: float = 0.4
    g: float = 9.81
    h_com: float = 1.0
    alpha: float = 3.6
    l_max: tuple = (0.10, 0.10)
    l_min: tuple = (-0.1, -0.1)
    v_min: tuple = (-0.1, 0.1)
    v_max_xy: tuple = (0.8, 0.4)
    omega_max: float = 0.156 * math.pi
    ell: float = 0.05
    sampling_time: float = 0.4
    tol: float = 1e-11
    tol_interior: float = 1e-9
    k0_tol: float = 1e-5

    def to_c(self):
        p = _lib.LipmpcParamsC()
        for f in ("N", "n_obs_max", "v_max", "max_iter", "flags", "finish_rounds"):
            setattr(p, f, int(getattr(self, f)))
        for f in ("dt", "g", "h_com", "alpha", "omega_max", "ell", "sampling_time", "tol", "tol_interior", "k0_tol"):
            setattr(p, f, float(getattr(self, f)))
        for f in ("l_max", "l_min", "v_min", "v_max_xy"):
            v = getattr(self, f)
            setattr(p, f, (C.c_double * 2)(float(v[0]), float(v[1])))
        return p

    @property
    def num_rows(self):
        return 9 * self.N + (self.N + 1) * self.n_obs_max

    @property
    def active_words(self):
        return (self.num_rows + 63) // 64


def _check(t, shape, dtype, device, name, required=False):
    """A buffer whose raw pointer goes to a kernel: a contiguous ``dtype`` tensor of ``shape`` on ``device``, or None when
    not ``required``; anything else is a ValueError naming it."""
    if t is None:
        if required:
            raise ValueError(f"{name} is required")
        return
    if t.shape != shape or t.dtype != dtype or t.device != device or not t.is_contiguous():
        raise ValueError(f"{name}: expected contiguous {dtype} {shape} on {device}, got {t.dtype} {tuple(t.shape)} on {t.device}")


# A buffer family is one shape table next to the class that owns it -- a function of B and the owner's sizes that returns
# name (the C ABI's parameter name) -> (dtype, shape, required) -- which allocation and checking both read.
def _alloc(table, names, device, new=torch.empty):
    return {k: new(table[k][1], dtype=table[k][0], device=device) for k in names}


def _check_table(table, bufs, device, what):
    """Caller-supplied buffers of a family: every required one present, every one given as ``_check`` wants it (whose test is
    repeated here: this runs per buffer on every launch, and only a failure needs the call and the buffer's name)."""
    for k, (dtype, shape, required) in table.items():
        t = bufs.get(k)
        if t is None:
            if required and k not in bufs:
                raise ValueError(f"{what}['{k}'] missing")
        elif t.shape != shape or t.dtype != dtype or t.device != device or not t.is_contiguous():
            _check(t, shape, dtype, device, f"{what}['{k}']")


def _named(bufs, names):
    """``bufs``' entries under ``names`` as keyword arguments of _lib.call (an optional buffer that is absent: None = NULL)."""
    return {k: bufs.get(k) for k in names}


def step_outputs(B, P):
    """Outputs of a step of a handle with the LipMpcParams ``P``, in the order alloc_outputs returns them."""
    f64, i32, i64, words = torch.float64, torch.int32, torch.int64, P.active_words
    return {"U": (f64, (B, P.N, 2), True), "X": (f64, (B, P.N + 1, 4), True), "theta": (f64, (B, P.N + 1), True),
            "omega": (f64, (B, P.N), True), "obj": (f64, (B,), True), "status": (i32, (B,), True), "iters": (i32, (B,), True),
            "active": (i64, (B, words), True), "c_eta": (f64, (B, P.n_obs_max, 4), False),
            "diag": (f64, (B, _lib.DIAG_WORDS), False), "working": (i64, (B, words), False)}


def fleet_state(B, k_max):
    """State of a host-driven fleet loop of at most ``k_max`` samples (fleet_update)."""
    f64, i32, i8 = torch.float64, torch.int32, torch.int8
    return {"state": (f64, (B, 5), True), "first_foot": (i8, (B,), True), "walking": (i8, (B,), True), "last_obj": (f64, (B,), True),
            "n_steps": (i32, (B,), True), "last_status": (i32, (B,), True), "n_overflow": (i32, (B,), True), "sample": (i32, (1,), True),
            "X_pred": (f64, (B, k_max + 1, 5), True), "U_pred": (f64, (B, k_max, 3), True)}


def recover_state(B):
    """The recovery counters of a fleet loop (fleet_update(..., recover=)): consecutive recovery samples, their total, and the
    safety margin of the last call (NaN where the safety test was not evaluated)."""
    f64, i32 = torch.float64, torch.int32
    return {"recover_run": (i32, (B,), True), "n_recover": (i32, (B,), True), "recover_margin": (f64, (B,), True)}


def rollout_outputs(B, k_max):
    """Outputs of the on-device closed loop of at most ``k_max`` samples (rollout)."""
    f64, i32 = torch.float64, torch.int32
    return {"X_pred": (f64, (B, k_max + 1, 5), True), "U_pred": (f64, (B, k_max, 3), True), "n_steps": (i32, (B,), True),
            "last_status": (i32, (B,), True), "total_iters": (i32, (B,), True)}


STEP_OUTPUTS, FLEET_STATE = tuple(step_outputs(0, LipMpcParams())), tuple(fleet_state(0, 0))             # the names
RECOVER_STATE = tuple(recover_state(0))
_STEP_OUTPUTS_GIVEN_C_ETA = tuple(k for k in STEP_OUTPUTS if k != "c_eta")      # the entry points that take the half-spaces as input


class BatchedLipMpc:
    """One handle = one (device, parameter set).  ``plan_step_batch`` solves B independent MPC
    steps; ``advance`` applies the reference's state update to the states in place."""

    def __init__(self, params: LipMpcParams, device: int | None = None):
        if not torch.cuda.is_available():
            raise RuntimeError("lipmpc needs a HIP device (torch.cuda.is_available() is False); there is no CPU path")
        self.lib = _lib.load()
        self.params = params
        self.device_index = torch.cuda.current_device() if device is None else int(device)
        self.device = torch.device("cuda", self.device_index)
        self._h = C.c_void_p()
        cp = params.to_c()
        _lib.check(self.lib.lipmpc_create(C.byref(cp), self.device_index, C.byref(self._h)), "lipmpc_create")
        # split launch (one kernel per solver body): the library says whether this handle's steps can use it
        self.auto_workspace = True
        self._ws, self._ws_cap = None, 0           # the workspace registered last
        self._ws_by_stream = {}                    # stream -> (workspace, capacity) of the eager launches on it: grow-only
        self._kept = {}                            # address -> every buffer ever registered with the library (_register)
        self._sched = None
        self._side_streams = False                 # the library made its side streams / events (first workspace registered)
        self._split_capable = int(self.lib.lipmpc_workspace_bytes(self._h, 1)) > 0
        self._warm, self._warm_cap = None, 0
        self.warm_words = int(self.lib.lipmpc_warm_words(C.byref(cp)))

    def _register(self, setter, capacity, **buffer):
        """Hand a buffer, under the setter's parameter name, to lipmpc_set_schedule / _set_workspace / _set_warm_start.  Whatever
        the library has accepted the handle keeps for as long as it lives: a captured graph may hold the pointer."""
        _lib.call(setter, h=self._h, capacity=capacity, **buffer)
        self._kept.update((b.data_ptr(), b) for b in buffer.values() if b is not None)

    def set_warm_start(self, capacity):
        """Warm-start records for this handle's step launches (lipmpc_set_warm_start): allocates a zeroed
        [capacity, warm_words] float64 record and registers it.  Every later plan_step_batch / plan_step_batch_c_eta /
        LidarSensor.sense_plan_step of at most ``capacity`` problems starts problem b from its record, shifted by one stage,
        and writes its own interior-point result back (word 0 = 1.0 after a SOLVED / UNCERTIFIED step, else 0.0: the next
        step starts cold).  Needs FLAG_WARM_START (ValueError otherwise).  Returns False, and registers nothing, where the
        library does not support it (N = 1, more than 14 obstacle slots, N > 8 with more than 4).  Grow-only: a capacity at or below the current
        one keeps the record; a larger one is refused while a graph is being captured (the graph holds the pointer)."""
        capacity = int(capacity)
        if not self.params.flags & FLAG_WARM_START:
            raise ValueError("set_warm_start needs a handle with FLAG_WARM_START (a warm solve keeps every row)")
        if capacity <= self._warm_cap:
            return True
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("set_warm_start: cannot grow the warm-start record while a graph is being captured")
        rec = torch.zeros((capacity, self.warm_words), dtype=torch.float64, device=self.device)
        try:
            self._register("lipmpc_set_warm_start", capacity, record=rec)
        except RuntimeError as e:
            if getattr(e, "code", None) != _LIPMPC_E_UNSUPPORTED:
                raise
            return False
        self._warm, self._warm_cap = rec, capacity
        return True

    @property
    def warm_record(self):
        """The registered [capacity, warm_words] warm-start record (include/lipmpc.h: word 0 = 1.0 when it holds a result,
        then q [2N] and z [num_rows] of the interior-point phase), or None."""
        return self._warm

    def reset_warm_start(self, mask=None):
        """Next step of all robots (mask None) or of the robots where ``mask`` [capacity] is true starts cold: zeroes
        word 0 of their records (respawned robots).  Asynchronous on the current stream."""
        if self._warm is None:
            return
        if mask is None:
            self._warm[:, 0].zero_()
        else:
            self._warm[:, 0].masked_fill_(torch.as_tensor(mask, device=self.device).to(torch.bool), 0.0)

    def _check_warm(self, B):
        if self._warm is not None and B > self._warm_cap:
            raise ValueError(f"batch of {B} problems > the warm-start record's capacity {self._warm_cap}")

    def set_workspace(self, capacity):
        """Split launch of this handle's step solves (lipmpc_set_workspace): for 32-lane problems (N > 8) in the exact mode
        the step runs as classification -> index lists -> one kernel per solver body (each with its own register
        allocation); same optimum and active sets as the single kernel, a status may differ only between SOLVED and UNCERTIFIED
        (a problem may run in another body there: last-bit differences).  The workspace holds one launch's class keys and
        lists, so two launches must never share one unless they are ordered.
        By default (``auto_workspace``) the handle manages this itself and this call is not needed: every step launch
        registers, right before its C call, a workspace of its own stream (grow-only per stream), and a launch being captured
        in a graph gets one of its own that no other launch or graph uses -- launches on different streams, graph replays and
        eager launches may then overlap freely (they share the handle's side streams, which only orders them).
        An explicit call registers ONE workspace of ``capacity`` problems (0 = back to the single dispatching kernel); with
        ``auto_workspace = False`` it stays registered, and the caller takes over the C contract: every step launch of the handle
        uses it, on any stream, so all of them -- graph replays included -- must be ordered on one stream.  Buffers the handle
        has registered are never freed while it lives (a captured graph may hold them); keep the handle alive as long as its
        graphs are replayed.  Refused (RuntimeError) while a graph is being captured before the handle's first workspace: the
        first one makes the handle's side streams and events."""
        capacity = int(capacity)
        ws = self._new_workspace(capacity)
        self._register_workspace(ws, capacity)

    def _new_workspace(self, capacity):
        """A workspace buffer of ``capacity`` problems, or None (not split-capable)."""
        nbytes = int(self.lib.lipmpc_workspace_bytes(self._h, capacity)) if capacity > 0 else 0
        if nbytes <= 0:
            return None
        if not self._side_streams and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("the first split launch (workspace) of a handle makes its side streams and events, which cannot "
                               "happen during a graph capture: run one step of the handle, or set_workspace, before capturing")
        return torch.empty((nbytes // 4,), dtype=torch.int32, device=self.device)

    def _register_workspace(self, ws, capacity):
        cap = capacity if ws is not None else 0
        self._register("lipmpc_set_workspace", cap, workspace=ws)
        self._ws, self._ws_cap = ws, cap
        self._side_streams = self._side_streams or ws is not None

    def _ensure_workspace(self, B):
        """Right before a step's C call (auto_workspace): register the workspace of the current stream, grown to B if needed,
        or, while a graph is being captured, a new one that belongs to this captured launch alone."""
        if not (self.auto_workspace and self._split_capable) or B < 1:
            return
        if torch.cuda.is_current_stream_capturing():
            self._register_workspace(self._new_workspace(B), B)
            return
        key = torch.cuda.current_stream(self.device).cuda_stream
        ws, cap = self._ws_by_stream.get(key, (None, 0))
        if B > cap:
            ws, cap = self._new_workspace(B), B
            self._ws_by_stream[key] = (ws, cap)
        self._register_workspace(ws, cap)

    def set_schedule(self, capacity):
        """Launch order for this handle's step solves (lipmpc_set_schedule): every plan_step_batch / plan_step_batch_c_eta of
        at most ``capacity`` problems leaves each problem's cost and the order -- costliest first, like with like -- the
        next launch of the same batch size places them in.  Pays off beyond the 4096 problems the GPU holds at once,
        when consecutive launches see the same or slowly moving problems; results never depend on it.  0 = off.
        One buffer for every launch of the handle, on any stream: launches with a schedule -- graph replays included -- must be
        ordered on one stream (the caller's to order, unlike the workspace).  A replaced buffer is kept while the handle lives
        (a graph captured with it still writes there)."""
        capacity = int(capacity)
        self._sched = (torch.zeros((int(self.lib.lipmpc_schedule_words(capacity)),), dtype=torch.int32, device=self.device)
                       if capacity > 0 else None)
        self._register("lipmpc_set_schedule", capacity, schedule=self._sched)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and C is not None:      # (C is None: interpreter shutdown)
            self.lib.lipmpc_destroy(h)
            self._h = None

    # ---- buffers --------------------------------------------------------------------------------
    def alloc_outputs(self, B, with_c_eta=False, with_diag=False, with_working=False):
        table, want = step_outputs(B, self.params), dict(c_eta=with_c_eta, diag=with_diag, working=with_working)
        return _alloc(table, [k for k, (_, _, required) in table.items() if required or want[k]], self.device)

    def _check_inputs(self, state, goal, first_foot, obs_xy, obs_nv, delta, need_obstacles=True):
        P, dev = self.params, self.device
        B = state.shape[0]
        _check(state, (B, 5), torch.float64, dev, "state", required=True)
        _check(goal, (B, 2), torch.float64, dev, "goal", required=True)
        _check(first_foot, (B,), torch.int8, dev, "first_foot", required=True)
        if P.n_obs_max > 0 and need_obstacles:
            _check(obs_xy, (B, P.n_obs_max, P.v_max, 2), torch.float64, dev, "obs_xy", required=True)
            _check(obs_nv, (B, P.n_obs_max), torch.int32, dev, "obs_nv", required=True)
        _check(delta, (B,), torch.float64, dev, "delta")
        return B

    # ---- the hot path -----------------------------------------------------------------------------
    def plan_step_batch(self, state, goal, first_foot, obs_xy=None, obs_nv=None, delta=None, out=None,
                        with_c_eta=False, with_diag=False, bounds=None, with_working=False):
        """state [B,5] (px,vx,py,vy,theta), goal [B,2], first_foot [B] int8 (+1 right / -1 left),
        obs_xy [B,n_obs_max,v_max,2] CCW rings, obs_nv [B,n_obs_max] int32, delta [B] or None,
        bounds [B,4] (V_MAX_x, V_MAX_y, ALPHA, OMEGA_MAX) per problem or None.
        Returns dict(U,X,theta,omega,obj,status,iters,active[,c_eta][,diag][,working]) of device tensors; results are
        valid once the current stream is synchronised.  ``active`` = the rows tight at the optimum (slack <= 1e-7: unique),
        ``working`` = the rows carrying a multiplier in the finish's certificate (include/lipmpc.h).
        Streams and graphs: launches of one handle on different streams need no ordering between them, and a step may be
        captured in a graph and replayed next to eager launches -- the split launch's workspace is per stream, and per captured
        launch (set_workspace; not with ``auto_workspace = False``).  The first split launch of a handle cannot be captured
        (RuntimeError, nothing enqueued): run one eagerly first.  What the caller orders: the schedule (set_schedule) and the
        warm-start records (set_warm_start) are one buffer per handle, so launches that use them must be ordered on one stream;
        inputs and outputs are the caller's as usual."""
        B = self._check_inputs(state, goal, first_foot, obs_xy, obs_nv, delta)
        _check(bounds, (B, 4), torch.float64, self.device, "bounds")
        if out is None:
            out = self.alloc_outputs(B, with_c_eta, with_diag, with_working)
        else:
            self._check_outputs(out, B)
        self._ensure_workspace(B)
        self._check_warm(B)
        _lib.call("lipmpc_plan_step_batch", h=self._h, B=B, state=state, goal=goal, first_foot=first_foot, delta=delta,
                  obs_xy=obs_xy, obs_nv=obs_nv, **_named(out, STEP_OUTPUTS), bounds=bounds,
                  hip_stream=torch.cuda.current_stream(self.device).cuda_stream)
        return out

    def plan_step_batch_c_eta(self, state, goal, first_foot, c_eta_in, delta=None, out=None, with_diag=False, bounds=None,
                              overflow=None, with_working=False):
        """The step with the LDCBF half-spaces given (lipmpc_plan_step_batch_c_eta): c_eta_in [B,n_obs_max,4] =
        (c_x, c_y, eta_x, eta_y) per slot, eta = (0,0) = empty slot; row j of stage k is eta_j.(p_k - c_j) - delta >= 0.
        This is what a subclass overriding the reference's _get_list_c_and_eta / _compute_single_lcbf hooks feeds.
        overflow [B] int32 or None: the flags of whoever produced the rows (LidarSensor.sense: the scan's clusters did not fit
        the obstacle slots); a flagged problem is not solved against its truncated list: status STATUS_SENSOR_OVERFLOW, NaN
        outputs (advance() leaves the robot where it is).  Streams and graphs: as plan_step_batch."""
        B = self._check_inputs(state, goal, first_foot, None, None, delta, need_obstacles=False)
        _check(c_eta_in, (B, self.params.n_obs_max, 4), torch.float64, self.device, "c_eta_in", required=True)
        _check(bounds, (B, 4), torch.float64, self.device, "bounds")
        _check(overflow, (B,), torch.int32, self.device, "overflow")
        if out is None:
            out = self.alloc_outputs(B, False, with_diag, with_working)
        else:
            self._check_outputs(out, B)
        self._ensure_workspace(B)
        self._check_warm(B)
        _lib.call("lipmpc_plan_step_batch_c_eta", h=self._h, B=B, state=state, goal=goal, first_foot=first_foot, delta=delta,
                  c_eta_in=c_eta_in, overflow=overflow, **_named(out, _STEP_OUTPUTS_GIVEN_C_ETA), bounds=bounds,
                  hip_stream=torch.cuda.current_stream(self.device).cuda_stream)
        return out

    def _check_outputs(self, out, B):
        """caller-supplied output buffers must have the shapes alloc_outputs gives (raw pointers go to the kernel)"""
        _check_table(step_outputs(B, self.params), out, self.device, "out")

    def advance(self, state, first_foot, out):
        """In place: state <- (A_l x + B_l U[:,0], theta[:,1]), first_foot <- -first_foot for the
        problems whose status is solved (HumanoidMpc.py:432-447)."""
        B = state.shape[0]
        _check(state, (B, 5), torch.float64, self.device, "state")
        _check(first_foot, (B,), torch.int8, self.device, "first_foot")
        self._check_outputs(out, B)
        _lib.call("lipmpc_advance_batch", h=self._h, B=B, state=state, first_foot=first_foot, **_named(out, ("U", "theta", "status")),
                  hip_stream=torch.cuda.current_stream(self.device).cuda_stream)

    def fleet_update(self, fleet, out, overflow=None, stop_obj=0.05, recover=None):
        """One sample of a host-driven fleet loop after ``plan_step_batch(..., out=out)`` on the same stream:
        stop rule, stop on a failed solve, state advance, counters and the trajectory row, in one launch
        (lipmpc_fleet_update_batch).  ``fleet`` = dict(state, first_foot, walking int8, last_obj, n_steps, last_status,
        n_overflow, sample int32[1], X_pred [B,k_max+1,5], U_pred [B,k_max,3]); the device-side sample counter
        advances by one per call.
        ``recover`` = dict(goal [B,2], c_eta [B,n_obs_max,4] or None, delta [B] or None, max_recover int >= 0, recover_run,
        n_recover int32 [B], recover_margin float64 [B] -- the buffers of ``recover_state``): the same launch with recovery
        (lipmpc_fleet_recover_update_batch).  A robot whose solve ended INFEASIBLE or MAX_ITER takes a capture step -- foot on
        p + v / beta, heading turned toward ``goal`` -- instead of stopping, if that point respects every row of ``c_eta`` (the
        rows the solve was given) and the robot has taken fewer than ``max_recover`` such samples in a row; include/lipmpc.h
        has the rule.  ``max_recover`` = 0 leaves ``fleet`` exactly as the call without ``recover`` does."""
        B, k_max = fleet["state"].shape[0], fleet["U_pred"].shape[1]
        _check_table(fleet_state(B, k_max), fleet, self.device, "fleet")
        self._check_outputs(out, B)
        _check(overflow, (B,), torch.int32, self.device, "overflow")
        if recover is not None:
            names = ("goal", "c_eta", "delta", "max_recover") + RECOVER_STATE
            if not isinstance(recover, dict) or set(recover) - set(names):
                raise ValueError(f"recover: a dict with the entries {names}")
            max_recover = recover.get("max_recover")
            if not isinstance(max_recover, int) or isinstance(max_recover, bool) or max_recover < 0:
                raise ValueError("recover['max_recover']: an int >= 0")
            _check(recover.get("goal"), (B, 2), torch.float64, self.device, "recover['goal']", required=True)
            _check(recover.get("c_eta"), (B, self.params.n_obs_max, 4), torch.float64, self.device, "recover['c_eta']")
            _check(recover.get("delta"), (B,), torch.float64, self.device, "recover['delta']")
            _check_table(recover_state(B), recover, self.device, "recover")
            _lib.call("lipmpc_fleet_recover_update_batch", h=self._h, B=B, k_max=int(k_max), stop_obj=float(stop_obj),
                      **_named(fleet, FLEET_STATE), **_named(out, ("U", "theta", "omega", "obj", "status")), overflow=overflow,
                      **_named(recover, ("goal", "c_eta", "delta")), max_recover=max_recover, **_named(recover, RECOVER_STATE),
                      hip_stream=torch.cuda.current_stream(self.device).cuda_stream)
            return
        _lib.call("lipmpc_fleet_update_batch", h=self._h, B=B, k_max=int(k_max), stop_obj=float(stop_obj), **_named(fleet, FLEET_STATE),
                  **_named(out, ("U", "theta", "omega", "obj", "status")), overflow=overflow,
                  hip_stream=torch.cuda.current_stream(self.device).cuda_stream)

    def rollout(self, state0, goal, first_foot, obs_xy=None, obs_nv=None, delta=None, k_max=100, mpc_step=1,
                stop_obj=0.05, bounds=None):
        """Closed loop on the device (HumanoidMpc.py:345-459) for B robots: returns dict(X_pred [B,k_max+1,5],
        U_pred [B,k_max,3], n_steps [B], last_status [B], total_iters [B]); rows beyond n_steps are undefined."""
        B = self._check_inputs(state0, goal, first_foot, obs_xy, obs_nv, delta)
        _check(bounds, (B, 4), torch.float64, self.device, "bounds")
        if int(k_max) < 1 or int(mpc_step) < 1:
            raise ValueError("k_max and mpc_step must be positive")
        table = rollout_outputs(B, k_max)
        out = _alloc(table, table, self.device)
        _lib.call("lipmpc_rollout_batch", h=self._h, B=B, k_max=int(k_max), mpc_step=int(mpc_step), stop_obj=float(stop_obj),
                  state0=state0, goal=goal, first_foot=first_foot, delta=delta, obs_xy=obs_xy, obs_nv=obs_nv, **out, bounds=bounds,
                  hip_stream=torch.cuda.current_stream(self.device).cuda_stream)
        return out

    def rollout_subgoals(self, state0, sub_goals, n_sub, first_foot, obs_xy=None, obs_nv=None, delta=None, k_max=100,
                         mpc_step=1, stop_obj=0.05, bounds=None):
        """Sub-goal sequencing for B robots (the hand-off of HumanoidMPCWithRRT.py:155-181): robot b walks to
        sub_goals[b, 0], then from where it stopped to sub_goals[b, 1], ... for n_sub[b] segments; every segment is
        a fresh closed loop (foot schedule restarts at first_foot[b], own k_max budget) kept with the reference's
        truncation, so a segment that uses all k_max samples hands over its last-but-one state.  A robot whose
        solve fails stops there.  One rollout launch per segment over the robots still walking.
        Returns dict(X_pred [B,S,k_max+1,5], U_pred [B,S,k_max,3], n_kept [B,S] kept inputs per segment
        (kept states = n_kept+1; -1 = segment not run), last_status [B], final_state [B,5])."""
        B = self._check_inputs(state0, sub_goals[:, 0].contiguous(), first_foot, obs_xy, obs_nv, delta)
        S = sub_goals.shape[1]
        dev = self.device
        out = dict(X_pred=torch.zeros((B, S, k_max + 1, 5), dtype=torch.float64, device=dev),
                   U_pred=torch.zeros((B, S, k_max, 3), dtype=torch.float64, device=dev),
                   n_kept=torch.full((B, S), -1, dtype=torch.int32, device=dev),
                   last_status=torch.zeros((B,), dtype=torch.int32, device=dev),
                   final_state=state0.clone())
        alive = torch.ones((B,), dtype=torch.bool, device=dev)
        sel = lambda t, i: None if t is None else t.index_select(0, i).contiguous()
        for s in range(S):
            idx = torch.nonzero(alive & (n_sub.to(dev) > s)).flatten()
            if idx.numel() == 0:
                break
            ro = self.rollout(sel(out["final_state"], idx), sel(sub_goals[:, s], idx), sel(first_foot, idx),
                              sel(obs_xy, idx), sel(obs_nv, idx), sel(delta, idx), k_max=k_max, mpc_step=mpc_step,
                              stop_obj=stop_obj, bounds=sel(bounds, idx))
            n = ro["n_steps"].to(torch.int64)
            kept = torch.where(n < k_max, n, torch.full_like(n, k_max - 1))        # HumanoidMpc.py:457-459
            out["X_pred"][idx, s] = ro["X_pred"]
            out["U_pred"][idx, s] = ro["U_pred"]
            out["n_kept"][idx, s] = kept.to(torch.int32)
            out["last_status"][idx] = ro["last_status"]
            out["final_state"][idx] = ro["X_pred"][torch.arange(idx.numel(), device=dev), kept]
            ok = (ro["last_status"] == STATUS_SOLVED) | (ro["last_status"] == STATUS_UNCERTIFIED)
            alive[idx] = ok
        return out


def unpack_active(active_words: np.ndarray, num_rows: int) -> np.ndarray:
    """[B,words] int64/uint64 -> [B,num_rows] bool in canonical row order."""
    w = np.ascontiguousarray(active_words).view(np.uint64)
    bits = (w[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)
    return bits.reshape(w.shape[0], -1)[:, :num_rows].astype(bool)


def pack_rings(obstacle_sets, n_obs_max, v_max):
    """list (per problem) of lists of (V,2) CCW rings -> (obs_xy [B,n_obs_max,v_max,2], obs_nv [B,n_obs_max])."""
    B = len(obstacle_sets)
    xy = np.zeros((B, n_obs_max, v_max, 2))
    nv = np.zeros((B, n_obs_max), np.int32)
    for b, rings in enumerate(obstacle_sets):
        if len(rings) > n_obs_max:
            raise ValueError(f"problem {b}: {len(rings)} obstacles > n_obs_max={n_obs_max}")
        for j, r in enumerate(rings):
            r = np.asarray(r, float)
            if r.shape[0] > v_max:
                raise ValueError(f"problem {b} obstacle {j}: {r.shape[0]} vertices > v_max={v_max}")
            xy[b, j, : r.shape[0]] = r
            nv[b, j] = r.shape[0]
    return xy, nv
