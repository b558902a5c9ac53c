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


def _ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _check(t, shape, dtype, device, name, required=False):
    """A buffer whose raw pointer goes to a kernel: a contiguous ``dtype`` tensor of ``shape`` on ``device``, or None when
    not ``required``; anything else is a ValueError naming it."""
    if t is None:
        if required:
            raise ValueError(f"{name} is required")
        return
    if tuple(t.shape) != shape or t.dtype != dtype or t.device != device or not t.is_contiguous():
        raise ValueError(f"{name}: expected contiguous {dtype} {shape} on {device}, got {t.dtype} {tuple(t.shape)} on {t.device}")


def _step_out_ptrs(out, c_eta_slot=False):
    """The output pointers of a step in the order of the C ABI: U .. working[, c_eta when the entry point has that slot],
    diag (absent optional outputs: NULL)."""
    names = ("U", "X", "theta", "omega", "obj", "status", "iters", "active", "working") + (("c_eta",) if c_eta_slot else ()) + ("diag",)
    return [_ptr(out.get(k)) for k in names]


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
        self._kept = []                            # every buffer ever registered with the library (a captured graph may hold it)
        self._side_streams = False                 # the library made its side streams / events (first workspace registered)
        self._split_capable = int(self.lib.lipmpc_workspace_bytes(self._h, 1)) > 0
        self._warm, self._warm_cap = None, 0
        self.warm_words = int(self.lib.lipmpc_warm_words(C.byref(cp)))

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
        rc = self.lib.lipmpc_set_warm_start(self._h, _ptr(rec), capacity)
        if rc == _LIPMPC_E_UNSUPPORTED:
            return False
        _lib.check(rc, "lipmpc_set_warm_start")
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
        """A workspace buffer of ``capacity`` problems that the handle keeps for its lifetime, or None (not split-capable)."""
        nbytes = int(self.lib.lipmpc_workspace_bytes(self._h, capacity)) if capacity > 0 else 0
        if nbytes <= 0:
            return None
        if not self._side_streams and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("the first split launch (workspace) of a handle makes its side streams and events, which cannot "
                               "happen during a graph capture: run one step of the handle, or set_workspace, before capturing")
        ws = torch.empty((nbytes // 4,), dtype=torch.int32, device=self.device)
        self._kept.append(ws)
        return ws

    def _register_workspace(self, ws, capacity):
        cap = capacity if ws is not None else 0
        _lib.check(self.lib.lipmpc_set_workspace(self._h, _ptr(ws), cap), "lipmpc_set_workspace")
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
        if self._sched is not None:
            self._kept.append(self._sched)
        _lib.check(self.lib.lipmpc_set_schedule(self._h, _ptr(self._sched), capacity), "lipmpc_set_schedule")

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and C is not None:      # (C is None: interpreter shutdown)
            self.lib.lipmpc_destroy(h)
            self._h = None

    # ---- buffers --------------------------------------------------------------------------------
    def alloc_outputs(self, B, with_c_eta=False, with_diag=False, with_working=False):
        P, dev = self.params, self.device
        f64 = dict(dtype=torch.float64, device=dev)
        out = dict(
            U=torch.empty((B, P.N, 2), **f64), X=torch.empty((B, P.N + 1, 4), **f64),
            theta=torch.empty((B, P.N + 1), **f64), omega=torch.empty((B, P.N), **f64),
            obj=torch.empty((B,), **f64),
            status=torch.empty((B,), dtype=torch.int32, device=dev),
            iters=torch.empty((B,), dtype=torch.int32, device=dev),
            active=torch.empty((B, P.active_words), dtype=torch.int64, device=dev),
        )
        if with_c_eta:
            out["c_eta"] = torch.empty((B, P.n_obs_max, 4), **f64)
        if with_diag:
            out["diag"] = torch.empty((B, _lib.DIAG_WORDS), **f64)
        if with_working:
            out["working"] = torch.empty((B, P.active_words), dtype=torch.int64, device=dev)
        return out

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
        stream = torch.cuda.current_stream(self.device).cuda_stream
        rc = self.lib.lipmpc_plan_step_batch(
            self._h, B, _ptr(state), _ptr(goal), _ptr(first_foot), _ptr(delta), _ptr(obs_xy), _ptr(obs_nv),
            *_step_out_ptrs(out, c_eta_slot=True), _ptr(bounds), C.c_void_p(stream))
        _lib.check(rc, "lipmpc_plan_step_batch")
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
        stream = torch.cuda.current_stream(self.device).cuda_stream
        rc = self.lib.lipmpc_plan_step_batch_c_eta(
            self._h, B, _ptr(state), _ptr(goal), _ptr(first_foot), _ptr(delta), _ptr(c_eta_in), _ptr(overflow),
            *_step_out_ptrs(out), _ptr(bounds), C.c_void_p(stream))
        _lib.check(rc, "lipmpc_plan_step_batch_c_eta")
        return out

    def _check_outputs(self, out, B):
        """caller-supplied output buffers must have the shapes alloc_outputs gives (raw pointers go to the kernel)"""
        P, dev = self.params, self.device
        ref = {"U": ((B, P.N, 2), torch.float64), "X": ((B, P.N + 1, 4), torch.float64),
               "theta": ((B, P.N + 1), torch.float64), "omega": ((B, P.N), torch.float64),
               "obj": ((B,), torch.float64), "status": ((B,), torch.int32), "iters": ((B,), torch.int32),
               "active": ((B, P.active_words), torch.int64)}
        for k, (shape, dt) in ref.items():
            if k not in out:
                raise ValueError(f"out['{k}'] missing")
            _check(out[k], shape, dt, dev, f"out['{k}']")
        _check(out.get("c_eta"), (B, P.n_obs_max, 4), torch.float64, dev, "out['c_eta']")
        _check(out.get("diag"), (B, _lib.DIAG_WORDS), torch.float64, dev, "out['diag']")
        _check(out.get("working"), (B, P.active_words), torch.int64, dev, "out['working']")

    def advance(self, state, first_foot, out):
        """In place: state <- (A_l x + B_l U[:,0], theta[:,1]), first_foot <- -first_foot for the
        problems whose status is solved (HumanoidMpc.py:432-447)."""
        B = state.shape[0]
        _check(state, (B, 5), torch.float64, self.device, "state")
        _check(first_foot, (B,), torch.int8, self.device, "first_foot")
        self._check_outputs(out, B)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        rc = self.lib.lipmpc_advance_batch(self._h, B, _ptr(state), _ptr(first_foot), _ptr(out["U"]),
                                           _ptr(out["theta"]), _ptr(out["status"]), C.c_void_p(stream))
        _lib.check(rc, "lipmpc_advance_batch")


    def fleet_update(self, fleet, out, overflow=None, stop_obj=0.05):
        """One sample of a host-driven fleet loop after ``plan_step_batch(..., out=out)`` on the same stream:
        stop rule, stop on a failed solve, state advance, counters and the trajectory row, in one launch
        (lipmpc_fleet_update_batch).  ``fleet`` = dict(state, first_foot, walking int8, last_obj, n_steps, last_status,
        n_overflow, sample int32[1], X_pred [B,k_max+1,5], U_pred [B,k_max,3]); the device-side sample counter
        advances by one per call."""
        B, k_max = fleet["state"].shape[0], fleet["U_pred"].shape[1]
        for name, shape, dt in (("state", (B, 5), torch.float64), ("first_foot", (B,), torch.int8), ("walking", (B,), torch.int8),
                                ("last_obj", (B,), torch.float64), ("n_steps", (B,), torch.int32), ("last_status", (B,), torch.int32),
                                ("n_overflow", (B,), torch.int32), ("sample", (1,), torch.int32),
                                ("X_pred", (B, k_max + 1, 5), torch.float64), ("U_pred", (B, k_max, 3), torch.float64)):
            if name not in fleet:
                raise ValueError(f"fleet['{name}'] missing")
            _check(fleet[name], shape, dt, self.device, f"fleet['{name}']")
        self._check_outputs(out, B)
        _check(overflow, (B,), torch.int32, self.device, "overflow")
        stream = torch.cuda.current_stream(self.device).cuda_stream
        rc = self.lib.lipmpc_fleet_update_batch(
            self._h, B, int(k_max), float(stop_obj), _ptr(fleet["state"]), _ptr(fleet["first_foot"]), _ptr(fleet["walking"]),
            _ptr(fleet["last_obj"]), _ptr(fleet["n_steps"]), _ptr(fleet["last_status"]), _ptr(fleet["n_overflow"]),
            _ptr(fleet["sample"]), _ptr(fleet["X_pred"]), _ptr(fleet["U_pred"]), _ptr(out["U"]), _ptr(out["theta"]),
            _ptr(out["omega"]), _ptr(out["obj"]), _ptr(out["status"]), _ptr(overflow), C.c_void_p(stream))
        _lib.check(rc, "lipmpc_fleet_update_batch")

    def rollout(self, state0, goal, first_foot, obs_xy=None, obs_nv=None, delta=None, k_max=100, mpc_step=1,
                stop_obj=0.05, bounds=None):
        """Closed loop on the device (HumanoidMpc.py:345-459) for B robots: returns dict(X_pred [B,k_max+1,5],
        U_pred [B,k_max,3], n_steps [B], last_status [B], total_iters [B]); rows beyond n_steps are undefined."""
        B = self._check_inputs(state0, goal, first_foot, obs_xy, obs_nv, delta)
        _check(bounds, (B, 4), torch.float64, self.device, "bounds")
        if int(k_max) < 1 or int(mpc_step) < 1:
            raise ValueError("k_max and mpc_step must be positive")
        dev = self.device
        out = dict(X_pred=torch.empty((B, k_max + 1, 5), dtype=torch.float64, device=dev),
                   U_pred=torch.empty((B, k_max, 3), dtype=torch.float64, device=dev),
                   n_steps=torch.empty((B,), dtype=torch.int32, device=dev),
                   last_status=torch.empty((B,), dtype=torch.int32, device=dev),
                   total_iters=torch.empty((B,), dtype=torch.int32, device=dev))
        stream = torch.cuda.current_stream(dev).cuda_stream
        rc = self.lib.lipmpc_rollout_batch(self._h, B, int(k_max), int(mpc_step), float(stop_obj), _ptr(state0), _ptr(goal),
                                           _ptr(first_foot), _ptr(delta), _ptr(obs_xy), _ptr(obs_nv), _ptr(out["X_pred"]),
                                           _ptr(out["U_pred"]), _ptr(out["n_steps"]), _ptr(out["last_status"]),
                                           _ptr(out["total_iters"]), _ptr(bounds), C.c_void_p(stream))
        _lib.check(rc, "lipmpc_rollout_batch")
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
