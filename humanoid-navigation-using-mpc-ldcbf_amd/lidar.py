"""LiDAR front end of the unknown-environment variant (BASELINE config 5) — host wrapper of
lipmpc_lidar_sense_batch and the drop-in HumanoidMPCUnknownEnvironment class
(HumanoidNavigation/MPC/HumanoidMPCVariants/HumanoidMPCUnknownEnvironment.py:13-68).  The true map is a list of convex vertex
rings, as in the reference, or an occupancy grid (GridMap, lipmpc_lidar_grid_c_eta_batch)."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .compat import HumanoidMPC, _ring_of
from .solver import _STEP_OUTPUTS_GIVEN_C_ETA, _alloc, _check, _check_table, _named, fleet_state, recover_state

NOISE_STD = 0.01           # range_finder_wth_polygons_dbscan.py:163
DBSCAN_EPS = 0.3           # :100
DBSCAN_MIN_SAMPLES = 3     # :100


def ray_table(resolution=360):
    """(cos, sin) of i * 2 pi / resolution through math.cos / math.sin, as the reference computes its rays (:28-36)."""
    step = 2 * math.pi / resolution
    return np.array([[math.cos(i * step), math.sin(i * step)] for i in range(resolution)])


def sensor_outputs(B, n_obs_max, v_max, resolution):
    """Outputs of a scan, in the order LidarSensor.alloc_outputs returns them; which of the optional ones a call needs is the
    call's to say."""
    f64, i32 = torch.float64, torch.int32
    return {"n_inferred": (i32, (B,), True), "overflow": (i32, (B,), True), "obs_xy": (f64, (B, n_obs_max, v_max, 2), False),
            "obs_nv": (i32, (B, n_obs_max), False), "c_eta": (f64, (B, n_obs_max, 4), False),
            "hits": (f64, (B, resolution, 2), False), "labels": (i32, (B, resolution), False),
            "pieces": (i32, (B, resolution), False)}


_SPLIT_SCAN_OUTPUTS = tuple(sensor_outputs(0, 0, 0, 0))                      # the names: what the *_split_batch entry points write
SENSOR_OUTPUTS = tuple(k for k in _SPLIT_SCAN_OUTPUTS if k != "pieces")      # what their parents write (no pieces)
_RING_SCAN_OUTPUTS = tuple(k for k in SENSOR_OUTPUTS if k != "c_eta")       # lipmpc_lidar_sense_batch has no c_eta


class GridMap:
    """An occupancy grid as the true map of a scan (include/lipmpc.h, lipmpc_lidar_grid_c_eta_batch): ``occ`` [W,H] (one map for
    every robot) or [B,W,H] (one per robot), a tensor or an array, cell (i, j) solid where ``occ[..., i, j]`` is nonzero;
    cell (i, j) is the rectangle [ox + i dx, ox + (i+1) dx) x [oy + j dy, oy + (j+1) dy) with ``origin`` = (ox, oy) and
    ``cell`` = (dx, dy) or one size for both.  Everything outside the grid is free."""

    def __init__(self, occ, origin, cell):
        if isinstance(occ, torch.Tensor):
            occ = (occ != 0).to(torch.uint8).contiguous()
        else:
            occ = np.ascontiguousarray(np.asarray(occ) != 0, dtype=np.uint8)
        if occ.ndim not in (2, 3) or min(occ.shape) < 1:
            raise ValueError("occ must be [W,H] or [B,W,H] with at least one cell")
        self.occ = occ
        self.origin = (float(origin[0]), float(origin[1]))
        self.cell = (float(cell), float(cell)) if np.isscalar(cell) else (float(cell[0]), float(cell[1]))
        if not (0.0 < self.cell[0] < math.inf and 0.0 < self.cell[1] < math.inf):
            raise ValueError("cell sizes must be positive and finite")
        self._origin_c, self._cell_c = (C.c_double * 2)(*self.origin), (C.c_double * 2)(*self.cell)      # read by the C call

    shared = property(lambda self: self.occ.ndim == 2)
    W = property(lambda self: int(self.occ.shape[-2]))
    H = property(lambda self: int(self.occ.shape[-1]))

    def _on(self, device):
        """Is ``occ`` a tensor on ``device``?  ("cuda" names the current device: the same place as its "cuda:i".)"""
        index = lambda d: torch.cuda.current_device() if d.type == "cuda" and d.index is None else d.index
        device = torch.device(device)
        return isinstance(self.occ, torch.Tensor) and self.occ.device.type == device.type and index(self.occ.device) == index(device)

    def to(self, device):
        """The same map with ``occ`` as a tensor on ``device``."""
        if self._on(device):
            return self
        return GridMap(torch.as_tensor(self.occ, device=device), self.origin, self.cell)

    @classmethod
    def from_planner(cls, out, b):
        """The grid problem ``b`` of ``RrtStarPlanner.plan_batch(..., with_grids=True)`` was planned on (``out``: that call's
        dict, with grid_dims, occ_d2 and grid_bounds).  The planner's cell (i, j) is the POINT min + (i * (max - min)) / W
        (include/lipmpc.h): here it is the centre of a cell of size (max - min) / W, so origin = min - cell / 2; the cells with
        occ_d2 = 0 are the solid ones."""
        W1, H1 = (int(v) for v in out["grid_dims"][b].cpu())
        min_x, max_x, min_y, max_y = (float(v) for v in out["grid_bounds"][b].cpu())
        cell = ((max_x - min_x) / (W1 - 1), (max_y - min_y) / (H1 - 1))
        occ = (out["occ_d2"][b, : W1 * H1] == 0).reshape(W1, H1)
        return cls(occ, (min_x - cell[0] / 2, min_y - cell[1] / 2), cell)

    def _args(self, B, device):
        """The map's arguments of the C calls, for a batch of B robots."""
        occ = self.occ
        if not self._on(device) or (not self.shared and occ.shape[0] != B):
            raise ValueError(f"grid: occ must be a tensor on {device}, [W,H] or [B,W,H] with B = {B} (GridMap.to)")
        return dict(W=self.W, H=self.H, grid_shared=int(self.shared), origin=C.addressof(self._origin_c),
                    cell=C.addressof(self._cell_c), occ=occ)


class LidarSensor:
    """Batched range_finder(): scan -> noise -> DBSCAN -> hulls, one wavefront per robot, rings in the layout
    BatchedLipMpc.plan_step_batch consumes.  ``LidarSensor.from_grid``: the same sensor over an occupancy grid.
    ``split_rays`` > 0 (at most resolution / 2; scans with ``c_eta=True``): every cluster is cut into pieces of at most that many
    consecutive rays, each with its own hull and (c, eta) row (include/lipmpc.h, lipmpc_lidar_c_eta_split_batch) -- one hull
    around the walls of a room holds the robot standing in it, the hulls of sectors of at most half a turn cannot."""

    @classmethod
    def from_grid(cls, grid, lidar_range=3.0, resolution=360, n_obs_max=12, v_max=32, device=None, split_rays=0):
        """A sensor whose true map is the GridMap ``grid`` (shared, or one map per robot of the batches it will scan): ``sense``
        (with ``c_eta=True``), ``sense_plan_step`` and ``alloc_outputs`` as for rings, same return dicts.  The robots are scanned
        in index order (no ``schedule``).  A robot standing in a solid cell gets no scan: n_inferred = 0, overflow = 1.  A
        (range, cell) pair whose window of cells within range exceeds 49152 cells is refused (RuntimeError, code -2)."""
        sn = cls([], lidar_range, resolution, n_obs_max, v_max, device, split_rays)
        sn.grid = grid.to(sn.device)
        return sn

    grid = None                # the GridMap of a sensor made by from_grid

    def __init__(self, env_rings, lidar_range=3.0, resolution=360, n_obs_max=12, v_max=32, device=None, split_rays=0):
        if not 0 <= int(split_rays) <= int(resolution) // 2:
            raise ValueError("split_rays: 0 (off) .. resolution / 2")
        if not torch.cuda.is_available():
            raise RuntimeError("lipmpc needs a HIP device; there is no CPU path")
        self.split_rays = int(split_rays)
        self.lib = _lib.load()
        self.device_index = torch.cuda.current_device() if device is None else int(device)
        self.device = torch.device("cuda", self.device_index)
        self.lidar_range, self.resolution, self.n_obs_max, self.v_max = float(lidar_range), int(resolution), n_obs_max, v_max
        rings = [np.asarray(r, float) for r in env_rings]
        self.n_env = len(rings)
        self.v_env = max([1] + [len(r) for r in rings])
        xy = np.zeros((max(self.n_env, 1), self.v_env, 2)); nv = np.zeros(max(self.n_env, 1), np.int32)
        for j, r in enumerate(rings):
            xy[j, :len(r)] = r; nv[j] = len(r)
        self.env_xy = torch.as_tensor(xy, device=self.device)
        self.env_nv = torch.as_tensor(nv, device=self.device)
        self.table = torch.as_tensor(ray_table(self.resolution), device=self.device)
        self._auto_sched = {}      # (batch size, stream) -> order buffer of sense(schedule="auto")

    def alloc_outputs(self, B, with_debug=False, rings=True, c_eta=False):
        """Output buffers of ``sense``: rings (obs_xy, obs_nv) and / or the assembled half-spaces c_eta [B,n_obs_max,4]."""
        table = sensor_outputs(B, self.n_obs_max, self.v_max, self.resolution)
        names = ("n_inferred", "overflow") + (("obs_xy", "obs_nv") if rings else ()) + (("c_eta",) if c_eta else ())
        out = _alloc(table, names, self.device, torch.zeros)
        if with_debug:
            out.update(_alloc(table, ("hits", "labels") + (("pieces",) if self.split_rays and c_eta else ()), self.device))
        return out

    def make_schedule(self, B):
        """An order buffer for ``sense(..., schedule=)`` (lipmpc_lidar_c_eta_batch): scratch in which the call ranks its B
        robots by an estimate of their reading counts and deals their scans out so that every SIMD gets a heavy one with light ones.  Nothing carries
        over between calls; results do not depend on it."""
        return torch.zeros((int(self.lib.lipmpc_lidar_schedule_words(B)),), dtype=torch.int32, device=self.device)

    def sense(self, state, noise=None, with_debug=False, out=None, env_xy=None, env_nv=None, c_eta=False, rings=True,
              schedule="auto", grid=None):
        """state [B,5] device tensor; noise [B,resolution,2] or None -> dict(n_inferred, overflow[, obs_xy, obs_nv][, c_eta]
        [, hits, labels][, pieces]).  ``pieces`` [B,resolution] (-2 no reading, -1 noise, else the number of the reading's piece)
        comes with ``with_debug`` from a sensor with ``split_rays`` > 0; such a sensor scans with ``c_eta=True`` only.  ``c_eta=True``: the constraint assembly runs in the same launch (lipmpc_lidar_c_eta_batch) and
        the dict carries c_eta [B,n_obs_max,4] = (c, eta) of every inferred hull at the robot's CoM -- what
        ``BatchedLipMpc.plan_step_batch_c_eta`` solves against; with ``rings=False`` the hulls never leave the kernel.
        ``schedule``: a buffer of ``make_schedule(B)``, None (robots scanned in index order), or "auto" (default): with
        ``c_eta=True`` and more than one round of waves the sensor keeps one order buffer per (batch size, current stream) and
        every scan first ranks its robots (estimated reading counts -> launch positions: two small kernels inside the call).  Any
        order gives the same results -- but scans that share a BUFFER must be ordered on one stream (the order kernel of one
        launch rewrites what another launch reads; a torn order would scan some robots twice and others not at all): a buffer
        of ``make_schedule`` handed to launches on two streams, or to two graphs replayed concurrently, is a caller's bug.
        Vertex slots beyond obs_nv keep whatever an earlier call left there when ``out`` is reused.
        ``env_xy`` [B,n_env,v_env,2] / ``env_nv`` [B,n_env] (device tensors): one true map PER ROBOT instead of the
        sensor's shared map (env_shared = 0 of the C ABI).
        A sensor over a grid (``from_grid``) scans through lipmpc_lidar_grid_c_eta_batch: ``c_eta=True`` is required, ``grid``
        (a GridMap on the sensor's device) replaces the sensor's map for this call, ``schedule`` must be "auto" or None."""
        B, dev = state.shape[0], self.device
        if out is None:
            out = self.alloc_outputs(B, with_debug, rings=rings or not c_eta, c_eta=c_eta)
        want_ce = "c_eta" in out
        _check_table(sensor_outputs(B, self.n_obs_max, self.v_max, self.resolution), out, dev, "out")
        _check(state, (B, 5), torch.float64, dev, "state", required=True)
        _check(noise, (B, self.resolution, 2), torch.float64, dev, "noise")
        stream = torch.cuda.current_stream(dev).cuda_stream
        grid = self.grid if grid is None else grid
        # the *_split_batch twins only where they are needed: the parents keep receiving exactly their own arguments
        split = self.split_rays > 0 or out.get("pieces") is not None
        if split and not want_ce:
            raise ValueError("split_rays / pieces: the split scans assemble the half-spaces (c_eta=True)")
        suffix, outputs = ("_split_batch", dict(_named(out, _SPLIT_SCAN_OUTPUTS), split_rays=self.split_rays)) if split else \
            ("_batch", _named(out, SENSOR_OUTPUTS))
        if grid is not None:
            if not want_ce or env_xy is not None or not (schedule is None or schedule == "auto"):
                raise ValueError("a grid scan assembles the half-spaces (c_eta=True), takes no rings as its map and no schedule")
            _lib.call("lipmpc_lidar_grid_c_eta" + suffix, device=self.device_index, B=B, resolution=self.resolution, **grid._args(B, dev),
                      lidar_range=self.lidar_range, eps=DBSCAN_EPS, min_samples=DBSCAN_MIN_SAMPLES, n_obs_max=self.n_obs_max,
                      v_max=self.v_max, state=state, ray_table=self.table, noise=noise, **outputs, hip_stream=stream)
            return out
        n_env, v_env, shared, exy, env = self.n_env, self.v_env, 1, self.env_xy, self.env_nv
        if env_xy is not None:
            if (env_xy.dim() != 4 or env_xy.shape[0] != B or env_xy.shape[3] != 2 or env_nv is None
                    or tuple(env_nv.shape) != (B, env_xy.shape[1]) or env_xy.dtype != torch.float64
                    or env_nv.dtype != torch.int32 or not env_xy.is_contiguous() or not env_nv.is_contiguous()
                    or env_xy.device != dev or env_nv.device != dev):
                raise ValueError("per-robot maps: env_xy [B,n_env,v_env,2] float64, env_nv [B,n_env] int32, contiguous, on the sensor's device")
            n_env, v_env, shared, exy, env = int(env_xy.shape[1]), int(env_xy.shape[2]), 0, env_xy, env_nv
        if isinstance(schedule, str):
            if schedule != "auto":
                raise ValueError('schedule: a make_schedule(B) buffer, None or "auto"')
            schedule = None
            if want_ce and B > 2048:                         # beyond one round of waves (two per SIMD) the start order matters
                # one buffer per (batch size, stream): scans sharing a schedule must be ordered on one stream -- the order
                # kernel of one launch rewrites what the next one reads
                key = (B, stream)
                if key not in self._auto_sched:
                    self._auto_sched[key] = self.make_schedule(B)
                schedule = self._auto_sched[key]
        if schedule is not None and (not want_ce or schedule.dtype != torch.int32 or schedule.device != dev or not schedule.is_contiguous()
                                     or schedule.numel() != int(self.lib.lipmpc_lidar_schedule_words(B))):
            raise ValueError("schedule: a buffer of make_schedule(B) for this B, with c_eta=True")
        if want_ce:
            entry, outputs = "lipmpc_lidar_c_eta" + suffix, dict(outputs, schedule=schedule)
        else:
            entry, outputs = "lipmpc_lidar_sense_batch", _named(out, _RING_SCAN_OUTPUTS)
        _lib.call(entry, device=self.device_index, B=B, resolution=self.resolution, n_env=n_env, v_env=v_env, env_shared=shared,
                  lidar_range=self.lidar_range, eps=DBSCAN_EPS, min_samples=DBSCAN_MIN_SAMPLES, n_obs_max=self.n_obs_max,
                  v_max=self.v_max, state=state, env_xy=exy, env_nv=env, ray_table=self.table, noise=noise, **outputs, hip_stream=stream)
        return out

    def sense_plan_step(self, solver, state, goal, first_foot, noise=None, delta=None, sen=None, out=None, schedule=None,
                        bounds=None):
        """One MPC step of the unknown-environment variant in one C call (lipmpc_sense_plan_step_batch): scan + constraint
        assembly, then ``solver``'s step against the assembled half-spaces.  ``solver``: a BatchedLipMpc whose
        n_obs_max / v_max are this sensor's.  Returns (sen, out) as ``sense(..., c_eta=True, rings=False)`` and
        ``plan_step_batch_c_eta`` would -- the same bits, whatever the solver served before (a sensor with ``split_rays`` > 0
        issues exactly those two calls on the current stream: the one-call entry points have no split twin): the step takes the split launch
        with the workspace of the current stream exactly as ``plan_step_batch_c_eta`` does (streams and graphs: as
        ``BatchedLipMpc.plan_step_batch``).  A ``schedule`` buffer, like the solver's schedule and warm-start records, is
        shared by every launch it is given to: those must be ordered on one stream."""
        P = solver.params
        if P.n_obs_max != self.n_obs_max or P.v_max != self.v_max or solver.device != self.device:
            raise ValueError("solver and sensor must share n_obs_max, v_max and the device")
        B = solver._check_inputs(state, goal, first_foot, None, None, delta, need_obstacles=False)
        _check(bounds, (B, 4), torch.float64, self.device, "bounds")
        solver._check_warm(B)
        if sen is None:
            sen = self.alloc_outputs(B, rings=False, c_eta=True)
        if out is None:
            out = solver.alloc_outputs(B)
        else:
            solver._check_outputs(out, B)
        table, handed_over = sensor_outputs(B, self.n_obs_max, self.v_max, self.resolution), ("c_eta", "n_inferred", "overflow")
        for k in handed_over:
            _check(sen.get(k), table[k][1], table[k][0], self.device, f"sen['{k}']", required=True)
        _check(noise, (B, self.resolution, 2), torch.float64, self.device, "noise")
        if schedule is not None and (schedule.dtype != torch.int32 or schedule.device != self.device or not schedule.is_contiguous()
                                     or schedule.numel() != int(self.lib.lipmpc_lidar_schedule_words(B))):
            raise ValueError("schedule: a buffer of make_schedule(B) for this B")
        solver._ensure_workspace(B)
        if self.grid is not None and schedule is not None:
            raise ValueError("a grid scan takes no schedule")
        if self.split_rays > 0:
            self.sense(state, noise, out=sen, c_eta=True, rings=False, schedule=schedule)
            solver.plan_step_batch_c_eta(state, goal, first_foot, sen["c_eta"], delta, out=out, overflow=sen["overflow"], bounds=bounds)
            return sen, out
        if self.grid is not None:
            _lib.call("lipmpc_sense_grid_plan_step_batch", h=solver._h, B=B, resolution=self.resolution, **self.grid._args(B, self.device),
                      lidar_range=self.lidar_range, eps=DBSCAN_EPS, min_samples=DBSCAN_MIN_SAMPLES, state=state, goal=goal,
                      first_foot=first_foot, delta=delta, ray_table=self.table, noise=noise, **_named(sen, handed_over),
                      **_named(out, _STEP_OUTPUTS_GIVEN_C_ETA), bounds=bounds,
                      hip_stream=torch.cuda.current_stream(self.device).cuda_stream)
            return sen, out
        _lib.call("lipmpc_sense_plan_step_batch", h=solver._h, B=B, resolution=self.resolution, n_env=self.n_env, v_env=self.v_env,
                  env_shared=1, lidar_range=self.lidar_range, eps=DBSCAN_EPS, min_samples=DBSCAN_MIN_SAMPLES, state=state, goal=goal,
                  first_foot=first_foot, delta=delta, env_xy=self.env_xy, env_nv=self.env_nv, ray_table=self.table, noise=noise,
                  **_named(sen, handed_over), schedule=schedule, **_named(out, _STEP_OUTPUTS_GIVEN_C_ETA), bounds=bounds,
                  hip_stream=torch.cuda.current_stream(self.device).cuda_stream)
        return sen, out


class HumanoidMPCUnknownEnvironment(HumanoidMPC):
    """The robot only perceives obstacles through its LiDAR (HumanoidMPCUnknownEnvironment.py:13-28): every sample the
    obstacle set is re-inferred on the GPU and handed to the step solver.  ``noise_seed`` seeds the readings' noise
    (the reference's is unseeded); ``noise_seed=None`` = noiseless readings.  ``split_rays``: as ``LidarSensor``'s (0 = one hull
    per cluster, as the reference)."""

    def __init__(self, goal, obstacles, N_horizon=3, N_mpc_timesteps=100, sampling_time=1e-3, init_state=None,
                 start_with_right_foot: bool = True, verbosity: int = 1, lidar_range: float = 3.0,
                 lidar_resolution: int = 360, noise_seed: int | None = 0, split_rays: int = 0, **kw):
        self.lidar_range, self.lidar_resolution, self.split_rays = lidar_range, lidar_resolution, int(split_rays)
        super().__init__(goal, obstacles, N_horizon, N_mpc_timesteps, sampling_time,
                         np.zeros(5) if init_state is None else init_state, start_with_right_foot, verbosity, **kw)
        # the reference scans `ch.points` (raw input order), HumanoidMPCUnknownEnvironment.py:46
        env = [np.asarray(o.points, float) if hasattr(o, "points") else np.asarray(o, float) for o in obstacles]
        self._env = env
        self._sensor = LidarSensor(env, lidar_range, lidar_resolution, device=self._device, split_rays=self.split_rays)
        self._big_sensor = None
        self._gen = None if noise_seed is None else torch.Generator(device=self._sensor.device).manual_seed(int(noise_seed))
        self.list_inferred_obstacles = []
        self.list_lidar_readings = []          # per scan: `resolution` entries, None or the noisy hit (x, y) -- the reference's
                                               # range_finder readings (HumanoidMPCUnknownEnvironment.py:66, HumanoidMpc.py:86)

    def _sense(self, x_k: float, y_k: float):
        """One scan at (x_k, y_k): (c_eta [n,4], rings) of the inferred obstacles, c / eta assembled in the scan's launch."""
        dev = self._sensor.device
        st = torch.tensor([[x_k, 0.0, y_k, 0.0, 0.0]], dtype=torch.float64, device=dev)
        noise = None
        if self._gen is not None:
            noise = NOISE_STD * torch.randn((1, self.lidar_resolution, 2), dtype=torch.float64, device=dev, generator=self._gen)
        out = self._sensor.sense(st, noise, c_eta=True, with_debug=True)
        torch.cuda.synchronize(dev)
        if int(out["overflow"][0]):
            # more clusters / longer hulls than the default slots: scan again (same noise) into the largest layout the
            # step solver takes; the reference constrains against every inferred obstacle (:55-64), so a scan that
            # still does not fit is an error, not a truncated obstacle list
            if self._big_sensor is None:
                self._big_sensor = LidarSensor(self._env, self.lidar_range, self.lidar_resolution, n_obs_max=50, v_max=32,
                                               device=self._device, split_rays=self.split_rays)
            out = self._big_sensor.sense(st, noise, c_eta=True, with_debug=True)
            torch.cuda.synchronize(dev)
            if int(out["overflow"][0]):
                raise RuntimeError("LiDAR scan inferred more obstacles / hull vertices than the solver holds (50 x 32)")
        n = int(out["n_inferred"][0])
        nv = out["obs_nv"][0].cpu().numpy()
        xy = out["obs_xy"][0].cpu().numpy()
        rings = [xy[j, :nv[j]].copy() for j in range(n)]
        self.list_inferred_obstacles.append(rings)
        hits = out["hits"][0].cpu().numpy()
        self.list_lidar_readings.append([None if h[0] != h[0] else (float(h[0]), float(h[1])) for h in hits])
        return out["c_eta"][0, :n].cpu().numpy(), rings

    def _get_list_c_and_eta(self, x_k: float, y_k: float):
        """The hook the reference's variant overrides (HumanoidMPCUnknownEnvironment.py:30-68): scan, cluster, hulls,
        closest point and normal per hull -- one launch (lipmpc_lidar_c_eta_batch); the step is then solved against
        these half-spaces through lipmpc_plan_step_batch_c_eta."""
        ce, _ = self._sense(x_k, y_k)
        return [r[:2].reshape(2, 1) for r in ce], [r[2:].reshape(2, 1) for r in ce]

    def _get_obstacle_rings(self, x_k: float, y_k: float):
        """The inferred obstacles as rings (one scan), for callers that want the polygons."""
        return self._sense(x_k, y_k)[1]


class UnknownEnvFleet:
    """B robots walking through one map that they only see through their LiDAR: the closed loop of
    HumanoidMPCUnknownEnvironment (HumanoidMpc.py:380-459 with _get_list_c_and_eta from
    HumanoidMPCUnknownEnvironment.py:30-68) for a whole batch and without a host round trip per sample — scan, step
    solve and state advance are enqueued back to back; with ``use_graph`` one sample is captured in a HIP graph and
    replayed.  One MPC solve per sample (sampling_time = DELTA_T), the reference's stop rule (previous objective <
    0.05) and stop-on-failed-solve per robot.  ``warm_start=True``: every solve starts from the robot's previous step,
    shifted by one stage (the reference's seeding, HumanoidMpc.py:448-455), through a warm-start record per robot that each
    run zeroes before its first sample (N >= 2, at most 14 obstacle slots).  ``grid=GridMap`` instead of ``env_rings``: the same
    loop over an occupancy grid (a robot that walks into a solid cell stops with STATUS_SENSOR_OVERFLOW).
    ``avoid=NeighbourRows(...)``: the robots keep apart -- every sample each robot's nearest neighbours in the batch are
    appended to its scan's half-spaces as LDCBF rows (lipmpc_neighbour_c_eta_batch) before the solve; a stopped robot stays
    where it is and stays an obstacle.
    ``mapper=OccupancyMapper(...)``: the robots map what they see -- every sample the scan's readings of the walking robots are
    integrated into the mapper's evidence grid (lipmpc_map_update_batch) between the scan and the solve, inside the captured
    graph; the loop itself is not disturbed (same X_pred / U_pred, bit for bit).  A run adds to the evidence the mapper holds
    (``mapper.reset()`` forgets it).  ``run_replanning`` plans on that map toward given goals; ``run_exploring`` needs no goals:
    the robots walk to the map's frontiers until none is left.
    ``split_rays`` > 0: the scans cut their clusters into sectors of at most that many rays (``LidarSensor``) -- what lets a robot
    walk INSIDE a room, whose walls are one cluster around it (tests/golden/EXPLORATION_ROOMS.md).
    ``recover`` = n > 0: a failed solve no longer ends the robot -- a robot whose solve ends INFEASIBLE or MAX_ITER takes a capture
    step (foot on p + v / beta, heading turned toward its working goal) and solves again on the next sample, for at most n
    samples in a row and only if the capture point respects every half-space the sample's solve was given, neighbour rows
    included (lipmpc_fleet_recover_update_batch; DESIGN.md has the argument).  A recovering robot is walking.  6 is a sensible
    value: on the recorded scenes a robot that recovery keeps needs one in a row (tests/golden/EXPLORATION_RECOVER.md).  0 (the default): every
    call and every bit as before.
    ``drift_sigma`` = s: the robots' odometry drifts -- what they believe about their position parts from the truth by a random walk
    of N(0, s^2) per sample and axis, and it is the believed pose that maps and plans (``run`` has the model).  ``matcher=
    ScanMatcher(...)`` (needs ``mapper``; shifts only, n_yaw = 0: the sensor is world-aligned): every sample the scan is matched
    against the map before it is added to it (lipmpc_scan_match_batch) and the pose corrected by the accepted offset.
    ``drift_sigma`` without a matcher shows the smear.  Both None (the default): every call and every bit as before."""

    def __init__(self, env_rings=None, N_horizon=3, lidar_range=3.0, resolution=360, n_obs_max=12, v_max=32,
                 exact=False, interior_tol=1e-6, device=None, warm_start=False, grid=None, avoid=None, mapper=None, split_rays=0,
                 drift_sigma=None, matcher=None, recover=0):
        from .solver import BatchedLipMpc, LipMpcParams, FLAG_INTERIOR, FLAG_WARM_START
        if (env_rings is None) == (grid is None):
            raise ValueError("the true map: env_rings or grid")
        if isinstance(recover, bool) or not isinstance(recover, int) or recover < 0:
            raise ValueError("recover: the most capture steps in a row, an int >= 0 (0 = a failed solve is final)")
        self.recover = recover
        if grid is not None:
            self.sensor = LidarSensor.from_grid(grid, lidar_range, resolution, n_obs_max, v_max, device, split_rays)
        else:
            self.sensor = LidarSensor(env_rings, lidar_range, resolution, n_obs_max, v_max, device, split_rays)
        self.warm_start = bool(warm_start)
        self.solver = BatchedLipMpc(LipMpcParams(N=N_horizon, n_obs_max=n_obs_max, v_max=v_max,
                                                 flags=(0 if exact else FLAG_INTERIOR) | (FLAG_WARM_START if warm_start else 0),
                                                 tol_interior=interior_tol),
                                    self.sensor.device_index)
        self.device = self.sensor.device
        if avoid is not None and avoid.device != self.device:
            raise ValueError("avoid: a NeighbourRows on the fleet's device")
        self.avoid = avoid
        if mapper is not None and (mapper.device != self.device or mapper.resolution != self.sensor.resolution
                                   or mapper.lidar_range != self.sensor.lidar_range):
            raise ValueError("mapper: an OccupancyMapper on the fleet's device, for the fleet's resolution and lidar_range")
        self.mapper = mapper
        if matcher is not None and mapper is None:
            raise ValueError("matcher: a ScanMatcher matches against the fleet's map: UnknownEnvFleet(..., mapper=OccupancyMapper(...))")
        if matcher is not None and matcher.n_yaw:
            raise ValueError("matcher: the fleet's sensor is world-aligned, its matcher searches shifts only (n_yaw = 0)")
        if drift_sigma is not None and not 0.0 <= float(drift_sigma) < math.inf:
            raise ValueError("drift_sigma: None or a standard deviation >= 0")
        self.matcher = matcher
        self.drift_sigma = None if drift_sigma is None else float(drift_sigma)
        # what ``run_exploring`` hands to its run as ``drift`` / ``drift_seed`` (its own parameter list is as it always was)
        self.exploring_drift, self.exploring_drift_seed = "seeded", 0

    def _plan_for(self, B, k_max, noise_mode, have_delta, stop_obj, use_graph, drift_mode=None):
        """Buffers (and, once captured, the HIP graph of one sample) of a run shape; kept across ``run`` calls, so a
        second run of the same shape replays the graph it already has.  ``drift_mode``: None (no drift model: the buffers and the
        sample of a fleet without one), "none", "seeded" or "given"."""
        key = (B, k_max, noise_mode, have_delta, float(stop_obj), bool(use_graph)) + (() if drift_mode is None else (drift_mode,))
        pl = getattr(self, "_plan", None)
        if pl is not None and pl["key"] == key:
            return pl
        dev, sn, sv = self.device, self.sensor, self.solver
        if self.warm_start and not sv.set_warm_start(B):      # (outside any capture; grow-only)
            raise ValueError("warm_start: the warm-start record needs N >= 2 and at most 14 obstacle slots")
        f64 = dict(dtype=torch.float64, device=dev)
        table = fleet_state(B, k_max)
        fl = _alloc(table, table, dev, torch.zeros)
        fl["first_foot"].fill_(1)
        fl["walking"].fill_(1)
        pl = dict(key=key, fl=fl, goal=torch.zeros((B, 2), **f64), delta=torch.zeros((B,), **f64) if have_delta else None,
                  sen=sn.alloc_outputs(B, rings=False, c_eta=True),      # hulls stay in the scan kernel: only (c, eta) rows reach HBM
                  out=sv.alloc_outputs(B), nbuf=None if noise_mode == "none" else torch.zeros((B, sn.resolution, 2), **f64),
                  gen=torch.Generator(device=dev) if noise_mode == "seeded" else None, graph=None,
                  # order buffer: every scan of rings ranks its robots before it starts them (a grid is scanned in index order)
                  sched=sn.make_schedule(B) if sn.grid is None else None)
        if self.avoid is not None:
            pl.update(nbr=self.avoid.alloc_outputs(B), n_crowded=torch.zeros((B,), dtype=torch.int32, device=dev),
                      crowded=torch.zeros((B,), dtype=torch.bool, device=dev))
        if self.mapper is not None:
            # the scan hands its readings over, and `walking` (int8) goes to the update as the int32 mask the C call takes
            pl["sen"].update(_alloc(sensor_outputs(B, sn.n_obs_max, sn.v_max, sn.resolution), ("hits",), dev, torch.zeros))
            pl["mask"] = torch.zeros((B,), dtype=torch.int32, device=dev)
        if self.recover:
            # the counters of lipmpc_fleet_recover_update_batch, and the margin of each robot's last evaluated safety test
            table = recover_state(B)
            pl["rec"] = _alloc(table, table, dev, torch.zeros)
            pl["last_margin"] = torch.zeros((B,), **f64)
            pl["not_evaluated"] = torch.zeros((B,), dtype=torch.bool, device=dev)
        if drift_mode is not None:
            # the odometry model: drift = believed - true position, this sample's draw, what the robots believe (state, goal, and
            # with a map the readings as placed at the believed pose), and the record of the run
            pl.update(drift=torch.zeros((B, 2), **f64), dbuf=torch.zeros((B, 2), **f64), dstep=torch.zeros((B, 2), **f64),
                      walkf=torch.zeros((B,), **f64), bstate=torch.zeros((B, 5), **f64), bgoal=torch.zeros((B, 2), **f64),
                      perr=torch.zeros((B,), **f64), pose_error=torch.zeros((k_max, B), **f64),
                      n_matched=torch.zeros((B,), dtype=torch.int32, device=dev),
                      dgen=torch.Generator(device=dev) if drift_mode == "seeded" else None)
            if self.mapper is not None:
                pl["bhits"] = torch.zeros((B, sn.resolution, 2), **f64)
            if self.matcher is not None:
                pl["mout"] = self.matcher.alloc_outputs(B, dev)
        self._plan = pl
        return pl

    def _drift_mode(self, drift):
        """How a run's ``drift`` argument is taken: None = the fleet has no drift model (no ``drift_sigma``, no ``matcher``, no
        given draws) and its sample is the one it always was; "given" = a tensor of draws; "seeded" = draws of N(0,
        drift_sigma^2) from the run's generator; "none" = no draws (a matcher alone, or ``drift=None``)."""
        if isinstance(drift, torch.Tensor):
            return "given"
        if drift is not None and drift != "seeded":
            raise ValueError('drift: "seeded", None or a tensor [k_max,B,2]')
        if self.drift_sigma is None and self.matcher is None:
            return None
        return "none" if drift is None or self.drift_sigma is None else "seeded"

    @staticmethod
    def _believed_positions(pl):
        """[B,2]: where the robots believe they are (true + drift); the true positions in a fleet without a drift model."""
        pos = pl["fl"]["state"][:, (0, 2)].contiguous()
        return pos if "drift" not in pl else pos + pl["drift"]

    def run(self, state0, goal, first_foot, k_max, noise="seeded", noise_seed=0, delta=None, stop_obj=0.05,
            use_graph=True, drift="seeded", drift_seed=0):
        """state0 [B,5], goal [B,2], first_foot [B] int8.  noise: "seeded" (N(0, 0.01) per reading from a generator
        seeded with noise_seed), None (noiseless) or a tensor [k_max,B,resolution,2].  Returns dict(X_pred
        [B,k_max+1,5], U_pred [B,k_max,3], n_steps [B] solved samples, last_status [B] (STATUS_SENSOR_OVERFLOW = 5: the
        robot was stopped because a scan's clusters did not fit the obstacle slots, or -- on a grid -- because it stands in a solid
        cell), overflow [B] number of such scans).  In a fleet with ``recover`` > 0 also n_recover [B] int32 recovery samples
        taken, recover_run [B] int32 those in a row at the end, and recover_margin [B] the margin of the robot's last evaluated
        safety test (NaN: never evaluated); a fleet without it returns exactly the entries it always did.  With ``avoid`` also n_crowded [B]: the number of samples in which a
        neighbour in range of the robot got no row (n_near > n_rows: more neighbours than k_rows or than free slots).
        One sample = noise draw (seeded mode), scan + constraint assembly, step solve, fleet update; with ``use_graph``
        it is captured once per run shape in a HIP graph (kept by the object) and replayed k_max times back to back.
        The returned tensors are the object's buffers: the next ``run`` of the same shape overwrites them.
        THE DRIFT MODEL (a fleet with ``drift_sigma`` or a ``matcher``, or a run given ``drift`` as a tensor; any other run takes
        the code path it always took, bit for bit).  ``state`` stays the TRUE state: it scans the world and is solved for.  A
        buffer ``drift`` [B,2] holds believed minus true position, zero at the start of a run.  Per sample: the walking robots'
        drift grows by the sample's draw -- ``drift="seeded"``: N(0, drift_sigma^2) per axis from a generator seeded with
        ``drift_seed``; a tensor [k_max,B,2]: the draws themselves; None: no draws --; after the scan the believed state and
        the readings as placed at the believed pose are true + drift; with a ``matcher`` they are matched against the evidence
        as it stands before this sample's update (walking robots only) and the offset is added to drift, believed state and
        readings; the map is updated with the believed state and readings; the solve (and the recovery) gets goal - drift,
        because goals live in the map's frame.  The result gains drift [B,2], pose_error [k_max,B] (|drift| after each sample)
        and n_matched [B] int32 (accepted non-zero offsets).  The model's limits: position drift only (no yaw), whole-cell
        corrections, and nothing already written into the map is ever corrected."""
        return self._run(state0, goal, first_foot, k_max, noise, noise_seed, delta, stop_obj, use_graph, drift=drift, drift_seed=drift_seed)

    def _run(self, state0, goal, first_foot, k_max, noise, noise_seed, delta, stop_obj, use_graph, before_sample=None, drift=None,
             drift_seed=0):
        """``run``; ``before_sample(k, pl)``: called on the host before sample k is enqueued (run_replanning's hook)."""
        dev, sv, sn, avoid, mapper, matcher = self.device, self.solver, self.sensor, self.avoid, self.mapper, self.matcher
        B = state0.shape[0]
        mode = "none" if noise is None else ("seeded" if isinstance(noise, str) else "given")
        dmode = self._drift_mode(drift)
        if dmode == "given":
            _check(drift, (int(k_max), B, 2), torch.float64, dev, "drift")
        pl = self._plan_for(B, int(k_max), mode, delta is not None, stop_obj, use_graph, dmode)
        fl, sen, out, nbuf, gen, rec = pl["fl"], pl["sen"], pl["out"], pl["nbuf"], pl["gen"], pl.get("rec")
        dgen = pl.get("dgen")
        pl["goal"].copy_(goal)
        if delta is not None:
            pl["delta"].copy_(delta)

        def reset():
            fl["state"].copy_(state0); fl["first_foot"].copy_(first_foot)
            fl["walking"].fill_(1); fl["last_obj"].fill_(float("inf"))
            for n in ("n_steps", "last_status", "n_overflow", "sample"):
                fl[n].zero_()
            fl["X_pred"].zero_(); fl["U_pred"].zero_(); fl["X_pred"][:, 0] = state0
            if avoid is not None:
                pl["n_crowded"].zero_()
            if rec is not None:
                rec["recover_run"].zero_(); rec["n_recover"].zero_()
                rec["recover_margin"].fill_(float("nan")); pl["last_margin"].fill_(float("nan"))
            sv.reset_warm_start()                            # every run starts cold (no-op without a record)
            if gen is not None:
                gen.manual_seed(int(noise_seed))
            if dmode is not None:
                pl["drift"].zero_(); pl["n_matched"].zero_(); pl["pose_error"].zero_()
            if dgen is not None:
                dgen.manual_seed(int(drift_seed))

        def drifting_sample():
            # the sample of a fleet whose odometry drifts: `state` is the truth, the map and the goals are in the believed frame
            drift_, bstate = pl["drift"], pl["bstate"]
            if gen is not None:
                nbuf.normal_(0.0, NOISE_STD, generator=gen)
            if dgen is not None:
                pl["dbuf"].normal_(0.0, self.drift_sigma, generator=dgen)
            if dmode != "none":
                pl["walkf"].copy_(fl["walking"])
                torch.mul(pl["dbuf"], pl["walkf"][:, None], out=pl["dstep"])
                drift_.add_(pl["dstep"])
            sn.sense(fl["state"], nbuf, out=sen, c_eta=True, rings=False, schedule=pl["sched"])
            if avoid is not None:
                nbr = avoid.append(fl["state"], sen["c_eta"], first_slot=sen["n_inferred"], out=pl["nbr"])
                torch.gt(nbr["n_near"], nbr["n_rows"], out=pl["crowded"])
                pl["n_crowded"].add_(pl["crowded"])
            bstate.copy_(fl["state"])
            torch.add(fl["state"][:, 0], drift_[:, 0], out=bstate[:, 0])
            torch.add(fl["state"][:, 2], drift_[:, 1], out=bstate[:, 2])
            if mapper is not None:
                bhits = pl["bhits"]
                torch.add(sen["hits"], drift_[:, None, :], out=bhits)
                pl["mask"].copy_(fl["walking"])
                if matcher is not None:
                    # against the evidence as it stands before this sample's update (the stream orders the two calls)
                    m = matcher.match(mapper, bstate, bhits, mask=pl["mask"], out=pl["mout"])
                    drift_.add_(m["offset"])
                    bstate[:, 0].add_(m["offset"][:, 0]); bstate[:, 2].add_(m["offset"][:, 1])
                    bhits.add_(m["offset"][:, None, :])
                    pl["n_matched"].add_(m["matched"])
                mapper.update(bstate, bhits, mask=pl["mask"])
            torch.sub(pl["goal"], drift_, out=pl["bgoal"])      # the goal lives in the map's frame, the solve in the true one
            sv.plan_step_batch_c_eta(fl["state"], pl["bgoal"], fl["first_foot"], sen["c_eta"], pl["delta"], out=out,
                                     overflow=sen["overflow"])
            torch.mul(drift_, drift_, out=pl["dstep"])
            torch.sum(pl["dstep"], dim=1, out=pl["perr"])
            pl["perr"].sqrt_()

        def sample():
            if dmode is not None:
                drifting_sample()
                return finish(pl["bgoal"])
            plain_sample()
            finish(pl["goal"])

        def plain_sample():
            # HumanoidMpc.py:387/:417 sense + solve; :392 stop rule, :419-429 failed solve ends the run, :432-447 advance
            # and the trajectory row: one bookkeeping launch (lipmpc_fleet_update_batch)
            if gen is not None:
                nbuf.normal_(0.0, NOISE_STD, generator=gen)
            if avoid is None and mapper is None:
                sn.sense_plan_step(sv, fl["state"], pl["goal"], fl["first_foot"], nbuf, pl["delta"], sen=sen, out=out, schedule=pl["sched"])
            else:
                # scan -> [neighbour rows behind the scan's] -> [the readings into the map] -> solve, back to back on the one stream
                sn.sense(fl["state"], nbuf, out=sen, c_eta=True, rings=False, schedule=pl["sched"])
                if avoid is not None:
                    nbr = avoid.append(fl["state"], sen["c_eta"], first_slot=sen["n_inferred"], out=pl["nbr"])
                    torch.gt(nbr["n_near"], nbr["n_rows"], out=pl["crowded"])
                    pl["n_crowded"].add_(pl["crowded"])
                if mapper is not None:
                    pl["mask"].copy_(fl["walking"])
                    mapper.update(fl["state"], sen["hits"], mask=pl["mask"])
                sv.plan_step_batch_c_eta(fl["state"], pl["goal"], fl["first_foot"], sen["c_eta"], pl["delta"], out=out,
                                         overflow=sen["overflow"])

        def finish(working):
            # ``working``: the goals the solve was given
            if rec is None:
                sv.fleet_update(fl, out, overflow=sen["overflow"], stop_obj=stop_obj)
            else:
                # the rows the solve was given (the scan's, then the neighbours') vouch for the capture step
                sv.fleet_update(fl, out, overflow=sen["overflow"], stop_obj=stop_obj,
                                recover=dict(rec, goal=working, c_eta=sen["c_eta"], delta=pl["delta"], max_recover=self.recover))
                # NaN = not evaluated in this sample (an evaluated margin is never NaN): keep the robot's last evaluated one
                torch.ne(rec["recover_margin"], rec["recover_margin"], out=pl["not_evaluated"])
                torch.where(pl["not_evaluated"], pl["last_margin"], rec["recover_margin"], out=pl["last_margin"])

        if use_graph and pl["graph"] is None:
            reset()
            if mode == "given":
                nbuf.copy_(noise[0])
            if dmode == "given":
                pl["dbuf"].copy_(drift[0])
            side = torch.cuda.Stream(dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                kept = None if mapper is None else mapper.evidence.clone()
                sample()                                     # warm-up outside capture (lazy initialisation)
                if kept is not None:
                    mapper.evidence.copy_(kept)              # the warm-up's scan is no part of the run
            torch.cuda.current_stream(dev).wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            if gen is not None:
                graph.register_generator_state(gen)          # the draw is part of the graph: every replay advances the stream
            if dgen is not None:
                graph.register_generator_state(dgen)
            with torch.cuda.graph(graph):
                sample()
            pl["graph"] = graph
        reset()
        for k in range(k_max):
            if before_sample is not None:
                before_sample(k, pl)
            if mode == "given":
                nbuf.copy_(noise[k])
            if dmode == "given":
                pl["dbuf"].copy_(drift[k])
            if use_graph:
                pl["graph"].replay()
            else:
                sample()
            if dmode is not None:
                pl["pose_error"][k].copy_(pl["perr"])
        res = dict(X_pred=fl["X_pred"], U_pred=fl["U_pred"], n_steps=fl["n_steps"], last_status=fl["last_status"],
                   overflow=fl["n_overflow"])
        if rec is not None:
            res.update(n_recover=rec["n_recover"], recover_run=rec["recover_run"], recover_margin=pl["last_margin"])
        if avoid is not None:
            res["n_crowded"] = pl["n_crowded"]
        if dmode is not None:
            res.update(drift=pl["drift"], pose_error=pl["pose_error"], n_matched=pl["n_matched"])
        return res

    def run_replanning(self, state0, goal, first_foot, k_max, planner, replan_every, lookahead, noise="seeded", noise_seed=0,
                       delta=None, stop_obj=0.05, use_graph=True, seeds=None, S_max=None, min_evidence=None, drift="seeded", drift_seed=0):
        """``run`` with a global planner on the map the fleet builds (``mapper`` is required): a robot that the reactive loop
        leaves in a dead end re-plans on what it has seen and walks out.  The loop is driven from the host, all per-robot work
        runs on the device, nothing is copied device -> host per sample.  Every ``replan_every`` samples (sample 0 included):
          - all B robots are planned in one ``planner.plan_grid_batch`` call, from their current positions to their final goals,
            on ``mapper.grid_map(min_evidence)`` (unknown cells count as free); ``seeds`` / ``S_max`` as ``plan_grid_batch``;
          - a robot that the stop rule stopped at a working goal that was not its final goal walks again (a robot that stopped
            at its final goal, or on a failed solve, stays stopped);
          - each robot's working goal becomes the first sub-goal of its path that is at least ``lookahead`` from the robot, or
            the final goal when none is or when the plan's status is anything other than RRT_FOUND (RRT_NO_OBSTACLE_GRID
            included: the map is empty, the robot heads straight for the goal; RRT_FIELD_UNSETTLED included: a tiled planner
            whose budget of rounds did not settle the field -- the next replan tries again).
        Returns what ``run`` returns, plus n_replans (int), rrt_status [B] of the last plan, working_goal [B,2] and walking [B]
        (int8) as the last sample left them: a robot ARRIVED if it is not walking, its last_status is SOLVED or UNCERTIFIED
        (the stop rule stopped it, not a failed solve) and its working goal is its final goal.
        ``drift`` / ``drift_seed``: as ``run``'s; in a fleet with a drift model every plan starts from the BELIEVED positions."""
        from .planner import RRT_FOUND
        from .solver import STATUS_SOLVED, STATUS_UNCERTIFIED
        if self.mapper is None:
            raise ValueError("run_replanning plans on the fleet's map: UnknownEnvFleet(..., mapper=OccupancyMapper(...))")
        replan_every, lookahead = int(replan_every), float(lookahead)
        if replan_every < 1 or not lookahead >= 0.0:
            raise ValueError("replan_every >= 1 and lookahead >= 0")
        if isinstance(seeds, torch.Tensor):
            seeds = seeds.cpu().numpy()                      # once, before the loop
        final = goal.to(device=self.device, dtype=torch.float64).contiguous()
        info = dict(n_replans=0, rrt_status=None)

        def replan(k, pl):
            if k % replan_every:
                return
            fl, working = pl["fl"], pl["goal"]
            pos = self._believed_positions(pl)
            plan = planner.plan_grid_batch(final, self.mapper.grid_map(min_evidence), pos, seeds=seeds, S_max=S_max)
            # stopped by the stop rule (not by a failed solve: that leaves its status), at a goal that was not the final one
            solved = (fl["last_status"] == STATUS_SOLVED) | (fl["last_status"] == STATUS_UNCERTIFIED)
            resume = (fl["walking"] == 0) & solved & (fl["last_obj"] < stop_obj) & (working != final).any(1)
            fl["walking"].masked_fill_(resume, 1)
            fl["last_obj"].masked_fill_(resume, float("inf"))          # the objective of the goal it has reached says nothing about the next
            working.copy_(select_working_goals(pos, final, plan["sub_goals"], plan["n_sub"], plan["status"], lookahead, RRT_FOUND))
            info["n_replans"] += 1
            info["rrt_status"] = plan["status"]

        res = self._run(state0, final, first_foot, k_max, noise, noise_seed, delta, stop_obj, use_graph, before_sample=replan, drift=drift,
                        drift_seed=drift_seed)
        res.update(info, working_goal=self._plan["goal"], walking=self._plan["fl"]["walking"])
        return res

    def run_exploring(self, state0, first_foot, k_max, explorer, replan_every, lookahead, noise="seeded", noise_seed=0, delta=None,
                      stop_obj=0.05, use_graph=True, S_max=None):
        """``run`` without goals: the fleet explores (``mapper`` is required; ``explorer``: a ``FrontierPlanner`` on the fleet's
        device).  Every robot walks to the nearest frontier of the map the fleet builds, until no frontier is left.  The loop is
        driven from the host, all per-robot work runs on the device, nothing is copied device -> host per sample or per replan.
        Before sample 0 one NOISE-FREE scan of ``state0`` goes into the map (without it no cell is free and nothing can be
        planned).  Every ``replan_every`` samples (sample 0 included) all robots are planned in one ``explorer.plan`` on
        ``mapper.evidence``:
          - a robot whose plan is RRT_FOUND gets as working goal the first sub-goal of its path that is at least ``lookahead``
            from it, or the frontier cell's centre when none is (``select_working_goals`` with its target as the goal);
          - a robot that is not walking, whose last_status is SOLVED or UNCERTIFIED, and whose plan is FOUND walks again: robots
            the stop rule stopped and robots parked earlier (a robot stopped by a failed solve stays stopped, as everywhere);
          - a robot whose plan is not FOUND is parked (walking = 0; it keeps its working goal).  That holds for
            RRT_FIELD_UNSETTLED too (a ``FrontierPlanner(tiled=True, rounds=n)`` whose budget did not settle the field): the robot
            walks again after a replan that settles, and since ``done`` reads RRT_NO_PATH only it never ends the fleet.
        After the last sample one closing plan on the final map and positions parks likewise and sets no goal; it is not counted.
        With a ``CoordinatedFrontierPlanner`` as ``explorer`` the robots claim frontier targets apart in every replan: the robots
        that may claim are those whose last_status is SOLVED or UNCERTIFIED -- a robot stopped for good by a failed solve must
        never hold a frontier, or the fleet never finishes -- and a robot in a capture step (``recover``) is a follower for that
        replan: it keeps its nearest-frontier plan.  The result then gains n_claims [n_replans] (device tensor: the claims of
        every replan; the closing plan's are not counted).  With any other explorer nothing changes.
        With a ``CoordinatedFrontierPlanner`` that has ``r_keep`` every replan (the closing one included) is ``explorer.replan``
        with the previous replan's targets as ``prev_target``: a robot's ``target_cell`` where that replan said RRT_FOUND, else
        -1, and -1 for everybody at the first replan; they are kept in a buffer of the fleet's own, on the device.  The result
        then gains n_kept [n_replans] (the keepers of every replan) and n_jumps [n_replans]: the robots whose target is FOUND at
        this replan and was at the previous one, and lies more than ``r_keep`` cells (Euclidean) from it.
        With an explorer whose plan dict carries ``n_regions`` (``gain_from="region"``) the result gains n_regions [n_replans,F,3]:
        per replan all regions, the kept ones and the kept ones beyond the table, of every map.  With any other explorer nothing new.
        The model's limits: with a plain ``FrontierPlanner`` every robot goes to ITS nearest frontier (no task assignment:
        ``CoordinatedFrontierPlanner`` adds it), and the walker cannot turn on the spot while walking -- a working goal that
        jumps behind a robot can make its solve INFEASIBLE.  That ends the robot's run only in a fleet without ``recover``: with
        it the robot takes a capture step and solves again (EXPLORATION_RECOVER.md).
        Returns what ``run`` returns, plus n_replans (int), explore_status [B] (RRT_*) of the closing plan, working_goal [B,2],
        walking [B] (int8), n_frontier and known_free [n_replans,F] (device tensors: per replan the frontier cells, and the cells
        with evidence <= -t_free, of every map), and done [B] (bool): not walking, not stopped by a failed solve, and the closing
        plan said RRT_NO_PATH -- for the robot nothing is left to explore.  The tensors are the object's or fresh ones; the
        next run of the same shape overwrites the former.
        In a fleet with a drift model (``run``) every plan, and the first look round, start from the BELIEVED positions; the run's
        ``drift`` and ``drift_seed`` are the fleet's ``exploring_drift`` ("seeded"; None or a tensor [k_max,B,2] as ``run`` takes
        them) and ``exploring_drift_seed`` (0), attributes to set before the call: this method's parameter list stays as it is."""
        from .planner import RRT_FOUND, RRT_NO_PATH, CoordinatedFrontierPlanner
        from .solver import STATUS_SOLVED, STATUS_UNCERTIFIED
        mapper = self.mapper
        if mapper is None:
            raise ValueError("run_exploring explores the fleet's map: UnknownEnvFleet(..., mapper=OccupancyMapper(...))")
        replan_every, lookahead, k_max = int(replan_every), float(lookahead), int(k_max)
        if replan_every < 1 or not lookahead >= 0.0:
            raise ValueError("replan_every >= 1 and lookahead >= 0")
        dev = self.device
        state0 = state0.to(device=dev, dtype=torch.float64).contiguous()
        B = state0.shape[0]
        ev = mapper.evidence if mapper.evidence.dim() == 3 else mapper.evidence[None]
        F = ev.shape[0]
        rows = (k_max + replan_every - 1) // replan_every
        t_free = mapper.w_miss if explorer.t_free is None else explorer.t_free
        n_frontier = torch.zeros((rows, F), dtype=torch.int32, device=dev)
        known_free = torch.zeros((rows, F), dtype=torch.int64, device=dev)
        plan_out = [None]                                    # the plan's buffers: made by the first plan, reused by every later one
        coordinated = isinstance(explorer, CoordinatedFrontierPlanner)
        n_claims = torch.zeros((rows,), dtype=torch.int32, device=dev) if coordinated else None
        keeping = coordinated and explorer.r_keep is not None
        if keeping:
            # the fleet's memory: every robot's target of the last replan (-1: none), and what it did to the claims
            prev = torch.full((B,), -1, dtype=torch.int32, device=dev)
            n_kept, n_jumps = (torch.zeros((rows,), dtype=torch.int32, device=dev) for _ in range(2))
        info = dict(n_replans=0)
        counts = {}                                          # n_regions [n_replans,F,3], with an explorer whose dict carries it

        def replan(k, pl, closing=False):
            if not closing and k % replan_every:
                return
            fl, working = pl["fl"], pl["goal"]
            if k == 0 and not closing:
                # the first look round, noise-free: the run's own scans start with sample 0
                self.sensor.sense(fl["state"], None, out=pl["sen"], c_eta=True, rings=False, schedule=pl["sched"])
                if "drift" in pl:
                    # (the drift is zero before sample 0: the same numbers, from the buffers the samples use)
                    believed = fl["state"].clone()
                    believed[:, (0, 2)] += pl["drift"]
                    mapper.update(believed, pl["sen"]["hits"] + pl["drift"][:, None, :])
                else:
                    mapper.update(fl["state"], pl["sen"]["hits"])
            pos = self._believed_positions(pl)
            solved = (fl["last_status"] == STATUS_SOLVED) | (fl["last_status"] == STATUS_UNCERTIFIED)
            claim = dict(may_claim=solved.to(torch.int8)) if coordinated else {}
            if keeping:
                claim["prev_target"] = prev
            plan = plan_out[0] = (explorer.replan if keeping else explorer.plan)(mapper, pos, S_max=64 if S_max is None else S_max,
                                                                                out=plan_out[0], **claim)
            found = plan["status"] == RRT_FOUND
            if not closing:
                resume = (fl["walking"] == 0) & solved & found
                fl["walking"].masked_fill_(resume, 1)
                fl["last_obj"].masked_fill_(resume, float("inf"))      # the objective of the goal it has reached says nothing about the next
                picked = select_working_goals(pos, plan["target"], plan["sub_goals"], plan["n_sub"], plan["status"], lookahead, RRT_FOUND)
                working.copy_(torch.where(found[:, None], picked, working))
                n_frontier[info["n_replans"]].copy_(plan["n_frontier"])
                known_free[info["n_replans"]].copy_((ev <= -t_free).sum((1, 2)))
                if coordinated:
                    n_claims[info["n_replans"]].copy_(plan["n_claims"][0])
                if "n_regions" in plan:
                    if "n_regions" not in counts:
                        counts["n_regions"] = torch.zeros((rows, F, 3), dtype=torch.int32, device=dev)
                    counts["n_regions"][info["n_replans"]].copy_(plan["n_regions"])
                if keeping:
                    tc, H = plan["target_cell"], ev.shape[2]
                    di = torch.div(tc, H, rounding_mode="floor") - torch.div(prev, H, rounding_mode="floor")
                    dj = torch.remainder(tc, H) - torch.remainder(prev, H)
                    jumped = found & (prev >= 0) & (di * di + dj * dj > explorer.r_keep ** 2)
                    n_jumps[info["n_replans"]].copy_(jumped.sum())
                    n_kept[info["n_replans"]].copy_(plan["n_kept"][0])
                    prev.copy_(torch.where(found, tc, torch.full_like(tc, -1)))
                info["n_replans"] += 1
            fl["walking"].masked_fill_(~found, 0)
            info["explore_status"] = plan["status"]

        res = self._run(state0, state0[:, (0, 2)], first_foot, k_max, noise, noise_seed, delta, stop_obj, use_graph, before_sample=replan,
                        drift=self.exploring_drift, drift_seed=self.exploring_drift_seed)
        fl = self._plan["fl"]
        replan(k_max, self._plan, closing=True)
        solved = (fl["last_status"] == STATUS_SOLVED) | (fl["last_status"] == STATUS_UNCERTIFIED)
        res.update(info, working_goal=self._plan["goal"], walking=fl["walking"], n_frontier=n_frontier, known_free=known_free,
                   done=(fl["walking"] == 0) & solved & (info["explore_status"] == RRT_NO_PATH))
        res.update(counts)
        if coordinated:
            res["n_claims"] = n_claims
        if keeping:
            res.update(n_kept=n_kept, n_jumps=n_jumps)
        return res


def select_working_goals(position, goal, sub_goals, n_sub, status, lookahead, found=0):
    """The goal-selection rule of ``UnknownEnvFleet.run_replanning`` on the device: per robot the first of its n_sub sub-goals
    with sqrt(dx * dx + dy * dy) >= lookahead from ``position``, else (or when status != found) its ``goal``.  position, goal
    [B,2]; sub_goals [B,S,2]; n_sub, status [B].  Restated in numpy by tests/map_oracle.py (select_goals)."""
    S = sub_goals.shape[1]
    dx, dy = sub_goals[:, :, 0] - position[:, None, 0], sub_goals[:, :, 1] - position[:, None, 1]
    dist = torch.sqrt(dx * dx + dy * dy)
    slot = torch.arange(S, device=sub_goals.device)[None, :]
    ok = (dist >= lookahead) & (slot < n_sub[:, None]) & (status == found)[:, None]
    first = torch.where(ok, slot, S).amin(1)
    pick = sub_goals[torch.arange(sub_goals.shape[0], device=sub_goals.device), first.clamp(max=S - 1)]
    return torch.where((first < S)[:, None], pick, goal)
