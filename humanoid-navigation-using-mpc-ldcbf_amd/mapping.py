"""Occupancy mapping: LiDAR scans integrated into an evidence grid on the device -- host wrapper of lipmpc_map_update_batch
(include/lipmpc.h).  ``OccupancyMapper.update`` adds one scan per robot (+w_hit on the cells the readings lie in, -w_miss on the
cells the rays passed through); ``grid_map`` thresholds the evidence into the ``GridMap`` that ``RrtStarPlanner.plan_grid_batch``
plans on and a grid sensor scans.  ``UnknownEnvFleet(..., mapper=OccupancyMapper(...))`` does the update every sample.
``ScanMatcher.match`` (lipmpc_scan_match_batch) finds where a scan fits the evidence best: the pose correction of a fleet whose
odometry drifts (``UnknownEnvFleet(..., mapper=, drift_sigma=, matcher=ScanMatcher(...))``)."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .lidar import GridMap, ray_table
from .solver import _alloc, _check, _check_table, _named

WEIGHT_MAX = 32767


class OccupancyMapper:
    """An evidence grid of ``W`` x ``H`` cells of size ``cell`` (one float or (dx, dy)) at ``origin`` -- the cell rectangles and
    the layout of a ``GridMap`` -- for scans of ``resolution`` rays of range ``lidar_range``.  ``per_robot=None``: one map that
    every robot adds into (integer atomics: the result does not depend on the order); ``per_robot=B``: one map per robot of
    batches of B.  ``w_hit`` / ``w_miss``: what a cell gains when a reading lies in it / loses when a ray passes through it
    (1..32767).  ``depth``: how far a reading is pushed along its ray before it is given a cell (default: half the smaller
    cell size; a grid scan's reading lies exactly on the face of its wall).  The update rule: include/lipmpc.h."""

    def __init__(self, W, H, origin, cell, lidar_range, resolution=360, per_robot=None, w_hit=3, w_miss=1, depth=None, device=None):
        if not torch.cuda.is_available():
            raise RuntimeError("lipmpc needs a HIP device (torch.cuda.is_available() is False); there is no CPU path")
        self.lib = _lib.load()
        self.device_index = torch.cuda.current_device() if device is None else int(device)
        self.device = torch.device("cuda", self.device_index)
        self.W, self.H, self.resolution = int(W), int(H), int(resolution)
        self.origin = (float(origin[0]), float(origin[1]))
        self.cell = (float(cell), float(cell)) if isinstance(cell, (int, float)) else (float(cell[0]), float(cell[1]))
        self.lidar_range = float(lidar_range)
        self.depth = 0.5 * min(self.cell) if depth is None else float(depth)
        self.w_hit, self.w_miss = int(w_hit), int(w_miss)
        self.per_robot = None if per_robot is None else int(per_robot)
        if self.W < 1 or self.H < 1 or not 1 <= self.resolution <= 384:
            raise ValueError("W, H >= 1 and resolution in 1..384")
        if not all(0.0 < c < math.inf for c in self.cell) or not all(math.isfinite(o) for o in self.origin):
            raise ValueError("cell sizes must be positive and finite, the origin finite")
        if not (0.0 <= self.lidar_range < math.inf) or not (0.0 <= self.depth < math.inf):
            raise ValueError("lidar_range and depth must be non-negative and finite")
        if not (1 <= self.w_hit <= WEIGHT_MAX and 1 <= self.w_miss <= WEIGHT_MAX):
            raise ValueError(f"w_hit and w_miss must be 1..{WEIGHT_MAX}")
        if self.per_robot is not None and self.per_robot < 1:
            raise ValueError("per_robot: None (a shared map) or the batch size")
        self._origin_c, self._cell_c = (C.c_double * 2)(*self.origin), (C.c_double * 2)(*self.cell)      # read by the C call
        shape = (self.W, self.H) if self.per_robot is None else (self.per_robot, self.W, self.H)
        self.evidence = torch.zeros(shape, dtype=torch.int32, device=self.device)
        self.table = torch.as_tensor(ray_table(self.resolution), device=self.device)

    shared = property(lambda self: self.per_robot is None)

    def reset(self):
        """Forget everything (evidence to zero, in place: a captured update keeps its pointer)."""
        self.evidence.zero_()

    def update(self, state, hits, mask=None):
        """One scan per robot into the evidence: state [B,5] (only p_x, p_y are read), hits [B,resolution,2] as a scan writes them
        (``sense(..., with_debug=True)["hits"]``, NaN = no reading), mask [B] int32 or None (0 = skip the robot).  Asynchronous
        on the current stream; makes no allocation, so it can be captured in a graph.  Returns ``evidence``."""
        dev = self.device
        B = state.shape[0]
        _check(state, (B, 5), torch.float64, dev, "state", required=True)
        _check(hits, (B, self.resolution, 2), torch.float64, dev, "hits", required=True)
        _check(mask, (B,), torch.int32, dev, "mask")
        if self.per_robot is not None and B != self.per_robot:
            raise ValueError(f"a mapper of {self.per_robot} per-robot maps takes batches of that size, not {B}")
        _lib.call("lipmpc_map_update_batch", device=self.device_index, B=B, resolution=self.resolution, W=self.W, H=self.H,
                  grid_shared=int(self.shared), origin=C.addressof(self._origin_c), cell=C.addressof(self._cell_c),
                  lidar_range=self.lidar_range, depth=self.depth, w_hit=self.w_hit, w_miss=self.w_miss, state=state, hits=hits,
                  ray_table=self.table, mask=mask, evidence=self.evidence, hip_stream=torch.cuda.current_stream(dev).cuda_stream)
        return self.evidence

    def grid_map(self, min_evidence=None):
        """The map as a ``GridMap`` on the mapper's device: solid where evidence >= min_evidence (default w_hit: one reading
        more than the passes that crossed the cell); unknown cells are free."""
        thr = self.w_hit if min_evidence is None else int(min_evidence)
        return GridMap(self.evidence >= thr, self.origin, self.cell)

    def free_map(self, max_evidence=None):
        """The cells KNOWN to be free as a ``GridMap`` (nonzero = free): evidence <= max_evidence (default -w_miss)."""
        thr = -self.w_miss if max_evidence is None else int(max_evidence)
        return GridMap(self.evidence <= thr, self.origin, self.cell)


def match_outputs(B):
    """The outputs of lipmpc_scan_match_batch: name -> (dtype, shape, required)."""
    return {"offset_cells": (torch.int32, (B, 2), True), "yaw_index": (torch.int32, (B,), True), "offset": (torch.float64, (B, 2), True),
            "score": (torch.int32, (B, 2), True), "n_used": (torch.int32, (B,), True), "matched": (torch.int8, (B,), True)}


class ScanMatcher:
    """A correlative scan matcher on a mapper's evidence (lipmpc_scan_match_batch): where is a robot on the map it builds?  Every
    whole-cell shift (a, b) with |a| <= ``n_x``, |b| <= ``n_y`` of the believed position -- and, with ``n_yaw`` > 0, every yaw
    (k - n_yaw) * ``yaw_step`` of the scan about it -- is scored by the evidence, clamped to +-``clamp`` (1..127), under the
    scan's hit cells; the best candidate is accepted if its score is at least ``min_score`` and beats the unshifted scan's by at
    least ``min_gain`` (>= 0).  The three scoring parameters have no defaults: nobody has measured one.  n_x, n_y, n_yaw: 0..16.
    The rule: include/lipmpc.h."""

    N_MAX, CLAMP_MAX = 16, 127

    def __init__(self, n_x, n_y, *, clamp, min_score, min_gain, n_yaw=0, yaw_step=None):
        self.n_x, self.n_y, self.n_yaw = int(n_x), int(n_y), int(n_yaw)
        self.clamp, self.min_score, self.min_gain = int(clamp), int(min_score), int(min_gain)
        if not all(0 <= n <= self.N_MAX for n in (self.n_x, self.n_y, self.n_yaw)):
            raise ValueError(f"n_x, n_y and n_yaw must be 0..{self.N_MAX}")
        if not 1 <= self.clamp <= self.CLAMP_MAX or self.min_gain < 0 or not -2 ** 31 <= self.min_score < 2 ** 31:
            raise ValueError(f"clamp must be 1..{self.CLAMP_MAX}, min_gain >= 0, min_score an int32")
        if self.n_yaw and (yaw_step is None or not math.isfinite(float(yaw_step))):
            raise ValueError("n_yaw > 0 needs a finite yaw_step")
        self.yaw_step = None if yaw_step is None else float(yaw_step)
        # (cos, sin) of (k - n_yaw) * yaw_step, evaluated once on the host: the kernel takes the table, it calls no cos or sin
        self.rot = None
        if self.n_yaw:
            ang = (np.arange(2 * self.n_yaw + 1) - self.n_yaw).astype(np.float64) * np.float64(self.yaw_step)
            self.rot = np.stack([np.cos(ang), np.sin(ang)], axis=1)
        self._tables = {}                                    # device -> the table there

    def alloc_outputs(self, B, device):
        table = match_outputs(B)
        return _alloc(table, table, device)

    def _rot_on(self, device):
        if self.rot is None:
            return None
        if device not in self._tables:
            self._tables[device] = torch.as_tensor(self.rot, device=device)
        return self._tables[device]

    def match(self, mapper, state, hits, mask=None, out=None):
        """Match one scan per robot against ``mapper.evidence``: state [B,5] the BELIEVED pose (only p_x, p_y are read), hits
        [B,resolution,2] the readings as placed at that pose (NaN = no reading), mask [B] int32 or None (0 = the robot gets
        zeros).  Geometry, lidar_range, depth and resolution are the mapper's.  Returns dict(offset_cells [B,2] int32, yaw_index
        [B] int32, offset [B,2] float64 = the shift in map units, score [B,2] int32 (best before the acceptance test, unshifted),
        n_used [B] int32, matched [B] int8) -- ``out`` when given (``alloc_outputs``): then the call makes no allocation and can
        be captured in a graph (with n_yaw > 0 after one call outside the capture: the first puts the yaw table on the device).
        Asynchronous on the current stream; the evidence is only read."""
        dev = mapper.device
        B = state.shape[0]
        _check(state, (B, 5), torch.float64, dev, "state", required=True)
        _check(hits, (B, mapper.resolution, 2), torch.float64, dev, "hits", required=True)
        _check(mask, (B,), torch.int32, dev, "mask")
        if mapper.per_robot is not None and B != mapper.per_robot:
            raise ValueError(f"a mapper of {mapper.per_robot} per-robot maps takes batches of that size, not {B}")
        if out is None:
            out = self.alloc_outputs(B, dev)
        else:
            _check_table(match_outputs(B), out, dev, "out")
        _lib.call("lipmpc_scan_match_batch", device=mapper.device_index, B=B, resolution=mapper.resolution, W=mapper.W, H=mapper.H,
                  grid_shared=int(mapper.shared), origin=C.addressof(mapper._origin_c), cell=C.addressof(mapper._cell_c),
                  lidar_range=mapper.lidar_range, depth=mapper.depth, n_x=self.n_x, n_y=self.n_y, n_yaw=self.n_yaw,
                  rot_table=self._rot_on(dev), clamp=self.clamp, min_score=self.min_score, min_gain=self.min_gain, state=state,
                  hits=hits, mask=mask, evidence=mapper.evidence, **_named(out, match_outputs(B)),
                  hip_stream=torch.cuda.current_stream(dev).cuda_stream)
        return out
