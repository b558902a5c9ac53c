"""Occupancy mapping: LiDAR scans integrated into an evidence grid on the device -- host wrapper of lipmpc_map_update_batch
(include/lipmpc.h).  ``OccupancyMapper.update`` adds one scan per robot (+w_hit on the cells the readings lie in, -w_miss on the
cells the rays passed through); ``grid_map`` thresholds the evidence into the ``GridMap`` that ``RrtStarPlanner.plan_grid_batch``
plans on and a grid sensor scans.  ``UnknownEnvFleet(..., mapper=OccupancyMapper(...))`` does the update every sample."""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib
from .lidar import GridMap, ray_table
from .solver import _check

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
