"""Neighbour LDCBF rows: the robots of one launch as each other's obstacles -- host wrapper of
lipmpc_neighbour_c_eta_batch (include/lipmpc.h).  ``NeighbourRows.append`` finds every robot's nearest neighbours among the B
robots of the batch and appends one half-space row per neighbour to its c_eta, after the rows of a LiDAR scan or on their own;
``BatchedLipMpc.plan_step_batch_c_eta`` solves against the result.  ``UnknownEnvFleet(..., avoid=NeighbourRows(...))`` does
this every sample."""
from __future__ import annotations

import math

import torch

from . import _lib
from .solver import _alloc, _check, _check_table, _named

K_ROWS_MAX = 16


def neighbour_outputs(B, k_rows):
    """Outputs of ``NeighbourRows.append`` next to c_eta, in the order it returns them."""
    i32 = torch.int32
    return {"n_rows": (i32, (B,), True), "n_near": (i32, (B,), True), "neighbours": (i32, (B, k_rows), False)}


NEIGHBOUR_OUTPUTS = tuple(neighbour_outputs(0, 0))                               # the names


class NeighbourRows:
    """``radius``: body radius, one float for every robot or a [B] tensor; ``sense_range``: a neighbour closer than this
    (strictly) is in range; ``k_rows``: rows per robot at most (1..16), nearest first; ``share``: 0.5 = the reciprocal model
    (each robot of a pair keeps to its half of the free space between the two discs: buffered Voronoi cell), 0 = the neighbour
    as a static disc.  The row model, the order and what is written where: include/lipmpc.h."""

    def __init__(self, radius=0.25, sense_range=1.5, k_rows=4, share=0.5, device=None):
        if not torch.cuda.is_available():
            raise RuntimeError("lipmpc needs a HIP device (torch.cuda.is_available() is False); there is no CPU path")
        self.lib = _lib.load()
        self.device_index = torch.cuda.current_device() if device is None else int(device)
        self.device = torch.device("cuda", self.device_index)
        self.sense_range, self.k_rows, self.share = float(sense_range), int(k_rows), float(share)
        if not 1 <= self.k_rows <= K_ROWS_MAX:
            raise ValueError(f"k_rows must be 1..{K_ROWS_MAX}")
        if not (0.0 < self.sense_range < math.inf) or not 0.0 <= self.share <= 1.0:
            raise ValueError("sense_range must be positive and finite, share in [0, 1]")
        if isinstance(radius, torch.Tensor):
            self._radius, self._radius_for = radius.to(device=self.device, dtype=torch.float64).contiguous(), None
        else:
            self._radius, self._radius_for = float(radius), {}            # B -> [B] tensor of the scalar
        self._ws_by_stream = {}                    # stream -> (workspace, capacity) of the eager calls on it: grow-only
        self._kept = []                            # workspaces of captured calls: a graph holds the pointer

    def radius(self, B):
        """The [B] radius tensor of a batch of B robots."""
        if self._radius_for is None:
            _check(self._radius, (B,), torch.float64, self.device, "radius", required=True)
            return self._radius
        if B not in self._radius_for:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("NeighbourRows: the first call for a batch size fills its radius tensor, which cannot happen "
                                   "during a graph capture: run one append of that size before capturing")
            self._radius_for[B] = torch.full((B,), self._radius, dtype=torch.float64, device=self.device)
        return self._radius_for[B]

    def alloc_outputs(self, B, with_neighbours=True):
        table = neighbour_outputs(B, self.k_rows)
        return _alloc(table, [k for k, (_, _, required) in table.items() if required or with_neighbours], self.device, torch.zeros)

    def _workspace(self, B):
        """The workspace of this call: the current stream's (grow-only), or, while a graph is being captured, one that belongs
        to the captured call alone -- as the solver's split-launch workspace."""
        nbytes = int(self.lib.lipmpc_neighbour_workspace_bytes(B))
        if nbytes < 0:
            raise ValueError(f"NeighbourRows: a batch of {B} robots is out of range")
        new = lambda: torch.empty((nbytes,), dtype=torch.uint8, device=self.device)
        if torch.cuda.is_current_stream_capturing():
            self._kept.append(new())
            return self._kept[-1]
        key = torch.cuda.current_stream(self.device).cuda_stream
        ws, cap = self._ws_by_stream.get(key, (None, 0))
        if B > cap:
            ws, cap = new(), B
            self._ws_by_stream[key] = (ws, cap)
        return ws

    def append(self, state, c_eta, first_slot=None, group=None, out=None):
        """state [B,5] (only p_x, p_y are read); c_eta [B,n_obs_max,4]: the rows are appended IN PLACE from slot
        first_slot[b] on (first_slot [B] int32, e.g. a scan's n_inferred; None = 0), the slots behind them zeroed, the slots
        before them untouched; group [B] int32 or None: only robots of equal group see each other, group < 0 = absent.
        Returns dict(n_rows [B], n_near [B] (n_near > n_rows: a neighbour in range got no row), neighbours [B,k_rows]
        (index per row, -1 beyond n_rows)) -- ``out`` or new tensors.  Asynchronous on the current stream; can be captured
        in a graph."""
        dev = self.device
        B = state.shape[0]
        _check(state, (B, 5), torch.float64, dev, "state", required=True)
        if c_eta is None or c_eta.dim() != 3 or not 1 <= c_eta.shape[1] <= 50:
            raise ValueError("c_eta: [B,n_obs_max,4] with 1..50 slots")
        n_obs_max = int(c_eta.shape[1])
        _check(c_eta, (B, n_obs_max, 4), torch.float64, dev, "c_eta", required=True)
        _check(first_slot, (B,), torch.int32, dev, "first_slot")
        _check(group, (B,), torch.int32, dev, "group")
        if out is None:
            out = self.alloc_outputs(B)
        else:
            _check_table(neighbour_outputs(B, self.k_rows), out, dev, "out")
        if B == 0:
            return out
        _lib.call("lipmpc_neighbour_c_eta_batch", device=self.device_index, B=B, n_obs_max=n_obs_max, k_rows=self.k_rows,
                  sense_range=self.sense_range, share=self.share, state=state, radius=self.radius(B), group=group,
                  first_slot=first_slot, workspace=self._workspace(B), c_eta=c_eta, **_named(out, NEIGHBOUR_OUTPUTS),
                  hip_stream=torch.cuda.current_stream(dev).cuda_stream)
        return out
