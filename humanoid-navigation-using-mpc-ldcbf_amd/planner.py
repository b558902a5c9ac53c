"""Batched RRT* sub-goal planner on the device: the global planner of the reference's HumanoidMPCWithRRT
(HumanoidMPCVariants/HumanoidMPCWithRRT.py:21-135) as ``lipmpc_rrt_plan_batch`` (include/lipmpc.h).

``RrtStarPlanner.plan_batch`` plans B problems in one call and returns ``sub_goals [B,S_max,2]`` / ``n_sub [B]`` in the form
``BatchedLipMpc.rollout_subgoals`` takes them; an instance is also the ``planner=`` of ``HumanoidMPCWithRRT``.

``GridFieldPlanner`` is the complete, deterministic planner on a given grid: a cost-to-go field from the goal
(``lipmpc_grid_field_batch``) and sub-goals down it (``lipmpc_grid_path_batch``), in the same output form.

``FrontierPlanner`` needs no goal: on the evidence grid an ``OccupancyMapper`` builds it finds the frontier of the known free
space, the cost-to-go to the nearest frontier cell (``lipmpc_grid_frontier_field_batch``) and sub-goals down it
(``lipmpc_grid_frontier_path_batch``).

``CoordinatedFrontierPlanner`` is ``FrontierPlanner`` for a fleet on one shared map: after the two calls the robots claim frontier
targets apart, nearest claim first (``lipmpc_grid_frontier_assign_batch``).

``InformedFrontierPlanner`` is ``FrontierPlanner`` with a utility from expected visibility: the unknown cells a robot would see
from every frontier cell (``lipmpc_grid_frontier_gain_batch``), a cost-to-go field whose sources start ahead by that gain
(``lipmpc_grid_frontier_utility_field_batch``) and sub-goals down it (``lipmpc_grid_frontier_utility_path_batch``).

``TiledCoordinatedFrontierPlanner`` and ``TiledInformedFrontierPlanner`` are those two on maps of up to 2^24 cells: the same outputs
by the tiled calls (``lipmpc_grid_frontier_assign_tiled_batch``; ``lipmpc_grid_frontier_gain_tiled_batch``,
``lipmpc_grid_frontier_utility_field_tiled_batch``, ``lipmpc_grid_frontier_utility_path_tiled_batch``).
"""
from __future__ import annotations

import ctypes as C
import functools
import inspect

import numpy as np
import torch

from . import _lib
from .solver import _alloc, _check_table, _named, pack_rings

RRT_FOUND, RRT_NO_PATH, RRT_START_OCCUPIED, RRT_GOAL_OCCUPIED, RRT_GRID_TOO_LARGE, RRT_NO_OBSTACLE_GRID, \
    RRT_PATH_OVERFLOW, RRT_OUTSIDE_GRID, RRT_FIELD_UNSETTLED = range(9)
RRT_STATUS_NAMES = ("FOUND", "NO_PATH", "START_OCCUPIED", "GOAL_OCCUPIED", "GRID_TOO_LARGE", "NO_OBSTACLE_GRID",
                    "PATH_OVERFLOW", "OUTSIDE_GRID", "FIELD_UNSETTLED")


FIELD_INF = 0xFFFFFFFF      # LIPMPC_FIELD_INF: a cell of a field that is blocked or has no path to the goal
FIELD_NO_CAP = 0x7FFFFFFF   # max_seg of "no spacing cap": no field value reaches it (a field stays below 7 * 2^17); the weighted
                            # path calls compare it with the length in steps alone, which stays below 7 * 2^24


def tiled_info():
    """(tile_w, tile_h, max_cells) of the tiled field calls (lipmpc_grid_tiled_info): a tile's cells along i and along j, and the
    cap on W * H.  Host only."""
    tw, th, cap = C.c_int32(), C.c_int32(), C.c_int64()
    _lib.call("lipmpc_grid_tiled_info", tile_w=C.addressof(tw), tile_h=C.addressof(th), max_cells=C.addressof(cap))
    return tw.value, th.value, cap.value


COST_MAX, R_CLEAR_MAX = 248, 31     # LIPMPC_COST_MAX; the largest r_clear (a disc row of 63 bits is one 64-bit window)


class _TiledKeywords(type):
    """The keyword-only ``tiled`` / ``rounds`` / ``r_clear`` / ``w_clear`` / ``paths`` / ``gain_from`` / ``target`` of the two field planners, taken off before
    ``__init__`` runs: the classes' ``__init__`` signatures -- which callers hand on positionally and through ``**kwargs`` -- stay what
    they were."""

    def __call__(cls, *args, tiled: bool = False, rounds: int | None = None, r_clear: int | None = None, w_clear: int | None = None,
                 paths: str = "lane", gain_from: str | None = None, target: str | None = None, **kwargs):
        self = cls.__new__(cls)
        self._init_paths(paths)
        self._init_tiled(tiled, rounds)
        self._init_clearance(r_clear, w_clear)
        self._init_regions(gain_from, target, kwargs)
        self.__init__(*args, **kwargs)
        return self


def _cost_keyword(method):
    """The keyword-only ``cost`` of ``field()``, ``plan_grid_batch()`` and ``plan()``: a caller's uint8 layer [M,W,H] (or [W,H] for
    one map) in place of the clearance layer, taken off before the method runs so that its signature stays what it was."""

    @functools.wraps(method)
    def with_cost(self, *args, cost=None, **kwargs):
        if cost is None:
            return method(self, *args, **kwargs)
        if not self._CLEARANCE or not self.tiled:
            raise ValueError(f"{type(self).__name__}: cost= needs GridFieldPlanner or FrontierPlanner with tiled=True (the weighted "
                             f"fields run on the tiled rounds only; the coordinated and the informed planners are unweighted)")
        self._given_cost = cost
        try:
            return method(self, *args, **kwargs)
        finally:
            self._given_cost = None
    return with_cost


class _TiledRounds(metaclass=_TiledKeywords):
    """What ``GridFieldPlanner`` and ``FrontierPlanner`` share with ``tiled=True``: the workspace of the tiled field calls (grown
    only, every buffer kept alive: work enqueued on an earlier one may still run; never reallocated while the stream is capturing)
    and the rounds.  ``rounds`` = an int: ONE call with that budget, no synchronisation, capturable; None: a budget from the
    round guarantee for an open map, then resumes with a doubled budget until every field is settled -- ``settled`` is read on the
    host, so this raises under stream capture."""

    _TILED = True               # False: a subclass whose further calls keep the one-workgroup cap
    _CLEARANCE = True           # False: a subclass whose further fields (claim rounds, utility field) are unweighted
    _given_cost = None          # the ``cost=`` of the call that is running (_cost_keyword)

    def _init_tiled(self, tiled, rounds):
        self.tiled, self.rounds = bool(tiled), None if rounds is None else int(rounds)
        if self.tiled and not self._TILED:
            raise ValueError(f"{type(self).__name__}: tiled=True is not supported ({self._TILED_WHY} the cap of 2^17 cells; "
                             f"the large-map class is {self._TILED_CLASS})")
        if self.rounds is not None and (not self.tiled or not 1 <= self.rounds <= 65536):
            raise ValueError(f"rounds {rounds}: 1..65536 or None, with tiled=True only")
        self._works = []            # every workspace ever handed to a call; the last one is the current one

    def _init_paths(self, paths):
        """WAVE-PER-ROBOT PATH CALLS (include/lipmpc.h): ``paths`` = "lane" (default), every path call is the one-lane call of the
        planner's form; "wave": the wave call of the same contract in its place -- the same output dict, bit for bit, the same buffers
        and stream, capturable wherever the lane form is.  It governs the planner's own path call (``plan_grid_batch`` / ``plan``); the
        walks inside the coordinated planners' claim calls stay one lane per robot."""
        if paths not in ("lane", "wave"):
            raise ValueError(f"paths {paths!r}: 'lane' (one lane per robot, the default) or 'wave' (one wavefront per robot)")
        self.paths = paths

    def _init_clearance(self, r_clear, w_clear):
        """SOFT CLEARANCE (include/lipmpc.h): ``r_clear`` 1..31 cells and ``w_clear`` 0..248, both or neither, no defaults (nobody
        has measured one).  With them every field is the WEIGHTED one over the clearance layer of the map."""
        self._costs = []            # the clearance layer's buffer: grown only, every buffer kept alive
        self.r_clear = self.w_clear = None
        if r_clear is None and w_clear is None:
            return
        if not self._CLEARANCE:
            raise ValueError(f"{type(self).__name__}: r_clear / w_clear are not supported (the claim rounds and the utility field are "
                             f"unweighted; soft clearance is GridFieldPlanner's and FrontierPlanner's, with tiled=True)")
        if r_clear is None or w_clear is None:
            raise ValueError("r_clear and w_clear go together: they have no defaults, nobody has measured one")
        if not self.tiled:
            raise ValueError("r_clear / w_clear need tiled=True: the weighted fields run on the tiled rounds only")
        self.r_clear, self.w_clear = int(r_clear), int(w_clear)
        if not 1 <= self.r_clear <= R_CLEAR_MAX or not 0 <= self.w_clear <= COST_MAX:
            raise ValueError(f"invalid clearance parameters (r_clear {r_clear}: 1..{R_CLEAR_MAX}, w_clear {w_clear}: 0..{COST_MAX})")

    region_rows = 1024          # R_max of the regions call a planner with gain_from="region" makes inside its plans

    _REGIONS = True             # False: a subclass that refuses gain_from / target whatever its keywords
    _GAIN_CALL = False          # True: a subclass that issues the gain call whatever its keywords

    def _init_regions(self, gain_from, target, keywords=()):
        """FRONTIER REGIONS (include/lipmpc.h): ``gain_from`` = "view" (the ray-marched visibility gain) / "region" (the size of the
        frontier cell's region, by ``lipmpc_grid_frontier_regions_batch`` with min_size = max(min_gain, 1): ``r_view`` must be None)
        and ``target`` = "cell" / "representative" (with "region" only: ``rep`` -- one cell per tabled region, the one nearest its
        centroid -- stands where the utility field, the utility path and the claim call take ``frontier``; the nearest-frontier field
        still comes from the real frontier).  Not given: "view" and "cell", no call and no bit changes.  The planners that issue
        the gain call take them; every other planner, and one with ``r_clear`` / ``w_clear``, refuses them."""
        if gain_from not in (None, "view", "region"):
            raise ValueError(f"gain_from {gain_from!r}: 'view' (the visibility gain, the default) or 'region' (the region's size)")
        if target not in (None, "cell", "representative"):
            raise ValueError(f"target {target!r}: 'cell' (the default) or 'representative' (one cell per region)")
        if target == "representative" and gain_from != "region":
            raise ValueError("target='representative' needs gain_from='region': the representatives are the regions call's")
        self.gain_from, self.target = gain_from or "view", target or "cell"
        self._region_works = []     # the regions call's workspace: grown only, every buffer kept alive
        if gain_from is None and target is None:
            return
        if self.r_clear is not None:
            raise ValueError(f"{type(self).__name__}: gain_from / target with r_clear / w_clear are not supported (regions with soft "
                             f"clearance are out of scope)")
        gain_call = self._GAIN_CALL or any(dict(keywords).get(k) is not None for k in ("w_gain", "g_cap"))
        if not gain_call or not self._REGIONS:
            raise ValueError(f"{type(self).__name__}: gain_from / target are not supported (they replace the gain call, which this "
                             f"planner does not issue: the informed planners and the coordinated ones with the gain keywords do)")

    def _region_table(self, F, W, H):
        """What a plan dict gains with gain_from="region": label, rep [F,W,H], table [F,region_rows,5], n_regions [F,3]."""
        if self.gain_from != "region":
            return {}
        table = regions_outputs(F, W, H, self.region_rows)
        return {k: table[k] for k in ("label", "rep", "table", "n_regions")}

    def _regions_call(self, F, W, H, min_size, R_max, out, size):
        """ONE lipmpc_grid_frontier_regions_batch on the current stream from out["frontier"] into out's label / rep / table /
        n_regions and ``size``, in the planner's own workspace."""
        name = "lipmpc_grid_frontier_regions_workspace_bytes"
        work = self._workspace(self._region_works, int(getattr(self.lib, name)(F, W, H, R_max)), name)
        _lib.call("lipmpc_grid_frontier_regions_batch", device=self.device_index, F=F, W=W, H=H, frontier=out["frontier"],
                  min_size=min_size, R_max=R_max, work=work, work_bytes=work.numel(), label=out["label"], size=size, rep=out["rep"],
                  table=out["table"], n_regions=out["n_regions"], hip_stream=torch.cuda.current_stream(self.device).cuda_stream)

    def _region_gain(self, ev, out):
        """gain := size: the regions call in the gain call's place (min_gain acts as the minimum size)."""
        F, W, H = ev.shape
        self._regions_call(F, W, H, max(self.min_gain, 1), self.region_rows, out, out["gain"])

    def _sources(self, out):
        """What stands where the utility field, the utility path and the claim call take ``frontier``."""
        return out["rep"] if self.target == "representative" else out["frontier"]

    def _clearance(self, M, W, H, occ=None, evidence=None, t_occ=0):
        """The clearance layer [M,W,H] uint8 of M maps given as occ bytes or as evidence, in the planner's own buffer."""
        if self.r_clear is None:
            raise ValueError("the planner has no r_clear / w_clear")
        need = M * W * H
        if not self._costs or self._costs[-1].numel() < need:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("the clearance layer's buffer must grow: run the call once before the capture")
            self._costs.append(torch.empty(need, dtype=torch.uint8, device=self.device))
        cost = self._costs[-1][:need].view(M, W, H)
        _lib.call("lipmpc_grid_clearance_cost_batch", device=self.device_index, M=M, W=W, H=H, occ=occ, evidence=evidence, t_occ=t_occ,
                  r_clear=self.r_clear, w_clear=self.w_clear, cost=cost, hip_stream=torch.cuda.current_stream(self.device).cuda_stream)
        return cost

    def _layer(self, M, W, H, **solid):
        """The cost layer of a call [M,W,H] -- the caller's ``cost=``, else the clearance layer -- or None: an unweighted planner."""
        cost = self._given_cost
        if cost is None:
            return None if self.r_clear is None else self._clearance(M, W, H, **solid)
        if not isinstance(cost, torch.Tensor) or cost.dtype != torch.uint8 or cost.device != self.device or not cost.is_contiguous() or \
                tuple(cost.shape) not in ((M, W, H),) + (((W, H),) if M == 1 else ()):
            raise ValueError(f"cost: a contiguous uint8 tensor [{M},{W},{H}]{' or [W,H]' if M == 1 else ''} on the planner's device")
        return cost.view(M, W, H)

    def _settled(self, out, F, key="settled"):
        """out[key] [F] int32, made if the caller's dict has none."""
        t = out.get(key)
        if t is None:
            t = out[key] = torch.empty((F,), dtype=torch.int32, device=self.device)
        elif t.shape != (F,) or t.dtype != torch.int32 or t.device != self.device or not t.is_contiguous():
            raise ValueError(f"out['{key}'] must be a contiguous int32 tensor [{F}] on the planner's device")
        return t

    def _workspace(self, works, need, what):
        """The current buffer of the grow-only list ``works``, of at least ``need`` bytes (< 0: the size call's refusal)."""
        if need < 0:
            _lib.check(need, what)
        if not works or works[-1].numel() < need:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("the tiled workspace must grow: run the call once before the capture")
            works.append(torch.empty(need, dtype=torch.uint8, device=self.device))
        return works[-1]

    def _run_tiled(self, name, F, W, H, out, works=None, key="settled", **args):
        """One tiled field call by the ``rounds`` rule.  ``works``: the call's own workspace list (default: the planner's first);
        ``key``: where in ``out`` its ``settled`` goes."""
        capturing = torch.cuda.is_current_stream_capturing()
        if self.rounds is None and capturing:
            raise RuntimeError("rounds=None reads `settled` on the host: give the planner a fixed `rounds` to capture its calls")
        work = self._workspace(self._works if works is None else works, int(self.lib.lipmpc_grid_tiled_workspace_bytes(F, W, H)),
                               "lipmpc_grid_tiled_workspace_bytes")
        settled = self._settled(out, F, key)
        stream = torch.cuda.current_stream(self.device).cuda_stream

        def call(budget, resume):
            _lib.call(name, device=self.device_index, F=F, W=W, H=H, **args, work=work, work_bytes=work.numel(), max_rounds=budget,
                      resume=resume, settled=settled, hip_stream=stream)
        if self.rounds is not None:
            return call(self.rounds, 0)
        tw, th, _ = tiled_info()
        budget = max(8, -(-W // tw) - (-H // th) + 1)
        call(budget, 0)
        while F and not bool(settled.all()):           # (ends: every round but the last lowers a word, and words are bounded below)
            budget = min(2 * budget, 65536)
            call(budget, 1)


MIN_SIZE_MAX, R_MAX_MAX = 1 << 24, 1 << 20     # the regions call's ranges


def regions_outputs(F, W, H, R_max):
    """Outputs of lipmpc_grid_frontier_regions_batch (``frontier_regions``, ``FrontierPlanner.regions``)."""
    i32 = torch.int32
    return {"label": (i32, (F, W, H), True), "size": (i32, (F, W, H), True), "rep": (torch.uint8, (F, W, H), True),
            "table": (i32, (F, R_max, 5), True), "n_regions": (i32, (F, 3), True)}


def _region_args(min_size, R_max):
    min_size, R_max = int(min_size), int(R_max)
    if not 1 <= min_size <= MIN_SIZE_MAX or not 0 <= R_max <= R_MAX_MAX:
        raise ValueError(f"invalid region parameters (min_size {min_size}: 1..2^24, R_max {R_max}: 0..2^20)")
    return min_size, R_max


def frontier_regions(frontier, min_size: int = 1, R_max: int = 1024, out=None):
    """The frontier REGIONS of a given mask (include/lipmpc.h, lipmpc_grid_frontier_regions_batch): ``frontier`` a contiguous uint8
    tensor [W,H] or [F,W,H] on a HIP device, any non-zero byte a frontier cell.  A region is a maximal 8-connected set of frontier
    cells.  Returns dict(label [F,W,H] int32: -1 off the frontier, else the region's least flat index; size [F,W,H] int32: the
    region's cell count, 0 off the frontier -- the layout and dtype of the gain call's ``gain``; rep [F,W,H] uint8: 1 on the
    representative of every tabled region; table [F,R_max,5] int32: per kept region (size >= ``min_size``) in ascending root order
    (root, size, centroid_cell, rep_cell, 0), rows past min(kept, R_max) untouched (0 in a fresh dict); n_regions [F,3]: all, kept,
    kept beyond R_max; work: the call's workspace, which lives with the outputs so that calls on two streams use two of them).
    ``out``: that dict, to write into (a captured graph replays into the same buffers; nothing is allocated then).  Asynchronous on
    the current stream; nine launches whatever the mask holds."""
    if not isinstance(frontier, torch.Tensor) or frontier.dtype != torch.uint8 or not frontier.is_cuda or not frontier.is_contiguous() or \
            frontier.dim() not in (2, 3):
        raise ValueError("frontier: a contiguous uint8 tensor [W,H] or [F,W,H] on a HIP device")
    min_size, R_max = _region_args(min_size, R_max)
    fr = frontier if frontier.dim() == 3 else frontier[None]
    F, W, H = fr.shape
    lib = _lib.load()
    need = int(lib.lipmpc_grid_frontier_regions_workspace_bytes(F, W, H, R_max))
    if need < 0:
        _lib.check(need, "lipmpc_grid_frontier_regions_workspace_bytes")
    table = dict(regions_outputs(F, W, H, R_max), work=(torch.uint8, (need,), True))
    if out is None:
        out = _alloc(table, ("label", "size", "rep", "n_regions", "work"), fr.device)
        out["table"] = torch.zeros(table["table"][1], dtype=torch.int32, device=fr.device)
    else:
        _check_table(table, out, fr.device, "out")
    _lib.call("lipmpc_grid_frontier_regions_batch", device=fr.device.index, F=F, W=W, H=H, frontier=fr, min_size=min_size, R_max=R_max,
              work=out["work"], work_bytes=need, **_named(out, ("label", "size", "rep", "table", "n_regions")),
              hip_stream=torch.cuda.current_stream(fr.device).cuda_stream)
    return out


def field_plan_outputs(B, F, W, H, S_max):
    """Outputs of GridFieldPlanner.plan_grid_batch, in the order it returns them (field, field_status: GridFieldPlanner.field's)."""
    f64, i32 = torch.float64, torch.int32
    return {"sub_goals": (f64, (B, S_max, 2), True), "n_sub": (i32, (B,), True), "status": (i32, (B,), True), "path_cost": (f64, (B,), True),
            "field": (torch.uint32, (F, W, H), True), "field_status": (i32, (F,), True)}


def frontier_outputs(B, F, W, H, S_max):
    """Outputs of FrontierPlanner.plan, in the order it returns them (field, frontier, n_frontier: FrontierPlanner.field's)."""
    f64, i32 = torch.float64, torch.int32
    return {"sub_goals": (f64, (B, S_max, 2), True), "n_sub": (i32, (B,), True), "status": (i32, (B,), True), "path_cost": (f64, (B,), True),
            "target": (f64, (B, 2), True), "target_cell": (i32, (B,), True), "field": (torch.uint32, (F, W, H), True),
            "frontier": (torch.uint8, (F, W, H), True), "n_frontier": (i32, (F,), True)}


def assign_outputs(B, W, H, S_max):
    """Outputs of CoordinatedFrontierPlanner.plan, in the order it returns them: FrontierPlanner.plan's on a shared map, the claim
    rounds, and the call's scratch field (``work``: it lives with the outputs so that a captured graph replays into one memory)."""
    i32 = torch.int32
    return dict(frontier_outputs(B, 1, W, H, S_max), claim_round=(i32, (B,), True), n_claims=(i32, (1,), True),
                work=(torch.uint32, (W, H), True))


def assign_keep_outputs(B, W, H, S_max):
    """Outputs of a CoordinatedFrontierPlanner with ``r_keep``: ``assign_outputs`` plus who kept the last target and how many."""
    return dict(assign_outputs(B, W, H, S_max), kept=(torch.int8, (B,), True), n_kept=(torch.int32, (1,), True))


def informed_outputs(B, F, W, H, S_max):
    """Outputs of InformedFrontierPlanner.plan, in the order it returns them: FrontierPlanner.plan's (field, frontier and n_frontier
    stay the nearest-frontier ones), then the gain, the utility field, its source count and the gain of every robot's target."""
    i32 = torch.int32
    return dict(frontier_outputs(B, F, W, H, S_max), gain=(i32, (F, W, H), True), ufield=(torch.uint32, (F, W, H), True),
                n_sources=(i32, (F,), True), target_gain=(i32, (B,), True))


def assign_utility_outputs(B, W, H, S_max):
    """Outputs of a CoordinatedFrontierPlanner with the gain keywords: ``assign_outputs`` plus the informed plan's gain and ufield
    [1,W,H], n_sources [1] and target_gain [B]."""
    table = informed_outputs(B, 1, W, H, S_max)
    return dict(assign_outputs(B, W, H, S_max), **{k: table[k] for k in ("gain", "ufield", "n_sources", "target_gain")})


def assign_keep_utility_outputs(B, W, H, S_max):
    """Outputs of GainKeepFrontierPlanner.plan / replan: ``assign_utility_outputs`` plus who kept the last target and how many."""
    return dict(assign_utility_outputs(B, W, H, S_max), kept=(torch.int8, (B,), True), n_kept=(torch.int32, (1,), True))


def plan_outputs(B, S_max, max_cells, n_samples):
    """Outputs of a plan, in the order RrtStarPlanner.plan_batch returns them."""
    f64, i32 = torch.float64, torch.int32
    return {"sub_goals": (f64, (B, S_max, 2), True), "n_sub": (i32, (B,), True), "status": (i32, (B,), True), "path_cost": (f64, (B,), True),
            "grid_dims": (i32, (B, 2), False), "occ_d2": (i32, (B, max_cells), False), "cost_grid": (f64, (B, max_cells), False),
            "tree": (f64, (B, n_samples + 2, 4), False)}


class RrtStarPlanner:
    """RRT* on the occupancy grid of the obstacles, cost vcost[v] + C[x] |p_v - x| with C = exp(-distance to the nearest
    obstacle) (HumanoidMPCWithRRT.py:98-135).  ``width_grid_size``, ``n`` and ``r_rewire`` are the reference's arguments
    (250, 1500, 80); ``seed`` is the default seed of every problem.  The sampler is this library's (splitmix64, see
    include/lipmpc.h): ``rrtplanner``'s own tree is not reproduced."""

    def __init__(self, width_grid_size: int = 250, n: int = 1500, r_rewire: int = 80, seed: int = 1,
                 device: int | None = None, *, margin: float = 3.0, max_cells: int | None = None):
        if not torch.cuda.is_available():
            raise RuntimeError("lipmpc needs a HIP device (torch.cuda.is_available() is False); there is no CPU path")
        self.lib = _lib.load()
        p = _lib.LipmpcRrtParamsC()
        _lib.check(self.lib.lipmpc_rrt_default_params(C.byref(p)), "lipmpc_rrt_default_params")
        p.width, p.n_samples, p.r_rewire, p.margin = int(width_grid_size), int(n), int(r_rewire), float(margin)
        if max_cells is not None:
            p.max_cells = int(max_cells)
        if self.lib.lipmpc_rrt_workspace_bytes(C.byref(p), 1) < 0:
            raise ValueError(f"invalid RRT* parameters (width {p.width}, n {p.n_samples}, r_rewire {p.r_rewire}, "
                             f"max_cells {p.max_cells}, margin {p.margin})")
        self.params = p
        self.seed = int(seed)
        self.device_index = torch.cuda.current_device() if device is None else int(device)
        self.device = torch.device("cuda", self.device_index)
        self._ws, self._ws_cap = None, 0
        self.last = None            # outputs of the last plan_batch

    @property
    def max_cells(self):
        return int(self.params.max_cells)

    def _workspace(self, B):
        if B > self._ws_cap:
            nbytes = int(self.lib.lipmpc_rrt_workspace_bytes(C.byref(self.params), B))
            self._ws, self._ws_cap = torch.empty((nbytes,), dtype=torch.uint8, device=self.device), B
        return self._ws

    def _dev(self, a, dt):
        if a is None:
            return None
        if isinstance(a, torch.Tensor):
            return a.to(device=self.device, dtype=dt).contiguous()
        return torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=self.device)

    def plan_batch(self, goal, obs_xy=None, obs_nv=None, start=None, seeds=None, S_max: int | None = None,
                   with_tree: bool = False, with_grids: bool = False):
        """Plan B problems.  goal [B,2]; obs_xy [B,n_obs_max,v_max,2] / obs_nv [B,n_obs_max] as ``pack_rings`` gives them;
        start [B,2] or None (= the origin, as the reference); seeds [B] (int64 / uint64 bit patterns), one int for every
        problem, or None (= the planner's seed).  S_max: sub-goal slots per problem (default n + 1, always enough).
        Returns dict(sub_goals [B,S_max,2] (rows past n_sub are 0), n_sub [B], status [B] (RRT_*), path_cost [B]) as
        device tensors; with_tree adds tree [B,n+2,4], with_grids grid_dims [B,2], occ_d2 [B,max_cells] (squared
        distance, 0 = occupied) and cost_grid [B,max_cells] (layouts: lipmpc_rrt_plan_batch, include/lipmpc.h), and grid_bounds
        [B,4] = (min_x, max_x, min_y, max_y), the world box of every grid (what ``GridMap.from_planner`` places the cells by)."""
        goal = self._dev(goal, torch.float64)
        if goal is None or goal.dim() != 2 or goal.shape[1] != 2:
            raise ValueError("goal must be [B,2]")
        B = goal.shape[0]
        xy, nv = self._dev(obs_xy, torch.float64), self._dev(obs_nv, torch.int32)
        if (xy is None) != (nv is None):
            raise ValueError("obs_xy and obs_nv go together")
        n_obs, v_max = (0, 3) if xy is None else (int(xy.shape[1]), int(xy.shape[2]))
        if xy is not None and (tuple(xy.shape) != (B, n_obs, v_max, 2) or tuple(nv.shape) != (B, n_obs)):
            raise ValueError(f"obs_xy must be [B,n_obs_max,v_max,2] and obs_nv [B,n_obs_max] with B = {B}")
        st = self._dev(start, torch.float64)
        if st is not None and tuple(st.shape) != (B, 2):
            raise ValueError("start must be [B,2] or None")
        seeds_d = self._seeds(seeds, B)
        S_max, table, out = self._outputs(B, S_max, with_tree, with_grids)
        if with_grids:
            out["grid_bounds"] = self._grid_bounds(goal, xy, nv, st)
        if B == 0:
            return out
        _lib.call("lipmpc_rrt_plan_batch", device=self.device_index, p=C.byref(self.params), B=B, obs_xy=xy, obs_nv=nv, n_obs_max=n_obs,
                  v_max=v_max, start=st, goal=goal, seed=seeds_d, workspace=self._workspace(B), **_named(out, table),
                  S_max=S_max, hip_stream=torch.cuda.current_stream(self.device).cuda_stream)
        self.last = out
        return out

    def _seeds(self, seeds, B):
        """[B] device tensor of seed bit patterns from ``seeds`` as plan_batch takes them."""
        if seeds is None or np.isscalar(seeds):
            sd = np.full(B, self.seed if seeds is None else int(seeds), dtype=np.uint64)
        else:
            if isinstance(seeds, torch.Tensor):
                seeds = seeds.cpu().numpy()
            vals = seeds.reshape(-1).tolist() if isinstance(seeds, np.ndarray) else list(seeds)   # (a list of Python
            sd = np.asarray([int(s) & ((1 << 64) - 1) for s in vals], dtype=np.uint64)        # ints may not fit int64)
            if sd.shape[0] != B:
                raise ValueError("seeds must have B entries")
        return torch.as_tensor(sd.view(np.int64), device=self.device)

    def _outputs(self, B, S_max, with_tree, with_grids):
        """(S_max, the shape table, zeroed output tensors) of a plan."""
        S_max = int(self.params.n_samples) + 1 if S_max is None else int(S_max)
        want = dict(grid_dims=with_grids, occ_d2=with_grids, cost_grid=with_grids, tree=with_tree)
        table = plan_outputs(B, S_max, self.max_cells, int(self.params.n_samples))
        return S_max, table, _alloc(table, [k for k, (_, _, required) in table.items() if required or want[k]], self.device, torch.zeros)

    def plan_grid_batch(self, goal, grid, start, seeds=None, S_max: int | None = None, with_tree: bool = False,
                        with_grids: bool = False):
        """Plan B problems on a GIVEN occupancy grid (lipmpc_rrt_plan_grid_batch): ``grid`` a GridMap -- shared, or one map per
        problem -- e.g. ``OccupancyMapper.grid_map()`` or ``GridMap.from_planner``; goal, start [B,2] (start None = the
        origin).  The planner's cells are the centres of the grid's cells; ``width_grid_size`` and ``margin`` play no part.
        Returns the dict of ``plan_batch``: status RRT_OUTSIDE_GRID where the start or the goal rounds to no cell of the grid,
        grid_dims = (W, H), grid_bounds = (origin + cell / 2, origin + (W - 1/2) cell) per axis."""
        goal = self._dev(goal, torch.float64)
        if goal is None or goal.dim() != 2 or goal.shape[1] != 2:
            raise ValueError("goal must be [B,2]")
        B = goal.shape[0]
        st = self._dev(start, torch.float64)
        if st is not None and tuple(st.shape) != (B, 2):
            raise ValueError("start must be [B,2] or None")
        if grid.W < 2 or grid.H < 2:
            raise ValueError("grid: at least 2 x 2 cells")
        grid = grid.to(self.device)
        seeds_d = self._seeds(seeds, B)
        S_max, table, out = self._outputs(B, S_max, with_tree, with_grids)
        if with_grids:
            (ox, oy), (dx, dy) = grid.origin, grid.cell
            gb = [ox + dx / 2.0, ox + (grid.W - 0.5) * dx, oy + dy / 2.0, oy + (grid.H - 0.5) * dy]
            out["grid_bounds"] = torch.tensor([gb], dtype=torch.float64, device=self.device).repeat(B, 1)
        if B == 0:
            return out
        _lib.call("lipmpc_rrt_plan_grid_batch", device=self.device_index, p=C.byref(self.params), B=B, **grid._args(B, self.device),
                  start=st, goal=goal, seed=seeds_d, workspace=self._workspace(B), **_named(out, table), S_max=S_max,
                  hip_stream=torch.cuda.current_stream(self.device).cuda_stream)
        self.last = out
        return out

    def _grid_bounds(self, goal, xy, nv, st):
        """[B,4] (min_x, max_x, min_y, max_y) of every problem's grid, by the rule of lipmpc_rrt_plan_batch (include/lipmpc.h):
        min / max over the start (None = the origin), the goal and every ring vertex, -/+ the margin.  min, max and one
        subtraction / addition: the same doubles as the kernel's (tests/test_lidar_grid_gpu.py holds the world coordinates of
        the device's sub-goals to them bit for bit)."""
        B = goal.shape[0]
        pts = torch.stack([torch.zeros_like(goal) if st is None else st, goal], 1)                     # [B,2,2]
        if xy is not None and xy.shape[1] > 0:
            valid = (torch.arange(xy.shape[2], device=self.device)[None, None, :] < nv[:, :, None]).reshape(B, -1, 1)
            v = xy.reshape(B, -1, 2)
            inf = torch.full_like(v, float("inf"))
            lo = torch.cat([pts, torch.where(valid, v, inf)], 1).amin(1)
            hi = torch.cat([pts, torch.where(valid, v, -inf)], 1).amax(1)
        else:
            lo, hi = pts.amin(1), pts.amax(1)
        m = float(self.params.margin)
        return torch.stack([lo[:, 0] - m, hi[:, 0] + m, lo[:, 1] - m, hi[:, 1] + m], 1)

    def plan(self, goal, rings, start=None, seed=None, S_max=None, with_tree=False, with_grids=False):
        """One problem from a list of (V,2) rings (any V >= 1)."""
        v_max = max([3] + [len(r) for r in rings])
        xy, nv = pack_rings([list(rings)], max(1, len(rings)), v_max)
        return self.plan_batch(np.asarray(goal, float).reshape(1, 2), xy, nv,
                               None if start is None else np.asarray(start, float).reshape(1, 2),
                               None if seed is None else [seed], S_max, with_tree, with_grids)

    def __call__(self, mpc):
        """planner= of HumanoidMPCWithRRT: the sub-goals [S,2] from the controller's obstacles and goal, starting at the
        origin as the reference does (:105, :155), or at init_state with honour_init_state=True.  Raises RuntimeError
        unless a path is found."""
        from .compat import _ring_of
        rings = [_ring_of(o) for o in mpc.obstacles]
        start = None
        if getattr(mpc, "honour_init_state", False):
            start = (float(mpc.init_state[0]), float(mpc.init_state[2]))
        out = self.plan(mpc.goal, rings, start)
        st, n = int(out["status"][0]), int(out["n_sub"][0])
        if st != RRT_FOUND:
            raise RuntimeError(f"RrtStarPlanner: no sub-goals ({RRT_STATUS_NAMES[st]})")
        return out["sub_goals"][0, :n].cpu().numpy()


class GridFieldPlanner(_TiledRounds):
    """A complete, deterministic planner on a GIVEN occupancy grid (include/lipmpc.h, GRID FIELD PLANNER): the cost-to-go field
    from the goal over the 8-connected unblocked cells (axial step 5, diagonal 7, no corner cut), then per robot a descent down
    the field, pulled taut into sub-goals.  A path that exists is found and is a shortest one in that metric; there is no seed;
    one field serves every robot that shares the map and the goal.
    ``r_inflate``: cells within this many cells (Euclidean) of a solid cell are blocked, 0..16 -- the body radius over the cell
    size, rounded up.  ``max_seg``: the sub-goals' spacing cap in field units (5 per cell), >= 5; None = no cap.
    Ring maps: plan on ``GridMap.from_planner(...)``.
    Keyword-only ``tiled`` / ``rounds``.  ``tiled=False``: one workgroup per field, maps of up to 2^17 cells (above: E_UNSUPPORTED).  ``tiled=True``: the tiled calls at
    every map size, up to 2^24 cells (include/lipmpc.h, TILED FIELDS) -- the same field bit for bit once ``settled``; ``rounds`` as
    ``_TiledRounds`` says; ``field()`` and ``plan_grid_batch()`` then return ``settled`` [F] too, and a robot whose field is not
    settled gets RRT_FIELD_UNSETTLED and no sub-goal.  ``UnknownEnvFleet.run_replanning`` treats that status as every status other
    than RRT_FOUND: until a later replan settles the robot's working goal is its final goal, and nothing ends the run.
    Keyword-only ``r_clear`` (1..31 cells) / ``w_clear`` (0..248), both or neither, no defaults, with ``tiled=True`` only: SOFT
    CLEARANCE (include/lipmpc.h).  Every plan then makes the clearance layer of the map -- a byte per cell that decays from ``w_clear``
    on a solid cell to 0 at ``r_clear`` cells from the nearest one -- and the field and the paths are the WEIGHTED ones, in which
    a path pays a cell's byte when it leaves the cell: paths keep clear of walls where there is room and still pass a door one cell
    wide, which ``r_inflate`` = 1 would close.  ``field()``, ``plan_grid_batch()`` then return cost [M,W,H] too; the keyword
    ``cost=`` of those methods takes any uint8 layer instead; ``clearance_cost(grid)`` returns the layer alone.  The cost is static
    per plan, and path_cost includes it.
    Keyword-only ``paths`` = "lane" (default) / "wave", in every form above: "wave" makes the path call by
    ``lipmpc_grid_path_wave_batch`` -- one wavefront walks one robot's path (include/lipmpc.h, WAVE-PER-ROBOT PATH CALLS) --, the same
    dict bit for bit, the same buffers and stream, capturable wherever the "lane" form is."""

    def __init__(self, r_inflate: int = 0, max_seg: int | None = None, device: int | None = None):
        if not torch.cuda.is_available():
            raise RuntimeError("lipmpc needs a HIP device (torch.cuda.is_available() is False); there is no CPU path")
        self.lib = _lib.load()
        self.r_inflate = int(r_inflate)
        self.max_seg = FIELD_NO_CAP if max_seg is None else int(max_seg)
        if not 0 <= self.r_inflate <= 16 or self.max_seg < 5:
            raise ValueError(f"invalid field planner parameters (r_inflate {r_inflate}: 0..16, max_seg {max_seg}: >= 5 or None)")
        self.device_index = torch.cuda.current_device() if device is None else int(device)
        self.device = torch.device("cuda", self.device_index)
        self.last = None            # outputs of the last plan_grid_batch

    def _goal(self, goal):
        goal = torch.as_tensor(goal).to(device=self.device, dtype=torch.float64).contiguous()
        if goal.dim() != 2 or goal.shape[1] != 2:
            raise ValueError("goal must be [1,2] or [B,2]")
        return goal

    def _field(self, goal, grid, out):
        if self.tiled:
            ga = grid._args(goal.shape[0], self.device)
            F, W, H = goal.shape[0], ga.pop("W"), ga.pop("H")
            cost = self._layer(1 if grid.shared else F, W, H, occ=ga["occ"])
            name, more = "lipmpc_grid_field_tiled_batch", {}
            if cost is not None:
                name, more, out["cost"] = "lipmpc_grid_field_weighted_batch", dict(cost=cost), cost
            return self._run_tiled(name, F, W, H, out, **ga, **more, goal=goal, r_inflate=self.r_inflate, field=out["field"],
                                   field_status=out["field_status"])
        _lib.call("lipmpc_grid_field_batch", device=self.device_index, F=goal.shape[0], **grid._args(goal.shape[0], self.device), goal=goal,
                  r_inflate=self.r_inflate, field=out["field"], field_status=out["field_status"],
                  hip_stream=torch.cuda.current_stream(self.device).cuda_stream)

    def clearance_cost(self, grid):
        """The clearance layer of ``grid`` (a GridMap) alone: [M,W,H] uint8, M = 1 for a shared map.  It lives in the planner's
        buffer: the next call that makes a layer overwrites it."""
        grid = grid.to(self.device)
        return self._clearance(1 if grid.shared else int(grid.occ.shape[0]), grid.W, grid.H, occ=grid.occ)

    @_cost_keyword
    def field(self, goal, grid, out=None):
        """The cost-to-go fields of ``goal`` [F,2] on ``grid`` (a GridMap: shared, or one map per goal).  Returns dict(field
        [F,W,H] uint32 (FIELD_INF = blocked or cut off), status [F]: 0 OK, 1 the goal's cell is outside the grid, 2 it is blocked
        -- then the whole field is FIELD_INF).  ``out``: dict(field, field_status) to write into.  A weighted planner (``r_clear``, or
        the keyword ``cost=``) adds cost [M,W,H]."""
        goal = self._goal(goal)
        F = goal.shape[0]
        grid = grid.to(self.device)
        table = field_plan_outputs(0, F, grid.W, grid.H, 1)
        names = ("field", "field_status")
        if out is None:
            out = _alloc(table, names, self.device)
        else:
            _check_table({k: table[k] for k in names}, out, self.device, "out")
        out.pop("cost", None)
        self._field(goal, grid, out)
        if self.tiled:
            return dict(field=out["field"], status=out["field_status"], settled=out["settled"], **({"cost": out["cost"]} if "cost" in out else {}))
        return dict(field=out["field"], status=out["field_status"])

    @_cost_keyword
    def plan_grid_batch(self, goal, grid, start, S_max: int | None = 64, seeds=None, out=None):
        """Plan B robots from ``start`` [B,2] on ``grid``.  ``goal`` [B,2]: one field per robot (``grid`` shared or one map per
        robot); ``goal`` [1,2]: ONE field that every robot descends (``grid`` shared) -- the caller opts in by the shape, rows
        are never compared.  ``seeds`` is accepted and ignored (the planner has none): an instance is a ``planner=`` of
        ``UnknownEnvFleet.run_replanning``.  Returns the dict of ``RrtStarPlanner.plan_grid_batch`` -- sub_goals [B,S_max,2] (rows
        past n_sub are 0 in a fresh ``out``, untouched in a given one; the last sub-goal is the goal itself, bit for bit), n_sub
        [B], status [B] (RRT_*), path_cost [B] (the path's length in cells) -- plus field [F,W,H] and field_status [F].
        ``out``: that dict, to write into (a captured graph replays into the same buffers).
        A weighted planner (``r_clear`` / ``w_clear``, or the keyword ``cost=`` [M,W,H] uint8 with ``tiled=True``) runs cost layer ->
        weighted field -> weighted path and adds cost [M,W,H] to the dict; path_cost then includes the penalties."""
        goal = self._goal(goal)
        start = torch.as_tensor(start).to(device=self.device, dtype=torch.float64).contiguous()
        if start.dim() != 2 or start.shape[1] != 2:
            raise ValueError("start must be [B,2]")
        B, F = start.shape[0], goal.shape[0]
        if F != B and F != 1:
            raise ValueError(f"goal must be [1,2] or [B,2] with B = {B}")
        grid = grid.to(self.device)
        S_max = 64 if S_max is None else int(S_max)
        table = field_plan_outputs(B, F, grid.W, grid.H, S_max)
        if out is None:
            out = _alloc(table, ("sub_goals", "n_sub", "status", "path_cost"), self.device, torch.zeros)
            out.update(_alloc(table, ("field", "field_status"), self.device))            # written whole by the field call
        else:
            _check_table(table, out, self.device, "out")
        if self.tiled:
            self._settled(out, F)
        if B == 0:
            return out
        out.pop("cost", None)                              # (a dict that comes back: the layer is this call's or none)
        self._field(goal, grid, out)
        ga = grid._args(F, self.device)
        path = dict(lipmpc_grid_path_tiled_batch=dict(settled=out["settled"])) if self.tiled else dict(lipmpc_grid_path_batch={})
        if "cost" in out:
            path = dict(lipmpc_grid_path_weighted_batch=dict(settled=out["settled"], cost=out["cost"]))
        if self.paths == "wave":
            path = dict(lipmpc_grid_path_wave_batch=dict(settled=out["settled"] if self.tiled else None, cost=out.get("cost")))
        (name, more), = path.items()
        _lib.call(name, device=self.device_index, B=B, F=F, **ga, **more, field=out["field"], field_status=out["field_status"],
                  goal=goal, start=start, r_inflate=self.r_inflate, max_seg=self.max_seg, S_max=S_max,
                  **_named(out, ("sub_goals", "n_sub", "status", "path_cost")), hip_stream=torch.cuda.current_stream(self.device).cuda_stream)
        self.last = out
        return out


class FrontierPlanner(_TiledRounds):
    """Nearest-frontier exploration (Yamauchi 1997) on an evidence grid (include/lipmpc.h, FRONTIER EXPLORER): a cell is solid
    with evidence >= ``t_occ``, free with evidence <= -``t_free`` and unknown otherwise; a FRONTIER cell is an unblocked cell with
    at least ``min_unknown`` unknown cells among its 8 neighbours; the field is the cost-to-go to the nearest frontier cell over the
    metric of ``GridFieldPlanner``, and every robot descends it to the centre of the frontier cell it reaches.  On a shared map one
    field serves every robot.  ``r_inflate``: free cells within this many cells of a solid one are blocked, 0..16 (unknown cells
    are impassable but not inflated).  ``t_free`` / ``t_occ``: None = the mapper's ``w_miss`` / ``w_hit``.  ``max_seg``: as
    ``GridFieldPlanner``'s.
    The model's limits: every robot heads for ITS nearest frontier -- there is no task assignment here, two robots side by side
    pick the same cell (``CoordinatedFrontierPlanner`` lets them claim targets apart), and the nearest cell may reveal next to
    nothing (``InformedFrontierPlanner`` weighs what a cell would show) -- and n_frontier == 0 (status RRT_NO_PATH
    for everybody) is how "nothing left to explore" is told.  The walker that follows these goals cannot turn on the spot while
    walking: a goal that jumps behind it can make its solve INFEASIBLE, which costs the robot a capture step in a fleet with
    ``recover`` and its run in one without.
    Keyword-only ``tiled`` / ``rounds``: as ``GridFieldPlanner``'s -- the tiled calls at every map size up to 2^24 cells, ``settled`` [F] in the
    dicts of ``field()`` and ``plan()``, RRT_FIELD_UNSETTLED (target_cell -1, target NaN) for a robot whose field is not settled.
    ``UnknownEnvFleet.run_exploring`` needs no change: its ``done`` reads RRT_NO_PATH only, so a robot whose replan came back
    unsettled is parked until a later replan settles, and never ends the fleet.
    Keyword-only ``r_clear`` / ``w_clear``: as ``GridFieldPlanner``'s, with ``tiled=True`` only -- the clearance layer from the solid
    cells of the evidence (unknown cells carry no cost: it would eat the frontier), the weighted frontier field and the weighted
    paths; ``field()`` and ``plan()`` return cost [F,W,H] too and take the keyword ``cost=``; ``clearance_cost(mapper)`` returns the
    layer alone.  ``CoordinatedFrontierPlanner``, ``InformedFrontierPlanner`` and their large-map classes refuse these keywords: the
    claim rounds and the utility field are unweighted.
    Keyword-only ``paths`` = "lane" (default) / "wave": as ``GridFieldPlanner``'s, in every form
    (``lipmpc_grid_frontier_path_wave_batch``); the informed classes take it for their utility path call
    (``lipmpc_grid_frontier_utility_path_wave_batch``) and the coordinated classes for the nearest-frontier plan."""

    def __init__(self, r_inflate: int = 2, min_unknown: int = 2, t_free: int | None = None, t_occ: int | None = None,
                 max_seg: int | None = None, device: int | None = None):
        self.r_inflate, self.min_unknown = int(r_inflate), int(min_unknown)
        self.t_free = None if t_free is None else int(t_free)
        self.t_occ = None if t_occ is None else int(t_occ)
        self.max_seg = FIELD_NO_CAP if max_seg is None else int(max_seg)
        if not 0 <= self.r_inflate <= 16 or not 1 <= self.min_unknown <= 8 or self.max_seg < 5 or \
                any(t is not None and not 1 <= t <= 1 << 30 for t in (self.t_free, self.t_occ)):
            raise ValueError(f"invalid frontier planner parameters (r_inflate {r_inflate}: 0..16, min_unknown {min_unknown}: 1..8, "
                             f"t_free {t_free}, t_occ {t_occ}: 1..2^30 or None, max_seg {max_seg}: >= 5 or None)")
        if not torch.cuda.is_available():
            raise RuntimeError("lipmpc needs a HIP device (torch.cuda.is_available() is False); there is no CPU path")
        self.lib = _lib.load()
        self.device_index = torch.cuda.current_device() if device is None else int(device)
        self.device = torch.device("cuda", self.device_index)
        self._placed = {}           # (origin, cell) -> the two host arrays the C call reads
        self.last = None            # outputs of the last plan

    def _map(self, m, origin=None, cell=None):
        """(evidence [F,W,H], t_free, t_occ, origin, cell) of a mapper or of an evidence tensor [W,H] / [F,W,H]."""
        if isinstance(m, torch.Tensor):
            ev, t_free, t_occ = m, self.t_free, self.t_occ
            if t_free is None or t_occ is None:
                raise ValueError("an evidence tensor has no weights: give the planner t_free and t_occ")
        else:
            ev = m.evidence
            t_free, t_occ = (m.w_miss if self.t_free is None else self.t_free), (m.w_hit if self.t_occ is None else self.t_occ)
            origin, cell = (m.origin if origin is None else origin), (m.cell if cell is None else cell)
        if ev.dtype != torch.int32 or ev.device != self.device or not ev.is_contiguous() or ev.dim() not in (2, 3):
            raise ValueError("evidence: a contiguous int32 tensor [W,H] or [F,W,H] on the planner's device")
        return (ev if ev.dim() == 3 else ev[None]), int(t_free), int(t_occ), origin, cell

    def _field(self, ev, t_free, t_occ, out):
        F, W, H = ev.shape
        if self.tiled:
            cost = self._layer(F, W, H, evidence=ev, t_occ=t_occ) if self._CLEARANCE else None
            name, more = "lipmpc_grid_frontier_field_tiled_batch", {}
            if cost is not None:
                name, more, out["cost"] = "lipmpc_grid_frontier_field_weighted_batch", dict(cost=cost), cost
            return self._run_tiled(name, F, W, H, out, evidence=ev, **more, t_free=t_free, t_occ=t_occ, r_inflate=self.r_inflate,
                                   min_unknown=self.min_unknown, frontier=out["frontier"], field=out["field"], n_frontier=out["n_frontier"])
        _lib.call("lipmpc_grid_frontier_field_batch", device=self.device_index, F=F, W=W, H=H, evidence=ev, t_free=t_free, t_occ=t_occ,
                  r_inflate=self.r_inflate, min_unknown=self.min_unknown, frontier=out["frontier"], field=out["field"],
                  n_frontier=out["n_frontier"], hip_stream=torch.cuda.current_stream(self.device).cuda_stream)

    def clearance_cost(self, mapper_or_evidence):
        """The clearance layer of a mapper or an evidence tensor alone: [F,W,H] uint8 (solid = evidence >= t_occ; unknown cells are
        no sources of cost).  It lives in the planner's buffer: the next call that makes a layer overwrites it."""
        ev, _, t_occ, _, _ = self._map(mapper_or_evidence)
        return self._clearance(*ev.shape, evidence=ev, t_occ=t_occ)

    @_cost_keyword
    def field(self, mapper_or_evidence, out=None):
        """The frontier and the cost-to-go to it of an ``OccupancyMapper`` (shared or per-robot maps) or of an evidence tensor
        [W,H] / [F,W,H].  Returns dict(field [F,W,H] uint32 (0 on frontier cells, FIELD_INF = blocked or cut off), frontier
        [F,W,H] uint8, n_frontier [F]: 0 = nothing left to explore, the whole field FIELD_INF).  ``out``: that dict, to write into.
        A weighted planner (``r_clear``, or the keyword ``cost=``) adds cost [F,W,H]."""
        ev, t_free, t_occ, _, _ = self._map(mapper_or_evidence)
        table = frontier_outputs(0, *ev.shape, 1)
        names = ("field", "frontier", "n_frontier")
        if out is None:
            out = _alloc(table, names, self.device)
        else:
            _check_table({k: table[k] for k in names}, out, self.device, "out")
        out.pop("cost", None)
        self._field(ev, t_free, t_occ, out)
        return {k: out[k] for k in names + (("settled",) if self.tiled else ()) + (("cost",) if "cost" in out else ())}

    def regions(self, mapper_or_evidence, min_size: int = 1, R_max: int = 1024, out=None):
        """The frontier REGIONS of a mapper or an evidence tensor (include/lipmpc.h, lipmpc_grid_frontier_regions_batch): the
        frontier field (tiled when the planner is), then the regions call on its ``frontier``, both on the current stream.  Returns
        ``frontier_regions``' label, size, rep, table and n_regions plus ``field()``'s dict.  ``out``: that dict, to write into.  The
        call's workspace is the planner's own: grown only, never under capture -- run the call once before capturing it."""
        ev, t_free, t_occ, _, _ = self._map(mapper_or_evidence)
        min_size, R_max = _region_args(min_size, R_max)
        F, W, H = ev.shape
        field = frontier_outputs(0, F, W, H, 1)
        table = dict({k: field[k] for k in ("field", "frontier", "n_frontier")}, **regions_outputs(F, W, H, R_max))
        if out is None:
            out = _alloc(table, tuple(k for k in table if k != "table"), self.device)
            out["table"] = torch.zeros(table["table"][1], dtype=torch.int32, device=self.device)
        else:
            _check_table(table, out, self.device, "out")
        out.pop("cost", None)
        self._field(ev, t_free, t_occ, out)
        self._regions_call(F, W, H, min_size, R_max, out, out["size"])
        names = ("frontier", "label", "size", "rep", "table", "n_regions", "field", "n_frontier")
        return {k: out[k] for k in names + (("settled",) if self.tiled else ()) + (("cost",) if "cost" in out else ())}

    @_cost_keyword
    def plan(self, mapper_or_evidence, start, origin=None, cell=None, S_max: int = 64, out=None):
        """Plan B robots from ``start`` [B,2] to their nearest frontier: on a shared map (a mapper without ``per_robot``, an
        evidence tensor [W,H] or [1,W,H]) every robot descends the one field, else there are B maps.  ``origin`` / ``cell``: the
        grid's placement, for an evidence tensor (a mapper brings its own).  Returns the planners' dict -- sub_goals [B,S_max,2]
        (rows past n_sub are 0 in a fresh ``out``, untouched in a given one; the last sub-goal is the centre of the frontier cell),
        n_sub [B], status [B] (RRT_FOUND, RRT_PATH_OVERFLOW, RRT_OUTSIDE_GRID, RRT_START_OCCUPIED; RRT_NO_PATH: no frontier
        left, or none within reach), path_cost [B] in cells -- plus target [B,2] (the frontier cell's centre; NaN unless FOUND or
        PATH_OVERFLOW), target_cell [B] (its index i * H + j, else -1), n_frontier [F], field and frontier [F,W,H].
        ``out``: that dict, to write into (a captured graph replays into the same buffers; nothing is allocated then).
        A weighted planner (``r_clear`` / ``w_clear``, or the keyword ``cost=`` [F,W,H] uint8 with ``tiled=True``) runs cost layer ->
        weighted field -> weighted path and adds cost [F,W,H] to the dict: "nearest" is then nearest in the weighted metric, and
        path_cost includes the penalties."""
        ev, t_free, t_occ, origin, cell = self._map(mapper_or_evidence, origin, cell)
        origin, cell, org_c, cell_c = self._placement(origin, cell)
        start = torch.as_tensor(start).to(device=self.device, dtype=torch.float64).contiguous()
        if start.dim() != 2 or start.shape[1] != 2:
            raise ValueError("start must be [B,2]")
        B, (F, W, H), S_max = start.shape[0], ev.shape, int(S_max)
        if F != B and F != 1:
            raise ValueError(f"{F} maps for {B} robots: one shared map, or one per robot")
        table = frontier_outputs(B, F, W, H, S_max)
        if out is None:
            out = _alloc(table, ("sub_goals", "n_sub", "status", "path_cost", "target", "target_cell"), self.device, torch.zeros)
            out.update(_alloc(table, ("field", "frontier", "n_frontier"), self.device))      # written whole by the field call
        else:
            _check_table(table, out, self.device, "out")
        if self.tiled:
            self._settled(out, F)
        if B == 0:
            return out
        out.pop("cost", None)                              # (a dict that comes back: the layer is this call's or none)
        self._field(ev, t_free, t_occ, out)
        path = dict(lipmpc_grid_frontier_path_tiled_batch=dict(settled=out["settled"])) if self.tiled else \
            dict(lipmpc_grid_frontier_path_batch={})
        if "cost" in out:
            path = dict(lipmpc_grid_frontier_path_weighted_batch=dict(settled=out["settled"], cost=out["cost"]))
        if self.paths == "wave":
            path = dict(lipmpc_grid_frontier_path_wave_batch=dict(settled=out["settled"] if self.tiled else None, cost=out.get("cost")))
        (name, more), = path.items()
        _lib.call(name, device=self.device_index, B=B, F=F, W=W, H=H, origin=C.addressof(org_c), **more,
                  cell=C.addressof(cell_c), evidence=ev, t_occ=t_occ, field=out["field"], n_frontier=out["n_frontier"], start=start,
                  r_inflate=self.r_inflate, max_seg=self.max_seg, S_max=S_max,
                  **_named(out, ("sub_goals", "n_sub", "status", "path_cost", "target_cell")),
                  hip_stream=torch.cuda.current_stream(self.device).cuda_stream)
        self._target(out, origin, cell, H)
        self.last = out
        return out

    def _placement(self, origin, cell):
        """(origin, cell) as pairs of floats, and the two host arrays the C calls read (kept: one pair per placement)."""
        if origin is None or cell is None:
            raise ValueError("an evidence tensor has no placement: give origin and cell")
        cell = (float(cell), float(cell)) if isinstance(cell, (int, float)) else (float(cell[0]), float(cell[1]))
        origin = (float(origin[0]), float(origin[1]))
        key = (origin, cell)
        if key not in self._placed:
            self._placed[key] = (C.c_double * 2)(*origin), (C.c_double * 2)(*cell)
        return (origin, cell) + self._placed[key]

    @staticmethod
    def _target(out, origin, cell, H):
        """out["target"] from out["target_cell"]: the centre by the contract's expression (double, one multiply and one add per
        axis: torch does not contract); NaN where the cell is -1."""
        tc = out["target_cell"]
        i, j = torch.div(tc, H, rounding_mode="floor"), torch.remainder(tc, H)
        xy = torch.stack([origin[0] + (i.double() + 0.5) * cell[0], origin[1] + (j.double() + 0.5) * cell[1]], 1)
        out["target"].copy_(torch.where((tc >= 0)[:, None], xy, torch.full_like(xy, float("nan"))))


class CoordinatedFrontierPlanner(FrontierPlanner):
    """``FrontierPlanner`` with task assignment on ONE shared map (include/lipmpc.h, lipmpc_grid_frontier_assign_batch): after
    the nearest-frontier plan the robots claim frontier targets apart by the greedy rule of coordinated exploration (Burgard et
    al. 2005, the utility discount taken as "within the claim radius = already taken").  Round by round the robot that is
    nearest to what is left of the frontier wins (ties to the lower index), gets its path to that cell, and every frontier cell
    within ``r_claim`` cells (Euclidean, 0..4096) of its target is taken out for the robots that follow; at most ``max_claims``
    rounds (0..4096).  Everything is an integer comparison: two calls give identical bits.
    The model's limits: a round is sequential by nature -- one relaxation of the whole map per claim, in one workgroup; robots
    that are left when the frontier or ``max_claims`` is used up are FOLLOWERS, who keep their plain nearest-frontier plan and so
    share a target; ``plan`` has no memory, so a replan may hand a robot another target than the last one.
    CLAIM HYSTERESIS (keywords ``r_keep`` 0..64, ``keep_ratio16`` 16..1024, ``keep_slack`` 0..4096; all three or none, no
    defaults: nobody has measured one; ``lipmpc_grid_frontier_assign_keep_batch``): ``replan(..., prev_target=)`` runs a keep
    phase ahead of the rounds.  A robot keeps what is left of its last target -- the nearest frontier cell within ``r_keep``
    cells of it -- when that cell is reachable and its cost is at most ``keep_ratio16`` / 16 times the cost to the robot's
    nearest frontier plus ``keep_slack`` cells; a keeper takes its disc like a winner, and keep attempts and rounds share the
    ``max_claims`` relaxations.  Without ``r_keep`` the very calls of before are made.  What remains: the keep test compares with
    the NEAREST frontier, not with what the rounds would have handed the robot; followers have no memory; the informed planners
    have none either.
    Keyword-only ``paths`` = "wave" governs the nearest-frontier plan that precedes the claims; the walks inside the claim calls -- a
    winner's or a keeper's path -- are unchanged, one lane per robot.
    GAIN-SEEDED CLAIMS (keywords ``r_view`` 1..64, ``w_gain`` 0..65535, ``g_cap`` 1..16384, all three or none, no defaults: nobody
    has measured one; ``min_gain`` 0..16384, default 0; ``lipmpc_grid_frontier_assign_utility_batch``): the robots claim apart
    what reveals most.  ``plan`` runs frontier field -> gain -> utility field -> utility path (``InformedFrontierPlanner``'s
    calls and parameters) -> the claim rounds with every round's field seeded as the utility field is and the winner's walk ended
    as the utility path's is; the discount stays the ``r_claim`` disc, no gain is recomputed after a claim.  The dict gains gain
    and ufield [1,W,H], n_sources [1] and target_gain [B]; followers keep their utility plan.  ``w_gain`` = 0 with ``min_gain`` =
    0 gives the plain claims, bit for bit.  ``paths`` = "wave" governs the utility path call only.  There is no hysteresis for
    these claims in this class: the gain keywords with ``r_keep`` / ``keep_ratio16`` / ``keep_slack``, and ``replan``, raise
    ValueError -- the class with both is ``GainKeepFrontierPlanner``; so do ``r_clear`` / ``w_clear`` / ``cost=``, as for every
    coordinated planner.  Without the keywords the very calls of before are made."""

    _TILED, _TILED_WHY, _TILED_CLASS = False, "the claim rounds keep", "TiledCoordinatedFrontierPlanner"
    _CLEARANCE = False
    _FRESH = ("field", "frontier", "n_frontier", "work")            # outputs written whole: a fresh dict gets them uninitialised
    _table = staticmethod(assign_outputs)
    _keep_table = staticmethod(assign_keep_outputs)                 # the table of a planner with ``r_keep``
    _gain_table = staticmethod(assign_utility_outputs)              # the table of a planner with ``r_view``
    _gain_keep_table = staticmethod(assign_keep_utility_outputs)    # the table of a planner with both (_GAIN_KEEP)
    _GAIN_KEEP, _GAIN_KEEP_CLASS = False, "GainKeepFrontierPlanner"  # True: the subclass whose claims have both
    _informed = None                                                # the class whose gain, utility field and utility path calls run

    def __init__(self, r_claim: int, max_claims: int = 64, **frontier_planner_kwargs):
        self.r_claim, self.max_claims = int(r_claim), int(max_claims)
        if not 0 <= self.r_claim <= 4096 or not 0 <= self.max_claims <= 4096:
            raise ValueError(f"invalid claim parameters (r_claim {r_claim}: 0..4096, max_claims {max_claims}: 0..4096)")
        # the keep parameters: keywords, taken off before the parent sees them (the signature stays what it was)
        keep = [frontier_planner_kwargs.pop(k, None) for k in ("r_keep", "keep_ratio16", "keep_slack")]
        misspelt = sorted(k for k in frontier_planner_kwargs if "keep" in k)
        if misspelt:
            raise TypeError(f"unexpected keyword {misspelt}: the keep parameters are r_keep, keep_ratio16 and keep_slack")
        # the gain parameters, likewise
        gain = [frontier_planner_kwargs.pop(k, None) for k in ("r_view", "w_gain", "g_cap", "min_gain")]
        region = self.gain_from == "region"
        if region:
            if gain[0] is not None:
                raise ValueError(f"gain_from='region' with r_view {gain[0]}: r_view must be None (the gain is the region's size, no ray "
                                 f"is marched)")
            if gain[1] is not None or gain[2] is not None:
                gain[0] = 0                                # (r_view 0 marks a planner whose gain is the region's size)
        misspelt = sorted(k for k in frontier_planner_kwargs if any(w in k for w in ("gain", "view", "cap")) or
                          (gain != [None] * 4 and k not in inspect.signature(FrontierPlanner.__init__).parameters))
        if misspelt:
            raise TypeError(f"unexpected keyword {misspelt}: the gain parameters are r_view, w_gain, g_cap and min_gain")
        if all(v is None for v in gain[:3]):
            if gain[3] is not None:
                raise ValueError("min_gain without r_view, w_gain and g_cap: the gain-seeded claims are switched on by those three")
            self.r_view = self.w_gain = self.g_cap = self.min_gain = None
        else:
            if any(v is None for v in gain[:3]):
                raise ValueError("r_view, w_gain and g_cap go together: they have no defaults, nobody has measured one")
            if keep != [None, None, None] and not self._GAIN_KEEP:
                raise ValueError(f"the gain keywords with r_keep / keep_ratio16 / keep_slack: there is no hysteresis for gain-seeded "
                                 f"claims in {type(self).__name__}; the class with both is {self._GAIN_KEEP_CLASS}")
            self.r_view, self.w_gain, self.g_cap, self.min_gain = (int(v) for v in gain[:3] + [gain[3] or 0])
            if not (region or 1 <= self.r_view <= 64) or not 0 <= self.w_gain <= 65535 or not 1 <= self.g_cap <= 16384 or \
                    not 0 <= self.min_gain <= 16384:
                raise ValueError(f"invalid gain parameters (r_view {gain[0]}: 1..64, w_gain {gain[1]}: 0..65535, g_cap {gain[2]}: "
                                 f"1..16384, min_gain {gain[3]}: 0..16384)")
            self._table = self._gain_table
        if keep[0] is None:
            if keep[1] is not None or keep[2] is not None:
                raise ValueError("keep_ratio16 / keep_slack without r_keep: the keep phase is switched on by r_keep")
            self.r_keep = self.keep_ratio16 = self.keep_slack = None
        else:
            if keep[1] is None or keep[2] is None:
                raise ValueError("r_keep needs keep_ratio16 and keep_slack: they have no defaults, nobody has measured one")
            self.r_keep, self.keep_ratio16, self.keep_slack = (int(v) for v in keep)
            if not 0 <= self.r_keep <= 64 or not 16 <= self.keep_ratio16 <= 1024 or not 0 <= self.keep_slack <= 4096:
                raise ValueError(f"invalid keep parameters (r_keep {keep[0]}: 0..64, keep_ratio16 {keep[1]}: 16..1024, "
                                 f"keep_slack {keep[2]}: 0..4096)")
            self._table = self._keep_table if self.r_view is None else self._gain_keep_table
        super().__init__(**frontier_planner_kwargs)

    @_cost_keyword
    def plan(self, mapper_or_evidence, start, origin=None, cell=None, S_max: int = 64, out=None, may_claim=None):
        """``FrontierPlanner.plan`` on a shared map (anything else: ValueError), then the claims.  ``may_claim`` [B] (bool or
        integers, None = everybody): the robots that may claim; the others keep their nearest-frontier plan and take nothing
        from anybody.  Returns the parent's dict -- a robot that claimed has the sub_goals, n_sub, status, path_cost, target_cell
        and target of its path to the cell it claimed -- plus claim_round [B] (the round a robot won, -1 for everyone else),
        n_claims [1] and ``work`` [W,H] (the call's scratch).  ``out``: that dict, to write into.
        With ``r_keep`` set this is ``replan`` with no previous targets.  With the gain keywords the plan that precedes the claims is
        ``InformedFrontierPlanner.plan``'s and the dict gains gain, ufield [1,W,H], n_sources [1] and target_gain [B]."""
        return self._plan(mapper_or_evidence, start, origin, cell, S_max, out, may_claim, None)

    def replan(self, mapper_or_evidence, start, origin=None, cell=None, S_max: int = 64, out=None, may_claim=None, prev_target=None):
        """``plan`` with memory (a planner with ``r_keep``; any other: ValueError).  ``prev_target`` [B] integers: per robot the
        ``target_cell`` of the last plan on this same grid, anything outside 0..W*H-1 (-1, say) = none; None = nobody has one.  A
        robot keeps what is left of that target by the keep rule ahead of the claim rounds.  Returns ``plan``'s dict plus kept [B]
        int8 (1 = the robot kept its target; its claim_round counts like a winner's) and n_kept [1]."""
        if self.r_view is not None and not self._GAIN_KEEP:
            raise ValueError(f"replan on a planner with the gain keywords: there is no hysteresis for gain-seeded claims in "
                             f"{type(self).__name__}; the class with both is {self._GAIN_KEEP_CLASS}")
        if self.r_keep is None:
            raise ValueError("replan needs a planner with r_keep, keep_ratio16 and keep_slack")
        return self._plan(mapper_or_evidence, start, origin, cell, S_max, out, may_claim, prev_target)

    def _plan(self, mapper_or_evidence, start, origin, cell, S_max, out, may_claim, prev_target):
        ev = self._map(mapper_or_evidence, origin, cell)[0]
        if ev.shape[0] != 1:
            raise ValueError(f"{ev.shape[0]} maps: the robots claim on ONE shared map")
        start = torch.as_tensor(start).to(device=self.device, dtype=torch.float64).contiguous()
        if start.dim() != 2 or start.shape[1] != 2:
            raise ValueError("start must be [B,2]")
        B, (_, W, H), S_max = start.shape[0], ev.shape, int(S_max)
        if may_claim is not None:
            may_claim = torch.as_tensor(may_claim).to(device=self.device)
            if tuple(may_claim.shape) != (B,):
                raise ValueError("may_claim must be [B]")
            may_claim = (may_claim != 0).to(torch.int8)
        if self.r_keep is not None:
            if prev_target is None:
                if self._none is None or self._none.shape[0] < B:               # (made once: nothing is allocated in a capture
                    if torch.cuda.is_current_stream_capturing():                #  that follows a call of this size)
                        raise RuntimeError("the planner's 'no previous target' row must grow: run the call once before the capture")
                    self._none = torch.full((max(B, 1),), -1, dtype=torch.int32, device=self.device)
                prev_target = self._none[:B]
            else:
                prev_target = torch.as_tensor(prev_target)
                if tuple(prev_target.shape) != (B,) or prev_target.dtype.is_floating_point or prev_target.dtype == torch.bool:
                    raise ValueError("prev_target must be [B] integers")
                prev_target = prev_target.to(device=self.device)
                if prev_target.dtype != torch.int32:                            # whatever is no cell of an int32 grid is "none"
                    prev_target = torch.where((prev_target >= 0) & (prev_target < W * H), prev_target, -1).to(torch.int32)
                prev_target = prev_target.contiguous()
        regions = self._region_table(1, W, H)
        table = dict(self._table(B, W, H, S_max), **regions)
        if out is None:
            out = _alloc(table, ("sub_goals", "n_sub", "status", "path_cost", "target", "target_cell"), self.device, torch.zeros)
            out.update(_alloc(table, self._FRESH, self.device))
            out.update(_alloc(regions, tuple(regions), self.device, torch.zeros))
            out.update(claim_round=torch.full((B,), -1, dtype=torch.int32, device=self.device),
                       n_claims=torch.zeros((1,), dtype=torch.int32, device=self.device))
            if self.r_keep is not None:
                out.update(_alloc(table, ("kept", "n_kept"), self.device, torch.zeros))
            if self.r_view is not None:
                out.update(_alloc(table, ("gain", "ufield", "n_sources"), self.device))
                out["target_gain"] = torch.full((B,), -1, dtype=torch.int32, device=self.device)
        else:
            _check_table(table, out, self.device, "out")
        if self.r_view is not None:
            return self._plan_gain(mapper_or_evidence, start, origin, cell, S_max, out, may_claim, prev_target)
        super().plan(mapper_or_evidence, start, origin, cell, S_max, out)      # (its table is part of this one)
        if B == 0:
            return out
        origin, cell, org_c, cell_c = self._placement(*self._map(mapper_or_evidence, origin, cell)[3:])
        if self.r_keep is None:
            self._claims(B, W, H, start, may_claim, org_c, cell_c, S_max, out)
        else:
            self._keep_claims(B, W, H, start, may_claim, prev_target, org_c, cell_c, S_max, out)
        self._target(out, origin, cell, H)
        self.last = out
        return out

    def _plan_gain(self, mapper_or_evidence, start, origin, cell, S_max, out, may_claim, prev_target=None):
        """The gain-seeded plan into ``out``: frontier field -> gain -> utility field -> utility path -> the claims (with ``r_keep``:
        the keep phase and the claims, ``prev_target`` as ``_plan`` made it)."""
        informed = self._informed or InformedFrontierPlanner
        ev, t_free, t_occ, origin, cell = self._map(mapper_or_evidence, origin, cell)
        origin, cell, org_c, cell_c = self._placement(origin, cell)
        B, (_, W, H) = start.shape[0], ev.shape
        if self.tiled:
            self._settled(out, 1)
        if B == 0:
            return out
        self._classes = t_free, t_occ                      # (what the tiled utility field call classifies the evidence by)
        self._field(ev, t_free, t_occ, out)
        informed._gain(self, ev, t_free, t_occ, out)
        informed._ufield(self, ev, out)
        informed._path(self, ev, t_occ, start, org_c, cell_c, S_max, out)
        if self.r_keep is None:
            self._gain_claims(B, W, H, start, may_claim, org_c, cell_c, S_max, out)
        else:
            self._gain_keep_claims(B, W, H, start, may_claim, prev_target, org_c, cell_c, S_max, out)
        self._target(out, origin, cell, H)
        self.last = out
        return out

    def _gain_claims(self, B, W, H, start, may_claim, org_c, cell_c, S_max, out):
        _lib.call("lipmpc_grid_frontier_assign_utility_batch", device=self.device_index, B=B, W=W, H=H, origin=C.addressof(org_c),
                  cell=C.addressof(cell_c), frontier=self._sources(out), field=out["field"], start=start, may_claim=may_claim,
                  r_inflate=self.r_inflate, r_claim=self.r_claim, max_claims=self.max_claims, max_seg=self.max_seg, S_max=S_max,
                  work=out["work"], **_named(out, ("sub_goals", "n_sub", "status", "path_cost", "target_cell", "claim_round", "n_claims")),
                  gain=out["gain"], w_gain=self.w_gain, g_cap=self.g_cap, min_gain=self.min_gain, target_gain=out["target_gain"],
                  hip_stream=torch.cuda.current_stream(self.device).cuda_stream)

    def _gain_keep_claims(self, B, W, H, start, may_claim, prev_target, org_c, cell_c, S_max, out):
        _lib.call("lipmpc_grid_frontier_assign_keep_utility_batch", device=self.device_index, B=B, W=W, H=H, origin=C.addressof(org_c),
                  cell=C.addressof(cell_c), frontier=self._sources(out), field=out["field"], start=start, may_claim=may_claim,
                  prev_target=prev_target, r_inflate=self.r_inflate, r_claim=self.r_claim, r_keep=self.r_keep,
                  keep_ratio16=self.keep_ratio16, keep_slack=self.keep_slack, max_claims=self.max_claims, max_seg=self.max_seg,
                  S_max=S_max, work=out["work"],
                  **_named(out, ("sub_goals", "n_sub", "status", "path_cost", "target_cell", "claim_round", "n_claims", "kept", "n_kept")),
                  gain=out["gain"], ufield=out["ufield"], w_gain=self.w_gain, g_cap=self.g_cap, min_gain=self.min_gain,
                  target_gain=out["target_gain"], hip_stream=torch.cuda.current_stream(self.device).cuda_stream)

    _none = None                # [>= B] int32 of -1: the prev_target of a plan without one

    def _keep_claims(self, B, W, H, start, may_claim, prev_target, org_c, cell_c, S_max, out):
        _lib.call("lipmpc_grid_frontier_assign_keep_batch", device=self.device_index, B=B, W=W, H=H, origin=C.addressof(org_c),
                  cell=C.addressof(cell_c), frontier=out["frontier"], field=out["field"], start=start, may_claim=may_claim,
                  prev_target=prev_target, r_inflate=self.r_inflate, r_claim=self.r_claim, r_keep=self.r_keep,
                  keep_ratio16=self.keep_ratio16, keep_slack=self.keep_slack, max_claims=self.max_claims, max_seg=self.max_seg,
                  S_max=S_max, work=out["work"],
                  **_named(out, ("sub_goals", "n_sub", "status", "path_cost", "target_cell", "claim_round", "n_claims", "kept", "n_kept")),
                  hip_stream=torch.cuda.current_stream(self.device).cuda_stream)

    def _claims(self, B, W, H, start, may_claim, org_c, cell_c, S_max, out):
        _lib.call("lipmpc_grid_frontier_assign_batch", device=self.device_index, B=B, W=W, H=H, origin=C.addressof(org_c),
                  cell=C.addressof(cell_c), frontier=out["frontier"], field=out["field"], start=start, may_claim=may_claim,
                  r_inflate=self.r_inflate, r_claim=self.r_claim, max_claims=self.max_claims, max_seg=self.max_seg, S_max=S_max,
                  work=out["work"], **_named(out, ("sub_goals", "n_sub", "status", "path_cost", "target_cell", "claim_round", "n_claims")),
                  hip_stream=torch.cuda.current_stream(self.device).cuda_stream)


class GainKeepFrontierPlanner(CoordinatedFrontierPlanner):
    """``CoordinatedFrontierPlanner`` with the gain keywords AND claim hysteresis (include/lipmpc.h,
    lipmpc_grid_frontier_assign_keep_utility_batch): the far, high-gain targets that the gain-seeded claims hand out jump between
    replans; here a robot keeps what is left of its last target -- the source of the current replan nearest to it within ``r_keep``
    cells -- when, as a utility (the anchor's own seed plus the cost to it), it is at most ``keep_ratio16`` / 16 times the robot's
    value in the shared utility field plus ``keep_slack`` cells.  A target whose gain has fallen pays for it through its seed; a
    keeper takes its disc like a winner; keep attempts and rounds share the ``max_claims`` relaxations; the rounds that follow are
    the gain-seeded ones.  ``plan()`` and ``replan(..., prev_target=)`` run frontier field -> gain -> utility field -> utility path
    -> that call; the dict is the gain-seeded planner's plus kept [B] int8 and n_kept [1].
    Every keyword is the parent's and none but ``min_gain`` has a default: nobody has measured one.  ``paths`` = "wave" governs the
    utility path call only; ``r_clear`` / ``w_clear`` / ``cost=`` raise ValueError, as for every coordinated planner.  With no
    previous targets the plan is the gain-seeded parent's, bit for bit; with ``w_gain`` = 0 and ``min_gain`` = 0 it is the parent's
    with ``r_keep``.  The large-map class is ``TiledGainKeepFrontierPlanner``."""

    _GAIN_KEEP = True
    _TILED_CLASS = "TiledGainKeepFrontierPlanner"

    def __init__(self, r_claim: int, max_claims: int = 64, *, r_view: int, w_gain: int, g_cap: int, min_gain: int = 0, r_keep: int,
                 keep_ratio16: int, keep_slack: int, **frontier_planner_kwargs):
        _gain_keep_init(super(), r_claim, max_claims, r_view, w_gain, g_cap, min_gain, r_keep, keep_ratio16, keep_slack,
                        frontier_planner_kwargs, self.gain_from == "region")


def _gain_keep_init(parent, r_claim, max_claims, r_view, w_gain, g_cap, min_gain, r_keep, keep_ratio16, keep_slack, kwargs, region=False):
    """What the two gain-keep classes' ``__init__`` share: every parameter is required (a None is as good as none), then the parent's
    checks and ranges."""
    given = dict(r_view=r_view, w_gain=w_gain, g_cap=g_cap, min_gain=min_gain, r_keep=r_keep, keep_ratio16=keep_ratio16,
                 keep_slack=keep_slack)
    missing = sorted(k for k, v in given.items() if v is None and k != "min_gain" and not (region and k == "r_view"))
    if missing:
        raise ValueError(f"{missing} None: r_view, w_gain, g_cap, r_keep, keep_ratio16 and keep_slack have no defaults, nobody has "
                         f"measured one")
    parent.__init__(r_claim, max_claims, **given, **kwargs)


def tiled_assign_outputs(B, W, H, S_max):
    """Outputs of TiledCoordinatedFrontierPlanner.plan: CoordinatedFrontierPlanner.plan's without its scratch field (the tiled claim
    call's workspace is the planner's own) and with claims_settled; ``settled`` [1] comes as in ``FrontierPlanner(tiled=True)``."""
    table = assign_outputs(B, W, H, S_max)
    del table["work"]
    return dict(table, claims_settled=(torch.int32, (1,), False))


def tiled_assign_keep_outputs(B, W, H, S_max):
    """Outputs of a TiledCoordinatedFrontierPlanner with ``r_keep``: ``tiled_assign_outputs`` plus kept and n_kept."""
    return dict(tiled_assign_outputs(B, W, H, S_max), kept=(torch.int8, (B,), True), n_kept=(torch.int32, (1,), True))


def tiled_assign_utility_outputs(B, W, H, S_max):
    """Outputs of a TiledCoordinatedFrontierPlanner with the gain keywords: ``assign_utility_outputs`` without ``work`` and with
    claims_settled; ``settled`` and ``usettled`` [1] come as in ``TiledInformedFrontierPlanner``."""
    table = assign_utility_outputs(B, W, H, S_max)
    del table["work"]
    return dict(table, claims_settled=(torch.int32, (1,), False))


def tiled_assign_keep_utility_outputs(B, W, H, S_max):
    """Outputs of TiledGainKeepFrontierPlanner.plan / replan: ``tiled_assign_utility_outputs`` plus kept and n_kept."""
    return dict(tiled_assign_utility_outputs(B, W, H, S_max), kept=(torch.int8, (B,), True), n_kept=(torch.int32, (1,), True))


CLAIM_MAX_LAUNCHES = 1 << 20    # max_claims * max_rounds of one lipmpc_grid_frontier_assign_tiled_batch


class _AlwaysTiled:
    """The large-map classes: ``tiled`` is always True, ``rounds`` stays the keyword of ``_TiledRounds``."""

    _TILED = True

    def _init_tiled(self, tiled, rounds):
        super()._init_tiled(True, rounds)


class TiledCoordinatedFrontierPlanner(_AlwaysTiled, CoordinatedFrontierPlanner):
    """``CoordinatedFrontierPlanner`` on maps of up to 2^24 cells (include/lipmpc.h, TILED EXPLORERS): the tiled nearest-frontier
    plan of ``FrontierPlanner(tiled=True)``, then the same claim rule with every round's field relaxed by tiled rounds
    (``lipmpc_grid_frontier_assign_tiled_batch``).  Returns the parent's dict without ``work``, plus ``settled`` [1] (the
    nearest-frontier field) and ``claims_settled`` [1]: 1 = the claim rounds ended by the rule and every output is the parent's, bit
    for bit; 0 = the given field or some round's field did not settle within the budget -- then the claims made so far are the
    rule's first ``n_claims`` rounds and everyone else keeps the nearest-frontier plan.
    Keyword-only ``rounds``: an int = the budget of the frontier field AND of every claim round, one call each, no synchronisation,
    capturable (``max_claims`` * ``rounds`` <= 2^20: the launches of one call); None = the frontier field as ``_TiledRounds`` says,
    then the claim call repeated with a doubled per-claim budget while ``claims_settled`` is 0, up to min(65536, 2^20 /
    ``max_claims``) -- at that cap the dict is returned with ``claims_settled`` 0.
    The cost is fixed by the budget, not by what the fleet needs: ``max_claims`` * (budget + 4) + 3 launches per claim call.  On
    small maps the one-workgroup parent is faster; it stays the default.  The limits that remain: the claim rounds are sequential
    (gain-seeded with the gain keywords, below); ``plan`` has no memory between plans.
    CLAIM HYSTERESIS: ``r_keep``, ``keep_ratio16``, ``keep_slack`` and ``replan(..., prev_target=)`` as the parent's, by
    ``lipmpc_grid_frontier_assign_keep_tiled_batch``: the dict gains kept [B] and n_kept [1], ``rounds`` is the budget of every
    SLOT (keep attempt or claim round), and a claim call costs ``max_claims`` * (budget + 5) + 3 launches.
    GAIN-SEEDED CLAIMS: ``r_view``, ``w_gain``, ``g_cap`` and ``min_gain`` as the parent's, by ``TiledInformedFrontierPlanner``'s calls
    and ``lipmpc_grid_frontier_assign_utility_tiled_batch``: the dict gains gain, ufield, n_sources, target_gain and ``usettled``
    [1] (the utility field), ``rounds`` is the budget of the two fields and of every claim round, and a claim call costs
    ``max_claims`` * (budget + 4) + 3 launches as without the keywords.  The gain keywords together with the keep keywords raise
    ValueError here: the class with both is ``TiledGainKeepFrontierPlanner``."""

    _FRESH = ("field", "frontier", "n_frontier")
    _table = staticmethod(tiled_assign_outputs)
    _keep_table = staticmethod(tiled_assign_keep_outputs)
    _gain_table = staticmethod(tiled_assign_utility_outputs)
    _gain_keep_table = staticmethod(tiled_assign_keep_utility_outputs)
    _GAIN_KEEP_CLASS = "TiledGainKeepFrontierPlanner"
    _LAUNCH_CAP = True              # False: a subclass whose claim call's launches do not grow with max_claims

    def __init__(self, r_claim: int, max_claims: int = 64, **frontier_planner_kwargs):
        if self._LAUNCH_CAP and self.rounds is not None and int(max_claims) * self.rounds > CLAIM_MAX_LAUNCHES:
            raise ValueError(f"max_claims {max_claims} * rounds {self.rounds}: at most 2^20, the launches of one claim call")
        super().__init__(r_claim, max_claims, **frontier_planner_kwargs)
        self._claim_works = []      # the claim call's own workspace: grown only, every buffer kept alive
        self._uworks = []           # the utility field's own workspace (a planner with the gain keywords)
        self._informed = self._informed or TiledInformedFrontierPlanner

    @_cost_keyword
    def plan(self, mapper_or_evidence, start, origin=None, cell=None, S_max: int = 64, out=None, may_claim=None):
        """``CoordinatedFrontierPlanner.plan`` by the tiled calls: its dict without ``work``, plus ``settled`` and ``claims_settled`` [1]."""
        if self.r_view is not None and out is not None:
            self._settled(out, 1, "usettled")
        out = super().plan(mapper_or_evidence, start, origin, cell, S_max, out, may_claim)
        self._settled(out, 1, "claims_settled")            # (B = 0: no call was made)
        if self.r_view is not None:
            self._settled(out, 1, "usettled")
        return out

    def replan(self, mapper_or_evidence, start, origin=None, cell=None, S_max: int = 64, out=None, may_claim=None, prev_target=None):
        """``CoordinatedFrontierPlanner.replan`` by the tiled calls: its dict without ``work``, plus ``settled`` and ``claims_settled`` [1]."""
        if self.r_view is not None and out is not None:
            self._settled(out, 1, "usettled")
        out = super().replan(mapper_or_evidence, start, origin, cell, S_max, out, may_claim, prev_target)
        self._settled(out, 1, "claims_settled")            # (B = 0: no call was made)
        if self.r_view is not None:
            self._settled(out, 1, "usettled")
        return out

    def _keep_claims(self, B, W, H, start, may_claim, prev_target, org_c, cell_c, S_max, out):
        self._claims(B, W, H, start, may_claim, org_c, cell_c, S_max, out, prev_target)

    def _gain_claims(self, B, W, H, start, may_claim, org_c, cell_c, S_max, out):
        self._claims(B, W, H, start, may_claim, org_c, cell_c, S_max, out, gain=True)

    def _gain_keep_claims(self, B, W, H, start, may_claim, prev_target, org_c, cell_c, S_max, out):
        self._claims(B, W, H, start, may_claim, org_c, cell_c, S_max, out, prev_target, gain=True)

    def _claims(self, B, W, H, start, may_claim, org_c, cell_c, S_max, out, prev_target=None, gain=False):
        capturing = torch.cuda.is_current_stream_capturing()
        if self.rounds is None and capturing:
            raise RuntimeError("rounds=None reads `claims_settled` on the host: give the planner a fixed `rounds` to capture its calls")
        name, keep = "lipmpc_grid_frontier_assign_tiled_batch", {}
        if gain:
            name = "lipmpc_grid_frontier_assign_utility_tiled_batch"
            keep = dict(gain=out["gain"], w_gain=self.w_gain, g_cap=self.g_cap, min_gain=self.min_gain, target_gain=out["target_gain"])
        if prev_target is not None:
            name = "lipmpc_grid_frontier_assign_keep_utility_tiled_batch" if gain else "lipmpc_grid_frontier_assign_keep_tiled_batch"
            keep = dict(keep, prev_target=prev_target, r_keep=self.r_keep, keep_ratio16=self.keep_ratio16, keep_slack=self.keep_slack,
                        kept=out["kept"], n_kept=out["n_kept"])
            if gain:
                keep.update(ufield=out["ufield"], usettled=out["usettled"])
        size = name.replace("_batch", "_workspace_bytes")
        work = self._workspace(self._claim_works, int(getattr(self.lib, size)(W, H)), size)
        done = self._settled(out, 1, "claims_settled")
        stream = torch.cuda.current_stream(self.device).cuda_stream

        def call(budget):
            _lib.call(name, device=self.device_index, B=B, W=W, H=H, origin=C.addressof(org_c),
                      cell=C.addressof(cell_c), frontier=self._sources(out) if gain else out["frontier"], field=out["field"],
                      settled=out["settled"], start=start,
                      may_claim=may_claim, r_inflate=self.r_inflate, r_claim=self.r_claim, max_claims=self.max_claims,
                      max_seg=self.max_seg, S_max=S_max, work=work, work_bytes=work.numel(), max_rounds=budget, **keep,
                      **_named(out, ("sub_goals", "n_sub", "status", "path_cost", "target_cell", "claim_round", "n_claims")),
                      claims_settled=done, hip_stream=stream)
        if self.rounds is not None:
            return call(self.rounds)
        tw, th, _ = tiled_info()
        cap = min(65536, CLAIM_MAX_LAUNCHES // max(self.max_claims, 1))
        budget = min(cap, max(8, -(-W // tw) - (-H // th) + 1))
        call(budget)
        while budget < cap and not bool(done[0]):
            budget = min(2 * budget, cap)
            call(budget)                                   # (the whole call again: it reproduces the rounds made so far and goes on)


class TiledGainKeepFrontierPlanner(TiledCoordinatedFrontierPlanner):
    """``GainKeepFrontierPlanner`` on maps of up to 2^24 cells, by ``TiledInformedFrontierPlanner``'s calls and
    ``lipmpc_grid_frontier_assign_keep_utility_tiled_batch``: its dict without ``work``, plus ``settled`` [1] (the nearest-frontier
    field), ``usettled`` [1] (the utility field) and ``claims_settled`` [1] -- 1 = every slot settled and every output is
    ``GainKeepFrontierPlanner``'s, bit for bit; 0 = one of the two given fields or some slot's field did not settle within the
    budget: then the keeps and claims made so far are the rule's first ``n_claims`` winners and everyone else keeps the utility plan.
    ``rounds`` as ``TiledCoordinatedFrontierPlanner``'s: the budget of the two fields and of every SLOT (keep attempt or claim
    round); a claim call costs ``max_claims`` * (budget + 5) + 3 launches.  No keyword but ``min_gain`` has a default."""

    _GAIN_KEEP = True

    def __init__(self, r_claim: int, max_claims: int = 64, *, r_view: int, w_gain: int, g_cap: int, min_gain: int = 0, r_keep: int,
                 keep_ratio16: int, keep_slack: int, **frontier_planner_kwargs):
        _gain_keep_init(super(), r_claim, max_claims, r_view, w_gain, g_cap, min_gain, r_keep, keep_ratio16, keep_slack,
                        frontier_planner_kwargs, self.gain_from == "region")


ROBOT_FIELDS_MAX_THREADS = 1 << 31    # B * (W * H + 64): the threads of one round launch of the per-robot fields


class _RobotFieldsKeywords(_TiledKeywords):
    """``_TiledKeywords`` for the class that has no untiled form: an explicit ``tiled=False`` is refused, not overruled."""

    def __call__(cls, *args, **kwargs):
        if "tiled" in kwargs and not kwargs["tiled"]:
            raise ValueError(f"{cls.__name__}: tiled=False is not supported (the per-robot fields are relaxed by the tiled rounds only; "
                             f"the one-workgroup class is CoordinatedFrontierPlanner)")
        return super().__call__(*args, **kwargs)


class RobotFieldsFrontierPlanner(TiledCoordinatedFrontierPlanner, metaclass=_RobotFieldsKeywords):
    """``TiledCoordinatedFrontierPlanner`` whose claims come from ONE single-source field per robot, all B of them relaxed in the same
    rounds (include/lipmpc.h, CLAIMS FROM PER-ROBOT FIELDS, ``lipmpc_grid_frontier_assign_robot_fields_batch``): the tiled
    nearest-frontier plan, then a claim call of ``budget`` + 8 launches whatever ``max_claims`` is -- every claim round and the whole
    keep phase are reductions over the fields in memory, and the winners' paths are walked a wavefront each, all at once.  Claiming
    for every robot (``max_claims`` = B) is no longer something to ration.
    The rule is the parent's greedy over (robot, frontier cell) pairs with these differences: a robot enters the map ONCE, at its
    start cell or the snap in the nearest-frontier field (the parent snaps again in every round's field: the two differ only for a
    robot that stands on an impassable cell); ``max_claims`` caps the winners, and a failed keep attempt costs nothing.
    ``plan`` / ``replan`` return the parent's dict (``tiled_assign_outputs``; with the keep keywords ``tiled_assign_keep_outputs``);
    ``claims_settled`` [1] = 1: the nearest-frontier field and every robot's field settled and the claims are the rule's; 0: nobody
    claimed, every row is the nearest-frontier plan's.
    Keyword-only ``r_keep`` / ``keep_ratio16`` / ``keep_slack``: all three or none, no defaults (nobody has measured one), the
    parent's ranges.  Keyword-only ``rounds``: an int = the budget of the frontier field and of the per-robot fields, one call each,
    no synchronisation, capturable; None = a cold call with the parent's starting budget, then resumed calls with a doubled budget
    until ``claims_settled`` -- one word read on the host per call, so this raises under stream capture.  ``paths`` governs the
    nearest-frontier plan.  The workspace is the planner's own: grown only, every buffer kept alive, never grown under capture.
    The limits: the workspace holds the B fields, 4 B W H bytes (33.5 MB for 64 robots on 362 x 362), and a fleet with
    B * (W * H + 64) > 2^31 is refused; there are no gain seeds (``r_view`` / ``w_gain`` / ``g_cap`` / ``min_gain``) and no clearance
    (``r_clear`` / ``w_clear`` / ``cost=``): ValueError, as is ``tiled=False``; the device still cannot end the rounds early."""

    _LAUNCH_CAP = False             # (max_claims * rounds <= 2^20 is the parent's claim call's: this one's launches are rounds + 8)
    _REGIONS = False                # (no gain seeds here, so nothing for gain_from / target to replace)

    def __init__(self, r_claim: int, max_claims: int = 64, *, r_keep: int | None = None, keep_ratio16: int | None = None,
                 keep_slack: int | None = None, **frontier_planner_kwargs):
        gain = sorted(k for k in ("r_view", "w_gain", "g_cap", "min_gain") if k in frontier_planner_kwargs)
        if gain:
            raise ValueError(f"{type(self).__name__}: {gain} not supported (the per-robot fields have no gain seeds; the gain-seeded "
                             f"claims are TiledCoordinatedFrontierPlanner's)")
        keep = dict(r_keep=r_keep, keep_ratio16=keep_ratio16, keep_slack=keep_slack)
        if any(v is not None for v in keep.values()) and any(v is None for v in keep.values()):
            raise ValueError("r_keep, keep_ratio16 and keep_slack go together: they have no defaults, nobody has measured one")
        super().__init__(r_claim, max_claims, **{k: v for k, v in keep.items() if v is not None}, **frontier_planner_kwargs)

    def _plan(self, mapper_or_evidence, start, origin, cell, S_max, out, may_claim, prev_target):
        ev = self._map(mapper_or_evidence, origin, cell)[0]
        B, (_, W, H) = len(start), ev.shape
        if B * (W * H + 64) > ROBOT_FIELDS_MAX_THREADS:
            raise ValueError(f"{B} robots on {W} x {H} cells: the per-robot fields need B * (W * H + 64) <= 2^31 (the threads of one "
                             f"round launch, and {4 * B * W * H / 2 ** 30:.1f} GiB of fields); claim with fewer robots per call or use "
                             f"TiledCoordinatedFrontierPlanner")
        return super()._plan(mapper_or_evidence, start, origin, cell, S_max, out, may_claim, prev_target)

    def _claim_call(self, B, W, H, start, may_claim, prev_target, org_c, cell_c, S_max, out, budget, resume):
        """ONE lipmpc_grid_frontier_assign_robot_fields_batch on the current stream: ``budget`` rounds, cold (``resume`` 0) or on the
        fields the call before left in the workspace (1)."""
        size = "lipmpc_grid_frontier_assign_robot_fields_workspace_bytes"
        work = self._workspace(self._claim_works, int(getattr(self.lib, size)(B, W, H)), size)
        keep = self.r_keep is not None
        _lib.call("lipmpc_grid_frontier_assign_robot_fields_batch", device=self.device_index, B=B, W=W, H=H,
                  origin=C.addressof(org_c), cell=C.addressof(cell_c), frontier=out["frontier"], field=out["field"],
                  settled=out["settled"], start=start, may_claim=may_claim, prev_target=prev_target, r_inflate=self.r_inflate,
                  r_claim=self.r_claim, r_keep=self.r_keep if keep else 0, keep_ratio16=self.keep_ratio16 if keep else 16,
                  keep_slack=self.keep_slack if keep else 0, max_claims=self.max_claims, max_seg=self.max_seg, S_max=S_max,
                  work=work, work_bytes=work.numel(), max_rounds=int(budget), resume=int(resume),
                  **_named(out, ("sub_goals", "n_sub", "status", "path_cost", "target_cell", "claim_round", "n_claims")),
                  kept=out["kept"] if keep else None, n_kept=out["n_kept"] if keep else None,
                  claims_settled=self._settled(out, 1, "claims_settled"), hip_stream=torch.cuda.current_stream(self.device).cuda_stream)

    def _claims(self, B, W, H, start, may_claim, org_c, cell_c, S_max, out, prev_target=None, gain=False):
        if self.rounds is None and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("rounds=None reads `claims_settled` on the host: give the planner a fixed `rounds` to capture its calls")
        call = functools.partial(self._claim_call, B, W, H, start, may_claim, prev_target, org_c, cell_c, S_max, out)
        if self.rounds is not None:
            return call(self.rounds, 0)
        tw, th, _ = tiled_info()
        budget = max(8, -(-W // tw) - (-H // th) + 1)
        call(budget, 0)
        done = out["claims_settled"]
        # (ends: every round but the last lowers a word, and words are bounded below; an unsettled nearest-frontier field cannot
        # happen here -- with rounds=None the field call before this one ran until it settled)
        while not bool(done[0]):
            budget = min(2 * budget, 65536)
            call(budget, 1)


class InformedFrontierPlanner(FrontierPlanner):
    """``FrontierPlanner`` with a utility from expected visibility (include/lipmpc.h, INFORMED EXPLORER): the GAIN of a frontier cell
    is the number of distinct unknown cells that a fan of 8 ``r_view`` rays from it reaches within ``r_view`` cells (1..64) before a
    solid cell; the UTILITY FIELD is the cost-to-go to the frontier in which a source starts at
    (``w_gain`` * (``g_cap`` - min(gain, ``g_cap``))) >> 4 instead of 0 -- ``w_gain`` (0..65535) sixteenths of a cost unit (5 per
    cell) for every cell it reveals less than ``g_cap`` (1..16384) -- and only frontier cells with gain >= ``min_gain`` (0..16384)
    are sources.  One field per shared map still serves every robot.  With ``g_cap`` well below the disc's cell count every cell that
    reveals enough starts at 0: robots go to the nearest good-enough frontier rather than all to the single best one.  With
    ``min_gain`` > 0 slivers are nobody's target, and a fleet stops (RRT_NO_PATH) when nothing worth seeing is left.  ``w_gain`` = 0
    with ``min_gain`` = 0 is ``FrontierPlanner``, bit for bit.  None of the three gain parameters has a default: nobody has measured
    one.  The other arguments are ``FrontierPlanner``'s.
    The model's limits: unknown cells do not occlude; there is no memory between plans (no hysteresis), so a replan may hand a robot
    another target; a shared field sends robots that stand together to the same cell, as the parent does.
    Keyword-only ``gain_from`` = "view" (default) / "region" and ``target`` = "cell" (default) / "representative" (include/lipmpc.h,
    FRONTIER REGIONS): with "region" ``r_view`` must be None, the gain call is replaced by ``lipmpc_grid_frontier_regions_batch`` with
    min_size = max(``min_gain``, 1), the gain of a frontier cell is the SIZE of its region, and the plan dict gains label, rep
    [F,W,H], table [F,1024,5] and n_regions [F,3]; with "representative" one cell per tabled region -- the region's own cell
    nearest its centroid -- stands where the utility field and the utility path take ``frontier``.  ``w_gain``, ``g_cap`` and
    ``min_gain`` keep their meaning and ranges.  The coordinated classes with the gain keywords take both options likewise."""

    _TILED, _TILED_WHY, _TILED_CLASS = False, "the gain call and the utility field keep", "TiledInformedFrontierPlanner"
    _CLEARANCE = False
    _GAIN_CALL = True
    _SETTLED = ()               # what the large-map subclass adds to the dicts of gain() and field()

    def __init__(self, r_view: int, w_gain: int, g_cap: int, min_gain: int = 0, **frontier_planner_kwargs):
        region = self.gain_from == "region"
        if region and r_view is not None:
            raise ValueError(f"gain_from='region' with r_view {r_view}: r_view must be None (the gain is the region's size, no ray is "
                             f"marched)")
        # (r_view 0 marks a planner whose gain is the region's size)
        self.r_view, self.w_gain, self.g_cap, self.min_gain = 0 if region else int(r_view), int(w_gain), int(g_cap), int(min_gain)
        if not (region or 1 <= self.r_view <= 64) or not 0 <= self.w_gain <= 65535 or not 1 <= self.g_cap <= 16384 or \
                not 0 <= self.min_gain <= 16384:
            raise ValueError(f"invalid gain parameters (r_view {r_view}: 1..64, w_gain {w_gain}: 0..65535, g_cap {g_cap}: 1..16384, "
                             f"min_gain {min_gain}: 0..16384)")
        super().__init__(**frontier_planner_kwargs)

    def _gain(self, ev, t_free, t_occ, out):
        if self.gain_from == "region":
            return self._region_gain(ev, out)
        F, W, H = ev.shape
        _lib.call("lipmpc_grid_frontier_gain_batch", device=self.device_index, F=F, W=W, H=H, evidence=ev, t_free=t_free, t_occ=t_occ,
                  frontier=out["frontier"], r_view=self.r_view, gain=out["gain"], hip_stream=torch.cuda.current_stream(self.device).cuda_stream)

    def _ufield(self, ev, out):
        F, W, H = ev.shape
        _lib.call("lipmpc_grid_frontier_utility_field_batch", device=self.device_index, F=F, W=W, H=H, frontier=self._sources(out),
                  field=out["field"], gain=out["gain"], w_gain=self.w_gain, g_cap=self.g_cap, min_gain=self.min_gain, ufield=out["ufield"],
                  n_sources=out["n_sources"], hip_stream=torch.cuda.current_stream(self.device).cuda_stream)

    def _fields(self, mapper_or_evidence, out, names):
        ev, t_free, t_occ, _, _ = self._map(mapper_or_evidence)
        regions = self._region_table(*ev.shape)
        table = dict(informed_outputs(0, *ev.shape, 1), **regions)
        if out is None:
            out = _alloc(table, names, self.device)
            out.update(_alloc(regions, tuple(regions), self.device, torch.zeros))      # (table rows past the kept regions stay 0)
        names = names + tuple(regions)
        if out is not None:
            _check_table({k: table[k] for k in names}, out, self.device, "out")
        self._field(ev, t_free, t_occ, out)
        self._gain(ev, t_free, t_occ, out)
        if "ufield" in names:
            self._ufield(ev, out)
        return {k: out[k] for k in names + tuple(k for k in self._SETTLED if k in out)}

    def gain(self, mapper_or_evidence, out=None):
        """``FrontierPlanner.field``'s dict plus gain [F,W,H] int32: per frontier cell the unknown cells seen from it, 0 elsewhere."""
        return self._fields(mapper_or_evidence, out, ("field", "frontier", "n_frontier", "gain"))

    def field(self, mapper_or_evidence, out=None):
        """``FrontierPlanner.field``'s dict (the nearest-frontier field) plus gain [F,W,H] int32, ufield [F,W,H] uint32 (the utility
        field: a source's seed where nothing dominates it, FIELD_INF = impassable or cut off) and n_sources [F] (0: nothing worth
        seeing is left, the whole ufield FIELD_INF).  ``out``: that dict, to write into."""
        return self._fields(mapper_or_evidence, out, ("field", "frontier", "n_frontier", "gain", "ufield", "n_sources"))

    def plan(self, mapper_or_evidence, start, origin=None, cell=None, S_max: int = 64, out=None):
        """``FrontierPlanner.plan`` down the utility field: shared or per-robot maps, the same arguments.  Returns the parent's dict
        -- sub_goals, n_sub, status (RRT_NO_PATH: no source left, or none within reach), path_cost (the walk's length in cells),
        target, target_cell; field, frontier and n_frontier stay the nearest-frontier ones -- plus gain [F,W,H], ufield [F,W,H],
        n_sources [F] and target_gain [B] (the gain of the target cell, -1 unless FOUND or PATH_OVERFLOW).  ``out``: that dict, to
        write into (a captured graph replays into the same buffers; nothing is allocated then)."""
        ev, t_free, t_occ, origin, cell = self._map(mapper_or_evidence, origin, cell)
        origin, cell, org_c, cell_c = self._placement(origin, cell)
        start = torch.as_tensor(start).to(device=self.device, dtype=torch.float64).contiguous()
        if start.dim() != 2 or start.shape[1] != 2:
            raise ValueError("start must be [B,2]")
        B, (F, W, H), S_max = start.shape[0], ev.shape, int(S_max)
        if F != B and F != 1:
            raise ValueError(f"{F} maps for {B} robots: one shared map, or one per robot")
        regions = self._region_table(F, W, H)
        table = dict(informed_outputs(B, F, W, H, S_max), **regions)
        if out is None:
            out = _alloc(table, ("sub_goals", "n_sub", "status", "path_cost", "target", "target_cell"), self.device, torch.zeros)
            out.update(_alloc(table, ("field", "frontier", "n_frontier", "gain", "ufield", "n_sources"), self.device))     # written whole
            out.update(_alloc(regions, tuple(regions), self.device, torch.zeros))
            out["target_gain"] = torch.full((B,), -1, dtype=torch.int32, device=self.device)
        else:
            _check_table(table, out, self.device, "out")
        if B == 0:
            return out
        self._field(ev, t_free, t_occ, out)
        self._gain(ev, t_free, t_occ, out)
        self._ufield(ev, out)
        self._path(ev, t_occ, start, org_c, cell_c, S_max, out)
        self._target(out, origin, cell, H)
        self.last = out
        return out

    def _path(self, ev, t_occ, start, org_c, cell_c, S_max, out):
        F, W, H = ev.shape
        name, more = "lipmpc_grid_frontier_utility_path_batch", {}
        if self.paths == "wave":
            name, more = "lipmpc_grid_frontier_utility_path_wave_batch", dict(settled=None)
        _lib.call(name, device=self.device_index, B=start.shape[0], F=F, W=W, H=H,
                  origin=C.addressof(org_c), cell=C.addressof(cell_c), evidence=ev, t_occ=t_occ,
                  frontier=self._sources(out), **_named(out, ("gain", "ufield", "n_sources")), **more, w_gain=self.w_gain, g_cap=self.g_cap, min_gain=self.min_gain,
                  start=start, r_inflate=self.r_inflate, max_seg=self.max_seg, S_max=S_max,
                  **_named(out, ("sub_goals", "n_sub", "status", "path_cost", "target_cell", "target_gain")),
                  hip_stream=torch.cuda.current_stream(self.device).cuda_stream)


class TiledInformedFrontierPlanner(_AlwaysTiled, InformedFrontierPlanner):
    """``InformedFrontierPlanner`` on maps of up to 2^24 cells (include/lipmpc.h, TILED EXPLORERS): the tiled nearest-frontier
    field, the gain by one workgroup per tile (``lipmpc_grid_frontier_gain_tiled_batch``), the utility field by tiled rounds in a
    workspace of its own (``lipmpc_grid_frontier_utility_field_tiled_batch``) and the paths down it
    (``lipmpc_grid_frontier_utility_path_tiled_batch``).  ``gain``, ``field`` and ``plan`` return the parent's dicts plus ``settled``
    [F] (the nearest-frontier field) and ``usettled`` [F] (the utility field); once both are 1 every output is the parent's, bit for
    bit.  A robot whose utility field is not settled gets RRT_FIELD_UNSETTLED, target_cell -1, target_gain -1 and no sub-goal; the
    utility field does not read the nearest-frontier field, so ``settled`` == 0 alone costs a robot nothing.
    Keyword-only ``rounds``: an int = the budget of each of the two fields, one call each, no synchronisation, capturable; None =
    each field resumed with doubled budgets until it is settled (reads ``settled`` on the host: raises under stream capture).
    The limits that remain are the parent's: unknown cells do not occlude, and there is no memory between plans."""

    def __init__(self, r_view: int, w_gain: int, g_cap: int, min_gain: int = 0, **frontier_planner_kwargs):
        super().__init__(r_view, w_gain, g_cap, min_gain, **frontier_planner_kwargs)
        self._uworks = []           # the utility field's own workspace: a resume of the frontier field still reads the other one

    _SETTLED = ("settled", "usettled")

    def _field(self, ev, t_free, t_occ, out):
        self._classes = t_free, t_occ                      # (what the utility field call classifies the evidence by)
        return super()._field(ev, t_free, t_occ, out)

    def _gain(self, ev, t_free, t_occ, out):
        if self.gain_from == "region":
            return self._region_gain(ev, out)
        F, W, H = ev.shape
        _lib.call("lipmpc_grid_frontier_gain_tiled_batch", device=self.device_index, F=F, W=W, H=H, evidence=ev, t_free=t_free,
                  t_occ=t_occ, frontier=out["frontier"], r_view=self.r_view, gain=out["gain"],
                  hip_stream=torch.cuda.current_stream(self.device).cuda_stream)

    def _ufield(self, ev, out):
        F, W, H = ev.shape
        t_free, t_occ = self._classes
        self._run_tiled("lipmpc_grid_frontier_utility_field_tiled_batch", F, W, H, out, works=self._uworks, key="usettled", evidence=ev,
                        t_free=t_free, t_occ=t_occ, r_inflate=self.r_inflate, frontier=self._sources(out), gain=out["gain"],
                        w_gain=self.w_gain, g_cap=self.g_cap, min_gain=self.min_gain, ufield=out["ufield"], n_sources=out["n_sources"])

    def plan(self, mapper_or_evidence, start, origin=None, cell=None, S_max: int = 64, out=None):
        """``InformedFrontierPlanner.plan`` by the tiled calls: its dict plus ``settled`` and ``usettled`` [F]."""
        F = self._map(mapper_or_evidence, origin, cell)[0].shape[0]
        if out is not None:
            self._settled(out, F)
            self._settled(out, F, "usettled")
        out = super().plan(mapper_or_evidence, start, origin, cell, S_max, out)
        for key in ("settled", "usettled"):                # (B = 0: no call was made)
            self._settled(out, F, key)
        return out

    def _path(self, ev, t_occ, start, org_c, cell_c, S_max, out):
        F, W, H = ev.shape
        name = "lipmpc_grid_frontier_utility_path_wave_batch" if self.paths == "wave" else "lipmpc_grid_frontier_utility_path_tiled_batch"
        _lib.call(name, device=self.device_index, B=start.shape[0], F=F, W=W, H=H,
                  origin=C.addressof(org_c), cell=C.addressof(cell_c), evidence=ev, t_occ=t_occ,
                  frontier=self._sources(out), **_named(out, ("gain", "ufield", "n_sources")), settled=out["usettled"], w_gain=self.w_gain, g_cap=self.g_cap,
                  min_gain=self.min_gain, start=start, r_inflate=self.r_inflate, max_seg=self.max_seg, S_max=S_max,
                  **_named(out, ("sub_goals", "n_sub", "status", "path_cost", "target_cell", "target_gain")),
                  hip_stream=torch.cuda.current_stream(self.device).cuda_stream)
