"""Time soft clearance (lipmpc_grid_clearance_cost_batch and the weighted tiled fields and paths) beside the existing tiled calls
-> profiles/clearance.json.  Needs the GPU; run from the repository root:

    python tools/clearance_bench.py [--parent-lib PATH/liblipmpc.so]

One process, every variant warmed up, then device events around `reps` back-to-back calls, the variants alternating in rounds;
median / min / max over 5 rounds, in ms per call.  Every timed step runs under a watchdog of its own (tools/field_tiled_bench.py's):
a step that does not come back within --limit seconds ends the process with status 124.
  - the cost layer alone at 362 x 362, 1024^2 and 4096^2 on an open map, a lattice of single solid cells every 16 cells and 3 % random
    solid cells, at r_clear 4 and 31;
  - the goal and the frontier field at 92 x 80 (the fleet scene of tools/field_bench.py), 362 x 362 (the baffle strip of
    tests/field_shape_cases.py) and 1024^2 (tools/field_tiled_bench.py's walls): the existing tiled call, the weighted call on a given
    layer, and the planner with r_clear 4 / w_clear 40 (layer + weighted field); field alone, and field + path for 16 robots.  Each
    call has a FIXED budget: the rounds its map needed to settle, counted first by resuming one round at a time, plus one; both counts
    (unweighted, weighted) are recorded.
  - --parent-lib: the library built from the PARENT commit (git worktree add ../parent HEAD~ && make -C ../parent/<package>/csrc).
    A child process of this run loads it (LIPMPC_LIB) and times the existing tiled variants alone; the code-object figures of the
    existing tiled kernels in both libraries are compared and recorded.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import lipmpc  # noqa: E402
import field_shape_cases as S  # noqa: E402
import field_tiled_bench as FT  # noqa: E402
from code_object import kernel_resources  # noqa: E402
from field_bench import fleet_scene  # noqa: E402

NEW = ("lipmpc_grid_clearance_cost_batch", "lipmpc_grid_field_weighted_batch", "lipmpc_grid_frontier_field_weighted_batch",
       "lipmpc_grid_path_weighted_batch", "lipmpc_grid_frontier_path_weighted_batch")
R_CLEAR, W_CLEAR = 4, 40
FIGURES = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")


class Weighted(FT.Tiled):
    """FT.Tiled by the weighted calls on a given layer."""

    def __init__(self, kind, arr, origin, cell, goal, r, cost):
        super().__init__(kind, arr, origin, cell, goal, r)
        self.cost = cost

    def call(self, rounds, resume=0):
        tail = dict(work=self.work, work_bytes=self.work.numel(), max_rounds=rounds, resume=resume, settled=self.settled,
                    hip_stream=torch.cuda.current_stream().cuda_stream)
        if self.kind == "goal":
            lipmpc._lib.call("lipmpc_grid_field_weighted_batch", device=0, F=1, **self.grid._args(1, torch.device("cuda", 0)), cost=self.cost,
                             goal=self.goal, r_inflate=self.r, field=self.field, field_status=self.status, **tail)
        else:
            lipmpc._lib.call("lipmpc_grid_frontier_field_weighted_batch", device=0, F=1, W=self.W, H=self.H, evidence=self.ev, cost=self.cost,
                             t_free=S.T_FREE, t_occ=S.T_OCC, r_inflate=self.r, min_unknown=self.mu, frontier=self.frontier, field=self.field,
                             n_frontier=self.status, **tail)


def field_maps():
    occ, origin, cell, goal = fleet_scene()
    maps = {"92x80": dict(occ=occ, origin=origin, cell=cell, goal=np.asarray(goal, float).reshape(1, 2), r=2)}
    c = S.strip_case(362, 362)
    maps["362x362"] = dict(occ=c["occ"], origin=S.ORIGIN, cell=S.CELL, goal=c["goal"], r=c["r"])
    maps["1024x1024"] = dict(occ=FT.walls(1024), origin=(0.0, 0.0), cell=(0.05, 0.05), goal=np.array([[0.025, 0.025]]), r=0)
    rng = np.random.default_rng(5)
    for m in maps.values():
        free = np.argwhere(m["occ"] == 0)
        pick = free[rng.integers(len(free), size=16)]
        m["start"] = np.stack([m["origin"][0] + (pick[:, 0] + 0.5) * m["cell"][0], m["origin"][1] + (pick[:, 1] + 0.5) * m["cell"][1]], 1)
        m["ev"] = np.where(m["occ"] != 0, S.T_OCC, -S.T_FREE).astype(np.int32)
        m["ev"][-2:, -2:] = 0                                   # the unknown block in the far corner: the frontier lies beside it
    return maps


def cost_maps(n):
    lattice = np.zeros((n, n), np.uint8)
    lattice[8::16, 8::16] = 1
    return {"open": np.zeros((n, n), np.uint8), "lattice": lattice, "random3": (np.random.default_rng(n).random((n, n)) < 0.03).astype(np.uint8)}


def buffers(table, dev):
    return {k: torch.zeros(shape, dtype=dt, device=dev) if dt != torch.uint32 else torch.empty(shape, dtype=dt, device=dev)
            for k, (dt, shape, _) in table.items()}


def field_variants(maps, weighted):
    """({name: call}, {name: rounds}, what to keep alive): per map and kind the planner calls with their fixed budgets."""
    dev = torch.device("cuda", 0)
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=dev)
    variants, info, keep = {}, {}, []
    for name, m in maps.items():
        W, H = m["occ"].shape
        grid, d_goal, d_start, d_ev = lipmpc.GridMap(m["occ"], m["origin"], m["cell"]).to(dev), t(m["goal"]), t(m["start"]), t(m["ev"])
        for kind in ("goal", "frontier"):
            arr = m["occ"] if kind == "goal" else m["ev"]
            need = {"tiled": FT.limited(FT.Tiled(kind, arr, m["origin"], m["cell"], m["goal"], m["r"]).rounds_needed)}
            ways = {"tiled": {}}
            if weighted:
                layer = lipmpc.GridFieldPlanner(tiled=True, r_clear=R_CLEAR, w_clear=W_CLEAR).clearance_cost(grid).clone()
                need["weighted"] = FT.limited(Weighted(kind, arr, m["origin"], m["cell"], m["goal"], m["r"], layer).rounds_needed)
                ways.update(weighted=dict(cost=layer), clearance=dict(r_clear=R_CLEAR, w_clear=W_CLEAR))
            info[f"{name}_{kind}"] = dict(rounds=need, priced_cells=int((layer != 0).sum()) if weighted else None)
            for way, more in ways.items():
                kw = dict(tiled=True, rounds=need["tiled" if way == "tiled" else "weighted"] + 1, **{k: v for k, v in more.items() if k != "cost"})
                given = {k: v for k, v in more.items() if k == "cost"}
                if kind == "goal":
                    pl = lipmpc.GridFieldPlanner(r_inflate=m["r"], max_seg=200, **kw)
                    out = buffers(lipmpc.planner.field_plan_outputs(16, 1, W, H, 256), dev)
                    field = lambda pl=pl, out=out, grid=grid, g=d_goal, given=given: pl.field(g, grid, out=out, **given)
                    plan = lambda pl=pl, out=out, grid=grid, g=d_goal, s=d_start, given=given: pl.plan_grid_batch(g, grid, s, S_max=256, out=out, **given)
                else:
                    pl = lipmpc.FrontierPlanner(r_inflate=m["r"], min_unknown=2, t_free=S.T_FREE, t_occ=S.T_OCC, max_seg=200, **kw)
                    out = buffers(lipmpc.planner.frontier_outputs(16, 1, W, H, 256), dev)
                    field = lambda pl=pl, out=out, e=d_ev, given=given: pl.field(e, out=out, **given)
                    plan = lambda pl=pl, out=out, e=d_ev, s=d_start, m=m, given=given: pl.plan(e, s, origin=m["origin"], cell=m["cell"], S_max=256,
                                                                                             out=out, **given)
                variants[f"{name}_{kind}_field_{way}"] = field
                variants[f"{name}_{kind}_field_plus_path_{way}"] = plan
                keep.append((pl, out))
    return variants, info, keep


def child(a):
    """The existing tiled variants alone, with whatever library LIPMPC_LIB names: the timings as JSON on stdout."""
    for name in NEW:                                           # (the parent's library has none of them: bind what it has)
        lipmpc._lib.SIGNATURES.pop(name)
    variants, info, keep = field_variants(field_maps(), weighted=False)
    ms = FT.rounds_of(variants, a.reps, a.rounds)
    for pl, out in keep:
        assert int(out["settled"].min()) == 1, "a timed budget did not settle"
    print("CHILD_JSON " + json.dumps(dict(library="the parent commit's build (--parent-lib)", maps=info, ms_per_call=ms)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clearance.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=float, default=120.0, help="seconds a single timed step may take")
    ap.add_argument("--largest", type=int, default=4096)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    FT.LIMIT[0] = a.limit
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: a timing taken elsewhere says nothing")
    if a.child:
        return child(a)
    dev = torch.device("cuda", 0)
    # -- the parent's library, in a child process of this run ----------------------------------------------------------------
    parent = dict(run=False, why="no --parent-lib given")
    if a.parent_lib:
        mine, theirs = kernel_resources(lipmpc._lib.LIB_PATH), kernel_resources(a.parent_lib)
        tiled = sorted(n for n in theirs if "tiled_" in n)
        same = {n: {f: theirs[n].get(f) for f in FIGURES} == {f: mine.get(n, {}).get(f) for f in FIGURES} for n in tiled}
        env = dict(os.environ, LIPMPC_LIB=os.path.abspath(a.parent_lib))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--rounds", str(a.rounds), "--limit", str(a.limit)],
                           env=env, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise SystemExit(f"the child ended with status {r.returncode}:\n{r.stderr[-2000:]}")
        line, = (ln for ln in r.stdout.splitlines() if ln.startswith("CHILD_JSON "))
        parent = dict(run=True, existing_tiled_kernels_have_the_same_figures=all(same.values()), kernels=len(tiled),
                      figures_compared=list(FIGURES), **json.loads(line[len("CHILD_JSON "):]))
    # -- the fields ------------------------------------------------------------------------------------------------------------
    variants, info, keep = field_variants(field_maps(), weighted=True)
    # -- the cost layer alone ----------------------------------------------------------------------------------------------------
    stream = lambda: torch.cuda.current_stream().cuda_stream
    for n in (362, 1024, 4096):
        if n > a.largest:
            continue
        for name, occ in cost_maps(n).items():
            d_occ, cost = torch.as_tensor(occ, device=dev), torch.empty((1, n, n), dtype=torch.uint8, device=dev)
            for r in (4, 31):
                variants[f"{n}x{n}_{name}_cost_r{r}"] = lambda d_occ=d_occ, cost=cost, n=n, r=r: lipmpc._lib.call(
                    "lipmpc_grid_clearance_cost_batch", device=0, M=1, W=n, H=n, occ=d_occ, evidence=None, t_occ=0, r_clear=r, w_clear=W_CLEAR,
                    cost=cost, hip_stream=stream())
            keep.append((d_occ, cost))
    ms = FT.rounds_of(variants, a.reps, a.rounds)
    for pl, out in keep:
        if isinstance(out, dict):
            assert int(out["settled"].min()) == 1, "a timed budget did not settle"
    tw, th, _ = lipmpc.tiled_info()
    out = {"what": "ms per call, device events around `reps` back-to-back calls (1 where a call takes more than 50 ms), median / min / max over "
                   "alternating rounds, one process; field calls with a fixed budget of `rounds` + 1 rounds, no host synchronisation.  _tiled: the "
                   "existing call; _weighted: the weighted call on a given layer; _clearance: the planner with r_clear / w_clear (layer + "
                   "weighted field); _cost_rN: the layer alone at r_clear N",
           "device": torch.cuda.get_device_name(0), "reps_per_round": a.reps, "rounds": a.rounds, "tile": [tw, th], "robots_per_path_call": 16,
           "r_clear": R_CLEAR, "w_clear": W_CLEAR, "maps": info, "ms_per_call": ms, "parent_library": parent}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
