"""Time the tiled field calls (lipmpc_grid_field_tiled_batch, lipmpc_grid_frontier_field_tiled_batch and their path calls) beside
the one-workgroup calls of the same build -> profiles/grid_field_tiled.json.  Needs the GPU; run from the repository root:

    python tools/field_tiled_bench.py

One process, every variant warmed up, then device events around `reps` back-to-back calls, the variants alternating in rounds;
median / min / max over the rounds, in ms per call.  Every timed step (a warm-up, a round of one variant, a count of rounds) runs
under a watchdog of its own: a step that does not come back within --limit seconds ends the process with status 124.
  - field, and field + path (16 robots), of both kinds at 92 x 80 (the fleet scene of tools/field_bench.py), 200 x 199 and 362 x 362
    (the baffle strips of tests/field_shape_cases.py): tiled against one workgroup -- the only sizes both can run;
  - the serpentine corridor of tests/test_field_shapes_gpu.py (19 601 cells) at 199 x 199 and 200 x 199: the goal field, both ways;
  - 1024^2, 2048^2 and 4096^2, an open field (goal in cell (0, 0)) and walls with alternating gaps: the tiled goal field alone.
A tiled call is timed with a FIXED budget: the rounds the map needed to settle, counted first by resuming one round at a time, plus
one; `rounds` in the output is that count, `settled` what the timed budget gave.
"""
import argparse
import json
import os
import sys
import threading

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import lipmpc  # noqa: E402
import field_shape_cases as S  # noqa: E402
from field_bench import fleet_scene  # noqa: E402
from lidar_grid_bench import events_ms  # noqa: E402

LIMIT = [120.0]


def limited(fn, *args):
    """fn(*args) and a device synchronisation under the step's watchdog."""
    watchdog = threading.Timer(LIMIT[0], lambda: (sys.stderr.write("field_tiled_bench: a step ran past its limit\n"), os._exit(124)))
    watchdog.daemon = True
    watchdog.start()
    try:
        r = fn(*args)
        torch.cuda.synchronize()
        return r
    finally:
        watchdog.cancel()


def rounds_of(variants, reps, rounds):
    """{name: median / min / max ms per call}; a variant whose warm-up call takes more than 50 ms is timed one call at a time."""
    n = {}
    for k, fn in variants.items():
        limited(fn)
        n[k] = 1 if limited(events_ms, fn, 1) > 50.0 else reps
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            ms[k].append(limited(events_ms, fn, n[k]))
    return {k: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "reps": n[k]} for k, v in ms.items()}


def walls(n, every=128, gap=64):
    """n x n: walls two cells thick every `every` rows, each with one gap of `gap` cells, alternately at either end."""
    occ = np.zeros((n, n), np.uint8)
    for k, i in enumerate(range(every, n - 2, every)):
        occ[i:i + 2, :] = 1
        occ[i:i + 2, (slice(8, 8 + gap) if k % 2 == 0 else slice(n - 8 - gap, n - 8))] = 0
    return occ


class Tiled:
    """One map and one kind: the C call with a budget, on buffers of its own."""

    def __init__(self, kind, arr, origin, cell, goal, r, mu=2):
        self.kind, dev = kind, torch.device("cuda", 0)
        W, H = arr.shape
        self.W, self.H, self.r, self.mu = W, H, r, mu
        self.field = torch.empty((1, W, H), dtype=torch.uint32, device=dev)
        self.status = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.settled = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.work = torch.empty(int(lipmpc._lib.load().lipmpc_grid_tiled_workspace_bytes(1, W, H)), dtype=torch.uint8, device=dev)
        if kind == "goal":
            self.grid = lipmpc.GridMap(arr, origin, cell).to(dev)
            self.goal = torch.as_tensor(np.asarray(goal, np.float64).reshape(1, 2), device=dev)
        else:
            self.ev = torch.as_tensor(np.ascontiguousarray(arr, np.int32), device=dev)
            self.frontier = torch.empty((1, W, H), dtype=torch.uint8, device=dev)

    def call(self, rounds, resume=0):
        tail = dict(work=self.work, work_bytes=self.work.numel(), max_rounds=rounds, resume=resume, settled=self.settled,
                    hip_stream=torch.cuda.current_stream().cuda_stream)
        if self.kind == "goal":
            lipmpc._lib.call("lipmpc_grid_field_tiled_batch", device=0, F=1, **self.grid._args(1, torch.device("cuda", 0)), goal=self.goal,
                             r_inflate=self.r, field=self.field, field_status=self.status, **tail)
        else:
            lipmpc._lib.call("lipmpc_grid_frontier_field_tiled_batch", device=0, F=1, W=self.W, H=self.H, evidence=self.ev, t_free=S.T_FREE,
                             t_occ=S.T_OCC, r_inflate=self.r, min_unknown=self.mu, frontier=self.frontier, field=self.field,
                             n_frontier=self.status, **tail)

    def rounds_needed(self):
        """Rounds until settled, one at a time (the last one is the round in which nothing falls)."""
        self.call(1)
        n = 1
        while int(self.settled[0]) == 0:
            self.call(1, 1)
            n += 1
        return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grid_field_tiled.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=float, default=120.0, help="seconds a single timed step may take")
    ap.add_argument("--largest", type=int, default=4096)
    a = ap.parse_args()
    LIMIT[0] = a.limit
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda", 0)
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=dev)
    tw, th, cap = lipmpc.tiled_info()
    variants, info = {}, {}

    # -- the sizes both can run ------------------------------------------------------------------------------------------
    occ, origin, cell, goal = fleet_scene()
    rng = np.random.default_rng(5)
    free = np.argwhere(occ == 0)
    start = np.stack([origin[0] + (free[rng.integers(len(free), size=16), 0] + 0.5) * cell[0],
                      origin[1] + (free[rng.integers(len(free), size=16), 1] + 0.5) * cell[1]], 1)
    ev = np.where(occ != 0, S.T_OCC, -S.T_FREE).astype(np.int32)
    ev[-2:, -2:] = 0
    maps = {"92x80": dict(occ=occ, ev=ev, origin=origin, cell=cell, goal=np.asarray(goal, float).reshape(1, 2), start=start, r=2)}
    for W, H in ((200, 199), (362, 362)):
        c = S.strip_case(W, H)
        maps[f"{W}x{H}"] = dict(occ=c["occ"], ev=c["ev"], origin=S.ORIGIN, cell=S.CELL, goal=c["goal"], start=c["start"], r=c["r"])
    keep = []
    for name, m in maps.items():
        W, H = m["occ"].shape
        grid, d_goal, d_start, d_ev = lipmpc.GridMap(m["occ"], m["origin"], m["cell"]).to(dev), t(m["goal"]), t(m["start"]), t(m["ev"])
        for kind in ("goal", "frontier"):
            probe = Tiled(kind, m["occ"] if kind == "goal" else m["ev"], m["origin"], m["cell"], m["goal"], m["r"])
            need = limited(probe.rounds_needed)
            info[f"{name}_{kind}"] = dict(rounds=need, tiles=-(-W // tw) * -(-H // th))
            for tiled in (False, True):
                kw = dict(tiled=True, rounds=need + 1) if tiled else {}
                if kind == "goal":
                    pl = lipmpc.GridFieldPlanner(r_inflate=m["r"], max_seg=200, **kw)
                    out = {k: torch.zeros(shape, dtype=dt, device=dev) if dt != torch.uint32 else torch.empty(shape, dtype=dt, device=dev)
                           for k, (dt, shape, _) in lipmpc.planner.field_plan_outputs(16, 1, W, H, 256).items()}
                    field = lambda pl=pl, out=out, grid=grid, g=d_goal: pl.field(g, grid, out=out)
                    plan = lambda pl=pl, out=out, grid=grid, g=d_goal, s=d_start: pl.plan_grid_batch(g, grid, s, S_max=256, out=out)
                else:
                    pl = lipmpc.FrontierPlanner(r_inflate=m["r"], min_unknown=2, t_free=S.T_FREE, t_occ=S.T_OCC, max_seg=200, **kw)
                    out = {k: torch.zeros(shape, dtype=dt, device=dev) if dt != torch.uint32 else torch.empty(shape, dtype=dt, device=dev)
                           for k, (dt, shape, _) in lipmpc.planner.frontier_outputs(16, 1, W, H, 256).items()}
                    field = lambda pl=pl, out=out, e=d_ev: pl.field(e, out=out)
                    plan = lambda pl=pl, out=out, e=d_ev, s=d_start, m=m: pl.plan(e, s, origin=m["origin"], cell=m["cell"], S_max=256, out=out)
                way = "tiled" if tiled else "one_workgroup"
                variants[f"{name}_{kind}_field_{way}"] = field
                variants[f"{name}_{kind}_field_plus_path_{way}"] = plan
                keep.append((pl, out))
    # -- the serpentine corridor -------------------------------------------------------------------------------------------
    for W, H in ((199, 199), (200, 199)):
        occ_s, cells = S.serpentine(W, H)
        g = np.array([S.centre(cells[0])])
        probe = Tiled("goal", occ_s, S.ORIGIN, S.CELL, g, 0)
        need = limited(probe.rounds_needed)
        info[f"serpentine_{W}x{H}"] = dict(rounds=need, cells=len(cells), tiles=-(-W // tw) * -(-H // th))
        grid, d_goal = lipmpc.GridMap(occ_s, S.ORIGIN, S.CELL).to(dev), t(g)
        for tiled in (False, True):
            pl = lipmpc.GridFieldPlanner(**(dict(tiled=True, rounds=need + 1) if tiled else {}))
            out = dict(field=torch.empty((1, W, H), dtype=torch.uint32, device=dev), field_status=torch.zeros((1,), dtype=torch.int32, device=dev))
            variants[f"serpentine_{W}x{H}_field_{'tiled' if tiled else 'one_workgroup'}"] = lambda pl=pl, out=out, grid=grid, g=d_goal: pl.field(g, grid, out=out)
            keep.append((pl, out))
    # -- large maps: tiled alone -------------------------------------------------------------------------------------------
    large = {}
    for n in (1024, 2048, 4096):
        if n > a.largest:
            continue
        for name, occ_n, g in (("open", np.zeros((n, n), np.uint8), (0.025, 0.025)), ("walls", walls(n), (0.025, 0.025))):
            probe = Tiled("goal", occ_n, (0.0, 0.0), (0.05, 0.05), g, 0)
            need = limited(probe.rounds_needed)
            info[f"{n}x{n}_{name}"] = dict(rounds=need, tiles=-(-n // tw) * -(-n // th))
            large[f"{n}x{n}_{name}"] = probe
            variants[f"{n}x{n}_{name}_field_tiled"] = lambda p=probe, r=need + 1: p.call(r)
    ms = rounds_of(variants, a.reps, a.rounds)
    for k, p in large.items():
        info[k]["settled"] = int(p.settled[0])
        info[k]["finite_cells"] = int((p.field.view(torch.int32) != -1).sum())
    for pl, out in keep:
        if "settled" in out:
            assert int(out["settled"].min()) == 1, "a timed budget did not settle"
    out = {"what": "ms per call, device events around `reps` back-to-back calls (1 where a call takes more than 50 ms), median / min / max "
                   "over alternating rounds, one process; tiled calls with a fixed budget of `rounds` + 1 rounds, no host synchronisation",
           "device": torch.cuda.get_device_name(0), "reps_per_round": a.reps, "rounds": a.rounds, "tile": [tw, th], "robots_per_path_call": 16,
           "maps": info, "ms_per_call": ms}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
