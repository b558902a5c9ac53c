"""Time the grid field planner (lipmpc_grid_field_batch, lipmpc_grid_path_batch) beside RRT* on a grid (lipmpc_rrt_plan_grid_batch,
unchanged code) -> profiles/grid_field.json.  Needs the GPU; run from the repository root:

    python tools/field_bench.py

One process, every variant warmed up, then device events around `reps` back-to-back calls, the variants alternating in rounds;
median / min / max over the rounds, in ms per call.  The map is the fleet scene of tests/golden/mapped_replanning.npz (92 x 80
cells of 0.05 m, the U-shaped wall), the goal its goal, the starts random free cells:
  - the field alone at F = 1 (one shared map) and at F = 4096 (one map per robot: the same map 4096 times);
  - the field alone at 251 x 201 cells with F = 1 (relaxed in global memory: the field does not fit the LDS);
  - the paths alone, 4096 robots down one field;
  - GridFieldPlanner.plan_grid_batch (field + paths) with one field for all robots at B = 1, 1024, 4096;
  - RrtStarPlanner.plan_grid_batch (n = 400, r_rewire = 30) on the same map at B = 1, 1024, 4096.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import lipmpc  # noqa: E402
from lidar_grid_bench import events_ms  # noqa: E402


def rounds_of(variants, reps, rounds, warm=3):
    for fn in variants.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            ms[k].append(events_ms(fn, reps))
    return {k: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))} for k, v in ms.items()}


def fleet_scene():
    d = np.load(os.path.join(ROOT, "tests", "golden", "mapped_replanning.npz"))
    (W, H), origin, cell = d["grid"].tolist(), tuple(float(v) for v in d["origin"]), tuple(float(v) for v in d["cell"])
    occ = np.zeros((W, H), np.uint8)
    for i0, j0, i1, j1 in d["walls"]:
        occ[i0:i1, j0:j1] = 1
    return occ, origin, cell, np.asarray(d["goal"], float)


def big_map(W=251, H=201):
    occ = np.zeros((W, H), np.uint8)
    for n, i in enumerate(range(30, W - 10, 40)):
        occ[i:i + 3, :] = 1
        gap = slice(10, 30) if n % 2 == 0 else slice(H - 30, H - 10)
        occ[i:i + 3, gap] = 0
    return occ


def free_starts(occ, origin, cell, n, seed):
    rng = np.random.default_rng(seed)
    ij = np.argwhere(occ == 0)
    ij = ij[rng.integers(len(ij), size=n)]
    return np.stack([origin[0] + (ij[:, 0] + rng.uniform(0.05, 0.95, n)) * cell[0], origin[1] + (ij[:, 1] + rng.uniform(0.05, 0.95, n)) * cell[1]], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grid_field.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--robots", type=int, default=4096)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda", 0)
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=dev)
    occ, origin, cell, goal = fleet_scene()
    W, H = occ.shape
    N = a.robots
    shared = lipmpc.GridMap(occ, origin, cell).to(dev)
    own = lipmpc.GridMap(t(np.broadcast_to(occ, (N, W, H))), origin, cell)
    big = lipmpc.GridMap(big_map(), (0.0, 0.0), 0.05).to(dev)
    big_goal = t([[0.05 * 245.5, 0.05 * 100.5]])
    goal1, goalN = t(goal[None]), t(np.tile(goal, (N, 1)))
    starts = t(free_starts(occ, origin, cell, N, 1))
    fp = lipmpc.GridFieldPlanner()
    rrt = lipmpc.RrtStarPlanner(n=400, r_rewire=30, seed=1, max_cells=1 << 13)
    table = lipmpc.planner.field_plan_outputs
    buf = lambda B, F, w, h: {k: torch.zeros(shape, dtype=dt, device=dev) if dt != torch.uint32 else torch.empty(shape, dtype=dt, device=dev)
                              for k, (dt, shape, _) in table(B, F, w, h, 64).items()}
    o1, oN, obig = buf(N, 1, W, H), buf(N, N, W, H), buf(1, 1, big.W, big.H)
    plans = {B: buf(B, 1, W, H) for B in (1, 1024, N)}
    fp.plan_grid_batch(goal1, shared, starts, out=o1)            # the field the path-only variant descends

    def paths_only():
        lipmpc._lib.call("lipmpc_grid_path_batch", device=0, B=N, F=1, **shared._args(1, dev), field=o1["field"], field_status=o1["field_status"],
                         goal=goal1, start=starts, r_inflate=0, max_seg=0x7FFFFFFF, S_max=64, sub_goals=o1["sub_goals"], n_sub=o1["n_sub"],
                         status=o1["status"], path_cost=o1["path_cost"], hip_stream=torch.cuda.current_stream(dev).cuda_stream)

    variants = {f"field_{W}x{H}_F1": lambda: fp.field(goal1, shared, out=o1),
                f"field_{W}x{H}_F{N}_per_robot_maps": lambda: fp.field(goalN, own, out=oN),
                f"field_{big.W}x{big.H}_F1_global_memory": lambda: fp.field(big_goal, big, out=obig),
                f"paths_B{N}_one_field": paths_only}
    for B in (1, 1024, N):
        variants[f"field_planner_plan_grid_batch_B{B}_one_field"] = lambda B=B: fp.plan_grid_batch(goal1, shared, starts[:B], out=plans[B])
        variants[f"rrt_plan_grid_batch_B{B}"] = lambda B=B: rrt.plan_grid_batch(goalN[:B], shared, starts[:B], seeds=np.arange(B), S_max=64)
    ms = rounds_of(variants, a.reps, a.rounds)
    torch.cuda.synchronize()
    found = {"field_planner": int((plans[N]["status"] == 0).sum()), "rrt": int((rrt.plan_grid_batch(goalN, shared, starts, seeds=np.arange(N), S_max=64)["status"] == 0).sum())}
    big_field = obig["field"].view(torch.int32)
    out = {"what": "ms per call, device events around `reps` back-to-back calls, median / min / max over alternating rounds, one process",
           "device": torch.cuda.get_device_name(0), "reps_per_round": a.reps, "rounds": a.rounds,
           "scene": {"grid": [W, H], "cell": list(cell), "goal": goal.tolist(), "robots": N, "rrt": {"n": 400, "r_rewire": 30, "max_cells": 1 << 13}},
           "big_map": {"grid": [big.W, big.H], "largest_finite_field": int(big_field[big_field != -1].max())},
           "largest_finite_field_scene": int(o1["field"].view(torch.int32)[o1["field"].view(torch.int32) != -1].max()),
           "found_of_robots": found, "ms_per_call": ms,
           "rrt_over_field_planner": {f"B{B}": ms[f"rrt_plan_grid_batch_B{B}"]["median"] / ms[f"field_planner_plan_grid_batch_B{B}_one_field"]["median"]
                                      for B in (1, 1024, N)}}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
