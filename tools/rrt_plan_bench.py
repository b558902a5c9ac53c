"""Timing of the on-device RRT* planner (lipmpc_rrt_plan_batch) -> profiles/rrt_plan.json.  Run on the GPU box from the
repository root:

    python tools/rrt_plan_bench.py                                   # wall time per call, oracle seconds per plan
    rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/rrt_<case> -- \\
        python tools/rrt_plan_bench.py --case <case> --reps 5 --no-json   # one run per case
    python tools/rrt_plan_bench.py --merge-stats /tmp/rrt_              # kernel times of the traced runs into the JSON

Cases: the SimulationMaze1 map with distinct seeds 0..B-1 at B = 1, 64 and 1024, and a mixed batch of B = 1024 (the
three RRT scenes and Simulation1Circles, seeds 0..255 each), all at the default parameters (250 cells, n = 1500,
r_rewire = 80).  Wall time: median over --reps calls of the stream-synchronised call (inputs already on the device).
Kernel times: per call, grid + distance transform = rrt_setup + rrt_grid + rrt_edt_col + rrt_edt_row, tree = rrt_star.
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

OUT = os.path.join(ROOT, "profiles", "rrt_plan.json")
CASES = {"maze1_B1": ("maze1", 1), "maze1_B64": ("maze1", 64), "maze1_B1024": ("maze1", 1024), "mixed_B1024": ("mixed", 1024)}
SCENES = ("SimulationRRT", "SimulationMaze1", "SimulationMaze2", "Simulation1Circles")


def scene(name):
    sc = np.load(os.path.join(ROOT, "tests", "golden", "pdf_scenarios.npz"))
    rings = [sc[name + "/rings"][j][: sc[name + "/nv"][j]] for j in range(len(sc[name + "/nv"]))]
    return rings, np.asarray(sc[name + "/goal"], float)


def batch(kind, B):
    if kind == "maze1":
        rings, goal = scene("SimulationMaze1")
        return [rings] * B, np.tile(goal, (B, 1)), np.arange(B)
    sets, goals, seeds = [], [], []
    for i in range(B):
        rings, goal = scene(SCENES[i % len(SCENES)])
        sets.append(rings)
        goals.append(goal)
        seeds.append(i // len(SCENES))
    return sets, np.array(goals), np.array(seeds)


def time_case(name, reps):
    import torch
    import lipmpc
    kind, B = CASES[name]
    sets, goals, seeds = batch(kind, B)
    xy, nv = lipmpc.pack_rings(sets, 9, 24)
    pl = lipmpc.RrtStarPlanner()
    dev = pl.device
    g, x, n = (torch.as_tensor(a, device=dev) for a in (goals, xy, nv))
    for _ in range(2):
        out = pl.plan_batch(g, x, n, seeds=seeds, S_max=64)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = pl.plan_batch(g, x, n, seeds=seeds, S_max=64)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    st = out["status"].cpu().numpy()
    return dict(B=B, map=kind, ms_per_call=float(np.median(ts)), ms_min=float(np.min(ts)), reps=reps,
                found=int(np.sum(st == 0)), plans_per_s=float(B / (np.median(ts) * 1e-3)))


def oracle_seconds():
    import rrt_oracle as R
    res = {}
    for name in ("SimulationRRT", "SimulationMaze1", "SimulationMaze2"):
        rings, goal = scene(name)
        t0 = time.perf_counter()
        for s in range(2):
            R.plan(rings, goal, seed=s)
        res[name] = (time.perf_counter() - t0) / 2
    return res


def merge_stats(prefix):
    with open(OUT) as f:
        data = json.load(f)
    for name in CASES:
        files = glob.glob(os.path.join(prefix + name, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            continue
        per = {}
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                k = row["Name"]
                for short in ("rrt_setup_kernel", "rrt_grid_kernel", "rrt_edt_col_kernel", "rrt_edt_row_kernel", "rrt_star_kernel"):
                    if short in k:
                        per[short] = float(row["TotalDurationNs"]) / int(row["Calls"]) * 1e-6
        grid = sum(per.get(k, 0.0) for k in ("rrt_setup_kernel", "rrt_grid_kernel", "rrt_edt_col_kernel", "rrt_edt_row_kernel"))
        data["cases"][name]["kernel_ms"] = dict(per, grid_and_edt=grid, tree=per.get("rrt_star_kernel", 0.0))
    with open(OUT, "w") as f:
        json.dump(data, f, indent=1)
    print(json.dumps(data, indent=1))


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES), default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-json", action="store_true")
    ap.add_argument("--merge-stats", default=None, help="prefix of the per-case rocprofv3 output directories")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    OUT = a.out
    if a.merge_stats:
        merge_stats(a.merge_stats)
        return
    names = [a.case] if a.case else list(CASES)
    cases = {n: time_case(n, a.reps) for n in names}
    for n, c in cases.items():
        print(n, c, flush=True)
    if a.no_json:
        return
    import torch
    data = dict(device=torch.cuda.get_device_name(0), params=dict(width=250, n=1500, r_rewire=80), cases=cases,
                oracle_s_per_plan=oracle_seconds())
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(data, f, indent=1)
    print(json.dumps(data, indent=1))


if __name__ == "__main__":
    main()
