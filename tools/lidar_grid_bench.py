"""Time the grid scan (lipmpc_lidar_grid_c_eta_batch: scan + clusters + hulls + (c, eta), one launch) for 4096 robots beside the
polygon scan of the same robots in the same process, on two maps:
  fixture  the cell-aligned boxes of tests/grid_lidar_oracle.py (grid and rings are the same set)
  config5  the map of bench.py's config-5 line (20 obstacles, synth seed 9), rasterised at 0.05 m (a cell is solid if its centre
           lies in an obstacle)
Rounds of (polygon in index order, polygon ranked, grid) alternate; per variant the median round and the spread are written with
the window size and the code-object figures to --out (default profiles/lidar_grid.json).  Needs the GPU.
Where the grid kernel's time goes: run it again with LIPMPC_LIB = a -DLIPMPC_LIDAR_PHASES build of the library and
LIPMPC_LIDAR_STOP=6 (the kernel ends when the window is staged) and =1 (when the rays are marched) into two other files, then
--merge-phases STAGED.json RAYS.json adds `phases_us` to --out, and --merge-trace RESULTS.db the per-dispatch times of the two
sense kernels from the database of a `rocprofv3 --kernel-trace --stats` run of this tool (no GPU needed for these steps)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import lipmpc  # noqa: E402
import grid_lidar_oracle as G  # noqa: E402


def events_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def rasterise(rings, origin, cell, W, H):
    """Cell solid if its centre lies in (or on) one of the convex CCW / CW rings."""
    cx = origin[0] + (np.arange(W) + 0.5) * cell
    cy = origin[1] + (np.arange(H) + 0.5) * cell
    X, Y = np.meshgrid(cx, cy, indexing="ij")
    occ = np.zeros((W, H), bool)
    for r in rings:
        a, b = r, np.roll(r, -1, axis=0)
        cr = [(b[k, 0] - a[k, 0]) * (Y - a[k, 1]) - (b[k, 1] - a[k, 1]) * (X - a[k, 0]) for k in range(len(r))]
        occ |= np.all([c >= 0 for c in cr], axis=0) | np.all([c <= 0 for c in cr], axis=0)
    return occ.astype(np.uint8)


def measure(name, grid_args, rings, pos, lidar_range, reps, rounds, dev):
    B = len(pos)
    occ, origin, cell = grid_args
    gs = lipmpc.LidarSensor.from_grid(lipmpc.GridMap(occ, origin, cell), lidar_range=lidar_range, n_obs_max=12, v_max=32)
    ps = lipmpc.LidarSensor(rings, lidar_range=lidar_range, n_obs_max=12, v_max=32)
    st = np.zeros((B, 5)); st[:, 0] = pos[:, 0]; st[:, 2] = pos[:, 1]
    state = torch.as_tensor(st, device=dev)
    noise = 0.01 * torch.randn((B, 360, 2), dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    sg, sp = gs.alloc_outputs(B, rings=False, c_eta=True), ps.alloc_outputs(B, rings=False, c_eta=True)
    sched = ps.make_schedule(B)
    variants = {"polygon_index_order": lambda: ps.sense(state, noise, out=sp, schedule=None),
                "polygon_ranked": lambda: ps.sense(state, noise, out=sp, schedule=sched),
                "grid": lambda: gs.sense(state, noise, out=sg)}
    for fn in variants.values():                              # warm up every shape
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            ms[k].append(events_ms(fn, reps))
    variants["grid"](); variants["polygon_index_order"](); torch.cuda.synchronize()
    nx, ny = G.window_half(lidar_range, cell)
    res = {"map": name, "robots": B, "grid_cells": [int(occ.shape[0]), int(occ.shape[1])], "cell": list(cell), "lidar_range": lidar_range,
           "solid_cells": int(np.asarray(occ).sum()), "window_cells": [2 * nx + 1, 2 * ny + 1], "window_bitmap_bytes": ((2 * nx + 1) * (2 * ny + 1) + 7) // 8,
           "reps_per_round": reps, "rounds": rounds,
           "ms_per_call": {k: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))} for k, v in ms.items()},
           "grid": {"mean_inferred": float(sg["n_inferred"].double().mean()), "robots_in_solid_cells_or_overflow": int(sg["overflow"].sum())},
           "polygon": {"mean_inferred": float(sp["n_inferred"].double().mean()), "overflow": int(sp["overflow"].sum())}}
    res["grid_over_polygon_index_order"] = res["ms_per_call"]["grid"]["median"] / res["ms_per_call"]["polygon_index_order"]["median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lidar_grid.json"))
    ap.add_argument("--robots", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--merge-phases", nargs=2, metavar=("STAGED.json", "RAYS.json"))
    ap.add_argument("--merge-trace", metavar="RESULTS.db")
    a = ap.parse_args()
    if a.merge_trace:
        import sqlite3
        out = json.load(open(a.out))
        cur = sqlite3.connect(a.merge_trace).cursor()
        out["kernel_trace_us"] = {"what": "per dispatch of 4096 robots, both maps, rocprofv3 --kernel-trace (a run of its own)"}
        for tag, name in (("grid", "%lidar_grid_scan_kernel%"), ("polygon", "%lidar_sense_kernel%")):
            n, mean, lo, hi = cur.execute("select count(*), avg(end - start), min(end - start), max(end - start) from kernels where name like ?", (name,)).fetchone()
            out["kernel_trace_us"][tag] = {"dispatches": n, "mean": mean / 1e3, "min": lo / 1e3, "max": hi / 1e3}
        json.dump(out, open(a.out, "w"), indent=1)
        if not a.merge_phases:
            return
    if a.merge_phases:
        out = json.load(open(a.out))
        staged, rays = (json.load(open(f)) for f in a.merge_phases)
        for m, m6, m1 in zip(out["maps"], staged["maps"], rays["maps"]):
            us = lambda mm, k: 1e3 * mm["ms_per_call"][k]["median"]
            m["phases_us"] = {"what": "median us per call of the kernel stopped after a phase (profiling build), launch included",
                              "grid": {"window_staged": us(m6, "grid"), "rays_marched": us(m1, "grid"), "whole_scan": us(m, "grid")},
                              "polygon_index_order": {"candidates_found": us(m6, "polygon_index_order"), "rays_cast": us(m1, "polygon_index_order"),
                                                      "whole_scan": us(m, "polygon_index_order")}}
        json.dump(out, open(a.out, "w"), indent=1)
        return
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda", 0)
    from importlib import import_module
    synth = import_module("humanoid-navigation-using-mpc-ldcbf_amd.synth")
    from code_object import kernel_resources
    out = {"what": "scan + clusters + hulls + (c, eta) in one launch, ms per call of `robots` robots, device events around `reps` back-to-back "
                   "calls, median / min / max over alternating rounds; 360 rays, range 1.5, noise given",
           "device": torch.cuda.get_device_name(0), "maps": []}
    fx = G.fixture(n_robots=a.robots)
    out["maps"].append(measure("fixture (cell-aligned boxes)", (fx["occ"], fx["origin"], fx["cell"]), fx["rings"], fx["pos"], 1.5, a.reps, a.rounds, dev))
    exy, env = synth.synthetic_fields(1, 20, -1.0, 6.0, (-5.0, -5.0), (50.0, 50.0), seed=9, delta=0.6)
    rings = [exy[0, j, : env[0, j]] for j in range(20) if env[0, j] > 0]
    gen = torch.Generator(device=dev).manual_seed(3)
    pos = (torch.rand((a.robots, 2), dtype=torch.float64, device=dev, generator=gen) * 7.0 - 1.0).cpu().numpy()       # bench.py's robots
    lo = np.floor(min(r.min() for r in rings) - 1.0); hi = np.ceil(max(r.max() for r in rings) + 1.0)
    n = int(round((hi - lo) / 0.05))
    occ = rasterise(rings, (lo, lo), 0.05, n, n)
    out["maps"].append(measure("config5 (bench.py's map, rasterised at 0.05)", (occ, (float(lo), float(lo)), (0.05, 0.05)), rings, pos, 1.5, a.reps, a.rounds, dev))
    res = kernel_resources(lipmpc._lib.LIB_PATH)
    for tag, key in (("grid", "lidar_grid_scan_kernel"), ("polygon", "lidar_sense_kernel")):
        r = next(v for k, v in res.items() if key in k)
        lds = r["group_segment_fixed_size"]
        out["kernel_" + tag] = {"vgpr": r["vgpr_count"], "sgpr": r["sgpr_count"], "scratch_bytes": r["private_segment_fixed_size"], "lds_bytes": lds,
                                "waves_per_cu": min(16, (160 * 1024) // lds), "waves_per_simd_by_registers": 4}
    out["not_measured"] = ["hardware counters of the grid kernel", "grids with a range / cell pair other than 1.5 / 0.05", "per-robot grids"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out["maps"], indent=1))


if __name__ == "__main__":
    main()
