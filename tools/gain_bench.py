"""Time the informed explorer (InformedFrontierPlanner: lipmpc_grid_frontier_gain_batch, lipmpc_grid_frontier_utility_field_batch,
lipmpc_grid_frontier_utility_path_batch) beside the nearest-frontier plan alone (FrontierPlanner.plan) -> profiles/frontier_gain.json.
Needs the GPU; run from the repository root:

    python tools/gain_bench.py [--parent-lib path/to/the/parent/commit's/liblipmpc.so]

One process, every variant warmed up, then device events around `reps` back-to-back calls, the variants alternating in rounds;
median / min / max over the rounds, in ms per call.
  - the recorded scene's first 64 x 56 map (tools/assign_bench.py's: the open field after the noise-free first scan of four
    side-by-side robots) at B = 3, 64 and 1024 and r_view 10 and 30: the gain call alone, field + path (FrontierPlanner.plan), and
    field + gain + utility field + path (InformedFrontierPlanner.plan);
  - a 362 x 362 map, near the cell cap, known free but for a lattice of 4 x 4 unknown blocks every 64, 32 and 16 cells -- hundreds
    to thousands of frontier cells -- at r_view 10 and B = 64: the gain alone and both plans, for the scaling with the frontier.
--parent-lib: the same field + path variants are timed first in a fresh child process that loads that library (LIPMPC_LIB), so that
both builds' figures come from one visit to the device; they run the same kernels, so they must agree within the round spread.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import lipmpc  # noqa: E402
from assign_bench import first_map  # noqa: E402
from field_bench import rounds_of  # noqa: E402

ROBOTS = (3, 64, 1024)
R_VIEWS = (10, 30)
W_GAIN, G_CAP, MIN_GAIN = 16, 120, 0
BIG, LATTICES = 362, (64, 32, 16)
NEW_CALLS = ("lipmpc_grid_frontier_gain_batch", "lipmpc_grid_frontier_utility_field_batch", "lipmpc_grid_frontier_utility_path_batch")


def lattice_map(step, n=BIG):
    ev = np.full((n, n), -1, np.int32)
    for i in range(step // 2, n - 4, step):
        for j in range(step // 2, n - 4, step):
            ev[i:i + 4, j:j + 4] = 0
    return ev


def starts_on(ev, origin, cell, n, seed, t_free):
    rng = np.random.default_rng(seed)
    ij = np.argwhere(ev <= -t_free)
    ij = ij[rng.integers(len(ij), size=n)]
    return np.stack([origin[0] + (ij[:, 0] + rng.uniform(0.05, 0.95, n)) * cell[0], origin[1] + (ij[:, 1] + rng.uniform(0.05, 0.95, n)) * cell[1]], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frontier_gain.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--nearest-only", action="store_true", help="(the child of --parent-lib: field + path alone, JSON on the last line)")
    a = ap.parse_args()
    parent = None
    if a.parent_lib:                                           # first, before this process opens the device
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--nearest-only", "--reps", str(a.reps), "--rounds", str(a.rounds)],
                               env=dict(os.environ, LIPMPC_LIB=os.path.abspath(a.parent_lib)), capture_output=True, text=True, timeout=300)
        if child.returncode != 0:
            raise SystemExit(f"the parent library's run failed ({child.returncode}):\n{child.stderr[-2000:]}")
        parent = json.loads(child.stdout.strip().splitlines()[-1])
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: a timing taken elsewhere says nothing")
    if a.nearest_only:
        for k in NEW_CALLS:                                    # a library of the parent commit has ABI 5 and none of these
            lipmpc._lib.SIGNATURES.pop(k)
    dev = torch.device("cuda", 0)
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=dev)
    buf = lambda table: {k: torch.zeros(shape, dtype=dt, device=dev) if dt != torch.uint32 else torch.empty(shape, dtype=dt, device=dev)
                         for k, (dt, shape, _) in table.items()}
    ev, origin, cell, scene_starts, cfg = first_map()
    W, H = ev.shape
    starts = starts_on(ev, origin, cell, max(ROBOTS), 1, cfg["w_miss"])
    starts[:len(scene_starts)] = scene_starts
    starts, d_ev = t(starts), t(ev)
    kw = dict(r_inflate=cfg["r_inflate"], min_unknown=cfg["min_unknown"], t_free=cfg["w_miss"], t_occ=cfg["w_hit"])
    near = lipmpc.FrontierPlanner(**kw)
    out_near = {B: buf(lipmpc.planner.frontier_outputs(B, 1, W, H, 64)) for B in ROBOTS}
    variants = {f"field_plus_path_B{B}": (lambda B=B: near.plan(d_ev, starts[:B], origin=origin, cell=cell, out=out_near[B])) for B in ROBOTS}
    if a.nearest_only:
        ms = rounds_of(variants, a.reps, a.rounds)
        torch.cuda.synchronize()
        print(json.dumps(ms))
        return
    informed = {r: lipmpc.InformedFrontierPlanner(r, W_GAIN, G_CAP, MIN_GAIN, **kw) for r in R_VIEWS}
    out_inf = {(r, B): buf(lipmpc.planner.informed_outputs(B, 1, W, H, 64)) for r in R_VIEWS for B in ROBOTS}
    ev3 = d_ev[None]
    for r in R_VIEWS:
        near._field(ev3, cfg["w_miss"], cfg["w_hit"], out_inf[(r, 3)])           # the frontier that the gain call alone reads
        variants[f"gain_alone_r{r}"] = lambda r=r: informed[r]._gain(ev3, cfg["w_miss"], cfg["w_hit"], out_inf[(r, 3)])
        for B in ROBOTS:
            variants[f"field_gain_ufield_path_r{r}_B{B}"] = lambda r=r, B=B: informed[r].plan(d_ev, starts[:B], origin=origin, cell=cell,
                                                                                             out=out_inf[(r, B)])
    # near the cell cap: the scaling with the number of frontier cells
    big_kw = dict(r_inflate=0, min_unknown=1, t_free=1, t_occ=3)
    big_near, big_inf = lipmpc.FrontierPlanner(**big_kw), lipmpc.InformedFrontierPlanner(10, W_GAIN, G_CAP, MIN_GAIN, **big_kw)
    big = {}
    for step in LATTICES:
        e = t(lattice_map(step))
        s = t(starts_on(lattice_map(step), (0.0, 0.0), (0.1, 0.1), 64, 2, 1))
        o_n, o_i = buf(lipmpc.planner.frontier_outputs(64, 1, BIG, BIG, 64)), buf(lipmpc.planner.informed_outputs(64, 1, BIG, BIG, 64))
        big[step] = (e, s, o_n, o_i)
        variants[f"big_lattice{step}_field_plus_path"] = lambda x=big[step]: big_near.plan(x[0], x[1], origin=(0.0, 0.0), cell=(0.1, 0.1), out=x[2])
        variants[f"big_lattice{step}_gain_alone"] = lambda x=big[step]: big_inf._gain(x[0][None], 1, 3, x[3])
        variants[f"big_lattice{step}_field_gain_ufield_path"] = lambda x=big[step]: big_inf.plan(x[0], x[1], origin=(0.0, 0.0), cell=(0.1, 0.1), out=x[3])
        big_inf.plan(e, s, origin=(0.0, 0.0), cell=(0.1, 0.1), out=o_i)          # (the frontier that the gain call alone reads)
    ms = rounds_of(variants, a.reps, a.rounds)
    torch.cuda.synchronize()
    out = {"what": "ms per call, device events around `reps` back-to-back calls, median / min / max over alternating rounds, one process",
           "device": torch.cuda.get_device_name(0), "reps_per_round": a.reps, "rounds": a.rounds,
           "scene": {"grid": [W, H], "cell": list(cell), "first_scan_from": [list(map(float, p)) for p in scene_starts],
                     "known_free_cells": int((ev <= -cfg["w_miss"]).sum()), "n_frontier": int(out_near[max(ROBOTS)]["n_frontier"][0]), **cfg},
           "w_gain": W_GAIN, "g_cap": G_CAP, "min_gain": MIN_GAIN,
           "scene_gain_min_max": {f"r{r}": [int(g[g > 0].min()), int(g.max())] for r in R_VIEWS for g in [out_inf[(r, 3)]["gain"]]},
           "big_map": {"grid": [BIG, BIG], "r_view": 10, "B": 64,
                       "n_frontier": {f"lattice{step}": int(big[step][3]["n_frontier"][0]) for step in LATTICES}},
           "ms_per_call": ms,
           "parent_library_field_plus_path_ms_per_call": parent,
           "parent_note": "the parent commit's library, timed in a child process of the same run just before this build's; the two run the same "
                          "field and path kernels" if parent else "not measured in this run"}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
