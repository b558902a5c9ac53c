"""Time the coordinated claim (CoordinatedFrontierPlanner.plan: lipmpc_grid_frontier_field_batch, lipmpc_grid_frontier_path_batch,
lipmpc_grid_frontier_assign_batch) beside the nearest-frontier plan alone (FrontierPlanner.plan: the first two calls)
-> profiles/frontier_assign.json.  Needs the GPU; run from the repository root:

    python tools/assign_bench.py

One process, every variant warmed up, then device events around `reps` back-to-back calls, the variants alternating in rounds;
median / min / max over the rounds, in ms per call.  The map is the first map of the recorded scene of
tests/golden/exploration_assigned.npz: the open field of tests/golden/make_exploration.py after the noise-free first scan of its four
side-by-side robots, through tests/map_oracle.py, at the scene's r_inflate and min_unknown.  The starts are those four robots'
and, beyond them, random known-free cells.
  - field + path (FrontierPlanner.plan) at B = 3, 64 and 1024;
  - field + path + assign (CoordinatedFrontierPlanner.plan, r_claim 15, max_claims 64) at the same B, with the rounds it ran.
The assign call is ONE workgroup and its rounds are sequential: the difference of the two is what a replan pays for the claims.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import lipmpc  # noqa: E402
import grid_lidar_oracle as G  # noqa: E402
import lidar_oracle as L  # noqa: E402
import map_oracle as M  # noqa: E402
from field_bench import rounds_of  # noqa: E402

ROBOTS = (3, 64, 1024)
R_CLAIM, MAX_CLAIMS = 15, 64


def first_map():
    """(evidence [W,H] int32, origin, cell, the scene's starts, its settings) after the noise-free first scan."""
    d = np.load(os.path.join(ROOT, "tests", "golden", "exploration_assigned.npz"))
    (W, H), origin, cell = d["grid"].tolist(), tuple(d["origin"].tolist()), tuple(d["cell"].tolist())
    occ = np.zeros((W, H), np.uint8)
    for i0, j0, i1, j1 in d["walls"]:
        occ[i0:i1, j0:j1] = 1
    table, rng = L.ray_table(360), float(d["lidar_range"])
    hits = np.full((len(d["starts"]), 360, 2), np.nan)
    for b, pos in enumerate(d["starts"]):
        h, valid = G.grid_hits(pos, occ, origin, cell, rng, table)
        hits[b][valid] = h[valid]
    w_hit, w_miss = (int(v) for v in d["weights"])
    ev = M.update(np.zeros((W, H), np.int64), d["starts"], hits, origin, cell, rng, table, w_hit=w_hit, w_miss=w_miss)
    return ev.astype(np.int32), origin, cell, d["starts"], dict(w_hit=w_hit, w_miss=w_miss, r_inflate=int(d["r_inflate"]), min_unknown=int(d["min_unknown"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frontier_assign.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda", 0)
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=dev)
    ev, origin, cell, scene_starts, cfg = first_map()
    W, H = ev.shape
    rng = np.random.default_rng(1)
    ij = np.argwhere(ev <= -cfg["w_miss"])
    n_max = max(ROBOTS)
    ij = ij[rng.integers(len(ij), size=n_max)]
    starts = np.stack([origin[0] + (ij[:, 0] + rng.uniform(0.05, 0.95, n_max)) * cell[0],
                       origin[1] + (ij[:, 1] + rng.uniform(0.05, 0.95, n_max)) * cell[1]], 1)
    starts[:len(scene_starts)] = scene_starts
    starts, d_ev = t(starts), t(ev)
    kw = dict(r_inflate=cfg["r_inflate"], min_unknown=cfg["min_unknown"], t_free=cfg["w_miss"], t_occ=cfg["w_hit"])
    near, coord = lipmpc.FrontierPlanner(**kw), lipmpc.CoordinatedFrontierPlanner(R_CLAIM, MAX_CLAIMS, **kw)
    buf = lambda table: {k: torch.zeros(shape, dtype=dt, device=dev) if dt != torch.uint32 else torch.empty(shape, dtype=dt, device=dev)
                         for k, (dt, shape, _) in table.items()}
    out_near = {B: buf(lipmpc.planner.frontier_outputs(B, 1, W, H, 64)) for B in ROBOTS}
    out_coord = {B: buf(lipmpc.planner.assign_outputs(B, W, H, 64)) for B in ROBOTS}
    variants = {}
    for B in ROBOTS:
        variants[f"field_plus_path_B{B}"] = lambda B=B: near.plan(d_ev, starts[:B], origin=origin, cell=cell, out=out_near[B])
        variants[f"field_plus_path_plus_assign_B{B}"] = lambda B=B: coord.plan(d_ev, starts[:B], origin=origin, cell=cell, out=out_coord[B])
    ms = rounds_of(variants, a.reps, a.rounds)
    torch.cuda.synchronize()
    out = {"what": "ms per call, device events around `reps` back-to-back calls, median / min / max over alternating rounds, one process",
           "device": torch.cuda.get_device_name(0), "reps_per_round": a.reps, "rounds": a.rounds,
           "scene": {"grid": [W, H], "cell": list(cell), "first_scan_from": [list(map(float, p)) for p in scene_starts],
                     "known_free_cells": int((ev <= -cfg["w_miss"]).sum()), "n_frontier": int(out_near[n_max]["n_frontier"][0]), **cfg},
           "r_claim": R_CLAIM, "max_claims": MAX_CLAIMS,
           "claim_rounds_run": {f"B{B}": int(out_coord[B]["n_claims"][0]) for B in ROBOTS},
           "robots_with_a_plan": {f"B{B}": int((out_near[B]["status"] == 0).sum()) for B in ROBOTS},
           "ms_per_call": ms}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
