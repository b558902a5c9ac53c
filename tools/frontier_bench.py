"""Time the frontier explorer (FrontierPlanner.field + .plan: lipmpc_grid_frontier_field_batch, lipmpc_grid_frontier_path_batch)
-> profiles/frontier.json.  Needs the GPU; run from the repository root:

    python tools/frontier_bench.py [--parent-lib variants/parent/liblipmpc.so]

One process, every variant warmed up, then device events around `reps` back-to-back calls, the variants alternating in rounds;
median / min / max over the rounds, in ms per call.  The map is 92 x 80 cells of 0.05 m: the U-shaped wall of
tests/golden/mapped_replanning.npz seen from three places through tests/map_oracle.py (a partly known map, as a fleet has it
after its first samples); the starts are random known-free cells.
  - field + plan on ONE shared map at B = 1, 4096 and 32768;
  - field + plan on one map PER ROBOT (the same map 64 times) at B = 64.
``--parent-lib``: a liblipmpc.so built from the PARENT commit (git worktree of HEAD~1, make -C <package>/csrc).  Its
lipmpc_grid_field_batch + lipmpc_grid_path_batch are timed in the same rounds on the same map thresholded (solid = evidence >=
w_hit, everything else free) toward a far-corner goal: what a planned walk to a GIVEN goal cost before this planner existed.
Without the option those entries are left out.
"""
import argparse
import ctypes as C
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
import lidar_oracle as L  # noqa: E402
import map_oracle as M  # noqa: E402
from field_bench import fleet_scene, rounds_of  # noqa: E402

SCAN_AT = ((1.6, 2.72), (2.6, 1.0), (4.3, 3.2))
LIDAR_RANGE, W_HIT, W_MISS = 1.5, 3, 1
SHARED_B, PER_ROBOT_B = (1, 4096, 32768), 64


def scanned_map():
    occ, origin, cell, _ = fleet_scene()
    table = L.ray_table(360)
    pos = np.array(SCAN_AT)
    hits = M.oracle_hits(pos, occ, origin, cell, LIDAR_RANGE, table)
    ev = M.update(np.zeros(occ.shape, np.int64), pos, hits, origin, cell, LIDAR_RANGE, table, w_hit=W_HIT, w_miss=W_MISS)
    return ev.astype(np.int32), origin, cell


def parent_calls(path, dev, occ, origin, cell, goal, starts, bufs):
    """{B: a call of the parent library's field + paths} through raw ctypes (this process's binding belongs to the current build)."""
    lib = C.CDLL(path)
    i32, i64, ptr = C.c_int32, C.c_int64, C.c_void_p
    lib.lipmpc_grid_field_batch.argtypes = [C.c_int, i64, i32, i32, i32, ptr, ptr, ptr, ptr, i32, ptr, ptr, ptr]
    lib.lipmpc_grid_path_batch.argtypes = [C.c_int, i64, i64, i32, i32, ptr, ptr, ptr, i32, ptr, ptr, ptr, ptr, i32, i32, i32, ptr, ptr, ptr, ptr, ptr]
    org_c, cell_c = (C.c_double * 2)(*origin), (C.c_double * 2)(*cell)
    W, H = occ.shape

    def call(B):
        o, s = bufs[B], torch.cuda.current_stream(dev).cuda_stream
        rc = lib.lipmpc_grid_field_batch(0, 1, W, H, 1, C.addressof(org_c), C.addressof(cell_c), occ.data_ptr(), goal.data_ptr(), 0,
                                         o["field"].data_ptr(), o["field_status"].data_ptr(), s)
        rc |= lib.lipmpc_grid_path_batch(0, B, 1, W, H, C.addressof(org_c), C.addressof(cell_c), occ.data_ptr(), 1, o["field"].data_ptr(),
                                         o["field_status"].data_ptr(), goal.data_ptr(), starts.data_ptr(), 0, 0x7FFFFFFF, 64,
                                         o["sub_goals"].data_ptr(), o["n_sub"].data_ptr(), o["status"].data_ptr(), o["path_cost"].data_ptr(), s)
        assert rc == 0
    call.keep = (org_c, cell_c, lib)
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frontier.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda", 0)
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=dev)
    ev, origin, cell = scanned_map()
    W, H = ev.shape
    rng = np.random.default_rng(1)
    ij = np.argwhere(ev <= -W_MISS)
    n_max = max(SHARED_B)
    ij = ij[rng.integers(len(ij), size=n_max)]
    starts = t(np.stack([origin[0] + (ij[:, 0] + rng.uniform(0.05, 0.95, n_max)) * cell[0],
                         origin[1] + (ij[:, 1] + rng.uniform(0.05, 0.95, n_max)) * cell[1]], 1))
    shared, own = t(ev), t(np.broadcast_to(ev, (PER_ROBOT_B, W, H)))
    fp = lipmpc.FrontierPlanner(t_free=W_MISS, t_occ=W_HIT)
    table = lipmpc.planner.frontier_outputs
    buf = lambda B, F: {k: torch.zeros(shape, dtype=dt, device=dev) if dt != torch.uint32 else torch.empty(shape, dtype=dt, device=dev)
                        for k, (dt, shape, _) in table(B, F, W, H, 64).items()}
    outs = {B: buf(B, 1) for B in SHARED_B}
    out_own = buf(PER_ROBOT_B, PER_ROBOT_B)

    def both(m, st, out):
        fp.field(m, out=out)                                   # (plan computes the field again: the issue's "field + plan")
        fp.plan(m, st, origin=origin, cell=cell, out=out)

    variants = {f"frontier_field_plus_plan_B{B}_shared_map": (lambda B=B: both(shared, starts[:B], outs[B])) for B in SHARED_B}
    variants[f"frontier_field_plus_plan_B{PER_ROBOT_B}_per_robot_maps"] = lambda: both(own, starts[:PER_ROBOT_B], out_own)
    if a.parent_lib:
        occ = t((ev >= W_HIT).astype(np.uint8))
        goal = t(np.array([[origin[0] + (W - 3.5) * cell[0], origin[1] + (H - 3.5) * cell[1]]]))
        ftable = lipmpc.planner.field_plan_outputs
        pbufs = {B: {k: torch.zeros(shape, dtype=dt, device=dev) if dt != torch.uint32 else torch.empty(shape, dtype=dt, device=dev)
                     for k, (dt, shape, _) in ftable(B, 1, W, H, 64).items()} for B in SHARED_B}
        pc = parent_calls(a.parent_lib, dev, occ, origin, cell, goal, starts, pbufs)
        for B in SHARED_B:
            variants[f"parent_grid_field_plus_path_B{B}_far_corner_goal"] = lambda B=B: pc(B)
    ms = rounds_of(variants, a.reps, a.rounds)
    torch.cuda.synchronize()
    top = outs[n_max]
    out = {"what": "ms per call, device events around `reps` back-to-back calls, median / min / max over alternating rounds, one process",
           "device": torch.cuda.get_device_name(0), "reps_per_round": a.reps, "rounds": a.rounds,
           "scene": {"grid": [W, H], "cell": list(cell), "scans_from": [list(p) for p in SCAN_AT], "known_free_cells": int((ev <= -W_MISS).sum()),
                     "solid_cells": int((ev >= W_HIT).sum()), "r_inflate": fp.r_inflate, "min_unknown": fp.min_unknown},
           "n_frontier": int(top["n_frontier"][0]), "found_of_robots": int((top["status"] == 0).sum()), "robots": n_max,
           "parent_library": bool(a.parent_lib), "ms_per_call": ms}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
