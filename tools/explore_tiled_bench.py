"""Time the tiled explorers (TiledInformedFrontierPlanner, TiledCoordinatedFrontierPlanner: lipmpc_grid_frontier_gain_tiled_batch,
lipmpc_grid_frontier_utility_field_tiled_batch, lipmpc_grid_frontier_utility_path_tiled_batch,
lipmpc_grid_frontier_assign_tiled_batch) beside the one-workgroup classes of the same build -> profiles/explore_tiled.json.  Needs
the GPU; run from the repository root:

    python tools/explore_tiled_bench.py [--parent-lib path/to/the/parent/commit's/liblipmpc.so]

The method of tools/field_tiled_bench.py: one process, every variant warmed up, then device events around `reps` back-to-back calls,
the variants alternating in rounds; median / min / max over the rounds, in ms per call; every step under a watchdog of its own.  A
tiled variant is timed with a FIXED budget -- the rounds the map needed, counted first, plus one -- so nothing in a timed region
synchronises with the host.
  - the informed plan (field + gain + utility field + path, B = 64), one workgroup against tiled, at 92 x 80, 200 x 199, 362 x 362;
  - the gain call alone, one workgroup against tiled, on the 362 x 362 lattice maps of tools/gain_bench.py (720 / 2420 / 9680
    frontier cells);
  - the coordinated plan (field + path + claims), one workgroup against tiled, on the recorded 64 x 56 map (r_claim 15, up to 64
    claims, B = 64) and at 362 x 362 with 4 claims;
  - tiled alone at 1024^2 and 2048^2: both plans on a lattice map;
  - --parent-lib: the existing field + path and informed plans at the three small sizes with that library, in a child process of
    the same run just before this build's: the existing kernels must run at their former time within the round spread.
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
import field_shape_cases as S  # noqa: E402
from assign_bench import first_map  # noqa: E402
from field_bench import fleet_scene  # noqa: E402
from field_tiled_bench import LIMIT, limited, rounds_of  # noqa: E402
from gain_bench import lattice_map, starts_on  # noqa: E402

B = 64
R_VIEW, W_GAIN, G_CAP, MIN_GAIN = 10, 16, 120, 0
R_CLAIM = 15
NEW_CALLS = ("lipmpc_grid_frontier_gain_tiled_lds_bytes", "lipmpc_grid_frontier_gain_tiled_batch", "lipmpc_grid_frontier_utility_field_tiled_batch",
             "lipmpc_grid_frontier_utility_path_tiled_batch", "lipmpc_grid_frontier_assign_tiled_workspace_bytes",
             "lipmpc_grid_frontier_assign_tiled_batch")


def small_maps():
    """{name: dict(ev, origin, cell, start [B,2], kw)}: the three sizes both ways can run."""
    occ, origin, cell, _ = fleet_scene()
    ev = np.where(occ != 0, S.T_OCC, -S.T_FREE).astype(np.int32)
    ev[-2:, -2:] = 0
    maps = {"92x80": dict(ev=ev, origin=origin, cell=cell, r=2)}
    for W, H in ((200, 199), (362, 362)):
        c = S.strip_case(W, H)
        maps[f"{W}x{H}"] = dict(ev=c["ev"], origin=S.ORIGIN, cell=S.CELL, r=c["r"])
    for k, m in maps.items():
        m["start"] = starts_on(m["ev"], m["origin"], m["cell"], B, 7, S.T_FREE)
        m["kw"] = dict(r_inflate=m["r"], min_unknown=2, t_free=S.T_FREE, t_occ=S.T_OCC, max_seg=200)
    return maps


def budget_for(make, plan, settled_keys, lo=1):
    """The least fixed `rounds` with which ``plan(make(rounds))`` comes back settled under every key, counted one at a time."""
    r = lo
    while True:
        out = limited(plan, make(r))
        if all(int(out[k].min()) == 1 for k in settled_keys):
            return r
        r += 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "explore_tiled.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=float, default=120.0, help="seconds a single timed step may take")
    ap.add_argument("--largest", type=int, default=2048)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--existing-only", action="store_true", help="(the child of --parent-lib: the existing plans alone, JSON on the last line)")
    a = ap.parse_args()
    LIMIT[0] = a.limit
    parent = None
    if a.parent_lib:                                           # first, before this process opens the device
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--existing-only", "--reps", str(a.reps), "--rounds", str(a.rounds)],
                               env=dict(os.environ, LIPMPC_LIB=os.path.abspath(a.parent_lib)), capture_output=True, text=True, timeout=300)
        if child.returncode != 0:
            raise SystemExit(f"the parent library's run failed ({child.returncode}):\n{child.stderr[-2000:]}")
        parent = json.loads(child.stdout.strip().splitlines()[-1])
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: a timing taken elsewhere says nothing")
    if a.existing_only:
        for k in NEW_CALLS:                                    # a library of the parent commit has ABI 5 and none of these
            lipmpc._lib.SIGNATURES.pop(k)
    dev = torch.device("cuda", 0)
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=dev)
    tw, th, _ = lipmpc.tiled_info()
    variants, info, keep = {}, {}, []
    gain_args = (R_VIEW, W_GAIN, G_CAP, MIN_GAIN)

    def planner_call(pl, m, ev, start, **more):
        """plan() into buffers of the planner's own (made by the first call)."""
        box = [None]
        keep.append((pl, box))

        def call(pl=pl):
            box[0] = pl.plan(ev, start, origin=m["origin"], cell=m["cell"], out=box[0], **more)
            return box[0]
        return call

    # -- the three sizes both ways can run: the informed plan ---------------------------------------------------------------
    maps = small_maps()
    for name, m in maps.items():
        ev, start = t(m["ev"]), t(m["start"])
        W, H = m["ev"].shape
        variants[f"{name}_nearest_plan_one_workgroup"] = planner_call(lipmpc.FrontierPlanner(**m["kw"]), m, ev, start)
        variants[f"{name}_informed_plan_one_workgroup"] = planner_call(lipmpc.InformedFrontierPlanner(*gain_args, **m["kw"]), m, ev, start)
        if a.existing_only:
            continue
        make = lambda r, m=m: lipmpc.TiledInformedFrontierPlanner(*gain_args, rounds=r, **m["kw"])
        need = budget_for(make, lambda pl, m=m, ev=ev, start=start: pl.plan(ev, start, origin=m["origin"], cell=m["cell"]), ("settled", "usettled"))
        info[f"{name}_informed"] = dict(rounds=need, tiles=-(-W // tw) * -(-H // th))
        variants[f"{name}_informed_plan_tiled"] = planner_call(make(need + 1), m, ev, start)
    if a.existing_only:
        ms = rounds_of(variants, a.reps, a.rounds)
        print(json.dumps(ms))
        return

    # -- the gain alone on the lattice maps ---------------------------------------------------------------------------------------
    big_kw = dict(r_inflate=0, min_unknown=1, t_free=1, t_occ=3)
    place = dict(origin=(0.0, 0.0), cell=(0.1, 0.1))
    old, new = lipmpc.InformedFrontierPlanner(*gain_args, **big_kw), lipmpc.TiledInformedFrontierPlanner(*gain_args, **big_kw)
    for step in (64, 32, 16):
        e = t(lattice_map(step))[None]
        o = old.gain(e[0])                                     # the frontier both gain calls read
        g_new = torch.empty_like(o["gain"])
        info[f"lattice{step}_gain"] = dict(n_frontier=int(o["n_frontier"][0]))
        variants[f"lattice{step}_gain_alone_one_workgroup"] = lambda e=e, o=o: old._gain(e, 1, 3, o)
        variants[f"lattice{step}_gain_alone_tiled"] = lambda e=e, o=o, g=g_new: new._gain(e, 1, 3, dict(frontier=o["frontier"], gain=g))
        keep.append((o, g_new, e))

    # -- the claims ---------------------------------------------------------------------------------------------------------------
    ev0, origin0, cell0, scene_starts, cfg = first_map()
    starts0 = starts_on(ev0, origin0, cell0, B, 1, cfg["w_miss"])
    starts0[:len(scene_starts)] = scene_starts
    kw0 = dict(r_inflate=cfg["r_inflate"], min_unknown=cfg["min_unknown"], t_free=cfg["w_miss"], t_occ=cfg["w_hit"])
    lat = lattice_map(64)
    claim_cases = {"64x56_claims64": (dict(origin=origin0, cell=cell0), t(ev0), t(starts0), 64, kw0),
                   "362x362_claims4": (place, t(lat), t(starts_on(lat, (0.0, 0.0), (0.1, 0.1), B, 2, 1)), 4, big_kw)}
    for name, (m, ev, start, claims, kw) in claim_cases.items():
        W, H = ev.shape
        variants[f"{name}_coordinated_plan_one_workgroup"] = planner_call(lipmpc.CoordinatedFrontierPlanner(R_CLAIM, claims, **kw), m, ev, start)
        make = lambda r, claims=claims, kw=kw: lipmpc.TiledCoordinatedFrontierPlanner(R_CLAIM, claims, rounds=r, **kw)
        need = budget_for(make, lambda pl, m=m, ev=ev, start=start: pl.plan(ev, start, origin=m["origin"], cell=m["cell"]),
                          ("settled", "claims_settled"))
        call = planner_call(make(need + 1), m, ev, start)
        variants[f"{name}_coordinated_plan_tiled"] = call
        info[f"{name}"] = dict(rounds=need, tiles=-(-W // tw) * -(-H // th), launches=claims * (need + 1 + 4) + 3, n_claims=int(limited(call)["n_claims"][0]))

    # -- large maps: tiled alone ----------------------------------------------------------------------------------------------------
    for n in (1024, 2048):
        if n > a.largest:
            continue
        lat_n = lattice_map(64, n)
        ev, start = t(lat_n), t(starts_on(lat_n, (0.0, 0.0), (0.1, 0.1), B, 3, 1))
        make = lambda r: lipmpc.TiledInformedFrontierPlanner(*gain_args, rounds=r, **big_kw)
        plan = lambda pl, ev=ev, start=start: pl.plan(ev, start, **place)
        need = budget_for(make, plan, ("settled", "usettled"))
        info[f"{n}x{n}_informed"] = dict(rounds=need, tiles=-(-n // tw) * -(-n // th), n_frontier=int(limited(plan, make(need))["n_frontier"][0]))
        variants[f"{n}x{n}_informed_plan_tiled"] = planner_call(make(need + 1), place, ev, start)
        make = lambda r: lipmpc.TiledCoordinatedFrontierPlanner(R_CLAIM, 4, rounds=r, **big_kw)
        need = budget_for(make, plan, ("settled", "claims_settled"))
        info[f"{n}x{n}_claims4"] = dict(rounds=need, launches=4 * (need + 1 + 4) + 3)
        variants[f"{n}x{n}_coordinated_plan_tiled"] = planner_call(make(need + 1), place, ev, start)

    ms = rounds_of(variants, a.reps, a.rounds)
    for pl, box in [k for k in keep if len(k) == 2]:
        for key in ("settled", "usettled", "claims_settled"):
            if isinstance(box[0], dict) and key in box[0]:
                assert int(box[0][key].min()) == 1, f"a timed budget did not settle ({key})"
    out = {"what": "ms per call, device events around `reps` back-to-back calls (1 where a call takes more than 50 ms), median / min / max "
                   "over alternating rounds, one process; tiled plans with a fixed budget of `rounds` + 1 rounds, no host synchronisation",
           "device": torch.cuda.get_device_name(0), "reps_per_round": a.reps, "rounds": a.rounds, "tile": [tw, th], "robots": B,
           "r_view": R_VIEW, "w_gain": W_GAIN, "g_cap": G_CAP, "min_gain": MIN_GAIN, "r_claim": R_CLAIM, "maps": info, "ms_per_call": ms,
           "parent_library_ms_per_call": parent,
           "parent_note": "the parent commit's library, timed in a child process of the same run just before this build's; the two run the same "
                          "one-workgroup kernels" if parent else "not measured in this run"}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
