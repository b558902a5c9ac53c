"""Time the claims from per-robot fields (RobotFieldsFrontierPlanner: tiled frontier field, path call,
lipmpc_grid_frontier_assign_robot_fields_batch) beside CoordinatedFrontierPlanner and TiledCoordinatedFrontierPlanner on the same
inputs -> profiles/frontier_robot_fields.json.  Needs the GPU; run from the repository root:

    python tools/robot_fields_bench.py [--parent-lib PATH] [--only NAME,...]

One process, every variant warmed up, then device events around `reps` back-to-back plans, the variants alternating in rounds;
median / min / max over 5 rounds, in ms per plan (tools/assign_bench.py's method and recorded map).
  - maps: the recorded 64 x 56 map at B = 4 (the scene's starts) and B = 64; an open 362 x 362 field at B = 4, 16 and 64; a 1024^2
    lattice map at B = 16 (tiled classes only: the one-workgroup class stops at 2^17 cells); max_claims = B everywhere;
  - every tiled plan runs with a FIXED budget: the rounds that very plan needed on that map (per class, plain and keeping apart),
    counted first by bisection, plus one.  The needs are recorded: a single-source field -- a robot's, or a keep slot's -- may need
    more rounds than the field of the whole frontier did;
  - with and without everyone keeping (previous targets = the planner's own last targets, r_keep 0, the most generous test);
  - the new call alone (lipmpc_grid_frontier_assign_robot_fields_batch on a settled frontier plan) and its launch count;
  - existing plans: with --parent-lib (the parent commit's library) the two existing classes are timed again in a freshly started
    child process that loads that library; the expectation is that the rounds overlap.  Without it the record says "not measured".
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
from gain_bench import lattice_map, starts_on  # noqa: E402

R_CLAIM = 15
ALL_KEEP = dict(r_keep=0, keep_ratio16=1024, keep_slack=4096)      # the target itself, at any cost: every attempt succeeds
NEW_CALLS = ("lipmpc_grid_frontier_assign_robot_fields_batch", "lipmpc_grid_frontier_assign_robot_fields_workspace_bytes")
ROUNDS = 5


def scenes():
    """name -> (evidence, origin, cell, starts, planner keywords, one workgroup possible, reps per round)."""
    from assign_checks import CELL, ORIGIN, T_FREE, T_OCC, centres, open_field
    ev, origin, cell, scene_starts, cfg = first_map()
    kw = dict(r_inflate=cfg["r_inflate"], min_unknown=cfg["min_unknown"], t_free=cfg["w_miss"], t_occ=cfg["w_hit"])
    out = {"recorded_64x56_B4": (ev, origin, cell, scene_starts, kw, True, 20),
           "recorded_64x56_B64": (ev, origin, cell, starts_on(ev, origin, cell, 64, 64, cfg["w_miss"]), kw, True, 10)}
    big, open_kw = open_field(362, 362), dict(r_inflate=2, min_unknown=2, t_free=T_FREE, t_occ=T_OCC)
    for B, reps in ((4, 3), (16, 2), (64, 1)):
        out[f"open_362x362_B{B}"] = (big, ORIGIN, CELL, starts_on(big, ORIGIN, CELL, B, B, T_FREE), open_kw, True, reps)
    lat = lattice_map(64, 1024)
    out["lattice_1024x1024_B16"] = (lat, ORIGIN, CELL, starts_on(lat, ORIGIN, CELL, 16, 16, 1), dict(open_kw, t_free=1, t_occ=3), False, 2)
    return out


def least_budget(make, plan, keys):
    """The least fixed `rounds` with which ``plan(make(rounds))`` comes back settled under every key (settledness is monotone in the
    budget): doubling, then bisection."""
    ok = lambda r: all(int(plan(make(r))[k].min()) == 1 for k in keys)
    hi = 1
    while not ok(hi):
        hi *= 2
    lo = hi // 2                                               # (lo failed, or is 0)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if ok(mid) else (mid, hi)
    return hi


def measure(scene, existing_only):
    """One scene: per class and variant (plain / everybody keeping) the least budget of ITS OWN plan, counted first, then the timed
    rounds at that budget + 1.  A keep slot relaxes a single-source field too, so the keeping plan of the tiled class may need more
    rounds than its plain plan."""
    ev, origin, cell, starts, kw, one_wg, reps = scene
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x), device="cuda")
    ev, start, B = t(ev), t(starts), len(starts)
    at = dict(origin=origin, cell=cell)
    classes = {"tiled": lipmpc.TiledCoordinatedFrontierPlanner}
    if one_wg:
        classes["one_workgroup"] = lipmpc.CoordinatedFrontierPlanner
    if not existing_only:
        classes["robot_fields"] = lipmpc.RobotFieldsFrontierPlanner
    info, variants, keep_alive = {"B": B, "grid": list(ev.shape), "max_claims": B, "r_claim": R_CLAIM, "reps_per_round": reps}, {}, []
    settled = ("settled", "claims_settled")
    for cname, cls in classes.items():
        budgeted = cname != "one_workgroup"
        for keeping in (False, True):
            key = f"{cname}_{'all_keeping' if keeping else 'plain'}"
            keep = ALL_KEEP if keeping else {}
            prev = None
            if keeping:                                        # the previous targets: the class's own plan, run until it settles
                o = cls(R_CLAIM, B, **keep, **kw).plan(ev, start, **at)
                prev = torch.where(o["claim_round"] >= 0, o["target_cell"], -1).to(torch.int32).contiguous()
            run = (lambda pl, out=None, p=prev: pl.replan(ev, start, **at, out=out, prev_target=p)) if keeping else \
                (lambda pl, out=None: pl.plan(ev, start, **at, out=out))
            more = {}
            if budgeted:
                need = least_budget(lambda r: cls(R_CLAIM, B, rounds=r, **keep, **kw), run, settled)
                info[f"{key}_rounds_needed"] = need
                more = dict(rounds=need + 1)
            pl = cls(R_CLAIM, B, **keep, **more, **kw)
            out = run(pl)                                      # fresh buffers, and the workspaces grow here
            torch.cuda.synchronize()
            variants[key] = lambda pl=pl, o=out, run=run: run(pl, o)
            keep_alive.append((pl, out))
            if budgeted:
                per_claim = 5 if keeping else 4
                info[f"{key}_claim_call_launches"] = pl.rounds + 8 if cname == "robot_fields" else B * (pl.rounds + per_claim) + 3
            if cname == "robot_fields" and not keeping:
                # the new call alone, on the settled frontier plan that `out` holds
                org, cs, org_c, cell_c = pl._placement(origin, cell)
                W, H = ev.shape
                variants["robot_fields_call_alone"] = lambda pl=pl, o=out, a=(org_c, cell_c): pl._claim_call(
                    B, W, H, start, None, None, a[0], a[1], 64, o, pl.rounds, 0)
                info["robot_fields_workspace_bytes"] = int(pl._claim_works[-1].numel())
    ms = rounds_of(variants, reps, ROUNDS, warm=2)
    torch.cuda.synchronize()
    for key, fn in variants.items():                           # after the timed rounds: what every timed plan did
        if key != "robot_fields_call_alone":
            o = fn()
            torch.cuda.synchronize()
            info[key] = {k: int(o[k][0]) for k in ("n_claims", "n_kept", "claims_settled") if k in o}
            if info[key].get("claims_settled", 1) != 1 or (key.endswith("all_keeping") and info[key]["n_kept"] != info[key]["n_claims"]):
                raise SystemExit(f"{key}: {info[key]} -- a timed plan that did not settle, or a claimer that did not keep")
    return {"scene": info, "ms_per_plan": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frontier_robot_fields.json"))
    ap.add_argument("--only", default=None, help="comma-separated scene names (default: all)")
    ap.add_argument("--parent-lib", default=None, help="the parent commit's library, for the existing plans")
    ap.add_argument("--existing-only", action="store_true", help="(the child of --parent-lib: the existing classes alone, JSON on the last line)")
    a = ap.parse_args()
    parent = None
    if a.parent_lib:                                           # first, before this process opens the device
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--existing-only"] + (["--only", a.only] if a.only else []),
                               env=dict(os.environ, LIPMPC_LIB=os.path.abspath(a.parent_lib)), capture_output=True, text=True, timeout=900)      # (the whole run took under 3 minutes on the MI355X, this child about a third of it)
        if child.returncode != 0:
            raise SystemExit(f"the parent library's run failed ({child.returncode}):\n{child.stdout[-2000:]}\n{child.stderr[-2000:]}")
        parent = json.loads(child.stdout.strip().splitlines()[-1])
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: a timing taken elsewhere says nothing")
    if a.existing_only:
        for k in NEW_CALLS:                                    # a library of the parent commit has ABI 5 and none of these
            lipmpc._lib.SIGNATURES.pop(k)
    maps = {}
    for name, scene in scenes().items():
        if a.only is None or name in a.only.split(","):
            maps[name] = measure(scene, a.existing_only)
            print(name, json.dumps(maps[name]), file=sys.stderr, flush=True)     # (a run that is cut short leaves what it measured)
    if a.existing_only:
        print(json.dumps({m: v["ms_per_plan"] for m, v in maps.items()}))
        return
    existing = "not measured (no --parent-lib)"
    if parent is not None:
        existing = {}
        for m, v in maps.items():
            for k, theirs in parent[m].items():
                mine = v["ms_per_plan"][k]
                existing[f"{m}/{k}"] = {"this_library": mine, "parent_library_in_a_child_process": theirs,
                                        "median_ratio": mine["median"] / theirs["median"],
                                        "rounds_overlap": mine["min"] <= theirs["max"] and theirs["min"] <= mine["max"]}
    out = {"what": "ms per plan (frontier field + path call + claim call), device events around `reps_per_round` back-to-back plans, "
                   "median / min / max over alternating rounds, one process; tiled plans at a fixed budget of the rounds needed + 1",
           "device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "keep_all_keeping": ALL_KEEP, "maps": maps, "existing_plans": existing}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
