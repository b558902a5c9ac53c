"""Time the gain-seeded claims (CoordinatedFrontierPlanner with r_view / w_gain / g_cap: frontier field, gain, utility field, utility
path, lipmpc_grid_frontier_assign_utility_batch) beside the coordinated plan and the informed plan -> profiles/frontier_assign_utility.json.
Needs the GPU; run from the repository root:

    python tools/assign_utility_bench.py [--parent-lib PATH]

One process, every variant warmed up, then device events around `reps` back-to-back calls, the variants alternating in rounds;
median / min / max over the rounds, in ms per call (tools/assign_bench.py's method, map and starts).
  - small map: the recorded 64 x 56 map at B = 3 / 64 / 1024 -- the coordinated plan, the informed plan and the gain-seeded plan at
    r_view 15 / w_gain 16 / g_cap 120 / min_gain 0, with the rounds the two claim calls ran;
  - cost per round: at B = 64 both claim planners with max_claims = ROUNDS, both running the same number of rounds (else the tool
    stops); the claim call alone is its plan minus the plan that precedes it (nearest-frontier / informed), and the per-round difference is recorded;
  - tiled: an open 362 x 362 field, four robots, 4 claims, a fixed budget: the tiled gain-seeded plan beside the tiled coordinated plan
    and the tiled informed plan;
  - unchanged calls: with --parent-lib (the previous commit's library) the coordinated and the informed plan are timed again in a
    freshly started child process that loads that library; the expectation is equality within the round spread.  Without it the
    record says "not measured".
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
R_CLAIM, MAX_CLAIMS, ROUNDS = 15, 64, 8
GAIN = dict(r_view=15, w_gain=16, g_cap=120, min_gain=0)
BIG, BIG_CLAIMS = 362, 4


def buf(table, dev):
    return {k: torch.zeros(shape, dtype=dt, device=dev) if dt != torch.uint32 else torch.empty(shape, dtype=dt, device=dev)
            for k, (dt, shape, _) in table.items()}


def small_map(dev, reps, rounds, with_new=True):
    """The variants on the recorded map: (ms, rounds run per claim planner)."""
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
    P = lipmpc.planner
    planners = {"nearest": (lipmpc.FrontierPlanner(**kw), lambda B: P.frontier_outputs(B, 1, W, H, 64)),
                "coordinated": (lipmpc.CoordinatedFrontierPlanner(R_CLAIM, MAX_CLAIMS, **kw), lambda B: P.assign_outputs(B, W, H, 64)),
                "informed": (lipmpc.InformedFrontierPlanner(*GAIN.values(), **kw), lambda B: P.informed_outputs(B, 1, W, H, 64)),
                f"coordinated_{ROUNDS}_rounds": (lipmpc.CoordinatedFrontierPlanner(R_CLAIM, ROUNDS, **kw), lambda B: P.assign_outputs(B, W, H, 64))}
    if with_new:
        planners["gain_seeded"] = (lipmpc.CoordinatedFrontierPlanner(R_CLAIM, MAX_CLAIMS, **GAIN, **kw),
                                   lambda B: P.assign_utility_outputs(B, W, H, 64))
        planners[f"gain_seeded_{ROUNDS}_rounds"] = (lipmpc.CoordinatedFrontierPlanner(R_CLAIM, ROUNDS, **GAIN, **kw),
                                                    lambda B: P.assign_utility_outputs(B, W, H, 64))
    variants, outs = {}, {}
    for name, (pl, table) in planners.items():
        for B in ((64,) if name.endswith("_rounds") else ROBOTS):
            outs[name, B] = buf(table(B), dev)
            variants[f"{name}_plan_B{B}"] = lambda pl=pl, B=B, o=outs[name, B]: pl.plan(d_ev, starts[:B], origin=origin, cell=cell, out=o)
    ms = rounds_of(variants, reps, rounds)
    torch.cuda.synchronize()
    ran = {f"{name}_B{B}": int(o["n_claims"][0]) for (name, B), o in outs.items() if "n_claims" in o}
    scene = {"grid": [W, H], "n_frontier": int(outs["nearest", n_max]["n_frontier"][0]), **cfg}
    return ms, ran, scene


def tiled(dev, reps, rounds):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from assign_checks import CELL, ORIGIN, T_FREE, T_OCC, centres, open_field
    ev = torch.as_tensor(open_field(BIG, BIG), device=dev)
    start = torch.as_tensor(centres([(BIG // 2, BIG // 2 + k) for k in range(4)]), device=dev)
    tw, th, _ = lipmpc.planner.tiled_info()
    budget = -(-BIG // tw) - (-BIG // th) + 1
    kw = dict(r_inflate=2, min_unknown=2, t_free=T_FREE, t_occ=T_OCC, rounds=budget)
    planners = {"tiled_coordinated": lipmpc.TiledCoordinatedFrontierPlanner(40, BIG_CLAIMS, **kw),
                "tiled_informed": lipmpc.TiledInformedFrontierPlanner(*GAIN.values(), **kw),
                "tiled_gain_seeded": lipmpc.TiledCoordinatedFrontierPlanner(40, BIG_CLAIMS, **GAIN, **kw)}
    outs = {k: pl.plan(ev, start, origin=ORIGIN, cell=CELL) for k, pl in planners.items()}
    variants = {f"{k}_plan_{BIG}x{BIG}": (lambda pl=pl, o=outs[k]: pl.plan(ev, start, origin=ORIGIN, cell=CELL, out=o)) for k, pl in planners.items()}
    ms = rounds_of(variants, max(2, reps // 4), rounds)
    torch.cuda.synchronize()
    info = {"grid": [BIG, BIG], "rounds_budget": budget, "max_claims": BIG_CLAIMS, "r_claim": 40,
            "claims_made": {k: int(o["n_claims"][0]) for k, o in outs.items() if "n_claims" in o},
            "claims_settled": {k: int(o["claims_settled"][0]) for k, o in outs.items() if "claims_settled" in o}}
    return ms, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frontier_assign_utility.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="the previous commit's library, for the unchanged calls")
    ap.add_argument("--child", action="store_true", help="(internal) time the unchanged calls with the library LIPMPC_LIB names; print JSON")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda", 0)
    if a.child:
        for name in [n for n in lipmpc._lib.SIGNATURES if "assign_utility" in n]:          # (the previous library has no such export)
            del lipmpc._lib.SIGNATURES[name]
        ms, _, _ = small_map(dev, a.reps, a.rounds, with_new=False)
        print("CHILD_JSON " + json.dumps(ms))
        return
    ms, ran, scene = small_map(dev, a.reps, a.rounds)
    med = lambda k: ms[k]["median"]
    plain_claims = med(f"coordinated_{ROUNDS}_rounds_plan_B64") - med("nearest_plan_B64")
    seeded_claims = med(f"gain_seeded_{ROUNDS}_rounds_plan_B64") - med("informed_plan_B64")
    run = {k: v for k, v in ran.items() if "_rounds" in k}
    if len(set(run.values())) != 1:
        raise SystemExit(f"the two claim calls ran different numbers of rounds: {run}")
    per_round = {"max_claims": ROUNDS, "rounds_run": run, "plain_claim_call_ms": plain_claims, "gain_seeded_claim_call_ms": seeded_claims,
                 "difference_per_round_ms": (seeded_claims - plain_claims) / max(1, next(iter(run.values()))),
                 "how": "claim call alone = its plan minus the plan that precedes it (nearest-frontier / informed), medians, B = 64"}
    tiled_ms, tiled_info = tiled(dev, a.reps, a.rounds)
    unchanged = "not measured (no --parent-lib)"
    if a.parent_lib:
        env = dict(os.environ, LIPMPC_LIB=os.path.abspath(a.parent_lib))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--rounds", str(a.rounds)], env=env,
                           capture_output=True, text=True, timeout=600)
        line = [x for x in r.stdout.splitlines() if x.startswith("CHILD_JSON ")]
        if r.returncode != 0 or not line:
            raise SystemExit(f"the child process with the parent's library failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        parent = json.loads(line[0][len("CHILD_JSON "):])
        unchanged = {k: {"this_library": ms[k], "parent_library_in_a_child_process": parent[k],
                         "median_ratio": ms[k]["median"] / parent[k]["median"]} for k in parent}
    out = {"what": "ms per call, device events around `reps` back-to-back calls, median / min / max over alternating rounds, one process",
           "device": torch.cuda.get_device_name(0), "reps_per_round": a.reps, "rounds": a.rounds, "scene": scene, "r_claim": R_CLAIM,
           "max_claims": MAX_CLAIMS, "gain": GAIN, "claim_rounds_run": ran, "ms_per_call": ms, "cost_per_round": per_round,
           "tiled": dict(tiled_info, ms_per_call=tiled_ms), "unchanged_calls": unchanged}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
