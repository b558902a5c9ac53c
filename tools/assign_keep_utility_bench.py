"""Time claim hysteresis for the gain-seeded claims (GainKeepFrontierPlanner / TiledGainKeepFrontierPlanner: frontier field, gain,
utility field, utility path, lipmpc_grid_frontier_assign_keep_utility_batch and its tiled form) beside the gain-seeded plan and the
plain keep plan -> profiles/frontier_assign_keep_utility.json.  Needs the GPU; run from the repository root:

    python tools/assign_keep_utility_bench.py [--parent-lib PATH]

One process, every variant warmed up, then device events around `reps` back-to-back calls, the variants alternating in rounds;
median / min / max over the rounds, in ms per call (tools/assign_bench.py's method and recorded map).
  - maps and calls: the recorded 64 x 56 map at B = 4 (one workgroup, slot field in LDS); an open 362 x 362 field, four robots (one
    workgroup, slot field in `work`); the same field by the tiled calls at a fixed budget;
  - plans: the nearest-frontier and the informed plan (what precedes the claims), the gain-seeded plan, the plain keep plan with
    every claimer keeping, the new plan with no previous targets and with every claimer keeping (previous targets = the planner's own
    last targets, r_keep 0, the most generous test: every attempt succeeds, so the claim call is n_kept keep slots and nothing else);
  - A KEEP SLOT of the new call against a keep slot of the plain keep call on the same map: (plan with everybody keeping - the plan
    that precedes its claims) / n_kept.  A seed is a constant offset to a single-source field, so the expectation is the same cost;
    the margin is the rounds' own spread;
  - existing plans: with --parent-lib (the previous commit's library) the nearest, informed, gain-seeded and plain keep plans are
    timed again in a freshly started child process that loads that library; the expectation is that the rounds overlap.  Without it
    the record says "not measured".
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

R_CLAIM, MAX_CLAIMS = 15, 64
GAIN = dict(r_view=15, w_gain=16, g_cap=120, min_gain=0)
ALL_KEEP = dict(r_keep=0, keep_ratio16=1024, keep_slack=4096)      # the target itself, at any cost: every attempt succeeds
BIG, BIG_R_CLAIM, BIG_CLAIMS = 362, 40, 4
EXISTING = ("nearest", "informed", "gain_seeded", "keep_all_keeping")


def plans(dev, classes, ev, start, origin, cell, kw, r_claim, max_claims, reps, rounds, with_new=True):
    """The six plans on one map: (ms per call, counts).  ``classes``: the planner classes of the map's form."""
    near_cls, informed_cls, claim_cls, new_cls = classes
    claims = (r_claim, max_claims)
    pls = {"nearest": near_cls(**kw), "informed": informed_cls(*GAIN.values(), **kw), "gain_seeded": claim_cls(*claims, **GAIN, **kw),
           "keep_all_keeping": claim_cls(*claims, **ALL_KEEP, **kw)}
    if with_new:
        pls["gain_keep_no_previous_target"] = new_cls(*claims, **GAIN, **ALL_KEEP, **kw)
        pls["gain_keep_all_keeping"] = new_cls(*claims, **GAIN, **ALL_KEEP, **kw)
    at = dict(origin=origin, cell=cell)
    outs, variants, prevs = {}, {}, {}
    for name, pl in pls.items():
        outs[name] = pl.plan(ev, start, **at)              # fresh buffers, and the workspaces grow here
        torch.cuda.synchronize()
        if name.endswith("all_keeping"):
            o = outs[name]
            prevs[name] = torch.where(o["claim_round"] >= 0, o["target_cell"], -1).to(torch.int32).contiguous()
            variants[name] = lambda pl=pl, o=o, p=prevs[name]: pl.replan(ev, start, **at, out=o, prev_target=p)
        else:
            variants[name] = lambda pl=pl, o=outs[name]: pl.plan(ev, start, **at, out=o)
    ms = rounds_of(variants, reps, rounds)
    torch.cuda.synchronize()
    count = lambda o, k: int(o[k][0]) if k in o else None
    counts = {name: {"n_claims": count(o, "n_claims"), "n_kept": count(o, "n_kept"), "claims_settled": count(o, "claims_settled")}
              for name, o in outs.items()}
    for name in prevs:
        if counts[name]["n_kept"] != counts[name]["n_claims"] or not counts[name]["n_kept"]:
            raise SystemExit(f"{name}: {counts[name]} -- not every claimer kept, the keep-slot figure would mix slots")
    return ms, counts


def keep_slot(ms, counts):
    """A keep slot of each call, from the medians, and the spread its two terms carry."""
    out = {}
    for name, before in (("keep_all_keeping", "nearest"), ("gain_keep_all_keeping", "informed")):
        n = counts[name]["n_kept"]
        spread = (ms[name]["max"] - ms[name]["min"] + ms[before]["max"] - ms[before]["min"]) / n
        out[name] = {"keep_slots": n, "ms_per_keep_slot": (ms[name]["median"] - ms[before]["median"]) / n, "spread_of_the_rounds_ms": spread,
                     "how": f"({name} - {before}) / n_kept, medians; spread = (max - min) of both terms / n_kept"}
    a, b = out["keep_all_keeping"], out["gain_keep_all_keeping"]
    out["difference_ms"] = b["ms_per_keep_slot"] - a["ms_per_keep_slot"]
    out["within_the_spread_of_the_rounds"] = abs(out["difference_ms"]) <= a["spread_of_the_rounds_ms"] + b["spread_of_the_rounds_ms"]
    return out


def small_map(dev, reps, rounds, with_new=True):
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=dev)
    ev, origin, cell, scene_starts, cfg = first_map()
    kw = dict(r_inflate=cfg["r_inflate"], min_unknown=cfg["min_unknown"], t_free=cfg["w_miss"], t_occ=cfg["w_hit"])
    classes = (lipmpc.FrontierPlanner, lipmpc.InformedFrontierPlanner, lipmpc.CoordinatedFrontierPlanner,
               getattr(lipmpc, "GainKeepFrontierPlanner", None))
    ms, counts = plans(dev, classes, t(ev), t(scene_starts), origin, cell, kw, R_CLAIM, MAX_CLAIMS, reps, rounds, with_new)
    return ms, counts, {"grid": list(ev.shape), "B": len(scene_starts), "r_claim": R_CLAIM, "max_claims": MAX_CLAIMS, **cfg}


def big_map(dev, reps, rounds, tiled, with_new=True):
    from assign_checks import CELL, ORIGIN, T_FREE, T_OCC, centres, open_field
    ev = torch.as_tensor(open_field(BIG, BIG), device=dev)
    start = torch.as_tensor(centres([(BIG // 2, BIG // 2 + k) for k in range(4)]), device=dev)
    kw = dict(r_inflate=2, min_unknown=2, t_free=T_FREE, t_occ=T_OCC)
    info = {"grid": [BIG, BIG], "B": 4, "r_claim": BIG_R_CLAIM, "max_claims": BIG_CLAIMS}
    if tiled:
        tw, th, _ = lipmpc.planner.tiled_info()
        budget = -(-BIG // tw) - (-BIG // th) + 1
        kw["rounds"] = info["rounds_budget"] = budget
        classes = (lambda **k: lipmpc.FrontierPlanner(tiled=True, **k), lipmpc.TiledInformedFrontierPlanner,
                   lipmpc.TiledCoordinatedFrontierPlanner, getattr(lipmpc, "TiledGainKeepFrontierPlanner", None))
    else:
        classes = (lipmpc.FrontierPlanner, lipmpc.InformedFrontierPlanner, lipmpc.CoordinatedFrontierPlanner,
                   getattr(lipmpc, "GainKeepFrontierPlanner", None))
    ms, counts = plans(dev, classes, ev, start, ORIGIN, CELL, kw, BIG_R_CLAIM, BIG_CLAIMS, max(2, reps // 4), rounds, with_new)
    return ms, counts, info


def measure(dev, reps, rounds, with_new=True):
    out = {}
    for name, run in (("recorded_map", lambda: small_map(dev, reps, rounds, with_new)),
                      (f"open_{BIG}x{BIG}_one_workgroup", lambda: big_map(dev, reps, rounds, False, with_new)),
                      (f"open_{BIG}x{BIG}_tiled", lambda: big_map(dev, reps, rounds, True, with_new))):
        ms, counts, scene = run()
        out[name] = {"scene": scene, "counts": counts, "ms_per_call": ms}
        if with_new:
            out[name]["keep_slot"] = keep_slot(ms, counts)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frontier_assign_keep_utility.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="the previous commit's library, for the existing plans")
    ap.add_argument("--child", action="store_true", help="(internal) time the existing plans with the library LIPMPC_LIB names; print JSON")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda", 0)
    if a.child:
        for name in [n for n in lipmpc._lib.SIGNATURES if "assign_keep_utility" in n]:     # (the previous library has no such export)
            del lipmpc._lib.SIGNATURES[name]
        print("CHILD_JSON " + json.dumps({k: v["ms_per_call"] for k, v in measure(dev, a.reps, a.rounds, with_new=False).items()}))
        return
    maps = measure(dev, a.reps, a.rounds)
    existing = "not measured (no --parent-lib)"
    if a.parent_lib:
        env = dict(os.environ, LIPMPC_LIB=os.path.abspath(a.parent_lib))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--rounds", str(a.rounds)], env=env,
                           capture_output=True, text=True, timeout=900)
        line = [x for x in r.stdout.splitlines() if x.startswith("CHILD_JSON ")]
        if r.returncode != 0 or not line:
            raise SystemExit(f"the child process with the parent's library failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        parent = json.loads(line[0][len("CHILD_JSON "):])
        existing = {}
        for m, v in maps.items():
            for k in EXISTING:
                mine, theirs = v["ms_per_call"][k], parent[m][k]
                existing[f"{m}/{k}"] = {"this_library": mine, "parent_library_in_a_child_process": theirs,
                                        "median_ratio": mine["median"] / theirs["median"],
                                        "rounds_overlap": mine["min"] <= theirs["max"] and theirs["min"] <= mine["max"]}
    out = {"what": "ms per call, device events around `reps` back-to-back calls, median / min / max over alternating rounds, one process",
           "device": torch.cuda.get_device_name(0), "reps_per_round": a.reps, "rounds": a.rounds, "gain": GAIN, "keep_all_keeping": ALL_KEEP,
           "maps": maps, "existing_plans": existing}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
