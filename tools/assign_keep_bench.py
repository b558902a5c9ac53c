"""Time claim hysteresis (lipmpc_grid_frontier_assign_keep_batch through CoordinatedFrontierPlanner) beside the existing claim call
-> profiles/frontier_assign_keep.json.  Needs the GPU; run from the repository root:

    python tools/assign_keep_bench.py [--parent-root DIR]

One process, every variant warmed up, then device events around `reps` back-to-back calls, the variants alternating in rounds;
median / min / max over the rounds, in ms per call (field + path + claims: one ``plan`` / ``replan``).  Two maps: the first map of
the recorded scene of tests/golden/exploration_assigned.npz (64 x 56, tools/assign_bench.py's) with its four robots, and an open
field of 362 x 362 cells (the largest square the one-workgroup calls take: the slot field lives in ``work``) with four robots side
by side.  Per map:
  - assign          CoordinatedFrontierPlanner.plan, the existing call;
  - keep_none       the planner with r_keep, no previous targets: the keep call's greedy rounds alone;
  - keep_all        the planner with r_keep, every robot's previous target = the target ``assign`` gave it, generous parameters:
                    every robot keeps, one relaxation from a single cell each.
``--parent-root``: a built checkout of the parent commit.  A child process of the same run imports the package from there and times
``assign`` with the same harness: the existing call must stay within the run's own round-to-round spread of the parent's.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.environ.get("LIPMPC_BENCH_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(HERE, "tests"), os.path.join(HERE, "oracle"), os.path.join(HERE, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import lipmpc  # noqa: E402
from assign_bench import MAX_CLAIMS, R_CLAIM, first_map  # noqa: E402
from field_bench import rounds_of  # noqa: E402

KEEP = dict(r_keep=6, keep_ratio16=1024, keep_slack=4096)
BIG = 362


def maps():
    ev, origin, cell, starts, cfg = first_map()
    big = np.zeros((BIG, BIG), np.int32)
    big[2:BIG - 2, 2:BIG - 2] = -cfg["w_miss"]
    big_starts = np.array([[origin[0] + 40.5 * cell[0], origin[1] + (180.5 + k) * cell[1]] for k in range(4)])
    return {"64x56": (ev, starts), f"{BIG}x{BIG}": (big, big_starts)}, origin, cell, cfg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "frontier_assign_keep.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--child", action="store_true", help="(internal) time `assign` alone and print JSON")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda", 0)
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=dev)
    scenes, origin, cell, cfg = maps()
    kw = dict(r_inflate=cfg["r_inflate"], min_unknown=cfg["min_unknown"], t_free=cfg["w_miss"], t_occ=cfg["w_hit"])
    coord = lipmpc.CoordinatedFrontierPlanner(R_CLAIM, MAX_CLAIMS, **kw)
    keeper = None if a.child else lipmpc.CoordinatedFrontierPlanner(R_CLAIM, MAX_CLAIMS, **KEEP, **kw)
    buf = lambda table: {k: torch.zeros(shape, dtype=dt, device=dev) if dt != torch.uint32 else torch.empty(shape, dtype=dt, device=dev)
                         for k, (dt, shape, _) in table.items()}
    variants, facts, alive = {}, {}, []
    for name, (ev, starts) in scenes.items():
        W, H = ev.shape
        d_ev, d_st = t(ev), t(starts)
        B = len(starts)
        out = buf(lipmpc.planner.assign_outputs(B, W, H, 64))
        variants[f"assign_{name}"] = lambda d_ev=d_ev, d_st=d_st, out=out: coord.plan(d_ev, d_st, origin=origin, cell=cell, out=out)
        variants[f"assign_{name}"]()
        facts[name] = {"claims": int(out["n_claims"][0])}
        if a.child:
            continue
        prev = torch.where(out["status"] == 0, out["target_cell"], torch.full_like(out["target_cell"], -1)).clone()
        o_none, o_all = (buf(lipmpc.planner.assign_keep_outputs(B, W, H, 64)) for _ in range(2))
        variants[f"keep_none_{name}"] = lambda d_ev=d_ev, d_st=d_st, o=o_none: keeper.replan(d_ev, d_st, origin=origin, cell=cell, out=o)
        variants[f"keep_all_{name}"] = lambda d_ev=d_ev, d_st=d_st, o=o_all, prev=prev: keeper.replan(d_ev, d_st, origin=origin, cell=cell, out=o,
                                                                                                   prev_target=prev)
        variants[f"keep_none_{name}"](), variants[f"keep_all_{name}"]()
        facts[name].update(kept_in_keep_all=int(o_all["n_kept"][0]), claims_in_keep_all=int(o_all["n_claims"][0]),
                           claims_in_keep_none=int(o_none["n_claims"][0]))
        alive.append((d_ev, d_st, prev))
    ms = rounds_of(variants, a.reps, a.rounds)
    torch.cuda.synchronize()
    if a.child:
        print("CHILD " + json.dumps(ms))
        return
    out = {"what": "ms per call (field + path + claims), device events around `reps` back-to-back calls, median / min / max over alternating "
                   "rounds, one process", "device": torch.cuda.get_device_name(0), "reps_per_round": a.reps, "rounds": a.rounds,
           "r_claim": R_CLAIM, "max_claims": MAX_CLAIMS, "keep": KEEP, "robots": 4, "facts": facts, "ms_per_call": ms}
    if a.parent_root:
        env = dict(os.environ, LIPMPC_BENCH_ROOT=os.path.abspath(a.parent_root))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--rounds", str(a.rounds)], env=env,
                           capture_output=True, text=True, timeout=600)
        line = [x for x in r.stdout.splitlines() if x.startswith("CHILD ")]
        if r.returncode or not line:
            raise SystemExit(f"the parent's child process failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
        out["parent_ms_per_call"] = json.loads(line[0][6:])
        out["parent_note"] = "the existing call with the parent commit's library, a child process of this run (the same harness)"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
