"""Time the scans with the sector split (lipmpc_lidar_c_eta_split_batch / lipmpc_lidar_grid_c_eta_split_batch) for 4096 robots:

    python tools/lidar_split_bench.py --parent-lib PATH/liblipmpc.so [--out profiles/lidar_split.json]

on two maps -- config5 (bench.py's config-5 map, 20 polygons, through the ring scan) and rooms (the three rooms of
tests/lidar_split_oracle.py as a grid, robots in free cells, through the grid scan) -- for
  parent     the parent commit's library (--parent-lib, loaded through LIPMPC_LIB), the scans as they were
  off        this build, split_rays = 0 (the parent entry points, which now pass 0 to the same launcher)
  split_30 / split_45   this build with the split on
The two libraries cannot live in one process, so the tool starts fresh worker processes of itself, parent and this build in
turn, `--sessions` times each; a worker times every variant of its library in alternating rounds (device events around `reps`
back-to-back calls).  Per variant: the median of all its rounds, min, max, and the medians of its sessions.  The requirement is on
`off` against `parent`: the difference of the medians within the run-to-run spread of this run (the larger of the two variants'
max - min over sessions' medians).  What the split itself costs is reported, not bounded.  Needs the GPU."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def worker(a):
    """One process, one library: ms per call of every variant on both maps -> one JSON line on stdout."""
    import torch
    from importlib import import_module
    import lipmpc
    import lidar_split_oracle as S
    if a.worker == "parent":                                  # the parent's library has no split entry points to bind
        for name in [n for n in lipmpc._lib.SIGNATURES if n.endswith("_split_batch")]:
            del lipmpc._lib.SIGNATURES[name]
    synth = import_module("humanoid-navigation-using-mpc-ldcbf_amd.synth")
    dev = torch.device("cuda", 0)
    B = a.robots
    splits = {"parent": 0} if a.worker == "parent" else {"off": 0, "split_30": 30, "split_45": 45}
    gen = torch.Generator(device=dev).manual_seed(3)
    noise = 0.01 * torch.randn((B, 360, 2), dtype=torch.float64, device=dev, generator=gen)

    def states(pos):
        st = np.zeros((B, 5)); st[:, 0] = pos[:, 0]; st[:, 2] = pos[:, 1]
        return torch.as_tensor(st, device=dev)

    # config5: bench.py's map and robots, the ring scan in index order
    exy, env = synth.synthetic_fields(1, 20, -1.0, 6.0, (-5.0, -5.0), (50.0, 50.0), seed=9, delta=0.6)
    rings = [exy[0, j, : env[0, j]] for j in range(20) if env[0, j] > 0]
    pos5 = (torch.rand((B, 2), dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(3)) * 7.0 - 1.0).cpu().numpy()
    # rooms: robots anywhere in the rooms, at least a cell from a wall
    occ, origin, cell = S.rooms_scene()
    rng = np.random.default_rng(0)
    posr = []
    while len(posr) < B:
        p = rng.uniform((0.3, 0.3), (6.1, 5.3))
        i, j = int(p[0] / cell[0]), int(p[1] / cell[1])
        if not occ[i - 1:i + 2, j - 1:j + 2].any():
            posr.append(p)
    posr = np.array(posr)
    calls, info = {}, {}
    for tag, split in splits.items():
        ps = lipmpc.LidarSensor(rings, lidar_range=1.5, n_obs_max=12, v_max=32, split_rays=split)
        gs = lipmpc.LidarSensor.from_grid(lipmpc.GridMap(occ, origin, cell), lidar_range=1.5, n_obs_max=12, v_max=32, split_rays=split)
        for name, sn, st in (("config5", ps, states(pos5)), ("rooms", gs, states(posr))):
            out = sn.alloc_outputs(B, rings=False, c_eta=True)
            calls[(name, tag)] = (lambda sn=sn, st=st, out=out: sn.sense(st, noise, out=out, schedule=None))
            calls[(name, tag)]()
            torch.cuda.synchronize()
            info[f"{name}/{tag}"] = {"mean_inferred": float(out["n_inferred"].double().mean()), "overflow": int(out["overflow"].sum())}

    def events_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.reps

    for fn in calls.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(a.rounds):
        for k, fn in calls.items():
            ms[k].append(events_ms(fn))
    print("RESULT " + json.dumps({"ms": {f"{m}/{t}": v for (m, t), v in ms.items()}, "info": info, "device": torch.cuda.get_device_name(0)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="liblipmpc.so built from the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lidar_split.json"))
    ap.add_argument("--robots", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sessions", type=int, default=3)
    ap.add_argument("--worker", choices=("parent", "this"))
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        raise SystemExit("--parent-lib: the parent commit's liblipmpc.so (build it in a checkout of the parent)")
    sessions, info, device = {}, {}, None
    for s in range(a.sessions):
        for which in ("parent", "this"):
            env = dict(os.environ)
            env.pop("LIPMPC_LIB", None)
            if which == "parent":
                env["LIPMPC_LIB"] = os.path.abspath(a.parent_lib)
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", which, "--robots", str(a.robots), "--reps", str(a.reps), "--rounds", str(a.rounds)]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                raise SystemExit(f"worker {which} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            res = json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))[7:])
            device = res["device"]
            info.update(res["info"])
            for k, v in res["ms"].items():
                sessions.setdefault(k, []).append(v)
    out = {"what": "scan + clusters [+ sector split] + hulls + (c, eta) in one launch, ms per call of `robots` robots in index order, device events "
                   "around `reps` back-to-back calls; per variant the median / min / max over every round of every session and the sessions' "
                   "medians; 360 rays, range 1.5, noise given, 12 x 32 slots",
           "device": device, "robots": a.robots, "reps_per_round": a.reps, "rounds_per_session": a.rounds, "sessions": a.sessions, "maps": {}}
    for k, per_session in sorted(sessions.items()):
        m, tag = k.split("/")
        allv = [x for v in per_session for x in v]
        out["maps"].setdefault(m, {})[tag] = {"median": float(np.median(allv)), "min": float(min(allv)), "max": float(max(allv)),
                                              "session_medians": [float(np.median(v)) for v in per_session], **info[k]}
    for m, v in out["maps"].items():
        spread = max(max(v[t]["session_medians"]) - min(v[t]["session_medians"]) for t in ("parent", "off"))
        diff = v["off"]["median"] - v["parent"]["median"]
        v["off_minus_parent_ms"] = diff
        v["run_to_run_spread_ms"] = spread
        v["off_within_spread_of_parent"] = bool(diff <= spread)
        for t in ("split_30", "split_45"):
            v[t + "_over_off"] = v[t]["median"] / v["off"]["median"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out["maps"], indent=1))


if __name__ == "__main__":
    main()
