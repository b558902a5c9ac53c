"""Time the correlative scan matcher (lipmpc_scan_match_batch) and the fleet sample around it -> profiles/scan_match.json.
Needs the GPU; run from the repository root:

    python tools/scan_match_bench.py [--parent-lib PATH]

The call: 4096 robots on the cell-aligned fixture, 360 rays, range 1.5, cells of 0.05, a shared evidence map of 512 x 512 cells
holding three scans of the batch.  lipmpc_map_update_batch on the same batch is the yardstick; the matcher at (n, n_yaw) = (4, 0),
(8, 0), (8, 4).  Device events around `reps` back-to-back calls, the variants alternating in rounds, median / min / max.
The fleet sample: one sample of the mapped fleet (UnknownEnvFleet(grid=, mapper=), B = 4096, a captured graph replayed k_max
times, ms per sample) with matcher=None -- the path this feature must not touch -- in child processes of this run, alternating
between this build and, with --parent-lib, a liblipmpc.so built from the parent commit (LIPMPC_LIB); beside it the same sample with
drift and matcher on.  Without --parent-lib the comparison is recorded as not measured.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

CELL, RANGE = (0.05, 0.05), 1.5
MATCHERS = {"match_n4": (4, 0), "match_n8": (8, 0), "match_n8_yaw4": (8, 4)}


def _stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def measure_call(B, reps, rounds, dev):
    import lipmpc
    import grid_lidar_oracle as G
    from lidar_grid_bench import events_ms
    fx = G.fixture(n_robots=B)
    gs = lipmpc.LidarSensor.from_grid(lipmpc.GridMap(fx["occ"], fx["origin"], fx["cell"]), lidar_range=RANGE, n_obs_max=12, v_max=32)
    st = np.zeros((B, 5)); st[:, 0] = fx["pos"][:, 0]; st[:, 2] = fx["pos"][:, 1]
    state = torch.as_tensor(st, device=dev)
    noise = 0.01 * torch.randn((B, 360, 2), dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    sen = gs.alloc_outputs(B, with_debug=True, rings=False, c_eta=True)
    gs.sense(state, noise, out=sen)
    mapper = lipmpc.OccupancyMapper(512, 512, (-5.0, -5.0), CELL, RANGE)
    scratch = lipmpc.OccupancyMapper(512, 512, (-5.0, -5.0), CELL, RANGE)      # what the timed updates add to
    for _ in range(3):
        mapper.update(state, sen["hits"])
    variants = {"map_update": lambda: scratch.update(state, sen["hits"])}
    matched = {}
    for name, (n, n_yaw) in MATCHERS.items():
        m = lipmpc.ScanMatcher(n, n, clamp=8, min_score=1, min_gain=1, n_yaw=n_yaw, yaw_step=0.01 if n_yaw else None)
        out = m.alloc_outputs(B, dev)
        m.match(mapper, state, sen["hits"], out=out)
        matched[name] = {"n_used_mean": float(out["n_used"].double().mean()), "matched": int(out["matched"].sum())}
        variants[name] = (lambda m=m, out=out: m.match(mapper, state, sen["hits"], out=out))
    for fn in variants.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            ms[k].append(events_ms(fn, reps))
    ms = {k: _stats(v) for k, v in ms.items()}
    return {"robots": B, "rays": 360, "cell": list(CELL), "lidar_range": RANGE, "evidence": "512 x 512 shared, three scans of the batch",
            "reps_per_round": reps, "rounds": rounds, "ms_per_call": ms, "outputs": matched,
            "match_over_update": {k: ms[k]["median"] / ms["map_update"]["median"] for k in MATCHERS},
            "bounded_by": "not measured: no hardware counters were taken"}


def child(variant, B, k_max, runs):
    """One process: ms per sample of the mapped fleet, ``runs`` runs after a warm-up run (which captures the graph)."""
    import lipmpc
    if os.environ.get("LIPMPC_LIB"):
        lipmpc._lib.SIGNATURES.pop("lipmpc_scan_match_batch", None)      # a library from before the symbol existed
    import grid_lidar_oracle as G
    dev = torch.device("cuda", 0)
    fx = G.fixture(n_robots=B)
    st = np.zeros((B, 5)); st[:, 0] = fx["pos"][:, 0]; st[:, 2] = fx["pos"][:, 1]
    st0 = torch.as_tensor(st, device=dev)
    goal = torch.tensor([[8.0, 8.0]] * B, dtype=torch.float64, device=dev)
    foot = torch.ones((B,), dtype=torch.int8, device=dev)
    mapper = lipmpc.OccupancyMapper(512, 512, (-5.0, -5.0), CELL, RANGE)
    kw, rkw = {}, {}
    if variant == "drift_matcher":
        kw = dict(drift_sigma=0.02, matcher=lipmpc.ScanMatcher(4, 4, clamp=8, min_score=20, min_gain=1))
    fleet = lipmpc.UnknownEnvFleet(grid=lipmpc.GridMap(fx["occ"], fx["origin"], fx["cell"]), N_horizon=3, lidar_range=RANGE, mapper=mapper, **kw)
    ms = []
    for i in range(runs + 1):
        mapper.reset()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fleet.run(st0, goal, foot, k_max, **rkw)
        b.record()
        torch.cuda.synchronize()
        if i:
            ms.append(a.elapsed_time(b) / k_max)
    print("RESULT " + json.dumps({"ms_per_sample": ms, "walking_samples": int(r["n_steps"].sum()),
                                  "n_matched": int(r["n_matched"].sum()) if "n_matched" in r else None}))


def measure_fleet(B, k_max, runs, rounds, parent_lib):
    variants = {"this_build": None, "drift_matcher": None}
    if parent_lib:
        variants["parent_build"] = os.path.abspath(parent_lib)
    ms, info = {k: [] for k in variants}, {}
    for _ in range(rounds):
        for name, lib in variants.items():
            env = dict(os.environ)
            env.pop("LIPMPC_LIB", None)
            if lib:
                env["LIPMPC_LIB"] = lib
            kind = "drift_matcher" if name == "drift_matcher" else "plain"
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind, "--robots", str(B), "--k-max", str(k_max),
                                "--runs", str(runs)], env=env, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise SystemExit(f"child {name} failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
            res = json.loads(next(l for l in p.stdout.splitlines() if l.startswith("RESULT "))[7:])
            ms[name] += res.pop("ms_per_sample")
            info[name] = res
    out = {"robots": B, "k_max": k_max, "runs_per_process": runs, "processes_per_variant": rounds,
           "what": "ms per sample of UnknownEnvFleet(grid=fixture, mapper=512 x 512 shared).run, graph replayed k_max times, seeded noise",
           "ms_per_sample": {k: _stats(v) for k, v in ms.items()}, "runs": info}
    if parent_lib:
        a, b = out["ms_per_sample"]["this_build"], out["ms_per_sample"]["parent_build"]
        out["this_over_parent_median"] = a["median"] / b["median"]
        out["inside_parent_spread"] = bool(b["min"] <= a["median"] <= b["max"])
    else:
        out["parent_build"] = "not measured: no --parent-lib given"
    return out


def compare_kernels(this_lib, parent_lib):
    """Registers, LDS, scratch and spills of every kernel of the parent's library against this build's kernel of the same name."""
    from code_object import kernel_resources
    fields = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")
    mine, theirs = kernel_resources(this_lib), kernel_resources(parent_lib)
    changed = sorted(k for k, r in theirs.items() if k not in mine or any(mine[k].get(f) != r.get(f) for f in fields))
    return {"parent_kernels": len(theirs), "changed_kernels": changed, "new_kernels": sorted(k for k in mine if k not in theirs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_match.json"))
    ap.add_argument("--robots", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--k-max", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--fleet-rounds", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: a timing taken elsewhere says nothing")
    if a.child:
        return child(a.child, a.robots, a.k_max, a.runs)
    import lipmpc
    from code_object import kernel_resources
    dev = torch.device("cuda", 0)
    out = {"what": "ms, device events, median / min / max over alternating rounds", "device": torch.cuda.get_device_name(0),
           "call": measure_call(a.robots, a.reps, a.rounds, dev)}
    del dev
    out["fleet_sample"] = measure_fleet(a.robots, a.k_max, a.runs, a.fleet_rounds, a.parent_lib)
    res = kernel_resources(lipmpc._lib.LIB_PATH)
    out["kernels"] = {}
    for key in ("scan_match_kernel", "map_update_kernel", "lidar_grid_scan_kernel"):
        r = next(v for k, v in res.items() if key in k)
        out["kernels"][key] = {"vgpr": r["vgpr_count"], "sgpr": r["sgpr_count"], "scratch_bytes": r["private_segment_fixed_size"],
                               "lds_bytes": r["group_segment_fixed_size"]}
    if a.parent_lib:
        out["kernel_figures_against_the_parent_library"] = compare_kernels(lipmpc._lib.LIB_PATH, a.parent_lib)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
