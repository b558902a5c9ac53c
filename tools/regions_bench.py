"""Time the frontier regions call (lipmpc_grid_frontier_regions_batch) beside the ray-marched gain it can stand in for, and the
plans with gain_from="view" against "region" -> profiles/frontier_regions.json.  Needs the GPU; run from the repository root:

    python tools/regions_bench.py [--parent-lib path/to/the/parent/commit's/liblipmpc.so]

One process, every variant warmed up, then device events around `reps` back-to-back calls, the variants alternating in rounds;
median / min / max over the rounds, in ms per call (tools/field_bench.py's rounds_of).
  - the call alone at 92 x 80, 362 x 362, 1024 x 1024 and 4096 x 4096 on three evidence maps each -- open (a known free square in
    the unknown: one ring of frontier), lattice (known free but for 4 x 4 unknown blocks every 16 cells: thousands of small rings) and
    random (3 % of the cells unknown) -- whose frontier is the tiled frontier field's; beside it, on the same frontier, the gain
    call at r_view 10 and 30: the one-workgroup call up to its 2^17-cell cap, the tiled call above it;
  - on the recorded scene's first 64 x 56 map (tools/assign_bench.py's) at B = 64: the informed plan and the gain-seeded claims with
    "view" (r_view 10) against "region", cell and representative targets.
--parent-lib: the existing plans (field + path, the informed plan, the gain-seeded claims) are timed first in a fresh child process
that loads that library (LIPMPC_LIB), so that both builds' figures come from one visit to the device, and every kernel of that
library is compared with this build's kernel of the same name: registers, LDS, scratch, spills (tests/code_object.py).
The JSON is rewritten after every size, so that a run that is cut short leaves what it measured.
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
from code_object import kernel_resources  # noqa: E402
from field_bench import rounds_of  # noqa: E402
from gain_bench import starts_on  # noqa: E402

SIZES = ((92, 80), (362, 362), (1024, 1024), (4096, 4096))
MASKS = ("open", "lattice", "random")
R_VIEWS = (10, 30)
GAIN_CAP = 1 << 17                                             # cells of the one-workgroup gain call
W_GAIN, G_CAP, MIN_GAIN, R_CLAIM, B = 16, 120, 0, 15, 64
NEW_CALLS = ("lipmpc_grid_frontier_regions_batch", "lipmpc_grid_frontier_regions_workspace_bytes")
KW = dict(r_inflate=0, min_unknown=1, t_free=1, t_occ=3)
FIGURES = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count",
           "sgpr_spill_count")


def evidence(kind, W, H):
    ev = np.zeros((W, H), np.int32)
    if kind == "open":
        ev[W // 8:W - W // 8, H // 8:H - H // 8] = -1
        return ev
    ev[:] = -1
    if kind == "lattice":
        for i in range(8, W - 4, 16):
            ev[i:i + 4, 8:H - 4:16] = ev[i:i + 4, 9:H - 4:16] = ev[i:i + 4, 10:H - 4:16] = ev[i:i + 4, 11:H - 4:16] = 0
    else:
        ev[np.random.default_rng(W + H).random((W, H)) < 0.03] = 0
    return ev


def existing_plans(dev):
    """The plans the parent commit has too, on the recorded scene's first map at B robots: {name: callable}."""
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=dev)
    ev, origin, cell, scene_starts, cfg = first_map()
    starts = starts_on(ev, origin, cell, B, 1, cfg["w_miss"])
    starts[:len(scene_starts)] = scene_starts
    starts, d_ev = t(starts), t(ev)
    kw = dict(r_inflate=cfg["r_inflate"], min_unknown=cfg["min_unknown"], t_free=cfg["w_miss"], t_occ=cfg["w_hit"])
    gain = dict(r_view=10, w_gain=W_GAIN, g_cap=G_CAP, min_gain=MIN_GAIN)
    planners = {"field_plus_path": lipmpc.FrontierPlanner(**kw),
                "informed_view_r10": lipmpc.InformedFrontierPlanner(10, W_GAIN, G_CAP, MIN_GAIN, **kw),
                "seeded_claims_view_r10": lipmpc.CoordinatedFrontierPlanner(R_CLAIM, B, **gain, **kw)}
    plan = lambda pl: (lambda out=pl.plan(d_ev, starts, origin=origin, cell=cell): pl.plan(d_ev, starts, origin=origin, cell=cell, out=out))
    return {k: plan(pl) for k, pl in planners.items()}, (d_ev, starts, origin, cell, kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frontier_regions.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--existing-only", action="store_true", help="(the child of --parent-lib: the existing plans alone, JSON on the last line)")
    a = ap.parse_args()
    parent, figures = None, None
    if a.parent_lib:                                           # first, before this process opens the device
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--existing-only", "--reps", str(a.reps), "--rounds", str(a.rounds)],
                               env=dict(os.environ, LIPMPC_LIB=os.path.abspath(a.parent_lib)), capture_output=True, text=True, timeout=300)
        if child.returncode != 0:
            raise SystemExit(f"the parent library's run failed ({child.returncode}):\n{child.stderr[-2000:]}")
        parent = json.loads(child.stdout.strip().splitlines()[-1])
        old, new = kernel_resources(os.path.abspath(a.parent_lib)), kernel_resources(lipmpc._lib.LIB_PATH)
        pick = lambda r: {f: r.get(f, 0) for f in FIGURES}
        figures = {"parent_kernels": len(old), "this_build_kernels": len(new), "new_kernels": sorted(k for k in new if k not in old),
                   "missing_kernels": sorted(k for k in old if k not in new),
                   "changed_kernels": {k: [pick(old[k]), pick(new[k])] for k in old if k in new and pick(old[k]) != pick(new[k])},
                   "new_kernel_figures": {k: pick(new[k]) for k in new if k not in old}}
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: a timing taken elsewhere says nothing")
    if a.existing_only:
        for k in NEW_CALLS:                                    # a library of the parent commit has ABI 5 and none of these
            lipmpc._lib.SIGNATURES.pop(k)
    dev = torch.device("cuda", 0)
    plans, (d_ev, starts, origin, cell, kw) = existing_plans(dev)
    if a.existing_only:
        ms = rounds_of(plans, a.reps, a.rounds)
        torch.cuda.synchronize()
        print(json.dumps(ms))
        return
    out = {"what": "ms per call, device events around `reps` back-to-back calls, median / min / max over alternating rounds, one process",
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "w_gain": W_GAIN, "g_cap": G_CAP, "min_gain": MIN_GAIN,
           "launches_per_regions_call": 9, "call_alone": {}, "kernel_figures_against_the_parent_library": figures,
           "parent_library_plans_ms_per_call": parent,
           "parent_note": "the parent commit's library, timed in a child process of the same run just before this build's; the two run the same "
                          "kernels" if parent else "not measured in this run"}

    def write():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)

    # the plans: view against region
    gain = dict(r_view=None, w_gain=W_GAIN, g_cap=G_CAP, min_gain=MIN_GAIN, gain_from="region")
    more = {"informed_region_cell": lipmpc.InformedFrontierPlanner(None, W_GAIN, G_CAP, MIN_GAIN, gain_from="region", **kw),
            "informed_region_representative": lipmpc.InformedFrontierPlanner(None, W_GAIN, G_CAP, MIN_GAIN, gain_from="region",
                                                                             target="representative", **kw),
            "seeded_claims_region_cell": lipmpc.CoordinatedFrontierPlanner(R_CLAIM, B, **gain, **kw),
            "seeded_claims_region_representative": lipmpc.CoordinatedFrontierPlanner(R_CLAIM, B, **gain, target="representative", **kw)}
    for k, pl in more.items():
        plans[k] = (lambda pl=pl, o=pl.plan(d_ev, starts, origin=origin, cell=cell): pl.plan(d_ev, starts, origin=origin, cell=cell, out=o))
    out["plans_ms_per_call"] = dict(rounds_of(plans, a.reps, a.rounds), B=B, grid=list(d_ev.shape), reps_per_round=a.reps)
    write()
    # the call alone beside the gain call, on the frontier field's frontier
    field = lipmpc.FrontierPlanner(tiled=True, **KW)
    for W, H in SIZES:
        reps = a.reps if W * H <= GAIN_CAP else max(2, a.reps // 4) if W * H <= 1 << 20 else 2
        variants, info = {}, {}
        keep = []
        for kind in MASKS:
            ev = torch.as_tensor(evidence(kind, W, H), device=dev)[None]
            f = field.field(ev)
            frontier = f["frontier"]
            o = lipmpc.frontier_regions(frontier)
            torch.cuda.synchronize()
            info[kind] = {"n_frontier": int(f["n_frontier"][0]), "n_regions": o["n_regions"][0].tolist(),
                          "largest_region": int(o["size"].max())}
            variants[f"{kind}_regions"] = lambda fr=frontier, o=o: lipmpc.frontier_regions(fr, out=o)
            for r in R_VIEWS:
                cls = lipmpc.InformedFrontierPlanner if W * H <= GAIN_CAP else lipmpc.TiledInformedFrontierPlanner
                pl = cls(r, W_GAIN, G_CAP, MIN_GAIN, **KW)
                g = {"frontier": frontier, "gain": torch.empty((1, W, H), dtype=torch.int32, device=dev)}
                variants[f"{kind}_gain_r{r}"] = lambda pl=pl, ev=ev, g=g: pl._gain(ev, KW["t_free"], KW["t_occ"], g)
            keep.append((ev, f, o))
        ms = rounds_of(variants, reps, a.rounds, warm=2)
        torch.cuda.synchronize()
        out["call_alone"][f"{W}x{H}"] = {"reps_per_round": reps, "gain_call": "one-workgroup" if W * H <= GAIN_CAP else "tiled",
                                         "workspace_bytes": int(lipmpc._lib.load().lipmpc_grid_frontier_regions_workspace_bytes(1, W, H, 1024)),
                                         "masks": info, "ms_per_call": ms}
        write()
        del keep, variants
        torch.cuda.empty_cache()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
