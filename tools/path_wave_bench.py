"""Time the wave-per-robot path calls beside the one-lane path calls on the same settled fields -> profiles/path_wave.json.  Needs
the GPU; run from the repository root:

    python tools/path_wave_bench.py [--parent-lib PATH/liblipmpc.so]

One process, every variant warmed up, then device events around `reps` back-to-back calls (1 where a call takes more than 50 ms), the
lane and the wave variants alternating in rounds; median / min / max over 5 rounds, in ms per call.  Every timed step runs under a
watchdog of its own (tools/field_tiled_bench.py's): a step that does not come back within --limit seconds ends the process with
status 124.
  - maps: 92 x 80 (the fleet scene of tools/field_bench.py), 200 x 199 and 362 x 362 (the baffle strip of tests/field_shape_cases.py)
    and 1024^2 (tools/field_tiled_bench.py's walls every 128 rows);
  - paths: goal, frontier, weighted goal (r_clear 4 / w_clear 40) and utility (r_view 15), each down ONE shared field that was settled
    before anything is timed; B = 1, 16, 1024 and 4096 robots at random free cells, and 32768 on 92 x 80;
  - spacing: max_seg 200 (the setting of the field + path rows in profiles/clearance.json) at every B, and no cap -- the planners'
    default, where the one-lane sight tests are quadratic in a straight stretch -- at B = 16 on the maps up to 362 x 362;
  - field + path: the planner's whole plan (paths="lane" / "wave") with a fixed budget, at B = 16;
  - --parent-lib: the library built from the PARENT commit (git worktree add ../parent HEAD~ && make -C ../parent/<package>/csrc).
    A child process of this run, started before this one touches the GPU, loads it (LIPMPC_LIB) and times the one-lane calls at
    B = 16; the code-object figures of EVERY kernel of that library are compared with this build's and recorded.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import lipmpc  # noqa: E402
import field_shape_cases as S  # noqa: E402
import field_tiled_bench as FT  # noqa: E402
from code_object import kernel_resources  # noqa: E402
from field_bench import fleet_scene  # noqa: E402

NEW = ("lipmpc_grid_path_wave_batch", "lipmpc_grid_frontier_path_wave_batch", "lipmpc_grid_frontier_utility_path_wave_batch")
R_CLEAR, W_CLEAR = 4, 40
INFORMED = dict(r_view=15, w_gain=16, g_cap=200, min_gain=0)
KINDS = ("goal", "frontier", "weighted", "utility")
CAPPED, S_MAX = 200, 256
FIGURES = ("vgpr_count", "sgpr_count", "agpr_count", "private_segment_fixed_size", "group_segment_fixed_size", "vgpr_spill_count",
           "sgpr_spill_count")
BATCHES = (1, 16, 1024, 4096)
PATH_OUT = ("sub_goals", "n_sub", "status", "path_cost")


def maps():
    occ, origin, cell, goal = fleet_scene()
    out = {"92x80": dict(occ=occ, origin=origin, cell=cell, goal=np.asarray(goal, float).reshape(1, 2), r=2, batches=BATCHES + (32768,))}
    for W, H in ((200, 199), (362, 362)):
        c = S.strip_case(W, H)
        out[f"{W}x{H}"] = dict(occ=c["occ"], origin=S.ORIGIN, cell=S.CELL, goal=c["goal"], r=c["r"], batches=BATCHES)
    out["1024x1024"] = dict(occ=FT.walls(1024), origin=(0.0, 0.0), cell=(0.05, 0.05), goal=np.array([[0.025, 0.025]]), r=0, batches=BATCHES)
    for m in out.values():
        free = np.argwhere(m["occ"] == 0)
        pick = free[np.random.default_rng(5).integers(len(free), size=max(m["batches"]))]
        m["start"] = np.stack([m["origin"][0] + (pick[:, 0] + 0.5) * m["cell"][0], m["origin"][1] + (pick[:, 1] + 0.5) * m["cell"][1]], 1)
        m["ev"] = np.where(m["occ"] != 0, S.T_OCC, -S.T_FREE).astype(np.int32)
        m["ev"][-2:, -2:] = 0                                   # the unknown block in the far corner: the frontier lies beside it
    return out


def planner(kind, m, max_seg, **kw):
    if kind in ("goal", "weighted"):
        more = dict(r_clear=R_CLEAR, w_clear=W_CLEAR) if kind == "weighted" else {}
        return lipmpc.GridFieldPlanner(r_inflate=m["r"], max_seg=max_seg, tiled=True, **more, **kw)
    common = dict(r_inflate=m["r"], min_unknown=2, t_free=S.T_FREE, t_occ=S.T_OCC, max_seg=max_seg, **kw)
    return lipmpc.FrontierPlanner(tiled=True, **common) if kind == "frontier" else lipmpc.TiledInformedFrontierPlanner(**INFORMED, **common)


class Paths:
    """One map, one kind, one batch: the plan once (rounds=None: every field settled), then the path call alone, either way, into the
    plan's own buffers."""

    def __init__(self, kind, m, B, max_seg):
        dev = torch.device("cuda", 0)
        t = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=dev)
        self.kind, self.m, self.B, self.max_seg = kind, m, B, lipmpc.planner.FIELD_NO_CAP if max_seg is None else max_seg
        self.start, self.goal, self.ev = t(m["start"][:B]), t(m["goal"]), t(m["ev"])
        self.grid = lipmpc.GridMap(m["occ"], m["origin"], m["cell"]).to(dev)
        self.pl = planner(kind, m, max_seg)
        self.out = self.plan(self.pl, None)
        torch.cuda.synchronize()
        for k in ("settled", "usettled"):
            assert int(self.out.get(k, torch.ones(1)).min()) == 1, f"{k}: the field did not settle"
        self.org, self.cs = self.pl._placement(m["origin"], m["cell"])[2:] if kind in ("frontier", "utility") else (None, None)

    def plan(self, pl, out):
        if self.kind in ("goal", "weighted"):
            return pl.plan_grid_batch(self.goal, self.grid, self.start, S_max=S_MAX, out=out)
        return pl.plan(self.ev, self.start, origin=self.m["origin"], cell=self.m["cell"], S_max=S_MAX, out=out)

    def path(self, wave):
        o, W, H = self.out, *self.m["occ"].shape
        tail = dict(start=self.start, r_inflate=self.m["r"], max_seg=self.max_seg, S_max=S_MAX, hip_stream=torch.cuda.current_stream().cuda_stream)
        if self.kind in ("goal", "weighted"):
            cost = dict(cost=o["cost"]) if self.kind == "weighted" else dict(cost=None) if wave else {}
            name = "lipmpc_grid_path_wave_batch" if wave else "lipmpc_grid_path_weighted_batch" if self.kind == "weighted" else "lipmpc_grid_path_tiled_batch"
            return lipmpc._lib.call(name, device=0, B=self.B, F=1, **self.grid._args(1, torch.device("cuda", 0)), **cost, field=o["field"],
                                    field_status=o["field_status"], settled=o["settled"], goal=self.goal, **{k: o[k] for k in PATH_OUT}, **tail)
        place = dict(origin=C.addressof(self.org), cell=C.addressof(self.cs), evidence=self.ev, t_occ=S.T_OCC)
        if self.kind == "frontier":
            name = "lipmpc_grid_frontier_path_wave_batch" if wave else "lipmpc_grid_frontier_path_tiled_batch"
            return lipmpc._lib.call(name, device=0, B=self.B, F=1, W=W, H=H, **place, **(dict(cost=None) if wave else {}), field=o["field"],
                                    n_frontier=o["n_frontier"], settled=o["settled"], **{k: o[k] for k in PATH_OUT + ("target_cell",)}, **tail)
        name = "lipmpc_grid_frontier_utility_path_wave_batch" if wave else "lipmpc_grid_frontier_utility_path_tiled_batch"
        return lipmpc._lib.call(name, device=0, B=self.B, F=1, W=W, H=H, **place, **{k: o[k] for k in ("frontier", "gain", "ufield", "n_sources")},
                                settled=o["usettled"], w_gain=INFORMED["w_gain"], g_cap=INFORMED["g_cap"], min_gain=INFORMED["min_gain"],
                                **{k: o[k] for k in PATH_OUT + ("target_cell", "target_gain")}, **tail)

    def outputs(self):
        torch.cuda.synchronize()
        return {k: self.out[k].cpu().numpy().copy() for k in PATH_OUT + (("target_cell",) if "target_cell" in self.out else ())}

    def budget(self):
        """A fixed budget that settles the plan's fields: doubled from 8 until it does."""
        rounds = 8
        while True:
            pl = planner(self.kind, self.m, None if self.max_seg == lipmpc.planner.FIELD_NO_CAP else self.max_seg, rounds=rounds)
            out = self.plan(pl, None)
            torch.cuda.synchronize()
            if all(int(out.get(k, torch.ones(1)).min()) == 1 for k in ("settled", "usettled")):
                return rounds
            rounds *= 2
            assert rounds <= 4096


def variants(which, lane_only=False):
    """({name: call}, {name: facts}, what to keep alive).  ``which``: (map, kind, B, max_seg) tuples."""
    all_maps, calls, facts, keep = maps(), {}, {}, []
    for name, kind, B, max_seg in which:
        p = FT.limited(Paths, kind, all_maps[name], B, max_seg)
        key = f"{name}_{kind}_B{B}_{'nocap' if max_seg is None else f'seg{max_seg}'}"
        ways = ("lane",) if lane_only else ("lane", "wave")
        got = {}
        for way in ways:
            FT.limited(p.path, way == "wave")
            got[way] = p.outputs()
            calls[f"{key}_path_{way}"] = lambda p=p, way=way: p.path(way == "wave")
        status = got["lane"]["status"]
        facts[key] = dict(found=int((status == lipmpc.RRT_FOUND).sum()), overflow=int((status == lipmpc.RRT_PATH_OVERFLOW).sum()),
                          most_sub_goals=int(got["lane"]["n_sub"].max()), longest_path_cells=float(np.nan_to_num(got["lane"]["path_cost"], nan=-1.0).max()))
        if not lane_only:
            for k, v in got["lane"].items():
                same = np.array_equal(v.view(np.int64) if v.dtype == np.float64 else v, got["wave"][k].view(np.int64) if v.dtype == np.float64 else got["wave"][k])
                assert same, f"{key}: {k} differs between the lane and the wave call"
            facts[key]["lane_and_wave_outputs_equal"] = True
        if B == 16 and max_seg == CAPPED:                     # field + path: the planner's whole plan, a fixed budget
            rounds = FT.limited(p.budget)
            facts[key]["rounds"] = rounds
            for way in ways:
                pl = planner(kind, all_maps[name], max_seg, rounds=rounds, paths=way) if not lane_only else planner(kind, all_maps[name], max_seg, rounds=rounds)
                out = FT.limited(p.plan, pl, None)
                calls[f"{key}_field_plus_path_{way}"] = lambda p=p, pl=pl, out=out: p.plan(pl, out)
                keep.append((pl, out))
        keep.append(p)
    return calls, facts, keep


def selection(parent=False):
    out = []
    for name, m in maps().items():
        for kind in KINDS:
            if parent:
                out.append((name, kind, 16, CAPPED))
                continue
            out += [(name, kind, B, CAPPED) for B in m["batches"]]
            if name != "1024x1024":
                out.append((name, kind, 16, None))
    return out


def child(a):
    """The one-lane calls alone at B = 16, with whatever library LIPMPC_LIB names: the timings as JSON on stdout."""
    for name in NEW:                                           # (the parent's library has none of them: bind what it has)
        lipmpc._lib.SIGNATURES.pop(name)
    calls, facts, keep = variants(selection(parent=True), lane_only=True)
    ms = FT.rounds_of(calls, a.reps, a.rounds)
    print("CHILD_JSON " + json.dumps(dict(library="the parent commit's build (--parent-lib)", facts=facts, ms_per_call=ms)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "path_wave.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=float, default=120.0, help="seconds a single timed step may take")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    FT.LIMIT[0] = a.limit
    if a.child:
        if not torch.cuda.is_available():
            raise SystemExit("needs the GPU: a timing taken elsewhere says nothing")
        return child(a)
    # -- the parent's library, in a child process started before this one touches the GPU -----------------------------------------
    parent = dict(run=False, why="no --parent-lib given")
    if a.parent_lib:
        mine, theirs = kernel_resources(lipmpc._lib.LIB_PATH), kernel_resources(a.parent_lib)
        same = {n: {f: theirs[n].get(f) for f in FIGURES} == {f: mine.get(n, {}).get(f) for f in FIGURES} for n in sorted(theirs)}
        env = dict(os.environ, LIPMPC_LIB=os.path.abspath(a.parent_lib))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--rounds", str(a.rounds), "--limit", str(a.limit)],
                           env=env, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit(f"the child ended with status {r.returncode}:\n{r.stderr[-2000:]}")
        line, = (ln for ln in r.stdout.splitlines() if ln.startswith("CHILD_JSON "))
        parent = dict(run=True, every_kernel_of_the_parent_has_the_same_figures_here=all(same.values()), kernels_compared=len(same),
                      kernels_that_differ=[n for n, ok in same.items() if not ok], kernels_new_here=sorted(set(mine) - set(theirs)),
                      figures_compared=list(FIGURES), **json.loads(line[len("CHILD_JSON "):]))
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: a timing taken elsewhere says nothing")
    calls, facts, keep = variants(selection())
    ms = FT.rounds_of(calls, a.reps, a.rounds)
    # -- the bar: at B = 16 on 362 x 362 the wave call takes at most a third of the lane call's time, the rounds apart -----------------
    bar = {}
    for kind in ("goal", "frontier"):
        for seg in (f"seg{CAPPED}", "nocap"):
            lane, wave = (ms[f"362x362_{kind}_B16_{seg}_path_{w}"] for w in ("lane", "wave"))
            bar[f"{kind}_{seg}"] = dict(lane_over_wave=lane["median"] / wave["median"], a_third_or_less=3.0 * wave["median"] <= lane["median"],
                                        rounds_do_not_overlap=wave["max"] < lane["min"])
    res = kernel_resources(lipmpc._lib.LIB_PATH)
    out = {"what": "ms per call, device events around `reps` back-to-back calls (1 where a call takes more than 50 ms), median / min / max over "
                   "alternating rounds, one process.  <map>_<kind>_B<robots>_<seg200|nocap>_path_<lane|wave>: the path call alone down one "
                   "shared settled field; _field_plus_path_: the planner's whole plan with paths=\"lane\" / \"wave\" and a fixed budget of "
                   "`rounds` rounds, no host synchronisation.  kind: goal / frontier = the tiled path calls, weighted = the weighted goal "
                   "path call, utility = the tiled utility path call",
           "device": torch.cuda.get_device_name(0), "reps_per_round": a.reps, "rounds": a.rounds, "r_clear": R_CLEAR, "w_clear": W_CLEAR,
           "informed": INFORMED, "S_max": S_MAX, "facts": facts, "ms_per_call": ms, "bar_362x362_B16": bar,
           "wave_kernels": {n: {f: r.get(f) for f in FIGURES} for n, r in res.items() if "wavewalk_" in n}, "parent_library": parent}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(dict(bar=bar, parent={k: v for k, v in parent.items() if k not in ("ms_per_call", "facts")}), indent=1))


if __name__ == "__main__":
    main()
