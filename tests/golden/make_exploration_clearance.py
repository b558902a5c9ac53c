"""Does soft clearance make the walker fail less?  CPU chains, recorded as tests/golden/EXPLORATION_CLEARANCE.md:

    python tests/golden/make_exploration_clearance.py [--write] [--scenes=rooms,open]

The chains of make_exploration_rooms.py (the three rooms, split_rays 60, 160 samples) and of make_exploration.py (the open field, one
hull per cluster, 100 samples), built from the committed oracles only, with ONE thing varied: how the nearest-frontier plan keeps
its paths off the walls.  Per scene and noise seed one chain per SETTING:
  r_inflate 3                     the recorded setting of both scenes (the hard disc alone)
  r_inflate 1, r_inflate 2        the hard disc alone, smaller
  r_inflate 1 or 2 + (r_clear, w_clear)   the hard disc, smaller, plus the clearance layer of tests/clearance_oracle.py: the weighted
                                  frontier field and the weighted walk (lipmpc_grid_frontier_field_weighted_batch and its path call)
Reported per setting: the chains that finish (the closing plan finds no frontier cell) and the sample at which they do, the robots
LOST (a failed solve is final in these chains: failed solves per robot are 0 or 1) and the sample at which each was, the coverage,
and the least and the mean distance, in cells, from the robots' positions after every step to the centre of the nearest solid cell
of the TRUE map.  Nothing is chosen here and nothing is claimed beyond the table.
"""
import math
import os
import sys
import time
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (HERE, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
import clearance_oracle as CO  # noqa: E402
import frontier_oracle as FR  # noqa: E402
import grid_lidar_oracle as G  # noqa: E402
import lidar_oracle as L  # noqa: E402
import lidar_split_oracle as S  # noqa: E402
import lipmpc_oracle as O  # noqa: E402
import make_exploration as E  # noqa: E402
import make_exploration_rooms as R  # noqa: E402
import map_oracle as M  # noqa: E402

W, H, ORIGIN, CELL, STARTS = E.W, E.H, E.ORIGIN, E.CELL, E.STARTS
SEEDS = tuple(range(6))
CLEAR = ((4, 40), (6, 40), (6, 120))                          # (r_clear, w_clear): 40 = the two-door example's weight, 8 cells of detour
SETTINGS = ((3, None), (1, None), (2, None)) + tuple((r, c) for r in (1, 2) for c in CLEAR)
SCENES = {"rooms": dict(occ=R.true_map, split=R.SPLIT_RAYS, k_max=R.K_MAX, noise=R.noise_of),
          "open": dict(occ=E.true_map, split=0, k_max=E.K_MAX, noise=E.noise_of)}
SOLVED = E.SOLVED


def name_of(setting):
    r, clear = setting
    return f"r_inflate {r}" + ("" if clear is None else f" + r_clear {clear[0]}, w_clear {clear[1]}")


def wall_distance(points, occ):
    """Per point [n,2] the distance in cells to the centre of the nearest solid cell of ``occ``."""
    solid = np.argwhere(occ != 0) + 0.5
    p = (np.asarray(points).reshape(-1, 2) - np.array(ORIGIN)) / np.array(CELL)
    return np.sqrt(((p[:, None, :] - solid[None, :, :]) ** 2).sum(-1)).min(1)


def chain(args):
    """One exploring run: make_exploration_rooms.py's chain, the plan by the setting.  args = (scene, seed, setting)."""
    scene, seed, (r_inflate, clear) = args
    sc = SCENES[scene]
    occ, table, noise, k_max, split = sc["occ"](), L.ray_table(E.RESOLUTION), sc["noise"](seed), sc["k_max"], sc["split"]
    P = O.Params(N=3, tol_interior=1e-6)
    A, Bm = O.lip_matrices(P)
    B = len(STARTS)
    state = np.array([[x, 0.0, y, 0.0, 0.0] for x, y in STARTS])
    foot = np.ones(B, int)
    working = state[:, (0, 2)].copy()
    walking, last_obj = np.ones(B, bool), np.full(B, math.inf)
    last_status, n_steps, lost_at = np.zeros(B, int), np.zeros(B, int), np.full(B, -1)
    ev = np.zeros((W, H), np.int64)
    finished_at, walked = -1, []

    def scan(b, nz):
        pos = state[b, (0, 2)]
        hits, valid = G.grid_hits(pos, occ, ORIGIN, CELL, E.LIDAR_RANGE, table)
        h = np.full((E.RESOLUTION, 2), np.nan)
        h[valid] = (hits + nz)[valid] if nz is not None else hits[valid]
        return h, valid, G.in_solid_cell(pos, occ, ORIGIN, CELL)

    def plan():
        if clear is None:
            return FR.plan_batch(ev, E.W_MISS, E.W_HIT, ORIGIN, CELL, state[:, (0, 2)], r_inflate, E.MIN_UNKNOWN, None, 64)
        layer = CO.clearance_cost_evidence(ev, E.W_HIT, *clear)
        return CO.frontier_plan_batch(ev, layer, E.W_MISS, E.W_HIT, ORIGIN, CELL, state[:, (0, 2)], r_inflate, E.MIN_UNKNOWN, None, 64)

    def assign(pl, closing):
        nonlocal working, walking, last_obj
        found = pl["status"] == FR.FOUND
        solved = np.isin(last_status, SOLVED)
        if not closing:
            resume = ~walking & solved & found
            walking = walking | resume
            last_obj = np.where(resume, math.inf, last_obj)
            sub = np.zeros((B, max(1, int(pl["n_sub"].max())), 2))
            for b in range(B):
                sub[b, :pl["n_sub"][b]] = pl["sub_goals"][b]
            picked = M.select_goals(state[:, (0, 2)], pl["target"], sub, pl["n_sub"], pl["status"], E.LOOKAHEAD)
            working = np.where(found[:, None], picked, working)
        walking = walking & found

    for k in range(k_max):
        if k % E.REPLAN_EVERY == 0:
            if k == 0:
                first = np.stack([scan(b, None)[0] for b in range(B)])
                M.update(ev, state[:, (0, 2)], first, ORIGIN, CELL, E.LIDAR_RANGE, table, w_hit=E.W_HIT, w_miss=E.W_MISS)
            pl = plan()
            assign(pl, False)
            if pl["n_frontier"][0] == 0 and finished_at < 0:
                finished_at = k
        if not walking.any() and finished_at >= 0:
            break
        scans = [scan(b, noise[k, b]) for b in range(B)]
        M.update(ev, state[:, (0, 2)], np.stack([s[0] for s in scans]), ORIGIN, CELL, E.LIDAR_RANGE, table, w_hit=E.W_HIT, w_miss=E.W_MISS,
                 mask=walking.astype(int))
        for b in range(B):
            walking[b] = walking[b] and last_obj[b] >= E.STOP_OBJ
            if not walking[b]:
                continue
            h, valid, solid = scans[b]
            cut = S.split_scan(h, valid, split, E.N_OBS_MAX, E.V_MAX)
            overflow = solid or bool(cut["overflow"])
            r = O.plan_step(state[b], working[b], int(foot[b]), cut["rings"] or [], 0.0, P, exact=False)
            last_status[b] = 5 if overflow else r["status"]
            if last_status[b] not in SOLVED:
                walking[b], lost_at[b] = False, k              # a failed solve is final
                continue
            last_obj[b] = r["obj"]
            state[b] = np.concatenate([A @ state[b, :4] + Bm @ r["U"][0], [r["theta"][1]]])
            foot[b], n_steps[b] = -foot[b], n_steps[b] + 1
            walked.append(state[b, (0, 2)].copy())
    pl = plan()
    assign(pl, True)
    left = int(pl["n_frontier"][0])
    if left == 0 and finished_at < 0:
        finished_at = k_max
    dist = wall_distance(walked, occ) if walked else np.array([np.nan])
    return dict(scene=scene, seed=seed, setting=(r_inflate, clear), lost=int((~np.isin(last_status, SOLVED)).sum()), lost_at=lost_at.tolist(),
                finished=left == 0, finished_at=finished_at, frontier_left=left, coverage=E.coverage(ev, occ), n_steps=n_steps.tolist(),
                last_status=last_status.tolist(), least=float(dist.min()), mean=float(dist.mean()))


def rows_of(rows, scene, setting):
    return [x for x in rows if x["scene"] == scene and x["setting"] == setting]


def table_of(rows, scene):
    out = ["| setting | finished | finished at sample, per seed | robots lost (of 18) | lost at sample, per seed | steps walked min-max | coverage min-max | "
           "least distance to a solid cell (cells) | mean distance (cells) |", "|---|---|---|---|---|---|---|---|---|"]
    for setting in SETTINGS:
        rs = rows_of(rows, scene, setting)
        if not rs:
            continue
        steps, cov = np.array([x["n_steps"] for x in rs]), [x["coverage"] for x in rs]
        out.append(f"| {name_of(setting)} | {sum(x['finished'] for x in rs)} of {len(rs)} | {[x['finished_at'] for x in rs]} | "
                   f"{sum(x['lost'] for x in rs)} | {[[a for a in x['lost_at'] if a >= 0] for x in rs]} | {steps.min()}-{steps.max()} | "
                   f"{min(cov):.4f}-{max(cov):.4f} | {min(x['least'] for x in rs):.2f} | {np.mean([x['mean'] for x in rs]):.2f} |")
    return out


def markdown(rows, scenes, left_out):
    out = ["# Exploring with soft clearance: what the CPU chains show", "",
           "Written by `tests/golden/make_exploration_clearance.py --write`.  The contracts are stated in `include/lipmpc.h` (SOFT CLEARANCE)",
           "and restated in `tests/clearance_oracle.py`; the chains are those of `make_exploration_rooms.py` (three rooms, `split_rays`",
           f"{R.SPLIT_RAYS}, {R.K_MAX} samples) and `make_exploration.py` (open field, {E.K_MAX} samples) with the plan by the setting of the row.",
           f"Seeds {list(SEEDS)}, three robots, so 18 robots per row.  FINISHED = the closing plan finds no frontier cell.  A robot is LOST",
           "when a solve fails: that is final in these chains (no `recover`).  Coverage counts the cells that are reachable at",
           f"`r_inflate` {E.R_INFLATE} on the true map, whatever the row's own radius, so the rows compare.  Distances are from the robots' positions after",
           "every step to the centre of the nearest solid cell of the true map, in cells.", ""]
    for scene in scenes:
        out += [f"## {'The three rooms' if scene == 'rooms' else 'The open field'}", ""] + table_of(rows, scene) + [""]
        lost = {setting: sum(x["lost"] for x in rows_of(rows, scene, setting)) for setting in SETTINGS}
        done = {setting: sum(x["finished"] for x in rows_of(rows, scene, setting)) for setting in SETTINGS}
        best = min((s for s in SETTINGS if s[1] is not None), key=lambda s: (lost[s], -done[s]))
        out += [f"Read off the table: with clearance the fewest robots lost is {lost[best]} ({name_of(best)}, {done[best]} of {len(SEEDS)} finished), against "
                f"{lost[3, None]} at `r_inflate` 3 alone ({done[3, None]} of {len(SEEDS)} finished), {lost[1, None]} at `r_inflate` 1 alone and {lost[2, None]} at "
                f"`r_inflate` 2 alone.  " + ("Clearance loses FEWER robots than the recorded hard disc here." if lost[best] < lost[3, None] else
                                            "Clearance is NO BETTER than the recorded hard disc here: it repairs part of what the smaller disc "
                                            "breaks and no more."), ""]
    if left_out:
        out += [f"Not run: {', '.join(left_out)}.", ""]
    out += ["Nothing here is a tuned setting: the three (`r_clear`, `w_clear`) pairs were written down before the chains ran (40 is the",
            "two-door example's weight, DESIGN section 20) and none was tried and dropped.", ""]
    return "\n".join(out)


def main():
    scenes = ["rooms", "open"]
    for a in sys.argv[1:]:
        if a.startswith("--scenes="):
            scenes = a.split("=", 1)[1].split(",")
    jobs = [(scene, s, setting) for scene in scenes for setting in SETTINGS for s in SEEDS]
    t0 = time.time()
    with Pool(min(16, os.cpu_count() or 1)) as pool:
        rows = pool.map(chain, jobs, chunksize=1)
    print(f"{len(jobs)} chains in {time.time() - t0:.0f} s")
    for scene in scenes:
        print("\n".join(table_of(rows, scene)))
        for x in (x for x in rows if x["scene"] == scene):
            print(f"   {scene} {name_of(x['setting'])} seed {x['seed']}: finished {x['finished']} at {x['finished_at']}, lost {x['lost']} at {x['lost_at']}, "
                  f"coverage {x['coverage']:.4f}, steps {x['n_steps']}, last status {x['last_status']}, frontier left {x['frontier_left']}, "
                  f"least {x['least']:.2f}, mean {x['mean']:.2f}")
    if "--write" in sys.argv:
        with open(os.path.join(HERE, "EXPLORATION_CLEARANCE.md"), "w") as f:
            f.write(markdown(rows, scenes, [f"the {s} scene" for s in SCENES if s not in scenes]))
        print("recorded", scenes)


if __name__ == "__main__":
    main()
