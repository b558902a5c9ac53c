"""Recovery from a failed solve, chosen and recorded on the CPU (tests/golden/EXPLORATION_RECOVER.md):

    python tests/golden/make_exploration_recover.py [--write]

The CPU chain of UnknownEnvFleet.run_exploring as make_exploration.py / make_exploration_rooms.py build it, from the committed
oracles only, with the fleet update of tests/recover_oracle.py (lipmpc_fleet_recover_update_batch): a robot whose solve ends
INFEASIBLE or MAX_ITER takes a capture step if its capture point respects every row the sample sensed, at most RECOVER samples
in a row.  Scenes: the open field of make_exploration.py at its chosen settings from three other start sets on which, without
recovery, at least one robot per seed ends in a failed solve (start sets that do not show that on every seed -- (0.8, 2.3) (0.8, 2.8)
(0.8, 3.3) and (0.6, 0.6) (1.1, 0.6) (0.6, 1.1) lose a robot on five and on three of the six seeds -- were replaced by their
nearest neighbours that do), and from a fourth, field_rest, on which one robot's solve fails near rest and recovery does not help;
and the three rooms of make_exploration_rooms.py at its chosen
split_rays.  One chain per scene, seed and RECOVER in (0, 6).  Prints the tables; --write records the settings, the seeds and
the counts as exploration_recover.npz and the tables as EXPLORATION_RECOVER.md.
"""
import math
import os
import sys
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (HERE, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
import frontier_oracle as FR  # noqa: E402
import grid_lidar_oracle as G  # noqa: E402
import lidar_oracle as L  # noqa: E402
import lidar_split_oracle as S  # noqa: E402
import lipmpc_oracle as O  # noqa: E402
import make_exploration as E  # noqa: E402
import make_exploration_rooms as R  # noqa: E402
import map_oracle as M  # noqa: E402
import recover_oracle as RO  # noqa: E402

W, H, ORIGIN, CELL = E.W, E.H, E.ORIGIN, E.CELL
LIDAR_RANGE, RESOLUTION, N_OBS_MAX, V_MAX = E.LIDAR_RANGE, E.RESOLUTION, E.N_OBS_MAX, E.V_MAX
NOISE_STD, STOP_OBJ, W_HIT, W_MISS = E.NOISE_STD, E.STOP_OBJ, E.W_HIT, E.W_MISS
R_INFLATE, MIN_UNKNOWN, REPLAN_EVERY, LOOKAHEAD = E.R_INFLATE, E.MIN_UNKNOWN, E.REPLAN_EVERY, E.LOOKAHEAD
SEEDS = tuple(range(6))
RECOVERS = (0, 6)
MAX_RECOVER = 6
SOLVED = E.SOLVED
# name -> (map, split_rays, k_max, starts)
SCENES = {
    "field_edge": ("field", 0, E.K_MAX, ((1.0, 2.3), (1.0, 2.8), (1.0, 3.3))),
    "field_corner": ("field", 0, E.K_MAX, ((0.6, 0.6), (1.0, 0.6), (0.6, 1.0))),
    "field_middle": ("field", 0, E.K_MAX, ((3.2, 2.8), (3.2, 2.3), (3.2, 3.3), (2.7, 2.8))),
    "field_rest": ("field", 0, E.K_MAX, ((0.8, 0.8), (1.3, 0.8), (0.8, 1.3))),
    "rooms": ("rooms", R.SPLIT_RAYS, R.K_MAX, R.STARTS),
}


def true_map(which):
    return E.true_map() if which == "field" else R.true_map()


def noise_of(seed, k_max, B):
    """The readings' noise of a seed, [k_max, B, RESOLUTION, 2]: what the GPU test hands the fleet as its given noise."""
    return NOISE_STD * np.random.default_rng(seed).standard_normal((k_max, B, RESOLUTION, 2))


def chain(args):
    """One exploring run.  args = (scene name, seed, max_recover)."""
    name, seed, max_recover = args
    which, split, k_max, starts = SCENES[name]
    B = len(starts)
    occ, table, noise = true_map(which), L.ray_table(RESOLUTION), noise_of(seed, k_max, B)
    P = O.Params(N=3, tol_interior=1e-6)
    A, Bm = O.lip_matrices(P)
    state = np.array([[x, 0.0, y, 0.0, 0.0] for x, y in starts])
    foot = np.ones(B, int)
    working = state[:, (0, 2)].copy()
    walking, last_obj = np.ones(B, bool), np.full(B, math.inf)
    last_status, n_steps = np.zeros(B, int), np.zeros(B, int)
    run, n_rec, longest, least, refused = np.zeros(B, int), np.zeros(B, int), 0, math.inf, np.zeros(B, bool)
    ev = np.zeros((W, H), np.int64)
    n_replans, finished_at = 0, -1

    def scan(b, nz):
        pos = state[b, (0, 2)]
        hits, valid = G.grid_hits(pos, occ, ORIGIN, CELL, LIDAR_RANGE, table)
        h = np.full((RESOLUTION, 2), np.nan)
        h[valid] = (hits + nz)[valid] if nz is not None else hits[valid]
        return h, valid, G.in_solid_cell(pos, occ, ORIGIN, CELL)

    def plan():
        return FR.plan_batch(ev, W_MISS, W_HIT, ORIGIN, CELL, state[:, (0, 2)], R_INFLATE, MIN_UNKNOWN, None, 64)

    def assign(pl, closing):
        nonlocal working, walking, last_obj
        found = pl["status"] == FR.FOUND
        solved = np.isin(last_status, SOLVED)
        if not closing:
            resume = ~walking & solved & found
            walking = walking | resume
            last_obj = np.where(resume, math.inf, last_obj)
            n_slots = max(1, int(pl["n_sub"].max()))
            sub = np.zeros((B, n_slots, 2))
            for b in range(B):
                sub[b, :pl["n_sub"][b]] = pl["sub_goals"][b]
            picked = M.select_goals(state[:, (0, 2)], pl["target"], sub, pl["n_sub"], pl["status"], LOOKAHEAD)
            working = np.where(found[:, None], picked, working)
        walking = walking & found

    for k in range(k_max):
        if k % REPLAN_EVERY == 0:
            if k == 0:                                         # the first look round, noise-free
                first = np.stack([scan(b, None)[0] for b in range(B)])
                M.update(ev, state[:, (0, 2)], first, ORIGIN, CELL, LIDAR_RANGE, table, w_hit=W_HIT, w_miss=W_MISS)
            pl = plan()
            assign(pl, False)
            n_replans += 1
            if pl["n_frontier"][0] == 0 and finished_at < 0:
                finished_at = k
        if not walking.any() and finished_at >= 0:
            break
        scans = [scan(b, noise[k, b]) for b in range(B)]
        M.update(ev, state[:, (0, 2)], np.stack([s[0] for s in scans]), ORIGIN, CELL, LIDAR_RANGE, table, w_hit=W_HIT, w_miss=W_MISS,
                 mask=walking.astype(int))
        for b in range(B):
            walking[b] = walking[b] and last_obj[b] >= STOP_OBJ
            if not walking[b]:
                continue
            h, valid, solid = scans[b]
            sc = S.split_scan(h, valid, split, N_OBS_MAX, V_MAX)
            overflow = solid or bool(sc["overflow"])
            rings = sc["rings"] or []
            r = O.plan_step(state[b], working[b], int(foot[b]), rings, 0.0, P, exact=False)
            last_status[b] = 5 if overflow else r["status"]
            if last_status[b] in SOLVED:
                last_obj[b] = r["obj"]
                state[b] = np.concatenate([A @ state[b, :4] + Bm @ r["U"][0], [r["theta"][1]]])
                foot[b], n_steps[b], run[b] = -foot[b], n_steps[b] + 1, 0
                continue
            # the rule of lipmpc_fleet_recover_update_batch (tests/recover_oracle.py)
            if last_status[b] in (RO.INFEASIBLE, RO.MAX_ITER) and run[b] < max_recover and np.all(np.isfinite(state[b, :4])):
                pos = state[b, (0, 2)]
                rows = np.array([np.concatenate(O.closest_point_and_normal(pos, ring)[:2]) for ring in rings]).reshape(-1, 4)
                margin = RO.safety_margin(RO.capture_point(state[b], P.beta), rows, 0.0)
                least = min(least, margin) if margin == margin else -math.inf
                if margin >= 0.0:
                    state[b] = RO.capture_advance(state[b].copy(), working[b], P)[2]
                    foot[b], run[b], n_rec[b] = -foot[b], run[b] + 1, n_rec[b] + 1
                    longest = max(longest, int(run[b]))
                    continue
                refused[b] = True
            walking[b] = False                                 # final
    pl = plan()
    assign(pl, True)
    left = int(pl["n_frontier"][0])
    if left == 0 and finished_at < 0:
        finished_at = k_max
    failed = ~np.isin(last_status, SOLVED)
    return dict(scene=name, seed=seed, recover=max_recover, n_failed=int(failed.sum()), failed=failed.tolist(), finished=left == 0,
                finished_at=finished_at, frontier_left=left, coverage=E.coverage(ev, occ), n_steps=n_steps.tolist(),
                last_status=last_status.tolist(), n_recover=n_rec.tolist(), longest_run=longest, least_margin=least,
                n_refused=int(refused.sum()), n_replans=n_replans, final=np.round(state[:, (0, 2)], 2).tolist())


def rows_of(rows, scene, recover):
    return sorted((x for x in rows if x["scene"] == scene and x["recover"] == recover), key=lambda x: x["seed"])


def kept(rows, scene):
    """Per seed: does the chain without recovery lose a robot that the chain with recovery keeps?"""
    return [bool(np.any(np.array(a["failed"]) & ~np.array(b["failed"])))
            for a, b in zip(rows_of(rows, scene, 0), rows_of(rows, scene, MAX_RECOVER))]


def markdown(rows):
    out = ["# Recovering from a failed solve: the capture step", "",
           "Written by `tests/golden/make_exploration_recover.py --write`; the rule is stated in `include/lipmpc.h`",
           "(`lipmpc_fleet_recover_update_batch`) and restated in `tests/recover_oracle.py`; the argument for the step is in DESIGN.md.", "",
           "One CPU chain of `UnknownEnvFleet.run_exploring` per scene, noise seed and `recover` (0 = a failed solve is final, as before;",
           f"{MAX_RECOVER} = at most that many capture steps in a row).  The open-field scenes are `make_exploration.py`'s map and chosen settings",
           "from other start positions; `rooms` is `make_exploration_rooms.py`'s recorded scene at its chosen `split_rays`.  FAILED = robots",
           "whose last status is not SOLVED / UNCERTIFIED; REFUSED = robots stopped because their capture point violated a sensed row.", ""]
    for name, (which, split, k_max, starts) in SCENES.items():
        out += [f"## `{name}`: {which}, starts {list(starts)}, `split_rays` {split}, `k_max` {k_max}", "",
                "| recover | seed | failed robots | recovery samples per robot | longest run | least margin | refused | finished at | coverage |",
                "|---|---|---|---|---|---|---|---|---|"]
        for rec in RECOVERS:
            for x in rows_of(rows, name, rec):
                lm = "-" if x["least_margin"] == math.inf else f"{x['least_margin']:.4f}"
                out.append(f"| {rec} | {x['seed']} | {x['n_failed']} | {x['n_recover']} | {x['longest_run']} | {lm} | {x['n_refused']} | "
                           f"{x['finished_at']} | {x['coverage']:.4f} |")
        on = rows_of(rows, name, MAX_RECOVER)
        cov = np.array([x["coverage"] for x in on])
        out += ["", f"With recovery: failed robots per seed at most {max(x['n_failed'] for x in on)} (the bar of the GPU test; at most one seed may",
                f"exceed it), coverage {cov.min():.4f}-{cov.max():.4f}: the GPU bar is min - (max - min) = {cov.min() - (cov.max() - cov.min()):.4f}.",
                f"Without recovery a robot is lost that recovery keeps on seeds {[s for s, k in zip(SEEDS, kept(rows, name)) if k]}.", ""]
    longest = max(x["longest_run"] for x in rows)
    per = {name: max(x["longest_run"] for x in rows_of(rows, name, MAX_RECOVER)) for name in SCENES}
    short = max(v for n, v in per.items() if n != "field_rest")
    out += [f"Longest run of consecutive recovery samples per scene: {per}.  Wherever recovery keeps a robot, {short} capture step in a row is",
            "enough: the velocity falls to 0.285 of itself per capture step, and from (near) rest the step is feasible.  `field_rest` is the",
            f"other case, recorded for it: one robot, close to a block, takes all {MAX_RECOVER} capture steps on "
            f"{sum(x['longest_run'] == MAX_RECOVER for x in rows_of(rows, 'field_rest', MAX_RECOVER))} of {len(SEEDS)} seeds and its solve stays",
            "INFEASIBLE; it ends where it ended without recovery.  A robot whose solve fails at rest is not recovered by standing, so a larger",
            f"value buys nothing.  `recover` = {MAX_RECOVER}, the value the fleet documents, is margin over the {short} the other scenes need.", ""]
    return "\n".join(out)


def main():
    with Pool(min(16, os.cpu_count() or 1)) as pool:
        rows = pool.map(chain, [(n, s, r) for n in SCENES for r in RECOVERS for s in SEEDS], chunksize=1)
    for name in SCENES:
        for rec in RECOVERS:
            rs = rows_of(rows, name, rec)
            print(f"{name} recover {rec}: {sum(x['finished'] for x in rs)} of {len(rs)} finish, failed robots {[x['n_failed'] for x in rs]}")
            for x in rs:
                print(f"   seed {x['seed']}: finished {x['finished']} at {x['finished_at']}, coverage {x['coverage']:.4f}, steps {x['n_steps']}, last status "
                      f"{x['last_status']}, recoveries {x['n_recover']}, longest run {x['longest_run']}, least margin {x['least_margin']:.4g}, "
                      f"refused {x['n_refused']}, frontier left {x['frontier_left']}, at {x['final']}")
        print(f"{name}: recovery keeps a robot the plain chain loses, per seed: {kept(rows, name)}")
    if "--write" in sys.argv:
        for name, sc in SCENES.items():                        # the premise of a start set: without recovery every seed loses a robot
            assert sc[0] != "field" or all(x["n_failed"] >= 1 for x in rows_of(rows, name, 0)), name
        rec = {"seeds": np.array(SEEDS), "max_recover": MAX_RECOVER, "scenes": np.array(list(SCENES)), "grid": np.array([W, H]),
               "origin": np.array(ORIGIN), "cell": np.array(CELL), "lidar_range": LIDAR_RANGE, "noise_std": NOISE_STD,
               "weights": np.array([W_HIT, W_MISS]), "r_inflate": R_INFLATE, "min_unknown": MIN_UNKNOWN, "replan_every": REPLAN_EVERY,
               "lookahead": LOOKAHEAD, "door": np.array(R.DOOR), "coverage_start": np.array(E.STARTS[0]), "longest_run": max(x["longest_run"] for x in rows)}
        for name, (which, split, k_max, starts) in SCENES.items():
            rec.update({f"{name}/map": which, f"{name}/split_rays": split, f"{name}/k_max": k_max, f"{name}/starts": np.array(starts),
                        f"{name}/kept_every_seed": all(kept(rows, name))})
            for r in RECOVERS:
                rs = rows_of(rows, name, r)
                rec.update({f"{name}/r{r}/n_failed": np.array([x["n_failed"] for x in rs]),
                            f"{name}/r{r}/coverage": np.array([x["coverage"] for x in rs]),
                            f"{name}/r{r}/finished_at": np.array([x["finished_at"] for x in rs]),
                            f"{name}/r{r}/n_recover": np.array([x["n_recover"] for x in rs]),
                            f"{name}/r{r}/longest_run": np.array([x["longest_run"] for x in rs]),
                            f"{name}/r{r}/n_refused": np.array([x["n_refused"] for x in rs]),
                            f"{name}/r{r}/last_status": np.array([x["last_status"] for x in rs])})
        np.savez(os.path.join(HERE, "exploration_recover.npz"), **rec)
        with open(os.path.join(HERE, "EXPLORATION_RECOVER.md"), "w") as f:
            f.write(markdown(rows))
        print("recorded", list(SEEDS))


if __name__ == "__main__":
    main()
