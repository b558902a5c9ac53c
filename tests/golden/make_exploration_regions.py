"""Frontier regions as the gain and representatives as the targets against the ray-marched gain and nearest-frontier exploration,
with the walker in the loop, recorded on the CPU (tests/golden/EXPLORATION_REGIONS.md):

    python tests/golden/make_exploration_regions.py [--write]

The CPU chain of UnknownEnvFleet.run_exploring as make_exploration_gain_kept.py builds it, from the committed oracles only, with
``recover`` = 6 and that file's parameters, on its two scenes and per noise seed once per rule:
  nearest                  every replan is tests/frontier_oracle.py's plan_batch (FrontierPlanner)
  informed by view         every replan is tests/gain_oracle.py's plan_batch (InformedFrontierPlanner) at R_VIEW, W_GAIN, G_CAP, MIN_GAIN
  informed by region       the same plan fed tests/regions_oracle.py's size as the gain (gain_from="region"; min_size = max(MIN_GAIN, 1))
  region + representative  ... and its rep in the place of the frontier (target="representative")
  kept region + rep r/q/s  every replan is tests/assign_keep_utility_oracle.py's plan_batch (GainKeepFrontierPlanner with both options,
                           r_keep = r, keep_ratio16 = q, keep_slack = s), the previous replan's FOUND targets as prev_target
A JUMP is a robot whose target is FOUND at this replan and at the previous one and lies more than JUMP_RADIUS cells from it.
Prints the table; --write records the counts as exploration_regions.npz and the tables as EXPLORATION_REGIONS.md.  Nothing is
asserted in advance: the tables say what came out.
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
import assign_keep_oracle as AK  # noqa: E402
import assign_keep_utility_oracle as KU  # noqa: E402
import assign_utility_oracle as AU  # noqa: E402
import frontier_oracle as FR  # noqa: E402
import gain_oracle as GO  # noqa: E402
import grid_lidar_oracle as G  # noqa: E402
import lidar_oracle as L  # noqa: E402
import lidar_split_oracle as S  # noqa: E402
import lipmpc_oracle as O  # noqa: E402
import make_exploration as E  # noqa: E402
import make_exploration_kept as EK  # noqa: E402
import map_oracle as M  # noqa: E402
import recover_oracle as RO  # noqa: E402
import regions_oracle as RG  # noqa: E402

W, H, ORIGIN, CELL = E.W, E.H, E.ORIGIN, E.CELL
LIDAR_RANGE, RESOLUTION, N_OBS_MAX, V_MAX = E.LIDAR_RANGE, E.RESOLUTION, E.N_OBS_MAX, E.V_MAX
NOISE_STD, STOP_OBJ, W_HIT, W_MISS = E.NOISE_STD, E.STOP_OBJ, E.W_HIT, E.W_MISS
R_INFLATE, MIN_UNKNOWN, REPLAN_EVERY, LOOKAHEAD = E.R_INFLATE, E.MIN_UNKNOWN, E.REPLAN_EVERY, E.LOOKAHEAD
SEEDS, SOLVED, MAX_RECOVER, R_CLAIM, MAX_CLAIMS, JUMP_RADIUS = EK.SEEDS, EK.SOLVED, EK.MAX_RECOVER, EK.R_CLAIM, EK.MAX_CLAIMS, EK.JUMP_RADIUS
R_VIEW, W_GAIN, G_CAP, MIN_GAIN = 15, 16, 120, 0
KEEP = (6, 24, 8)                                             # (r_keep, keep_ratio16, keep_slack): EXPLORATION_GAIN_KEPT.md's tight one
R_MAX = 1024                                                  # the planners' table rows
RULES = ("nearest", "informed by view", "informed by region", "region + representative", "kept region + rep %d/%d/%d" % KEEP)
SCENES = EK.SCENES


def chain(args):
    """One exploring run.  args = (scene, rule, seed)."""
    scene, rule, seed = args
    sc = SCENES[scene]
    starts, k_max = sc["starts"], sc["k_max"]
    min_gain = MIN_GAIN
    keep = tuple(int(v) for v in rule.split()[-1].split("/")) if "/" in rule else None
    B = len(starts)
    occ, table = sc["occ"](), L.ray_table(RESOLUTION)
    noise = NOISE_STD * np.random.default_rng(seed).standard_normal((k_max, B, RESOLUTION, 2))
    P = O.Params(N=3, tol_interior=1e-6)
    A, Bm = O.lip_matrices(P)
    state = np.array([[x, 0.0, y, 0.0, 0.0] for x, y in starts])
    foot = np.ones(B, int)
    working = state[:, (0, 2)].copy()
    walking, last_obj = np.ones(B, bool), np.full(B, math.inf)
    last_status, n_steps = np.zeros(B, int), np.zeros(B, int)
    run, n_rec = np.zeros(B, int), np.zeros(B, int)
    ev = np.zeros((W, H), np.int64)
    prev = np.full(B, -1, np.int64)                           # the last replan's FOUND targets: every rule's, for the jumps
    n_replans, finished_at, n_claims, n_kept, n_jumps, n_failed_solves = 0, -1, [], [], [], 0

    def scan(b, nz):
        pos = state[b, (0, 2)]
        hits, valid = G.grid_hits(pos, occ, ORIGIN, CELL, LIDAR_RANGE, table)
        h = np.full((RESOLUTION, 2), np.nan)
        h[valid] = (hits + nz)[valid] if nz is not None else hits[valid]
        return h, valid, G.in_solid_cell(pos, occ, ORIGIN, CELL)

    def plan():
        pos = state[:, (0, 2)]
        if rule == "nearest":
            return FR.plan_batch(ev, W_MISS, W_HIT, ORIGIN, CELL, pos, R_INFLATE, MIN_UNKNOWN, None, 64)
        if rule == "informed by view":
            return GO.plan_batch(ev, W_MISS, W_HIT, ORIGIN, CELL, pos, R_VIEW, W_GAIN, G_CAP, min_gain, R_INFLATE, MIN_UNKNOWN, None, 64)
        near = FR.plan_batch(ev, W_MISS, W_HIT, ORIGIN, CELL, pos, R_INFLATE, MIN_UNKNOWN, None, 64)
        reg = RG.regions_batch(near["frontier"], max(min_gain, 1), R_MAX)
        if rule != "informed by region":                       # representatives stand where the calls take the frontier
            near = dict(near, frontier=reg["rep"])
        informed = GO.plan_batch(ev, W_MISS, W_HIT, ORIGIN, CELL, pos, 1, W_GAIN, G_CAP, min_gain, R_INFLATE, MIN_UNKNOWN, None, 64,
                                 gain=reg["size"], nearest=near)
        if keep is None:
            return informed
        return KU.plan_batch(ev, W_MISS, W_HIT, ORIGIN, CELL, pos, R_CLAIM, 1, W_GAIN, G_CAP, prev, *keep, min_gain, MAX_CLAIMS,
                             R_INFLATE, MIN_UNKNOWN, None, 64, may_claim=np.isin(last_status, SOLVED), informed=informed)

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
            n_claims.append(int(pl.get("n_claims", 0)))
            n_kept.append(int(pl.get("n_kept", 0)))
            tc, found = pl["target_cell"].astype(np.int64), pl["status"] == FR.FOUND
            d2 = (tc // H - prev // H) ** 2 + (tc % H - prev % H) ** 2
            n_jumps.append(int((found & (prev >= 0) & (d2 > JUMP_RADIUS ** 2)).sum()))
            prev = np.where(found, tc, -1)
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
            ss = S.split_scan(h, valid, sc["split"], N_OBS_MAX, V_MAX)
            overflow = solid or bool(ss["overflow"])
            rings = ss["rings"] or []
            r = O.plan_step(state[b], working[b], int(foot[b]), rings, 0.0, P, exact=False)
            last_status[b] = 5 if overflow else r["status"]
            if last_status[b] in SOLVED:
                last_obj[b] = r["obj"]
                state[b] = np.concatenate([A @ state[b, :4] + Bm @ r["U"][0], [r["theta"][1]]])
                foot[b], n_steps[b], run[b] = -foot[b], n_steps[b] + 1, 0
                continue
            n_failed_solves += 1
            # the rule of lipmpc_fleet_recover_update_batch (tests/recover_oracle.py)
            if last_status[b] in (RO.INFEASIBLE, RO.MAX_ITER) and run[b] < MAX_RECOVER and np.all(np.isfinite(state[b, :4])):
                pos = state[b, (0, 2)]
                rows = np.array([np.concatenate(O.closest_point_and_normal(pos, ring)[:2]) for ring in rings]).reshape(-1, 4)
                if RO.safety_margin(RO.capture_point(state[b], P.beta), rows, 0.0) >= 0.0:
                    state[b] = RO.capture_advance(state[b].copy(), working[b], P)[2]
                    foot[b], run[b], n_rec[b] = -foot[b], run[b] + 1, n_rec[b] + 1
                    continue
            walking[b] = False                                 # final
    pl = plan()
    assign(pl, True)
    left = int(pl["n_frontier"][0])
    if left == 0 and finished_at < 0:
        finished_at = k_max
    failed = ~np.isin(last_status, SOLVED)
    return dict(scene=scene, rule=rule, seed=seed, finished=left == 0, finished_at=finished_at if left == 0 else -1,
                coverage=E.coverage(ev, occ), n_failed=int(failed.sum()), n_failed_solves=n_failed_solves, n_recover=int(n_rec.sum()),
                n_replans=n_replans, n_claims=int(sum(n_claims)), n_kept=int(sum(n_kept)), n_jumps=int(sum(n_jumps)))


COUNTS = ("finished_at", "n_failed_solves", "n_recover", "n_jumps", "n_kept", "n_claims", "n_failed")


def rows_of(rows, scene, rule):
    return sorted((x for x in rows if x["scene"] == scene and x["rule"] == rule), key=lambda x: x["seed"])


def markdown(rows):
    out = ["# Frontier regions as gain and target against the ray-marched gain and the nearest frontier", "",
           "Written by `tests/golden/make_exploration_regions.py --write`; the rule is stated in `include/lipmpc.h`",
           "(`lipmpc_grid_frontier_regions_batch`) and restated in `tests/regions_oracle.py`; DESIGN.md §25.", "",
           f"One CPU chain of `UnknownEnvFleet.run_exploring` per scene, rule and noise seed, `recover` = {MAX_RECOVER}, `r_claim` = {R_CLAIM},",
           f"`max_claims` = {MAX_CLAIMS}, `r_view` = {R_VIEW} (by view only), `w_gain` = {W_GAIN}, `g_cap` = {G_CAP}, `min_gain` = {MIN_GAIN} (so min_size = "
           f"{max(MIN_GAIN, 1)}), `R_max` = {R_MAX}; the numbers after `kept region + rep` are `r_keep`/`keep_ratio16`/`keep_slack`.",
           "FINISHED AT = the first replan sample that finds no frontier cell left (-1: never within `k_max`); FAILED SOLVES = solves that",
           "ended neither SOLVED nor UNCERTIFIED, summed over the robots; JUMPS = over all replans the robots whose target is FOUND at this",
           f"replan and the previous one and lies more than {JUMP_RADIUS} cells from it; LOST = robots whose last status is a failure.", ""]
    for scene, sc in SCENES.items():
        out += [f"## {scene}: {len(sc['starts'])} robots at {list(sc['starts'])}, `k_max` = {sc['k_max']}, `split_rays` = {sc['split']}", "",
                "| rule | seed | finished at | failed solves | jumps | lost | capture steps | keeps | coverage |",
                "|---|---|---|---|---|---|---|---|---|"]
        for rule in RULES:
            for x in rows_of(rows, scene, rule):
                out.append(f"| {rule} | {x['seed']} | {x['finished_at']} | {x['n_failed_solves']} | {x['n_jumps']} | {x['n_failed']} | "
                           f"{x['n_recover']} | {x['n_kept']} | {x['coverage']:.4f} |")
        out += ["", "Over the six seeds:", "",
                "| rule | finished (of 6) | finishing samples | failed solves | jumps | lost | least coverage |",
                "|---|---|---|---|---|---|---|"]
        for rule in RULES:
            rs = rows_of(rows, scene, rule)
            out.append(f"| {rule} | {sum(x['finished'] for x in rs)} | {[x['finished_at'] for x in rs]} | {sum(x['n_failed_solves'] for x in rs)} | "
                       f"{sum(x['n_jumps'] for x in rs)} | {sum(x['n_failed'] for x in rs)} | {min(x['coverage'] for x in rs):.4f} |")
        out.append("")
    out += ["Six seeds of two scenes are what was run, recorded as it came; nothing here makes a parameter a default, and no test asserts",
            "that a rule finishes sooner.", ""]
    return "\n".join(out)


def main():
    jobs = [(sc, r, s) for sc in SCENES for r in RULES for s in SEEDS]
    with Pool(min(12, os.cpu_count() or 1)) as pool:
        rows = pool.map(chain, jobs, chunksize=1)
    text = markdown(rows)
    print(text)
    if "--write" in sys.argv:
        rec = {"seeds": np.array(SEEDS), "gain": np.array((R_VIEW, W_GAIN, G_CAP, MIN_GAIN)), "keep": np.array(KEEP), "r_max": R_MAX, "jump_radius": JUMP_RADIUS,
               "max_recover": MAX_RECOVER, "r_claim": R_CLAIM, "max_claims": MAX_CLAIMS, "rules": np.array(RULES)}
        for scene in SCENES:
            for key in COUNTS + ("coverage",):
                rec[f"{scene}/{key}"] = np.array([[x[key] for x in rows_of(rows, scene, rule)] for rule in RULES])
        np.savez(os.path.join(HERE, "exploration_regions.npz"), **rec)
        with open(os.path.join(HERE, "EXPLORATION_REGIONS.md"), "w") as f:
            f.write(text)
        print("recorded", list(SEEDS))


if __name__ == "__main__":
    main()
