"""Coordinated exploration against nearest-frontier exploration, chosen and recorded on the CPU
(tests/golden/EXPLORATION_ASSIGNED.md):

    python tests/golden/make_exploration_assigned.py [--write]

The CPU chain of UnknownEnvFleet.run_exploring as make_exploration_recover.py builds it, from the committed oracles only, on the
open field of make_exploration.py at its chosen settings, with ``recover`` = 6 (a working goal that jumps costs a capture step, not
the run).  The fleet starts SIDE BY SIDE, 0.2 m apart -- the start from which the nearest-frontier rule sends everybody to one spot
-- and is run twice per noise seed:
  nearest    every replan is tests/frontier_oracle.py's plan_batch (FrontierPlanner)
  assigned   every replan is tests/assign_oracle.py's plan_batch (CoordinatedFrontierPlanner: R_CLAIM, MAX_CLAIMS), the robots
             that may claim being those whose last status is SOLVED / UNCERTIFIED
Prints the table; --write records the settings, the seeds and the counts as exploration_assigned.npz and the tables as
EXPLORATION_ASSIGNED.md.
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
import assign_oracle as AS  # noqa: E402
import frontier_oracle as FR  # noqa: E402
import grid_lidar_oracle as G  # noqa: E402
import lidar_oracle as L  # noqa: E402
import lidar_split_oracle as S  # noqa: E402
import lipmpc_oracle as O  # noqa: E402
import make_exploration as E  # noqa: E402
import map_oracle as M  # noqa: E402
import recover_oracle as RO  # noqa: E402

W, H, ORIGIN, CELL = E.W, E.H, E.ORIGIN, E.CELL
LIDAR_RANGE, RESOLUTION, N_OBS_MAX, V_MAX = E.LIDAR_RANGE, E.RESOLUTION, E.N_OBS_MAX, E.V_MAX
NOISE_STD, STOP_OBJ, W_HIT, W_MISS, K_MAX = E.NOISE_STD, E.STOP_OBJ, E.W_HIT, E.W_MISS, E.K_MAX
R_INFLATE, MIN_UNKNOWN, REPLAN_EVERY, LOOKAHEAD = E.R_INFLATE, E.MIN_UNKNOWN, E.REPLAN_EVERY, E.LOOKAHEAD
SEEDS = tuple(range(6))
SOLVED = E.SOLVED
MAX_RECOVER = 6
R_CLAIM, MAX_CLAIMS = 15, 64
STARTS = ((0.8, 2.5), (0.8, 2.7), (0.8, 2.9), (0.8, 3.1))   # side by side along the edge the recorded scene starts from
RULES = ("nearest", "assigned")


def noise_of(seed, B=len(STARTS)):
    """The readings' noise of a seed, [K_MAX, B, RESOLUTION, 2]: what the GPU test hands the fleet as its given noise."""
    return NOISE_STD * np.random.default_rng(seed).standard_normal((K_MAX, B, RESOLUTION, 2))


def chain(args):
    """One exploring run.  args = (rule, seed)."""
    rule, seed = args
    B = len(STARTS)
    occ, table, noise = E.true_map(), L.ray_table(RESOLUTION), noise_of(seed)
    P = O.Params(N=3, tol_interior=1e-6)
    A, Bm = O.lip_matrices(P)
    state = np.array([[x, 0.0, y, 0.0, 0.0] for x, y in STARTS])
    foot = np.ones(B, int)
    working = state[:, (0, 2)].copy()
    walking, last_obj = np.ones(B, bool), np.full(B, math.inf)
    last_status, n_steps = np.zeros(B, int), np.zeros(B, int)
    run, n_rec = np.zeros(B, int), np.zeros(B, int)
    ev = np.zeros((W, H), np.int64)
    n_replans, finished_at, n_claims, n_failed_solves, first_targets = 0, -1, [], 0, None

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
        return AS.plan_batch(ev, W_MISS, W_HIT, ORIGIN, CELL, pos, R_CLAIM, MAX_CLAIMS, R_INFLATE, MIN_UNKNOWN, None, 64,
                             may_claim=np.isin(last_status, SOLVED))

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

    for k in range(K_MAX):
        if k % REPLAN_EVERY == 0:
            if k == 0:                                         # the first look round, noise-free
                first = np.stack([scan(b, None)[0] for b in range(B)])
                M.update(ev, state[:, (0, 2)], first, ORIGIN, CELL, LIDAR_RANGE, table, w_hit=W_HIT, w_miss=W_MISS)
            pl = plan()
            if k == 0:
                first_targets = [(int(t) // H, int(t) % H) for t in pl["target_cell"]]
            assign(pl, False)
            n_replans += 1
            n_claims.append(int(pl.get("n_claims", 0)))
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
            sc = S.split_scan(h, valid, 0, N_OBS_MAX, V_MAX)
            overflow = solid or bool(sc["overflow"])
            rings = sc["rings"] or []
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
        finished_at = K_MAX
    failed = ~np.isin(last_status, SOLVED)
    return dict(rule=rule, seed=seed, finished=left == 0, finished_at=finished_at, frontier_left=left, coverage=E.coverage(ev, occ),
                n_steps=n_steps.tolist(), n_failed=int(failed.sum()), n_failed_solves=n_failed_solves, n_recover=n_rec.tolist(),
                last_status=last_status.tolist(), n_replans=n_replans, n_claims=n_claims, first_targets=first_targets,
                final=np.round(state[:, (0, 2)], 2).tolist())


def rows_of(rows, rule):
    return sorted((x for x in rows if x["rule"] == rule), key=lambda x: x["seed"])


def verdict(rows):
    """(assigned finishes sooner on every seed by more than the seed spread, text)."""
    near, asg = rows_of(rows, "nearest"), rows_of(rows, "assigned")
    fa = np.array([[x["finished_at"] if x["finished"] else K_MAX + 1 for x in r] for r in (near, asg)])
    spread = int(max(fa[0].max() - fa[0].min(), fa[1].max() - fa[1].min()))
    gain = fa[0] - fa[1]
    return bool((gain > spread).all()), fa, spread, gain


def markdown(rows):
    sooner, fa, spread, gain = verdict(rows)
    out = ["# Coordinated exploration against nearest-frontier exploration", "",
           "Written by `tests/golden/make_exploration_assigned.py --write`; the rule is stated in `include/lipmpc.h`",
           "(`lipmpc_grid_frontier_assign_batch`) and restated in `tests/assign_oracle.py`; the argument for it is in DESIGN.md.", "",
           f"The open field of `make_exploration.py` at its chosen settings, `recover` = {MAX_RECOVER}, `k_max` = {K_MAX}; {len(STARTS)} robots side by",
           f"side at {list(STARTS)}.  One CPU chain of `UnknownEnvFleet.run_exploring` per noise seed and rule: `nearest` = `FrontierPlanner`,",
           f"`assigned` = `CoordinatedFrontierPlanner(r_claim={R_CLAIM}, max_claims={MAX_CLAIMS})`.  FINISHED AT = the first replan sample that",
           "finds no frontier cell left (-1: never within `k_max`); FAILED SOLVES = solves that ended neither SOLVED nor UNCERTIFIED, summed",
           "over the robots (with `recover` most cost a capture step, not the robot); LOST = robots whose last status is a failure.", "",
           "| rule | seed | finished at | steps per robot | failed solves | lost | coverage | claims per replan |", "|---|---|---|---|---|---|---|---|"]
    for rule in RULES:
        for x in rows_of(rows, rule):
            out.append(f"| {rule} | {x['seed']} | {x['finished_at'] if x['finished'] else -1} | {x['n_steps']} | {x['n_failed_solves']} | {x['n_failed']} | "
                       f"{x['coverage']:.4f} | {' '.join(map(str, x['n_claims'])) if rule == 'assigned' else '-'} |")
    x0 = rows_of(rows, "nearest")[0], rows_of(rows, "assigned")[0]
    cov = {rule: np.array([x["coverage"] for x in rows_of(rows, rule)]) for rule in RULES}
    out += ["", f"First replan (the noise-free first scan; the same on every seed): nearest sends the robots to cells {x0[0]['first_targets']},",
            f"assigned to {x0[1]['first_targets']}.", "",
            f"Finishing sample per seed: nearest {fa[0].tolist()}, assigned {fa[1].tolist()} ({K_MAX + 1} = not finished); the larger seed spread of the two is",
            f"{spread} samples and the gain nearest - assigned per seed is {gain.tolist()}.",
            ("Assigned finishes sooner on every seed by more than the seed spread: the GPU test asserts that the device's assigned run finishes "
             f"no later than sample {int(fa[0].min())}, the CPU nearest chain's earliest." if sooner else
             "Assigned does NOT finish sooner on every seed by more than the seed spread, so the GPU test records the device's finishing "
             "sample and does not assert on it.  What the chains show: the claims spread the fleet over the ring at once -- the first "
             "replan's targets above -- but a claim is made anew at every replan with no memory of the last, so a robot's target can "
             "jump as the map grows; the walker cannot turn on the spot, a jump behind it costs failed solves and capture steps, and "
             "the samples a robot spends recovering are samples it does not explore."),
            "", f"Coverage: nearest {cov['nearest'].min():.4f}-{cov['nearest'].max():.4f}, assigned {cov['assigned'].min():.4f}-{cov['assigned'].max():.4f}; the GPU bar for",
            f"the assigned run is min - (max - min) = {cov['assigned'].min() - (cov['assigned'].max() - cov['assigned'].min()):.4f}, with at most one seed missing it.",
            f"Failed solves over all seeds: nearest {sum(x['n_failed_solves'] for x in rows_of(rows, 'nearest'))}, assigned "
            f"{sum(x['n_failed_solves'] for x in rows_of(rows, 'assigned'))}; robots lost: nearest {sum(x['n_failed'] for x in rows_of(rows, 'nearest'))}, "
            f"assigned {sum(x['n_failed'] for x in rows_of(rows, 'assigned'))}.", ""]
    return "\n".join(out)


def main():
    with Pool(min(12, os.cpu_count() or 1)) as pool:
        rows = pool.map(chain, [(r, s) for r in RULES for s in SEEDS], chunksize=1)
    for rule in RULES:
        for x in rows_of(rows, rule):
            print(f"{rule} seed {x['seed']}: finished {x['finished']} at {x['finished_at']}, coverage {x['coverage']:.4f}, steps {x['n_steps']}, failed solves "
                  f"{x['n_failed_solves']}, lost {x['n_failed']}, recoveries {x['n_recover']}, claims {x['n_claims']}, first targets {x['first_targets']}, at {x['final']}")
    sooner, fa, spread, gain = verdict(rows)
    print("finishing samples", fa.tolist(), "spread", spread, "gain", gain.tolist(), "assert sooner:", sooner)
    if "--write" in sys.argv:
        rec = {"seeds": np.array(SEEDS), "k_max": K_MAX, "max_recover": MAX_RECOVER, "r_claim": R_CLAIM, "max_claims": MAX_CLAIMS,
               "starts": np.array(STARTS), "grid": np.array([W, H]), "origin": np.array(ORIGIN), "cell": np.array(CELL), "walls": np.array(E.WALLS),
               "lidar_range": LIDAR_RANGE, "noise_std": NOISE_STD, "weights": np.array([W_HIT, W_MISS]), "r_inflate": R_INFLATE,
               "min_unknown": MIN_UNKNOWN, "replan_every": REPLAN_EVERY, "lookahead": LOOKAHEAD, "assigned_sooner_every_seed": sooner,
               "seed_spread": spread}
        for rule in RULES:
            rs = rows_of(rows, rule)
            n = max(len(x["n_claims"]) for x in rs)
            rec.update({f"{rule}/finished": np.array([x["finished"] for x in rs]), f"{rule}/finished_at": np.array([x["finished_at"] for x in rs]),
                        f"{rule}/steps": np.array([x["n_steps"] for x in rs]), f"{rule}/failed_solves": np.array([x["n_failed_solves"] for x in rs]),
                        f"{rule}/lost": np.array([x["n_failed"] for x in rs]), f"{rule}/coverage": np.array([x["coverage"] for x in rs]),
                        f"{rule}/n_replans": np.array([x["n_replans"] for x in rs]),
                        f"{rule}/n_claims": np.array([x["n_claims"] + [-1] * (n - len(x["n_claims"])) for x in rs]),
                        f"{rule}/first_targets": np.array(rs[0]["first_targets"])})
        np.savez(os.path.join(HERE, "exploration_assigned.npz"), **rec)
        with open(os.path.join(HERE, "EXPLORATION_ASSIGNED.md"), "w") as f:
            f.write(markdown(rows))
        print("recorded", list(SEEDS))


if __name__ == "__main__":
    main()
