"""The dead-end scene of tests/test_map_fleet_gpu.py, chosen and recorded on the CPU (tests/golden/MAPPED_REPLANNING.md):

    python tests/golden/make_mapped_replanning.py [--write]

A U-shaped wall, open side toward the start, between start and goal, as an occupancy grid.  Per noise seed two CPU chains of
the fleet's sample, built from the committed oracles only -- grid scan (tests/grid_lidar_oracle.py), clusters and hulls
(oracle/lidar_oracle.py), step solve and state advance (oracle/lipmpc_oracle.py: interior mode, tol_interior 1e-6, N = 3),
scan integration and goal selection (tests/map_oracle.py), planning on the map (tests/rrt_grid_oracle.py):
  plain       UnknownEnvFleet.run: the reactive loop alone
  replanning  UnknownEnvFleet.run_replanning: every REPLAN_EVERY samples a plan on the map built so far
A chain ARRIVES if the stop rule stops it at the final goal within K_MAX samples.  Prints the table; --write records the
seeds and the chains' step counts as mapped_replanning.npz.
"""
import math
import os
import sys
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
import grid_lidar_oracle as G  # noqa: E402
import lidar_oracle as L  # noqa: E402
import lipmpc_oracle as O  # noqa: E402
import map_oracle as M  # noqa: E402
import rrt_grid_oracle as RG  # noqa: E402

# -- the scene (cells of 0.05 m; the evidence grid has the true map's geometry) ----------------------------------------
W, H, ORIGIN, CELL = 92, 80, (1.0, 0.0), (0.05, 0.05)
# (i0, j0, i1, j1): the back wall (x 3.4 .. 3.55, from y = 1.4 to the grid's upper edge), the lower arm and the upper arm (x 2.8 .. 3.4);
# the U opens toward -x, the only way round is below y = 1.4
WALLS = ((48, 28, 51, 80), (36, 28, 48, 31), (36, 77, 48, 80))
START, GOAL = (1.6, 2.72), (4.6, 2.7)
LIDAR_RANGE, RESOLUTION, N_OBS_MAX, V_MAX = 1.5, 360, 12, 32
NOISE_STD, STOP_OBJ, K_MAX = 0.01, 0.05, 100
W_HIT, W_MISS = 3, 1
REPLAN_EVERY, LOOKAHEAD = 3, 2.0
RRT_N, RRT_R, RRT_SEED, RRT_MAX_CELLS = 400, 30, 1, 1 << 14
SEEDS = tuple(range(8))


def true_map():
    occ = np.zeros((W, H), np.uint8)
    for i0, j0, i1, j1 in WALLS:
        occ[i0:i1, j0:j1] = 1
    return occ


def noise_of(seed):
    """The readings' noise of a seed, [K_MAX, RESOLUTION, 2]: what the GPU test hands the fleet as its given noise."""
    return NOISE_STD * np.random.default_rng(seed).standard_normal((K_MAX, RESOLUTION, 2))


def chain(args):
    seed, replanning = args
    occ, table, noise = true_map(), L.ray_table(RESOLUTION), noise_of(seed)
    P = O.Params(N=3, tol_interior=1e-6)
    A, Bm = O.lip_matrices(P)
    state, foot = np.array([START[0], 0.0, START[1], 0.0, 0.0]), 1
    final = np.array(GOAL, float)
    working = final.copy()
    walking, last_obj, last_status, n_steps, n_replans = True, math.inf, 0, 0, 0
    ev = np.zeros((W, H), np.int64)
    arrived_at = -1
    for k in range(K_MAX):
        pos = state[[0, 2]]
        if replanning and k % REPLAN_EVERY == 0:
            plan = RG.plan_grid(ev >= W_HIT, ORIGIN, CELL, final, start=pos, seed=RRT_SEED, n=RRT_N, r_rewire=RRT_R, max_cells=RRT_MAX_CELLS)
            if (not walking) and last_status in (0, 4) and last_obj < STOP_OBJ and not np.array_equal(working, final):
                walking, last_obj = True, math.inf
            sub = plan["sub_goals"][None] if plan["n_sub"] else np.zeros((1, 1, 2))
            working = M.select_goals(pos[None], final[None], sub, [plan["n_sub"]], [plan["status"]], LOOKAHEAD)[0]
            n_replans += 1
        # scan -> clusters -> hulls
        hits, valid = G.grid_hits(pos, occ, ORIGIN, CELL, LIDAR_RANGE, table)
        overflow = G.in_solid_cell(pos, occ, ORIGIN, CELL)
        pts = (hits + noise[k])[valid]
        rings = []
        if len(pts):
            labels = L.dbscan_labels(pts)
            rings = [r for r in (L.hull_ring(pts[labels == c]) for c in range(labels.max() + 1)) if r is not None]
            overflow = overflow or len(rings) > N_OBS_MAX or any(len(r) > V_MAX for r in rings)
        if walking:                                           # the update's mask is `walking` as the sample finds it
            h = np.full((RESOLUTION, 2), np.nan)
            h[valid] = pts
            M.update(ev, pos[None], h[None], ORIGIN, CELL, LIDAR_RANGE, table, w_hit=W_HIT, w_miss=W_MISS)
        # solve + fleet update (lipmpc_fleet_update_batch)
        walking = walking and last_obj >= STOP_OBJ
        if not walking:
            if arrived_at < 0 and last_status in (0, 4) and last_obj < STOP_OBJ and np.array_equal(working, final):
                arrived_at = k
            if not replanning or arrived_at >= 0:
                break
            continue
        r = O.plan_step(state, working, foot, rings, 0.0, P, exact=False)
        last_status = 5 if overflow else r["status"]
        if last_status not in (0, 4):
            walking = False
            break                                             # a failed solve is final in both loops
        last_obj = r["obj"]
        state = np.concatenate([A @ state[:4] + Bm @ r["U"][0], [r["theta"][1]]])
        foot, n_steps = -foot, n_steps + 1
    dist = float(np.hypot(state[0] - GOAL[0], state[2] - GOAL[1]))
    return seed, replanning, arrived_at, n_steps, last_status, dist, n_replans, (round(float(state[0]), 2), round(float(state[2]), 2))


def main():
    jobs = [(s, rp) for s in SEEDS for rp in (False, True)]
    with Pool(min(16, os.cpu_count() or 1)) as pool:
        rows = pool.map(chain, jobs)
    for rp in (False, True):
        r = [x for x in rows if x[1] == rp]
        print("replanning" if rp else "plain", f": {sum(x[2] >= 0 for x in r)} of {len(r)} arrive")
        for x in r:
            print(f"   seed {x[0]}: arrived at sample {x[2]}, {x[3]} steps, last status {x[4]}, final distance {x[5]:.3f} at {x[7]}, {x[6]} replans")
    if "--write" in sys.argv:
        plain = {x[0]: x for x in rows if not x[1]}
        rep = {x[0]: x for x in rows if x[1]}
        keep = [s for s in SEEDS if plain[s][2] < 0 and rep[s][2] >= 0]
        np.savez(os.path.join(HERE, "mapped_replanning.npz"), seeds=np.array(keep), k_max=K_MAX,
                 grid=np.array([W, H]), origin=np.array(ORIGIN), cell=np.array(CELL), walls=np.array(WALLS), start=np.array(START),
                 goal=np.array(GOAL), lidar_range=LIDAR_RANGE, noise_std=NOISE_STD, weights=np.array([W_HIT, W_MISS]),
                 replan_every=REPLAN_EVERY, lookahead=LOOKAHEAD, rrt=np.array([RRT_N, RRT_R, RRT_SEED, RRT_MAX_CELLS]),
                 plain_steps=np.array([plain[s][3] for s in keep]), replanning_steps=np.array([rep[s][3] for s in keep]),
                 replanning_arrived_at=np.array([rep[s][2] for s in keep]), all_seeds=np.array(SEEDS),
                 plain_arrived=np.array([plain[s][2] >= 0 for s in SEEDS]), replanning_arrived=np.array([rep[s][2] >= 0 for s in SEEDS]))
        print("recorded", keep)


if __name__ == "__main__":
    main()
