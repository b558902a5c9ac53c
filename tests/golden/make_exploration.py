"""The exploration scene of tests/test_frontier_fleet_gpu.py, chosen and recorded on the CPU (tests/golden/EXPLORATION.md):

    python tests/golden/make_exploration.py [--write] [--sweep]

An open field with three blocks and a wall segment, as an occupancy grid; three robots start along one edge and share one
evidence map.  Per noise seed two CPU chains of the fleet's sample, built from the committed oracles only -- grid scan
(tests/grid_lidar_oracle.py), clusters and hulls (oracle/lidar_oracle.py), step solve and state advance
(oracle/lipmpc_oracle.py: interior mode, tol_interior 1e-6, N = 3), scan integration and goal selection (tests/map_oracle.py),
frontier field and paths (tests/frontier_oracle.py):
  exploring   UnknownEnvFleet.run_exploring: every REPLAN_EVERY samples every robot is sent to its nearest frontier
  reactive    UnknownEnvFleet.run toward the far corner: the loop that needs a goal handed to it
A chain FINISHES if its closing plan finds no frontier cell left on the shared map.  COVERAGE is the share of the cells of the true
map that are connected to the start, farther than R_INFLATE from a solid cell, and known free (evidence <= -W_MISS) at the end.
Prints the table; --write records the settings, the seeds and the chains' counts as exploration.npz; --sweep runs the other
settings that EXPLORATION.md lists.
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
import field_oracle as FO  # noqa: E402
import frontier_oracle as FR  # noqa: E402
import grid_lidar_oracle as G  # noqa: E402
import lidar_oracle as L  # noqa: E402
import lipmpc_oracle as O  # noqa: E402
import map_oracle as M  # noqa: E402

# -- the scene (cells of 0.1 m; the evidence grid has the true map's geometry) ----------------------------------------
W, H, ORIGIN, CELL = 64, 56, (0.0, 0.0), (0.1, 0.1)
# (i0, j0, i1, j1): no outer walls -- the sensor model wraps each cluster of readings in ONE convex hull, and a robot inside a closed
# room stands inside the hull of its walls (EXPLORATION.md) -- but three convex blocks and a wall segment in an open field
WALLS = ((22, 16, 28, 22), (22, 34, 28, 40), (42, 25, 48, 31), (34, 44, 36, 54))
STARTS = ((0.8, 1.0), (0.8, 2.8), (0.8, 4.6))
FAR_CORNER = (5.6, 4.8)                                       # the reactive loop's goal
LIDAR_RANGE, RESOLUTION, N_OBS_MAX, V_MAX = 1.5, 360, 12, 32
NOISE_STD, STOP_OBJ, K_MAX = 0.01, 0.05, 100
W_HIT, W_MISS = 3, 1
R_INFLATE, MIN_UNKNOWN, REPLAN_EVERY, LOOKAHEAD = 3, 2, 3, 0.6
SEEDS = tuple(range(6))
SOLVED = (0, 4)                                               # STATUS_SOLVED, STATUS_UNCERTIFIED


def true_map():
    occ = np.zeros((W, H), np.uint8)
    for i0, j0, i1, j1 in WALLS:
        occ[i0:i1, j0:j1] = 1
    return occ


def noise_of(seed, B=len(STARTS)):
    """The readings' noise of a seed, [K_MAX, B, RESOLUTION, 2]: what the GPU test hands the fleet as its given noise."""
    return NOISE_STD * np.random.default_rng(seed).standard_normal((K_MAX, B, RESOLUTION, 2))


def reachable(occ, r_inflate=R_INFLATE):
    """The cells that count for the coverage: unblocked at r_inflate on the TRUE map and connected to the first start."""
    blocked = FO.blocked_cells(occ, r_inflate)
    s = FO.cell_of(STARTS[0], ORIGIN, CELL, W, H)
    seen, todo = {s}, [s]
    while todo:
        i, j = todo.pop()
        for a, b, _ in FO.moves_from(blocked, i, j):
            if (a, b) not in seen:
                seen.add((a, b))
                todo.append((a, b))
    out = np.zeros((W, H), bool)
    out[tuple(np.array(sorted(seen)).T)] = True
    return out


def coverage(ev, occ, r_inflate=R_INFLATE):
    cells = reachable(occ, r_inflate)
    return float((np.asarray(ev)[cells] <= -W_MISS).sum() / cells.sum())


def chain(args):
    """One run.  args = (seed, exploring, settings) with settings = dict(r_inflate, min_unknown, replan_every, lookahead)."""
    seed, exploring, cfg = args
    r_inflate, min_unknown, replan_every, lookahead = cfg["r_inflate"], cfg["min_unknown"], cfg["replan_every"], cfg["lookahead"]
    occ, table, noise = true_map(), L.ray_table(RESOLUTION), noise_of(seed)
    P = O.Params(N=3, tol_interior=1e-6)
    A, Bm = O.lip_matrices(P)
    B = len(STARTS)
    state = np.array([[x, 0.0, y, 0.0, 0.0] for x, y in STARTS])
    foot = np.ones(B, int)
    working = state[:, (0, 2)].copy() if exploring else np.tile(FAR_CORNER, (B, 1))
    walking, last_obj = np.ones(B, bool), np.full(B, math.inf)
    last_status, n_steps = np.zeros(B, int), np.zeros(B, int)
    ev = np.zeros((W, H), np.int64)
    n_replans, n_frontier, known_free, finished_at = 0, [], [], -1

    def scan(b, nz):
        pos = state[b, (0, 2)]
        hits, valid = G.grid_hits(pos, occ, ORIGIN, CELL, LIDAR_RANGE, table)
        pts = (hits + nz)[valid] if nz is not None else hits[valid]
        h = np.full((RESOLUTION, 2), np.nan)
        h[valid] = pts
        return pts, h, G.in_solid_cell(pos, occ, ORIGIN, CELL)

    def plan():
        return FR.plan_batch(ev, W_MISS, W_HIT, ORIGIN, CELL, state[:, (0, 2)], r_inflate, min_unknown, None, 64)

    def assign(pl, closing):
        nonlocal working, walking, last_obj
        found = pl["status"] == FR.FOUND
        solved = np.isin(last_status, SOLVED)
        if not closing:
            resume = ~walking & solved & found
            walking = walking | resume
            last_obj = np.where(resume, math.inf, last_obj)
            S = max(1, int(pl["n_sub"].max()))
            sub = np.zeros((B, S, 2))
            for b in range(B):
                sub[b, :pl["n_sub"][b]] = pl["sub_goals"][b]
            picked = M.select_goals(state[:, (0, 2)], pl["target"], sub, pl["n_sub"], pl["status"], lookahead)
            working = np.where(found[:, None], picked, working)
        walking = walking & found

    for k in range(K_MAX):
        if exploring and k % replan_every == 0:
            if k == 0:                                         # the first look round, noise-free
                first = np.stack([scan(b, None)[1] for b in range(B)])
                M.update(ev, state[:, (0, 2)], first, ORIGIN, CELL, LIDAR_RANGE, table, w_hit=W_HIT, w_miss=W_MISS)
            pl = plan()
            assign(pl, False)
            n_replans += 1
            n_frontier.append(int(pl["n_frontier"][0]))
            known_free.append(int((ev <= -W_MISS).sum()))
            if pl["n_frontier"][0] == 0 and finished_at < 0:
                finished_at = k
        if not walking.any() and (not exploring or finished_at >= 0):
            break
        # one sample: every robot's scan, the walking robots' readings into the one map, then the solves and the fleet update
        scans = [scan(b, noise[k, b]) for b in range(B)]
        M.update(ev, state[:, (0, 2)], np.stack([s[1] for s in scans]), ORIGIN, CELL, LIDAR_RANGE, table, w_hit=W_HIT, w_miss=W_MISS,
                 mask=walking.astype(int))
        for b in range(B):
            walking[b] = walking[b] and last_obj[b] >= STOP_OBJ
            if not walking[b]:
                continue
            pts, _, overflow = scans[b]
            rings = []
            if len(pts):
                labels = L.dbscan_labels(pts)
                rings = [r for r in (L.hull_ring(pts[labels == c]) for c in range(labels.max() + 1)) if r is not None]
                overflow = overflow or len(rings) > N_OBS_MAX or any(len(r) > V_MAX for r in rings)
            r = O.plan_step(state[b], working[b], int(foot[b]), rings, 0.0, P, exact=False)
            last_status[b] = 5 if overflow else r["status"]
            if last_status[b] not in SOLVED:
                walking[b] = False                             # a failed solve is final
                continue
            last_obj[b] = r["obj"]
            state[b] = np.concatenate([A @ state[b, :4] + Bm @ r["U"][0], [r["theta"][1]]])
            foot[b], n_steps[b] = -foot[b], n_steps[b] + 1
    status, left = None, -1
    if exploring:
        pl = plan()
        assign(pl, True)
        status, left = pl["status"], int(pl["n_frontier"][0])
        if pl["n_frontier"][0] == 0 and finished_at < 0:
            finished_at = K_MAX
    done = ~walking & np.isin(last_status, SOLVED) & (status == FR.NO_PATH) if exploring else np.zeros(B, bool)
    return dict(seed=seed, exploring=exploring, finished=left == 0, n_done=int(done.sum()), frontier_left=left, finished_at=finished_at,
                coverage=coverage(ev, occ, r_inflate), coverage_r2=coverage(ev, occ, R_INFLATE), n_steps=n_steps.tolist(),
                last_status=last_status.tolist(), n_failed=int((~np.isin(last_status, SOLVED)).sum()), n_replans=n_replans,
                n_frontier=n_frontier, known_free=known_free, explore_status=None if status is None else status.tolist(),
                final=np.round(state[:, (0, 2)], 2).tolist())


CHOSEN = dict(r_inflate=R_INFLATE, min_unknown=MIN_UNKNOWN, replan_every=REPLAN_EVERY, lookahead=LOOKAHEAD)


def table(rows, title):
    print(title)
    for x in rows:
        print(f"   seed {x['seed']}: finished {x['finished']} at sample {x['finished_at']}, coverage {x['coverage']:.4f}, steps {x['n_steps']}, "
              f"last status {x['last_status']}, {x['n_replans']} replans, frontier cells left {x['frontier_left']}, done {x['n_done']}, explore status {x['explore_status']}, at {x['final']}")


def main():
    with Pool(min(16, os.cpu_count() or 1)) as pool:
        if "--sweep" in sys.argv:
            for cfg in [dict(CHOSEN, lookahead=la, replan_every=re) for la in (0.3, 0.6, 1.0) for re in (3, 5, 10)] + \
                       [dict(CHOSEN, r_inflate=r, min_unknown=mu) for r, mu in ((1, 1), (2, 2), (2, 1), (2, 3), (3, 1), (3, 3))]:
                rows = pool.map(chain, [(s, True, cfg) for s in SEEDS])
                print(cfg, ": finished", sum(x["finished"] for x in rows), "of", len(rows), "; coverage",
                      " ".join(f"{x['coverage']:.3f}" for x in rows), "; failed solves", [x["n_failed"] for x in rows],
                      "; finished at", [x["finished_at"] for x in rows])
            return
        rows = pool.map(chain, [(s, ex, CHOSEN) for s in SEEDS for ex in (True, False)])
    ex = [x for x in rows if x["exploring"]]
    re = [x for x in rows if not x["exploring"]]
    table(ex, f"exploring {CHOSEN}: {sum(x['finished'] for x in ex)} of {len(ex)} finish")
    table(re, "reactive, toward the far corner")
    cov = np.array([x["coverage"] for x in ex])
    print(f"coverage: exploring min {cov.min():.4f} max {cov.max():.4f} spread {cov.max() - cov.min():.4f}; reactive max "
          f"{max(x['coverage'] for x in re):.4f}")
    if "--write" in sys.argv:
        np.savez(os.path.join(HERE, "exploration.npz"), seeds=np.array(SEEDS), k_max=K_MAX, grid=np.array([W, H]), origin=np.array(ORIGIN),
                 cell=np.array(CELL), walls=np.array(WALLS), starts=np.array(STARTS), far_corner=np.array(FAR_CORNER),
                 lidar_range=LIDAR_RANGE, noise_std=NOISE_STD, weights=np.array([W_HIT, W_MISS]), r_inflate=R_INFLATE,
                 min_unknown=MIN_UNKNOWN, replan_every=REPLAN_EVERY, lookahead=LOOKAHEAD,
                 exploring_finished=np.array([x["finished"] for x in ex]), exploring_finished_at=np.array([x["finished_at"] for x in ex]),
                 exploring_coverage=cov, exploring_steps=np.array([x["n_steps"] for x in ex]),
                 exploring_failed=np.array([x["n_failed"] for x in ex]), exploring_replans=np.array([x["n_replans"] for x in ex]),
                 reactive_coverage=np.array([x["coverage"] for x in re]), reactive_steps=np.array([x["n_steps"] for x in re]),
                 reactive_failed=np.array([x["n_failed"] for x in re]))
        print("recorded", list(SEEDS))


if __name__ == "__main__":
    main()
