"""Golden occupancy grids and distance transforms for the RRT* planner (tests/test_rrt_*.py), made with scipy the way the
reference's HumanoidMPCWithRRT makes them (HumanoidMPCVariants/HumanoidMPCWithRRT.py:21-112):

    python tests/golden/make_rrt_golden.py

(``rrtplanner`` is not installed, so the reference module itself cannot be imported; its grid steps are restated here
with the same scipy calls.)  Per obstacle set: bounds min / max over {origin, goal, every vertex} -/+ 3, H = ceil(250 *
aspect), vertices rounded to cells with np.round, every cell of the half-open box of the rounded vertices kept if
``scipy.spatial.Delaunay(rounded).find_simplex(cell) >= 0``, then ``scipy.ndimage.distance_transform_edt(1 - grid)``.

Sets: the four scenes of pdf_scenarios.npz with a RRT-style map (SimulationRRT, SimulationMaze1, SimulationMaze2,
Simulation1Circles) and 24 seeded random sets of 1-7 convex hulls (16 with radii 0.03-1.5 m, 8 with radii 0.03-0.12 m:
hulls a few cells across, where rounding moves vertices the most).  A random set on which the reference would raise
(Qhull refuses collinear / coincident rounded vertices, or a hull with no cell in its half-open box) has no reference
answer and is drawn again; tests/test_rrt_oracle.py covers the rule there without a golden.

Output rrt_grid_golden.npz (data only): names, rings [S,n_obs,v_max,2], nv, goal [S,2], bounds [S,4] (min_x, max_x,
min_y, max_y), dims [S,2] (W+1, H+1), occ_packed (np.packbits of every grid, flattened [x, y], concatenated), occ_off
[S+1] (byte offsets), d2_dy (int32: the squared distances differenced along y, d2[x, y] = cumsum over y' <= y, every grid
flattened [x, y] and concatenated; differenced because that compresses ten times better), d2_off [S+1].
"""
import math
import os

import numpy as np
from scipy.ndimage import distance_transform_edt
from scipy.spatial import ConvexHull, Delaunay

HERE = os.path.dirname(os.path.abspath(__file__))
SCENES = ("SimulationRRT", "SimulationMaze1", "SimulationMaze2", "Simulation1Circles")
WIDTH, MARGIN, N_OBS, V_MAX = 250, 3.0, 9, 24


def reference_grid(rings, goal):
    """The grid steps of HumanoidMPCWithRRT.py:32-90 and the distance of :108, with the same scipy calls."""
    allv = np.concatenate(rings)
    lo_x = min(0, goal[0], allv[:, 0].min()) - MARGIN
    lo_y = min(0, goal[1], allv[:, 1].min()) - MARGIN
    hi_x = max(0, goal[0], allv[:, 0].max()) + MARGIN
    hi_y = max(0, goal[1], allv[:, 1].max()) + MARGIN
    H = math.ceil(WIDTH * ((hi_y - lo_y) / (hi_x - lo_x)))
    grid = np.zeros((WIDTH + 1, H + 1))
    for r in rings:
        cx = np.round(((r[:, 0] - lo_x) / (hi_x - lo_x)) * WIDTH).astype(int)
        cy = np.round(((r[:, 1] - lo_y) / (hi_y - lo_y)) * H).astype(int)
        tri = Delaunay(np.stack([cx, cy], 1))                        # raises on degenerate rounded vertices
        cells = [(i, j) for i in range(cx.min(), cx.max()) for j in range(cy.min(), cy.max())
                 if tri.find_simplex([i, j]) >= 0]
        if not cells:
            raise ValueError("no cell inside the hull's half-open box")   # the reference's indexing fails there
        cells = np.array(cells)
        grid[cells[:, 0], cells[:, 1]] = 1
    d = distance_transform_edt(1 - grid)
    d2 = np.rint(d * d).astype(np.int64)
    assert np.array_equal(np.sqrt(d2.astype(float)), d), "d2 is not the square of the transform"
    return (lo_x, hi_x, lo_y, hi_y), grid.astype(bool), d2


def random_set(rng, tiny):
    rings = []
    for _ in range(int(rng.integers(1, 8))):
        c = rng.uniform(-1.0, 7.0, 2)
        rad = rng.uniform(0.03, 0.12 if tiny else 1.5)
        pts = c + rad * rng.uniform(-1, 1, (int(rng.integers(3, 9)), 2))
        h = ConvexHull(pts)
        rings.append(pts[h.vertices])
    goal = rng.uniform(-1.0, 7.0, 2)
    return rings, goal


def main():
    sc = np.load(os.path.join(HERE, "pdf_scenarios.npz"))
    sets = []
    for name in SCENES:
        rings = [sc[name + "/rings"][j][: sc[name + "/nv"][j]] for j in range(len(sc[name + "/nv"]))]
        sets.append((name, rings, np.asarray(sc[name + "/goal"], float)))
    rng = np.random.default_rng(2024)
    n_ok, n_raised = 0, 0
    while n_ok < 24:
        tiny = n_ok >= 16
        rings, goal = random_set(rng, tiny)
        try:
            reference_grid(rings, goal)
        except Exception:                      # Qhull error / empty box: the reference raises too
            n_raised += 1
            continue
        sets.append((f"random{n_ok:02d}" + ("_tiny" if tiny else ""), rings, goal))
        n_ok += 1
    S = len(sets)
    xy = np.zeros((S, N_OBS, V_MAX, 2))
    nv = np.zeros((S, N_OBS), np.int32)
    goals, bounds, dims = np.zeros((S, 2)), np.zeros((S, 4)), np.zeros((S, 2), np.int32)
    occ, d2s, occ_off, d2_off = [], [], [0], [0]
    for s, (name, rings, goal) in enumerate(sets):
        for j, r in enumerate(rings):
            xy[s, j, : len(r)] = r
            nv[s, j] = len(r)
        goals[s] = goal
        b, og, d2 = reference_grid(rings, goal)
        bounds[s], dims[s] = b, og.shape
        occ.append(np.packbits(og.reshape(-1)))
        d2s.append(np.diff(d2, axis=1, prepend=0).reshape(-1).astype(np.int32))
        occ_off.append(occ_off[-1] + len(occ[-1]))
        d2_off.append(d2_off[-1] + len(d2s[-1]))
        print(f"{name:20s} dims {og.shape} occupied {int(og.sum())}")
    print(f"{n_raised} random sets drawn again (the reference raises on them)")
    np.savez_compressed(os.path.join(HERE, "rrt_grid_golden.npz"), names=np.array([s[0] for s in sets]), rings=xy,
                        nv=nv, goal=goals, bounds=bounds, dims=dims, occ_packed=np.concatenate(occ),
                        occ_off=np.array(occ_off, np.int64), d2_dy=np.concatenate(d2s), d2_off=np.array(d2_off, np.int64))


if __name__ == "__main__":
    main()
