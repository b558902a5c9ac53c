"""CPU: tests/grid_lidar_oracle.py -- the numpy restatement of the grid scan's contract (include/lipmpc.h,
lipmpc_lidar_grid_c_eta_batch) -- against the polygon oracle (oracle/lidar_oracle.py, pinned to the reference's range_finder) on
a map where the two geometries are the same set, and the contract's own rules by hand."""
import numpy as np

import grid_lidar_oracle as G
import lidar_oracle as L


def test_grid_oracle_agrees_with_polygon_oracle_on_cell_aligned_boxes():
    """The cell-aligned fixture (axis-aligned boxes whose corners are ox + a * cell): the grid march and the reference's
    ray-edge intersection place the same geometric point by different arithmetic.  Bars (conditions, not measurements): hits
    that both report agree within 1e-12; at most 0.1 % of the rays may disagree on hit / no hit (rays through a box corner or at
    the range limit).  Measured on the CPU with this contract: 12 boxes, 21 600 rays, 0 disagreements, largest distance between
    corresponding hits 1.8e-15."""
    fx = G.fixture()
    assert len(fx["rings"]) >= 8 and len(fx["pos"]) == 60
    tab = L.ray_table(fx["resolution"])
    rays = disagree = n_hits = 0
    worst = 0.0
    for p in fx["pos"]:
        gh, gv = G.grid_hits(p, fx["occ"], fx["origin"], fx["cell"], fx["lidar_range"], tab)
        ph, pv = L.lidar_hits(p, fx["rings"], fx["lidar_range"], tab)
        rays += len(gv)
        disagree += int((gv != pv).sum())
        both = gv & pv
        n_hits += int(both.sum())
        if both.any():
            worst = max(worst, float(np.abs(gh[both] - ph[both]).max()))
    print(f"{len(fx['rings'])} boxes, {rays} rays, {n_hits} common hits, {disagree} disagreements, max |dhit| = {worst:.3g}")
    assert n_hits > rays // 10
    assert worst < 1e-12
    assert disagree <= rays // 1000


def test_grid_contract_rules_by_hand():
    """Start cell, hit placement, the tie rule, the stop rule, the robot in a solid cell, the robot outside the grid."""
    tab = L.ray_table(8)                                  # rays at 0, 45, 90, ... degrees
    occ = np.zeros((8, 8), np.uint8)
    occ[5, 2] = 1                                         # the cell [2.5, 3) x [1, 1.5) of a 0.5 m grid at the origin
    org, cell = (0.0, 0.0), (0.5, 0.5)
    hits, valid = G.grid_hits((1.25, 1.25), occ, org, cell, 3.0, tab)
    assert valid.tolist() == [True] + [False] * 7 and hits[0].tolist() == [2.5, 1.25]      # entered through its x = 2.5 face
    # strictly below the range: the same wall at exactly 1.25 m is not a reading, a hair more range and it is
    assert not G.grid_hits((1.25, 1.25), occ, org, cell, 1.25, tab)[1].any()
    assert G.grid_hits((1.25, 1.25), occ, org, cell, 1.2500001, tab)[1][0]
    # the tie rule: the 45 degree ray from a cell centre crosses x and y boundaries together and steps in x first, so of the two
    # cells that touch the diagonal at a corner only the x-neighbour (i + 1, j) is visited
    d = np.zeros((8, 8), np.uint8); d[3, 2] = 1
    t8 = np.array([[1.0, 1.0]])                           # direction (1, 1) exactly: the crossings tie bit for bit
    h, v = G.grid_hits((1.25, 1.25), d, org, cell, 2.0, t8)
    assert v[0] and h[0].tolist() == [1.5, 1.5]
    d = np.zeros((8, 8), np.uint8); d[2, 3] = 1           # the y-neighbour at the same corner is passed by
    assert not G.grid_hits((1.25, 1.25), d, org, cell, 0.7, t8)[1].any()
    # a robot in a solid cell has no scan; one outside the grid sees into it; one far away sees nothing
    assert G.in_solid_cell((2.75, 1.25), occ, org, cell) and not G.grid_hits((2.75, 1.25), occ, org, cell, 3.0, tab)[1].any()
    hits, valid = G.grid_hits((-1.0, 1.25), occ, org, cell, 4.0, tab)
    assert valid[0] and hits[0].tolist() == [2.5, 1.25]
    assert not G.grid_hits((1e12, 1.25), occ, org, cell, 4.0, tab)[1].any() and G.robot_cell((1e12, 0.0), org, cell) is None
    assert not G.grid_hits((float("nan"), 1.25), occ, org, cell, 4.0, tab)[1].any()
    # the window the kernel stages: (2 floor(range / cell) + 5)^2 cells, at most 49152
    assert G.window_half(1.5, (0.05, 0.05)) == (32, 32) and G.window_half(1.0, (0.3, 0.5)) == (5, 4)
    assert G.window_fits(3.0, (0.05, 0.05)) and not G.window_fits(3.0, (0.01, 0.01))
