"""Inputs of the window tests of the grid scan and the map update, shared by tests/test_window_cases_oracle.py (CPU: does every
case reach what it is meant to reach, on the oracles alone?), tests/test_lidar_grid_windows_gpu.py and
tests/test_map_windows_gpu.py (the two kernels against tests/grid_lidar_oracle.py and tests/map_oracle.py on the same inputs).
numpy only; every input is seeded.

Both kernels keep a window of ww x wh = (2 nx + 1) x (2 ny + 1) cells around the robot as a bitmap in LDS, nx, ny =
floor(reach / cell) + 2, walk it 64 cells per trip with an incremental (li, lj) stepper, and are refused above 49152 cells.  A CASE
is dict(id, lidar_range, cell, origin, W, H, occ [W,H] or [B,W,H] uint8, pos [B,2], resolution, depth, window (ww, wh) of the
scan, map_window (ww, wh) of the update with ``depth``, noisy: run the scan with noise too, far: robots that have a cell but whose
window does not meet the grid, unplaced: robots that cannot be given a cell, w_hit, w_miss, ev_seed: None or the seed of a non-zero
evidence grid the update starts from, readings: None or {robot: [R,2] hand-written readings uploaded as they are}).  The window
shapes are derived through G.window_half / M.window_half and asserted HERE, so that a change of the rule fails at import.
"""
import functools
import math

import numpy as np

import grid_lidar_oracle as G
import lidar_oracle as L
import map_oracle as M

TRIP = 64                                  # window cells per trip of either kernel's stepper
CAP = G.WINDOW_CELLS
LAST_TRIPS = 760                           # the cap cases must reach bits beyond this trip


def _rect(origin, cell, W, H):
    lo = np.array(origin, float)
    return lo, lo + np.array(cell, float) * (W, H)


def _free_robots(rng, occ, origin, cell, n, margin):
    """n robots uniform over the grid's rectangle grown by ``margin`` metres, none in a solid cell."""
    lo, hi = _rect(origin, cell, *occ.shape)
    out = []
    while len(out) < n:
        p = rng.uniform(lo - margin, hi + margin)
        if not G.in_solid_cell(p, occ, origin, cell):
            out.append(p)
    return np.array(out)


def _inner_robot(rng, occ, origin, cell, half):
    """A robot in a free cell whose whole window of half-sizes ``half`` (+ 1) lies inside the grid, or None when no cell is."""
    W, H = occ.shape
    nx, ny = half[0] + 1, half[1] + 1
    if W <= 2 * nx or H <= 2 * ny:
        return None
    for _ in range(1000):
        i, j = int(rng.integers(nx, W - nx)), int(rng.integers(ny, H - ny))
        if not occ[i, j]:
            return np.array(origin) + (np.array([i, j]) + rng.uniform(0.2, 0.8, 2)) * np.array(cell)
    return None


def _far(origin, cell, W, H, lidar_range, k=0):
    """A robot with a cell of its own whose window cannot meet the grid."""
    lo, hi = _rect(origin, cell, W, H)
    away = 3.0 * lidar_range + 10.0 * max(cell) + 1.0
    return [(hi[0] + away, lo[1]), (lo[0], lo[1] - away), (lo[0] - away, hi[1] + away)][k % 3]


def _case(id_, lidar_range, cell, origin, occ, pos, window, depth, map_window=None, resolution=360, noisy=True, far=(), unplaced=(),
          w_hit=3, w_miss=1, ev_seed=None, readings=None):
    cell = (float(cell), float(cell)) if np.isscalar(cell) else (float(cell[0]), float(cell[1]))
    W, H = occ.shape[-2:]
    nx, ny = G.window_half(lidar_range, cell)
    assert (2 * nx + 1, 2 * ny + 1) == tuple(window), (id_, "scan window", (2 * nx + 1, 2 * ny + 1), window)
    mx, my = M.window_half(lidar_range, depth, cell)
    map_window = tuple(window if map_window is None else map_window)
    assert (2 * mx + 1, 2 * my + 1) == map_window, (id_, "map window", (2 * mx + 1, 2 * my + 1), map_window)
    pos = np.ascontiguousarray(pos, float)
    assert occ.dtype == np.uint8 and (occ.ndim == 2 or len(occ) == len(pos))
    return dict(id=id_, lidar_range=float(lidar_range), cell=cell, origin=(float(origin[0]), float(origin[1])), W=W, H=H, occ=occ, pos=pos,
                resolution=int(resolution), depth=float(depth), window=tuple(window), map_window=map_window, noisy=noisy,
                far=tuple(far), unplaced=tuple(unplaced), w_hit=w_hit, w_miss=w_miss, ev_seed=ev_seed, readings=readings)


def _random_case(id_, seed, lidar_range, cell, origin, W, H, p, n, window, depth, margin=None, per_robot=False, **kw):
    """A map whose cells are solid with probability p, n robots in free cells over the grid and a margin around it -- robot 0 with
    its whole window inside the grid where the grid is large enough --, and one far robot at the end."""
    rng = np.random.default_rng(seed)
    cell2 = (cell, cell) if np.isscalar(cell) else cell
    if per_robot:
        occ = np.stack([(rng.random((W, H)) < p * (0.5 + b / n)).astype(np.uint8) for b in range(n + 1)])
        shared = np.zeros((W, H), np.uint8)                  # (robots are drawn anywhere: some stand in solid cells of their map)
    else:
        occ = shared = (rng.random((W, H)) < p).astype(np.uint8)
    pos = _free_robots(rng, shared, origin, cell2, n, 0.6 * lidar_range if margin is None else margin)
    first = _inner_robot(rng, shared, origin, cell2, G.window_half(lidar_range, cell2))
    if first is not None:
        pos[0] = first
    pos = np.concatenate([pos, [_far(origin, cell2, W, H, lidar_range)]])
    return _case(id_, lidar_range, cell, origin, occ, pos, window, depth, far=(n,), **kw)


# -- window shapes ------------------------------------------------------------------------------------------------------------
THIN = 1.0 / 4912.5                        # range 1.0: floor(4912.5) + 2 = 4914 -> 9829 cells, x 5 = 49145 <= 49152
OVER = 1.0 / 4913.5                        # 9831 x 5 = 49155: refused
CAP_DEPTH = 5e-5                           # (1 + 5e-5) * 4912.5 = 4912.7: the same window
OVER_DEPTH = 2e-4                          # (1 + 2e-4) * 4912.5 = 4913.5: 9831 x 5, refused by its depth alone

REFUSED = dict(id="w5x9831", lidar_range=1.0, cell=(2.0, OVER), window=(5, 9831))
REFUSED_BY_DEPTH = dict(id="w5x9829_depth", lidar_range=1.0, cell=(2.0, THIN), depth=OVER_DEPTH, window=(5, 9829), map_window=(5, 9831))


def _thin_occ(rng, W, H, p):
    """Cells of 2 m x 0.2 mm: a ray runs through up to 4912 cells of one column; solid with probability p (a free path of ~ 1 / p
    cells, i.e. of about the range)."""
    return (rng.random((W, H)) < p).astype(np.uint8)


def _thin_case(id_, seed, transpose, n, per_robot=False, **kw):
    rng = np.random.default_rng(seed)
    W, H = 4, 24000                                         # 8 m x 4.9 m
    cell, window = (2.0, THIN), (5, 9829)
    if per_robot:
        occ = np.stack([_thin_occ(rng, W, H, 1.0 / (3000 + 1500 * b)) for b in range(n + 1)])
    else:
        occ = _thin_occ(rng, W, H, 1.0 / 5000)
    # robots within a metre of a column boundary (they see into the next column) and in the middle of a column; robot 0's window
    # inside the grid along the thin axis
    pos = np.stack([rng.choice([1.1, 1.6, 2.3, 3.9, 4.4, 5.0], n), rng.uniform(-0.2, H * THIN + 0.2, n)], 1)
    pos[0] = (2.3, 0.5 * H * THIN + 0.013)
    pos = np.concatenate([pos, [(3.0, H * THIN + 7.0)]])
    cj = int(math.floor(pos[0, 1] / THIN))
    if not per_robot:                                       # a reading at the far end of the window: solid cells 0.99 m ahead of robot 0
        occ[:, cj - 3000:cj + 4850] = 0
        occ[1, cj + 4850:cj + 4900] = 1
    # ... and solid cells in the window's last column (two columns from robot 0's: staged, beyond any reading), in its last trips
    (occ[0] if per_robot else occ)[3, cj + 4860:cj + 4900] = 1
    for b in range(len(pos) - 1):                           # the robots' own cells are free
        (occ[b] if per_robot else occ)[int(pos[b, 0] // 2.0) % W, int(np.clip(math.floor(pos[b, 1] / THIN), 0, H - 1))] = 0
    if transpose:
        occ = np.ascontiguousarray(np.swapaxes(occ, -1, -2))
        pos, cell, window = pos[:, ::-1], cell[::-1], window[::-1]
    return _case(id_, 1.0, cell, (0.0, 0.0), occ, pos, window, CAP_DEPTH, noisy=False, far=(n,), **kw)


def _shape_cases():
    c = []
    # 9 x 5 = 45 cells < one trip; range < the cell's height: a dense map, or no ray meets anything
    c.append(_random_case("w9x5", 101, 1.0, (0.4, 1.5), (0.3, -0.2), 40, 30, 0.30, 40, (9, 5), 0.1, w_hit=5, w_miss=2, ev_seed=1))
    c.append(_random_case("w23x23", 102, 0.95, 0.1, (0.3, -0.2), 60, 50, 0.05, 32, (23, 23), 0.03, w_hit=2, w_miss=3))
    c.append(_random_case("w35x35", 103, 1.55, 0.1, (0.3, -0.2), 80, 70, 0.04, 32, (35, 35), 0.04))
    c.append(_random_case("w63x63", 104, 1.48, 0.05, (0.3, -0.2), 140, 130, 0.02, 32, (63, 63), 0.015))
    c.append(_random_case("w65x65", 105, 1.5, 0.05, (0.3, -0.2), 140, 130, 0.02, 32, (65, 65), 0.025))
    c.append(_random_case("w11x305", 106, 1.505, (0.4, 0.01), (0.3, -0.2), 40, 700, 0.01, 24, (11, 305), 0.002, margin=0.5))
    c.append(_random_case("w305x11", 107, 1.505, (0.01, 0.4), (0.3, -0.2), 700, 40, 0.01, 24, (305, 11), 0.002, margin=0.5, ev_seed=2))
    c.append(_random_case("w221x221", 108, 5.42, 0.05, (0.3, -0.2), 300, 300, 0.003, 12, (221, 221), 0.02, margin=1.0, noisy=False,
                          w_hit=9, w_miss=4))
    c.append(_thin_case("w5x9829", 109, False, 6, w_hit=11, w_miss=5))
    c.append(_thin_case("w9829x5", 110, True, 6, w_hit=4, w_miss=7, ev_seed=3))
    # one map per robot, at a small window and at the cap
    c.append(_random_case("per_robot_23", 111, 0.95, 0.1, (0.3, -0.2), 60, 50, 0.06, 16, (23, 23), 0.03, per_robot=True))
    c.append(_thin_case("per_robot_cap", 112, False, 5, per_robot=True))
    return c


# -- resolutions --------------------------------------------------------------------------------------------------------------
SCAN_RESOLUTIONS = (1, 2, 4, 7, 8, 63, 64, 65, 192, 193, 383, 384)
MAP_RESOLUTIONS = (63, 65, 193)


def _resolution_case(R):
    """The 35 x 35 window on a 12 % map.  With one or two rays a robot is kept only if a ray of its scan has a reading (one reading
    per robot on average is otherwise out of reach); the far robot at the end has none."""
    rng = np.random.default_rng(200 + R)
    lidar_range, cell, origin, W, H = 1.55, (0.1, 0.1), (0.3, -0.2), 64, 56
    occ = (rng.random((W, H)) < 0.12).astype(np.uint8)
    table = L.ray_table(R)
    pos = []
    while len(pos) < 24:
        p = _free_robots(rng, occ, origin, cell, 1, 0.5)[0]
        if R > 2 or G.grid_hits(p, occ, origin, cell, lidar_range, table)[1].all():
            pos.append(p)
    pos = np.concatenate([pos, [_far(origin, cell, W, H, lidar_range, R)]])
    return _case(f"res{R}", lidar_range, cell, origin, occ, pos, (35, 35), 0.04, resolution=R, far=(24,))


# -- exact positions ------------------------------------------------------------------------------------------------------------
EXACT_RIM = (56, 20)                                          # cell of the exact cases' robot 5


def _exact_case(R):
    """Cells of 2^-4 at an integer origin, range 1: robots exactly on an x boundary, on a y boundary and on a corner of their cell
    (first crossings at t = 0); solid cells on the robots' axes, and beside the diagonals on the side a ray enters only when a
    t_x == t_y tie goes to x (the cell (a + sign_x, b) next to a diagonal cell (a, b))."""
    c, origin, W, H = 2.0 ** -4, (2.0, 2.0), 112, 112
    occ = np.zeros((W, H), np.uint8)
    # (the corner robots have x0 == y0: cos and sin of 45 degrees differ in their last bit, and only where x0 + range * cos and
    # y0 + range * sin round alike is d_x == d_y and every crossing of the diagonal ray a tie)
    sites = {"x": (24, 84, 0.0, 0.5), "y": (84, 24, 0.5, 0.0), "corner": (40, 40, 0.0, 0.0), "corner2": (88, 88, 0.0, 0.0),
             "centre": (64, 64, 0.5, 0.5)}
    pos = []
    for ci, cj, fx, fy in sites.values():
        pos.append((origin[0] + (ci + fx) * c, origin[1] + (cj + fy) * c))
        for k in (6, 11):                                    # on the axes
            occ[ci + k, cj] = occ[ci - k, cj] = occ[ci, cj + k] = occ[ci, cj - k] = 1
        for k in (2, 5, 9):                                  # beside the four diagonals of a robot on its cell's lower-left corner
            occ[ci + k + 1, cj + k] = occ[ci - 2 - k, cj + k] = occ[ci - 2 - k, cj - 1 - k] = occ[ci + k + 1, cj - 1 - k] = 1
    # a robot on a corner with solid cells whose near face is EXACTLY the range (16 cells) away along its four axis rays and
    # nothing in front of them: found at t = 1, at a distance that is not strictly below the range -- no reading
    ci, cj = EXACT_RIM
    pos.append((origin[0] + ci * c, origin[1] + cj * c))
    occ[ci + 16, cj] = occ[ci - 17, cj] = occ[ci, cj + 16] = occ[ci, cj - 17] = 1
    pos.append(_far(origin, (c, c), W, H, 1.0))
    return _case(f"exact{R}", 1.0, c, origin, occ, np.array(pos), (37, 37), 2.0 ** -6, resolution=R, far=(len(sites) + 1,))


# -- coordinates ----------------------------------------------------------------------------------------------------------------
def _large_origin_case():
    """(ox + a dx) - x0 at |ox| = 1e6: the crossings are formed from doubles 1.2e-10 apart."""
    return _random_case("origin1e6", 301, 1.5, 0.05, (1e6 + 0.3, -1e6 - 0.2), 120, 120, 0.03, 24, (65, 65), 0.025, margin=0.0)


def _cell_limit_case():
    """Cells of 2^-10 at origin 0: robots at +-2^20 have cell index +-2^30 (no cell: no reading, nothing mapped), robots one cell
    inside of that have index +-(2^30 - 1) (a cell, far from the grid); the ordinary robots in front of them scan a 64 x 64 grid."""
    rng = np.random.default_rng(302)
    c, W, H = 2.0 ** -10, 64, 64
    occ = (rng.random((W, H)) < 0.05).astype(np.uint8)
    pos = list(_free_robots(rng, occ, (0.0, 0.0), (c, c), 12, 0.01))
    big = 2.0 ** 20
    placed = [(big - c, 0.01), (-big + c, 0.01), (0.01, big - c), (0.01, -big + c)]
    unplaced = [(big, 0.01), (-big, 0.01), (0.01, big), (0.01, -big)]
    pos = np.array(pos + placed + unplaced)
    return _case("cell2p30", 0.02, c, (0.0, 0.0), occ, pos, (45, 45), 2.0 ** -12, far=range(12, 16), unplaced=range(16, 20))


# -- grids ------------------------------------------------------------------------------------------------------------------------
def _grid_cases():
    c = []
    rng = np.random.default_rng(401)
    one = np.ones((1, 1), np.uint8)                          # a single solid cell, robots around it and one in it
    lo = np.array((0.5, 0.5))
    pos = np.concatenate([lo + 0.05 + rng.uniform(-0.8, 0.8, (23, 2)), [lo + 0.05], [_far(lo, (0.1, 0.1), 1, 1, 0.95)]])
    c.append(_case("g1x1", 0.95, 0.1, lo, one, pos, (23, 23), 0.03, far=(24,)))
    c.append(_random_case("g3000x1", 402, 1.5, 0.05, (0.3, -0.2), 3000, 1, 0.05, 32, (65, 65), 0.025, margin=1.0))
    c.append(_random_case("g1x3000", 403, 1.5, 0.05, (0.3, -0.2), 1, 3000, 0.05, 32, (65, 65), 0.025, margin=1.0))
    # a grid that lies wholly inside the window of the robots in it (20 < 32 cells), robots inside it and outside it
    c.append(_random_case("g20x20", 404, 1.5, 0.05, (0.3, -0.2), 20, 20, 0.06, 32, (65, 65), 0.025, margin=1.2))
    return c


# -- a range of zero ----------------------------------------------------------------------------------------------------------------
def _range0_case():
    """lidar_range = 0: a 5 x 5 window, every ray has d = 0 and ends where it starts.  No reading; the map gets hand-written
    readings in the cells around the robot (its depth is the whole reach)."""
    rng = np.random.default_rng(501)
    cell, origin, W, H, R = (0.1, 0.08), (0.3, -0.2), 30, 24, 16
    occ = (rng.random((W, H)) < 0.2).astype(np.uint8)
    pos = np.concatenate([_free_robots(rng, occ, origin, cell, 15, 0.15), [_far(origin, cell, W, H, 0.0)]])
    readings = {}
    for b in range(len(pos)):
        h = np.full((R, 2), np.nan)
        h[:6] = pos[b] + rng.uniform(-2.4, 2.4, (6, 2)) * cell
        readings[b] = h
    return _case("range0", 0.0, cell, origin, occ, pos, (5, 5), 0.02, resolution=R, far=(15,), readings=readings)


# -- hand-written readings ------------------------------------------------------------------------------------------------------------
def _synthetic_case():
    """The 65 x 65 map case with robot 2's readings written by hand, ray by ray: the robot's own position (L = 0), an infinite,
    an overflowing, a half-NaN, a denormal coordinate, a reading in the robot's own cell, one beyond the window, an ordinary one."""
    base = _random_case("synthetic", 601, 1.5, 0.05, (0.3, -0.2), 140, 130, 0.02, 16, (65, 65), 0.025, resolution=16)
    p = np.array([3.012, 2.513])
    base["pos"][2] = p
    h = np.full((16, 2), np.nan)
    h[0] = p
    h[1] = (np.inf, p[1])
    h[2] = (1e300, p[1] + 0.3)
    h[3] = (np.nan, p[1])
    h[4] = (p[0], np.nan)
    h[5] = (5e-324, p[1] - 0.4)
    h[6] = p + (0.004, -0.003)
    h[7] = p + (9.0 * math.cos(2.2), 9.0 * math.sin(2.2))
    h[8] = p + (0.61, 0.42)
    h[9] = (-1e300, -1e300)
    h[10] = (p[0] - 0.7, 5e-324 + p[1])
    base["readings"] = {2: h}
    return base


CASE_IDS = ("w9x5", "w23x23", "w35x35", "w63x63", "w65x65", "w11x305", "w305x11", "w221x221", "w5x9829", "w9829x5", "per_robot_23",
            "per_robot_cap") + tuple(f"res{R}" for R in SCAN_RESOLUTIONS) + ("exact4", "exact8", "origin1e6", "cell2p30", "g1x1",
                                                                              "g3000x1", "g1x3000", "g20x20", "range0", "synthetic")
NOT_SCANNED = ("synthetic",)                                 # map only: the scan of its inputs is the w65x65 case's
NOT_MAPPED = tuple(f"res{R}" for R in SCAN_RESOLUTIONS if R not in MAP_RESOLUTIONS) + ("per_robot_23", "per_robot_cap")
SCAN_IDS = tuple(i for i in CASE_IDS if i not in NOT_SCANNED)
MAP_IDS = tuple(i for i in CASE_IDS if i not in NOT_MAPPED)
CAP_IDS = ("w221x221", "w5x9829", "w9829x5", "per_robot_cap")
NOISE_FREE_IDS = CAP_IDS                                      # the scan runs with noise too, except at the cap (the oracle is the slow part)
EDGE_IDS = ("w23x23", "w35x35", "w63x63", "w11x305", "w305x11")       # last row and last column of the window must hold something
EXACT_IDS = ("exact4", "exact8")


@functools.lru_cache(maxsize=None)
def all_cases():
    """{id: case}, built once (read only)."""
    cases = _shape_cases() + [_resolution_case(R) for R in SCAN_RESOLUTIONS] + [_exact_case(4), _exact_case(8), _large_origin_case(),
                                                                                _cell_limit_case()] + _grid_cases()
    cases += [_range0_case(), _synthetic_case()]
    out = {c["id"]: c for c in cases}
    assert tuple(out) == CASE_IDS, tuple(out)
    return out


def case(id_):
    return all_cases()[id_]


def occ_of(c, b):
    return c["occ"] if c["occ"].ndim == 2 else c["occ"][b]


def noise_of(c):
    """The case's noise sample [B,R,2]: the sensor's sigma of 0.01 m, seeded by the case's name."""
    rng = np.random.default_rng(sum(map(ord, c["id"])))
    return 0.01 * rng.standard_normal((len(c["pos"]), c["resolution"], 2))


@functools.lru_cache(maxsize=None)
def scan_oracle(id_):
    """[(hits [R,2], valid [R], counts)] per robot of a case, by tests/grid_lidar_oracle.py: computed once and shared (read only)."""
    c = case(id_)
    table = L.ray_table(c["resolution"])
    return [G.grid_hits(p, occ_of(c, b), c["origin"], c["cell"], c["lidar_range"], table, counts=True) for b, p in enumerate(c["pos"])]


def oracle_hits(id_):
    """hits [B,R,2] (NaN = no reading) of the case, noise-free, as the device's scan must write them."""
    c = case(id_)
    out = np.full((len(c["pos"]), c["resolution"], 2), np.nan)
    for b, (h, valid, _) in enumerate(scan_oracle(id_)):
        out[b, valid] = h[valid]
    return out


def corner_reading(c, b=0):
    """A reading in the LAST ROW AND LAST COLUMN of robot b's map window: a quarter of a cell inside the cell (ci + nx, cj + ny), so
    that the push by ``depth`` (less than half a cell along the ray) leaves it there."""
    ci, cj = G.robot_cell(c["pos"][b], c["origin"], c["cell"])
    nx, ny = M.window_half(c["lidar_range"], c["depth"], c["cell"])
    return (c["origin"][0] + (ci + nx + 0.25) * c["cell"][0], c["origin"][1] + (cj + ny + 0.25) * c["cell"][1])


def map_readings(c, hits):
    """The readings the map tests upload: ``hits`` [B,R,2] of the case's scan (a copy) with the case's hand-written readings in
    their robots' rows, and robot 0's ray 0 replaced by ``corner_reading`` (cases without hand-written readings for robot 0)."""
    hits = np.array(hits, float)
    for b, h in (c["readings"] or {}).items():
        hits[b] = h
    if not (c["readings"] and 0 in c["readings"]):
        hits[0, 0] = corner_reading(c)
    return hits


def map_mask(c):
    """One masked robot per case: robot 1."""
    mask = np.ones(len(c["pos"]), np.int32)
    mask[1] = 0
    return mask


def evidence0(c):
    """The evidence the update starts from: zeros, or a seeded int32 pattern [W,H] (the same for every per-robot map)."""
    if c["ev_seed"] is None:
        return np.zeros((c["W"], c["H"]), np.int32)
    return np.random.default_rng(c["ev_seed"]).integers(-1000, 1000, (c["W"], c["H"])).astype(np.int32)


def window_bit(c, b, cells, half):
    """Bit index li * wh + lj of grid cells [n,2] in robot b's window of half-sizes ``half``."""
    ci, cj = G.robot_cell(c["pos"][b], c["origin"], c["cell"])
    cells = np.asarray(cells).reshape(-1, 2)
    return (cells[:, 0] - (ci - half[0])) * (2 * half[1] + 1) + (cells[:, 1] - (cj - half[1]))


def staged_solid(c, b):
    """(li, lj) [n,2] of the solid cells of the grid in robot b's scan window: the bits the scan stages."""
    cell0 = G.robot_cell(c["pos"][b], c["origin"], c["cell"])
    if cell0 is None:
        return np.zeros((0, 2), np.int64)
    nx, ny = G.window_half(c["lidar_range"], c["cell"])
    i0, j0 = cell0[0] - nx, cell0[1] - ny
    a, b_ = max(i0, 0), max(j0, 0)
    sub = occ_of(c, b)[a:max(min(i0 + 2 * nx + 1, c["W"]), a), b_:max(min(j0 + 2 * ny + 1, c["H"]), b_)]
    return np.argwhere(sub != 0) + (a - i0, b_ - j0)


def map_marks(c, hits, b):
    """(passed, hit, (wi0, wj0), counts) of robot b by tests/map_oracle.py on the readings ``hits`` [B,R,2], or None."""
    return M.robot_marks(c["pos"][b], hits[b], c["origin"], c["cell"], c["lidar_range"], L.ray_table(c["resolution"]), c["depth"], counts=True)


def map_deltas(c, hits, mask):
    """[B,W,H] int64: what each robot's scan adds to the evidence, by tests/map_oracle.py (a masked robot: nothing)."""
    table = L.ray_table(c["resolution"])
    out = np.zeros((len(c["pos"]), c["W"], c["H"]), np.int64)
    for b, p in enumerate(c["pos"]):
        if mask[b]:
            out[b] = M.robot_delta(p, hits[b], c["W"], c["H"], c["origin"], c["cell"], c["lidar_range"], table, c["depth"], c["w_hit"], c["w_miss"])[0]
    return out
