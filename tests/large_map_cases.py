"""Inputs of the large-map tests, shared by tests/test_large_map_oracle.py (CPU: does every case reach what it claims, on the
oracles alone?) and tests/test_large_map_gpu.py (grid scan, map update, the tiled planners and UnknownEnvFleet.run_exploring
against the oracles on the same inputs, above the 2^17 cells the one-workgroup planners stop at).  numpy, the library's host-only
tiled_info and the committed oracles; every shape but 363 x 362 is derived from the tile sides TW x TH (cells along i and along j)
and the 4096 side cap, every input is seeded, oracles are computed once per case and shared, read only.

A SHAPE is dict(id, W, H, origin, cell, occ [W,H] uint8, stations {name: (x, y)} (insertion order = robot order), anchor (CI, CJ):
the cell at a tile border the centre stations stand round, box: the region whose truth the preset evidence holds, notch: cells of the
box that stay unknown all the same):
  first_refused  363 x 362, the first shape the one-workgroup calls refuse: 12 x 6 tiles.  The anchor is the four-tile corner
                 nearest the middle; the preset box is 3 x 3 tiles' worth of cells round it, all free but the anchor block.
  long_j         (TW + 1) x 4096: 2 x 64 tiles, the second tile row ONE cell wide.  A corridor of known cells runs along the
                 whole long side between the map's last row and a solid wall, and ends 24 cells before the far end: what lies
                 beyond is unknown, so the nearest frontier of the near-end stations is in the last tile column.
  long_i         4096 x (TW + 1), long_j transposed (map, stations and placement): 128 x 1 tiles, tiles_j = 1.
The placement is tests/grid_checks.py's anisotropic one, origin (-0.35, 0.2), cell (0.1, 0.125); long_i has it transposed with
its map, origin (0.2, -0.35), cell (0.125, 0.1).  (With cell (0.1, 0.125) a window at range 1.5 is 35 x 29 cells: 35 > TW + 1
along i, but 29 < TW + 1 along j.  Only the transposed placement makes the window wider than BOTH long maps, which is what the
long maps are here for; LONG_WINDOW_WIDER is asserted below.)

STATIONS, in robot order: origin (cell (1, 1): the window hangs over both low edges), far_corner (the last free cell before the
block on (W - 1, H - 1): the largest flat indices, the window over both high edges), corner (three cells inside the anchor: the
anchor block in range), border (x exactly ox + CI dx, CI a multiple of TW: a cell boundary that is a tile border, the march's
tie rule), outside (four cells outside the grid, a block in range), solid (in a cell of the anchor block), far (no window on
the grid: contributes nothing).

``corner_wake`` at the end is the one small map here (3 x 2 tiles): the case in which only the corner flag of a tiled round wakes
the diagonal tile -- the large shapes cannot hold it, since wherever a wave crosses a four-tile corner the side tiles' rims fall too."""
import functools

import numpy as np

import assign_oracle as AO
import field_tiled_cases as T
import frontier_oracle as FR
import gain_oracle as GO
import grid_lidar_oracle as G
import lidar_oracle as L
import map_oracle as M
from grid_checks import CELL, ORIGIN

TW, TH, MAX_CELLS = T.TW, T.TH, T.MAX_CELLS
SIDE_CAP = 4096
OLD_CAP = 1 << 17
RANGE, RESOLUTION, W_HIT, W_MISS = 1.5, 360, 3, 1             # the exploration goldens'
T_FREE, T_OCC = W_MISS, W_HIT                                  # a planner on a mapper: its weights are the thresholds
NOISE_STD = 0.01
R_INFLATE, MIN_UNKNOWN, MAX_SEG, S_MAX = 1, 3, 400, 64         # (3 unknown neighbours: a cell beside one or two cells that a reading
                                                               # pushed past a block's corner turned unknown again is no frontier cell;
                                                               # max_seg 400 = 80 cells: a 4000-cell path is 50 sub-goals)
INFORMED = dict(r_view=8, w_gain=16, g_cap=120, min_gain=2)
CLAIMS = dict(r_claim=12, max_claims=3)
IDS = ("first_refused", "long_j", "long_i")
LONG_IDS = ("long_j", "long_i")
STATIONS = ("origin", "far_corner", "corner", "border", "outside", "solid", "far")
IN_GRID = ("origin", "far_corner", "corner", "border", "solid")
MASKED = ("origin", "corner")                                  # the two stations the first map update skips
RUNNERS = ("corner", "border", "origin", "far_corner")         # the four robots of the exploring run
CORRIDOR = 10                                                  # cells across the long maps' corridor
GAP = 24                                                       # unknown cells between the corridor's end and the far end


def _centre(c, origin, cell, off=(0.5, 0.5)):
    return (origin[0] + (c[0] + off[0]) * cell[0], origin[1] + (c[1] + off[1]) * cell[1])


def _square():
    W, H = 363, 362
    ci, cj = TW * int(round(W / TW / 2)), TH * int(round(H / TH / 2))
    occ = np.zeros((W, H), np.uint8)
    box = (ci - 3 * TW // 2, ci + 3 * TW // 2, cj - 3 * TH // 2, cj + 3 * TH // 2)
    return W, H, (ci, cj), occ, box, (-4.0, 3.3), []


def _long_j():
    W, H = TW + 1, SIDE_CAP
    ci, cj = TW, TH                                            # the first four-tile corner along the long side
    occ = np.zeros((W, H), np.uint8)
    wall = W - CORRIDOR - 1
    occ[wall, :H - GAP] = 1                                    # the corridor's wall: rows wall + 1 .. W - 1 are the corridor
    occ[6:8, TH + 8:TH + 11] = 1                               # a block in range of the outside station
    box = (wall, W, 0, H - GAP)
    # three cells of the corridor's last-but-one row, near its end, stay unknown: the cell of the LAST row beside them -- the
    # one-cell tile row -- is then a frontier cell (at the corridor's flat end a cell of the map's edge row has two unknown neighbours)
    notch = [(W - 2, H - GAP - 6 + k) for k in range(3)]
    return W, H, (ci, cj), occ, box, (-4.0, TH + 6.3), notch


def _shape(id_):
    W, H, (ci, cj), occ, box, outside, notch = _square() if id_ == "first_refused" else _long_j()
    origin, cell = ORIGIN, CELL
    occ[W - 3:, H - 4:] = 1                                    # covers cells of the last row and column, (W - 1, H - 1) included
    occ[ci - 1:ci + 1, cj - 1:cj + 1] = 1                      # the anchor block: straddles the corner where four tiles meet
    occ[5:8, 4:7] = 1                                          # within range of the origin corner
    away = 3.0 * RANGE + 10.0 * max(cell) + 1.0
    st = dict(origin=_centre((1, 1), origin, cell, (0.3, 0.6)),
              far_corner=_centre((W - 4, H - 5), origin, cell, (0.7, 0.4)),
              corner=_centre((ci - 3, cj - 3), origin, cell, (0.2, 0.3)),
              border=(origin[0] + ci * cell[0], origin[1] + (cj - 5 + 0.37) * cell[1]),
              outside=_centre(outside, origin, cell, (0.0, 0.0)),
              solid=_centre((ci - 1, cj - 1), origin, cell, (0.4, 0.6)),
              far=(origin[0] + W * cell[0] + away, origin[1] - away))
    if id_ == "long_i":                                        # the transpose: map, stations, placement; the tile border is along i again
        occ, W, H, origin, cell = np.ascontiguousarray(occ.T), H, W, origin[::-1], cell[::-1]
        st = {k: v[::-1] for k, v in st.items()}
        ci, cj, box, notch = cj, ci, (box[2], box[3], box[0], box[1]), [c[::-1] for c in notch]
        st["border"] = (origin[0] + TW * cell[0], origin[1] + (cj - 3 + 0.37) * cell[1])      # (tiles_j = 1: the one tile border is along i)
    assert tuple(st) == STATIONS
    return dict(id=id_, W=W, H=H, origin=tuple(origin), cell=tuple(cell), occ=occ, stations=st, anchor=(ci, cj), box=box, notch=notch)


@functools.lru_cache(maxsize=None)
def shape(id_):
    return _shape(id_)


def positions(s, names=STATIONS):
    return np.array([s["stations"][n] for n in names], np.float64)


def index(name, names=STATIONS):
    return names.index(name)


def tiles(s):
    """(tiles along i, tiles along j)."""
    return -(-s["W"] // TW), -(-s["H"] // TH)


def tile_of_flat(s, flat):
    return (flat // s["H"]) // TW, (flat % s["H"]) // TH


def scan_half(s):
    return G.window_half(RANGE, s["cell"])


def map_half(s):
    return M.window_half(RANGE, M.default_depth(s["cell"]), s["cell"])


def window_wider_than_the_map(s):
    """Is the scan window, (2 nx + 1) x (2 ny + 1) cells round a robot's cell, wider than the whole map along one axis?  (Then no
    station on the map has a window row that lies inside the grid from end to end along that axis.)"""
    nx, ny = scan_half(s)
    return 2 * nx + 1 > s["W"] or 2 * ny + 1 > s["H"]


LONG_WINDOW_WIDER = all(window_wider_than_the_map(shape(i)) for i in LONG_IDS)
assert LONG_WINDOW_WIDER


def per_robot_occ(s, names=STATIONS):
    """[B,W,H]: the map once per robot, and in robot b's map one more 2 x 2 block three cells from ITS station (where one fits
    the grid) -- a block that moves with the robot, so a kernel that reads another robot's map sees another scan."""
    occ = np.repeat(s["occ"][None], len(names), 0)
    for b, n in enumerate(names):
        c = G.robot_cell(s["stations"][n], s["origin"], s["cell"])
        for di, dj in ((3, -3), (-3, 3), (3, 3), (-3, -3)):          # the first place round the station where the block fits the grid
            i, j = c[0] + di, c[1] + dj
            if 0 <= i and i + 2 <= s["W"] and 0 <= j and j + 2 <= s["H"]:
                occ[b, i:i + 2, j:j + 2] = 1
                break
    return occ


def noise(s, K=None, names=STATIONS):
    """The given noise: [B,R,2], or [K,B,R,2] for a run of K samples -- the sensor's sigma, seeded by the shape's name (as
    tests/test_frontier_fleet_gpu.py makes a run's)."""
    rng = np.random.default_rng(sum(map(ord, s["id"])))
    return NOISE_STD * rng.standard_normal(((K,) if K else ()) + (len(names), RESOLUTION, 2))


def preset(s):
    """The evidence a test starts from: the true map in the shape's box (-w_miss on a free cell, +w_hit on a solid one), the rest
    unknown."""
    i0, i1, j0, j1 = s["box"]
    ev = np.zeros((s["W"], s["H"]), np.int32)
    ev[i0:i1, j0:j1] = np.where(s["occ"][i0:i1, j0:j1] != 0, W_HIT, -W_MISS)
    for c in s["notch"]:
        ev[tuple(c)] = 0
    return ev


def random_evidence(s, seed):
    """A seeded pattern in -5 .. 5: what the update tests start from, so that addition is checked and not assignment."""
    return np.random.default_rng(seed).integers(-5, 6, (s["W"], s["H"])).astype(np.int32)


def mask(names=STATIONS):
    return np.array([0 if n in MASKED else 1 for n in names], np.int32)


def hand_made_hits(s, names=STATIONS):
    """[B,R,2] readings written by hand: per robot a ring of readings at 0.4 .. 1.4 m on every fourth ray, NaN rows (no reading),
    half-NaN rows, an infinite one and one in the robot's own cell."""
    table = L.ray_table(RESOLUTION)
    pos = positions(s, names)
    rng = np.random.default_rng(len(s["id"]) + 7)
    hits = np.full((len(pos), RESOLUTION, 2), np.nan)
    for b, p in enumerate(pos):
        rays = np.arange(b % 4, RESOLUTION, 4)
        hits[b, rays] = p + rng.uniform(0.4, 1.4, (len(rays), 1)) * table[rays]
        hits[b, rays[1], 0] = np.nan
        hits[b, rays[2], 1] = np.nan
        hits[b, rays[3], 0] = np.inf
        hits[b, rays[4]] = p + (0.004, -0.003)
    return hits


# -- oracles, computed once ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scan_oracle(id_, per_robot=False):
    """[(hits [R,2], valid [R])] per station by tests/grid_lidar_oracle.py, on the shared map or on ``per_robot_occ``."""
    s = shape(id_)
    occ = per_robot_occ(s) if per_robot else None
    table = L.ray_table(RESOLUTION)
    return [G.grid_hits(p, s["occ"] if occ is None else occ[b], s["origin"], s["cell"], RANGE, table) for b, p in enumerate(positions(s))]


def oracle_hits(id_, noise_=None):
    """hits [B,R,2] (NaN = no reading) as the device's scan must write them."""
    out = np.full((len(STATIONS), RESOLUTION, 2), np.nan)
    for b, (h, valid) in enumerate(scan_oracle(id_)):
        out[b, valid] = h[valid] if noise_ is None else (h + noise_[b])[valid]
    return out


def update(s, ev, pos, hits, mask_=None):
    """tests/map_oracle.py's update with the shapes' settings (in place, returned)."""
    return M.update(ev, pos, hits, s["origin"], s["cell"], RANGE, L.ray_table(RESOLUTION), None, W_HIT, W_MISS, mask_)


@functools.lru_cache(maxsize=None)
def sample_evidence(id_):
    """int32 [W,H]: the preset plus one noise-free scan of every station, by the oracles."""
    s = shape(id_)
    return update(s, preset(s).astype(np.int64), positions(s), oracle_hits(id_)).astype(np.int32)


def frontier_plan(s, ev, pos):
    return FR.plan_batch(ev, T_FREE, T_OCC, s["origin"], s["cell"], pos, R_INFLATE, MIN_UNKNOWN, MAX_SEG, S_MAX)


def informed_plan(s, ev, pos, nearest=None):
    return GO.plan_batch(ev, T_FREE, T_OCC, s["origin"], s["cell"], pos, INFORMED["r_view"], INFORMED["w_gain"], INFORMED["g_cap"],
                         INFORMED["min_gain"], R_INFLATE, MIN_UNKNOWN, MAX_SEG, S_MAX, nearest=nearest)


def claim_plan(s, ev, pos, nearest=None, may_claim=None):
    return AO.plan_batch(ev, T_FREE, T_OCC, s["origin"], s["cell"], pos, CLAIMS["r_claim"], CLAIMS["max_claims"], R_INFLATE, MIN_UNKNOWN,
                         MAX_SEG, S_MAX, may_claim, nearest=nearest)


@functools.lru_cache(maxsize=None)
def plan_oracle(id_, kind):
    """The oracle's plan of all stations on ``sample_evidence``: kind "frontier", "informed" or "claims"."""
    s = shape(id_)
    ev, pos = sample_evidence(id_), positions(s)
    if kind == "frontier":
        return frontier_plan(s, ev, pos)
    return (informed_plan if kind == "informed" else claim_plan)(s, ev, pos, nearest=plan_oracle(id_, "frontier"))


def claim_fields(want):
    """The field of every claim round of an assign oracle's result, restated from its records: the sources left before round k."""
    fld = want["nearest"]["field"][0]
    passable = fld != AO.INF
    sources = (want["nearest"]["frontier"][0] != 0) & passable
    out = []
    for t in want["targets"]:
        out.append(AO.field_of(passable, sources))
        sources = sources & ~AO.disc(*fld.shape, t, CLAIMS["r_claim"])
    return out


def changes_down(ufld):
    """Per cell, how often its descent path down a utility field changes tile (a source that holds its own seed: 0); -1 on INF
    (tests/test_gain_tiled_gpu.py's helper, without torch)."""
    W, H = ufld.shape
    changes = np.full((W, H), -1, np.int64)
    for flat in np.argsort(ufld, axis=None, kind="stable"):
        c = (int(flat) // H, int(flat) % H)
        if ufld[c] == GO.INF:
            break
        try:
            n = T.descent_step(ufld, c)
            changes[c] = changes[n] + (T.tile_of(c) != T.tile_of(n))
        except AssertionError:
            changes[c] = 0
    return changes


@functools.lru_cache(maxsize=None)
def budgets(id_, kind):
    """A fixed budget of rounds from the round guarantee (field_tiled_cases.rounds_to_settle) on the oracle's own fields: for the
    frontier field; for "informed" the larger of that and the utility field's; for "claims" the largest of that and every claim
    round's field's."""
    near = plan_oracle(id_, "frontier")
    b = T.rounds_to_settle(near["field"][0])
    if kind == "informed":
        b = max(b, int(changes_down(plan_oracle(id_, "informed")["ufield"][0]).max()) + 2)
    if kind == "claims":
        b = max([b] + [T.rounds_to_settle(f) for f in claim_fields(plan_oracle(id_, "claims"))])
    return b


@functools.lru_cache(maxsize=None)
def per_robot_sample_evidence(id_):
    """int32 [B,W,H]: one map per station -- the preset, and in map b the noise-free scan of station b alone."""
    s = shape(id_)
    ev = np.repeat(preset(s)[None].astype(np.int64), len(STATIONS), 0)
    return update(s, ev, positions(s), oracle_hits(id_)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def per_robot_plan_oracle(kind):
    """The oracle's plan on ``per_robot_sample_evidence`` of 363 x 362 (F = B): kind "frontier" or "informed"."""
    s = shape("first_refused")
    ev, pos = per_robot_sample_evidence("first_refused"), positions(s)
    if kind == "frontier":
        return frontier_plan(s, ev, pos)
    return informed_plan(s, ev, pos, nearest=per_robot_plan_oracle("frontier"))


# -- the corner flag: a small map on which ONLY a corner cell's fall wakes the diagonal tile -------------------------------------
def corner_wake():
    """3 x 2 tiles, everything solid but three one-cell corridors that meet at the four-tile corner (TW, TH), each with an unknown
    cell behind its far end (r_inflate 0, min_unknown 1: the corridor's last cell is its frontier):
      C = (TW, TH), first cell of tile (1, 1): its corridor runs 40 cells down column TH into tile (2, 1) -- C gets v = 200 in ROUND 2;
      A = (TW - 1, TH), tile (0, 1), and B = (TW, TH - 1), tile (1, 0): corridors of 41 cells inside their own tiles -- both get
          v + 5 = 205 in round 1, and never fall again (C offers them v + 5);
      D = (TW - 1, TH - 1), last cell of tile (0, 0), no other free cell in its tile: 210 through A or B after round 2, and 207
          through C's diagonal -- which tile (0, 0) learns of only if C's fall, the fall of a CORNER cell of tile (1, 1), wakes it:
          no cell on the rim of tiles (0, 1) and (1, 0) falls after round 1.
    Returns dict(ev, start (the centres of D, A, B, C), cells dict(A, B, C, D), origin, cell)."""
    W, H, n = 3 * TW, 2 * TH, 40
    assert n > TW and n + 1 < TH and TW - 1 >= 1
    ev = np.full((W, H), W_HIT, np.int32)
    A, B, C, D = (TW - 1, TH), (TW, TH - 1), (TW, TH), (TW - 1, TH - 1)
    ev[TW:TW + n + 1, TH] = -W_MISS
    ev[TW + n + 1, TH] = 0
    ev[TW - 1, TH:TH + n + 2] = -W_MISS
    ev[TW - 1, TH + n + 2] = 0
    ev[TW, TH - 1 - (n + 1):TH] = -W_MISS
    ev[TW, TH - 1 - (n + 2)] = 0
    ev[D] = -W_MISS
    start = np.array([_centre(c, ORIGIN, CELL) for c in (D, A, B, C)])
    return dict(ev=ev, start=start, cells=dict(A=A, B=B, C=C, D=D), origin=ORIGIN, cell=CELL, r=0, mu=1)


@functools.lru_cache(maxsize=None)
def corner_wake_oracle():
    c = corner_wake()
    return FR.plan_batch(c["ev"], T_FREE, T_OCC, c["origin"], c["cell"], c["start"], c["r"], c["mu"], None, S_MAX)
