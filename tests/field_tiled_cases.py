"""Inputs of the tiled field tests, shared by tests/test_field_tiled_oracle.py (CPU: does every case reach what it claims?) and
tests/test_field_tiled_gpu.py (the tiled calls against the oracles on the same inputs).  numpy and the library's host-only
lipmpc_grid_tiled_info: every shape is derived from the tile sides TW x TH (cells along i and along j), none is written down.

A CASE is dict(id, occ [W,H] or [F,W,H] uint8 and goal [F,2] for the goal field, ev (occ's shape) int32 for the frontier field,
start [B,2], r, mu (min_unknown), max_seg, S_max).  ``ev`` holds occ's solid cells at T_OCC, the case's unknown cells at 0 and every
other cell at -T_FREE.  Oracles are computed once per case and planner and shared, read only."""
import functools

import numpy as np

import field_oracle as Fo
import field_shape_cases as S
import frontier_oracle as FR
import lipmpc

ORIGIN, CELL, T_FREE, T_OCC = S.ORIGIN, S.CELL, S.T_FREE, S.T_OCC
TW, TH, MAX_CELLS = lipmpc.planner.tiled_info()
centre = S.centre


def tile_of(c):
    return c[0] // TW, c[1] // TH


def tile_changes(cells):
    """How often a path of cells changes tile."""
    return sum(tile_of(a) != tile_of(b) for a, b in zip(cells[:-1], cells[1:]))


def _ev(occ, unknown):
    ev = np.full(occ.shape, -T_FREE, np.int32)
    ev[occ != 0] = T_OCC
    for c in unknown:
        ev[tuple(c)] = 0
    return ev


def _case(id_, occ, goal_cell, start_cells, unknown, r=0, mu=1, extra_starts=(), max_seg=S.MAX_SEG, S_max=S.S_MAX):
    """One shared map; the goal a little off its cell's centre, the starts at cell centres (+ given points)."""
    occ = np.asarray(occ, np.uint8)
    goal = np.array([centre(goal_cell) + (0.01, -0.02)])
    start = np.array([centre(c) for c in start_cells] + [np.asarray(p, np.float64) for p in extra_starts]).reshape(-1, 2)
    return dict(id=id_, occ=occ, ev=_ev(occ, unknown), goal=goal, start=start, r=r, mu=mu, max_seg=max_seg, S_max=S_max)


def _strip(id_, W, H, n_baffles=4):
    """field_shape_cases' strip: baffles across the short side, r_inflate 2, the unknown 2 x 2 block in the far corner, 16 starts
    (cell (0, 0), a solid cell, NaN, outside, random points)."""
    c = S.strip_case(W, H, n_baffles)
    return dict(id=id_, occ=c["occ"], ev=c["ev"], goal=c["goal"], start=c["start"], r=c["r"], mu=S.MU, max_seg=c["max_seg"], S_max=c["S_max"])


def _stack(id_, cases):
    """F = B per-robot maps from one-robot shared cases of one shape."""
    one = cases[0]
    return dict(id=id_, occ=np.stack([c["occ"] for c in cases]), ev=np.stack([c["ev"] for c in cases]),
                goal=np.concatenate([c["goal"] for c in cases]), start=np.concatenate([c["start"][:1] for c in cases]),
                r=one["r"], mu=one["mu"], max_seg=one["max_seg"], S_max=one["S_max"])


# -- the cases -----------------------------------------------------------------------------------------------------------
def two_by_two():
    return _case("2x2", np.zeros((2, 2)), (1, 1), [(0, 0), (1, 1)], unknown=[(1, 1)])


def spiral_side():
    return 2 * TW + 8


def spiral():
    """tests/field_oracle.py's spiral (263 cells at n = 24) at n = 2 TW + 8: a one-cell corridor that winds through every tile, from
    (1, 1) to the centre.  The goal is the centre end; the last corridor cell is unknown, so the one before it is the frontier."""
    occ, cells = Fo.spiral(spiral_side())
    c = _case("spiral", occ, cells[-2], [cells[0], cells[len(cells) // 2]], unknown=[cells[-1]], max_seg=250, S_max=1024)
    c["occ"][cells[-1]] = 1                                # (for the goal field the unknown cell is a wall: both corridors end at cells[-2])
    c["cells"] = cells[:-1]
    return c


CORNER = ((TW - 1, TH - 1), (TW - 1, TH), (TW, TH - 1), (TW, TH))      # the four cells round the corner where four tiles meet


def corner_goals():
    """A goal in each of the four cells round a 4-tile corner of an open 2 TW x 2 TH map (the frontier maps: that cell unknown, its
    eight neighbours, which lie in all four tiles, the frontier)."""
    far = [(2 * TW - 1, 2 * TH - 1), (0, 0), (0, 2 * TH - 1), (2 * TW - 1, 0)]
    return _stack("corner_goals", [_case("", np.zeros((2 * TW, 2 * TH)), g, [s], unknown=[g]) for g, s in zip(CORNER, far)])


def corner_cuts():
    """The no-corner-cut rule across tiles: the moving cell (TW, TH), the diagonal's target (TW - 1, TH - 1) -- the goal --, and the
    two side cells (TW - 1, TH) and (TW, TH - 1), each in a tile of its own.  Three maps: both side cells free, one solid, both solid.
    (The frontier maps: the cell beyond the target unknown, mu = 3 -- the target is the one free cell with three unknown neighbours.)"""
    cases = []
    unknown = [(TW - 2, TH - 2), (TW - 2, TH - 1), (TW - 1, TH - 2)]
    for solid in ((), (CORNER[1],), (CORNER[1], CORNER[2])):
        occ = np.zeros((2 * TW, 2 * TH))
        for c in solid:
            occ[c] = 1
        cases.append(_case("", occ, CORNER[0], [CORNER[3]], unknown=unknown, mu=3))
    return _stack("corner_cuts", cases)


def big_disc():
    """r_inflate = 16 round ONE solid cell at (TW, TH): its disc spans the tile borders i = TW and j = TH, and row i's run of blocked
    cells j = TH - 16 .. TH + 16 crosses the bitmap-word border at cell index TW * 2 TH + TH (a multiple of 32)."""
    occ = np.zeros((2 * TW, 2 * TH))
    occ[TW, TH] = 1
    return _case("disc16", occ, (2 * TW - 1, 2 * TH - 1), [(0, 0), (TW, TH - 16), (TW - 16, TH), (TW, TH - 17), (TW + 12, TH + 12)],
                 unknown=[(2 * TW - 1, 2 * TH - 1), (2 * TW - 2, 2 * TH - 1)], r=16, mu=2)


def no_frontier():
    c = _strip("no_frontier", TW + 3, TH + 3, 2)
    c["ev"] = _ev(c["occ"], [])
    return c


def bad_goals():
    """F = B = 2 goals on one map: outside the grid, and in a blocked cell."""
    c = _strip("bad_goals", TW + 3, TH + 3, 2)
    solid = tuple(np.argwhere(c["occ"] != 0)[0])
    c["goal"] = np.array([(ORIGIN[0] - 1.0, ORIGIN[1] + 0.3), centre(solid)])
    c["start"] = c["start"][:2].copy()
    c["start"][1] = centre((0, 0))
    return c


def three_maps():
    """F = B = 3 maps of one shape with 0, 2 and 6 baffles: paths of different lengths, so different numbers of rounds."""
    W, H = 3 * TW + 1, 2 * TH + 5
    cases = [_strip("", W, H, n) if n else dict(_strip("", W, H, 1), occ=np.zeros((W, H), np.uint8)) for n in (0, 2, 6)]
    cases[0]["ev"] = _ev(cases[0]["occ"], [(W - 1, H - 1), (W - 2, H - 1), (W - 1, H - 2), (W - 2, H - 2)])
    return _stack("three_maps", cases)


def many_robots():
    c = _strip("130_robots", 3 * TW + 1, 2 * TH + 5)
    rng = np.random.default_rng(130)
    c["start"] = np.concatenate([c["start"], S.points(rng, 3 * TW + 1, 2 * TH + 5, 130 - len(c["start"]), margin=0.5)])
    return c


def first_refused():
    """363 x 362: the first shape lipmpc_grid_field_batch refuses."""
    c = _strip("363x362", 363, 362)
    c["start"] = c["start"][:6]
    return c


BUILDERS = {"2x2": two_by_two, "one_tile": lambda: _strip("one_tile", TW, TH), "over_under": lambda: _strip("over_under", TW + 1, TH - 1),
            "under_over": lambda: _strip("under_over", TH - 1, TW + 1), "baffles": lambda: _strip("baffles", 3 * TW + 1, 2 * TH + 5),
            "spiral": spiral, "corner_goals": corner_goals, "corner_cuts": corner_cuts, "disc16": big_disc, "no_frontier": no_frontier,
            "bad_goals": bad_goals, "three_maps": three_maps, "130_robots": many_robots, "363x362": first_refused}
IDS = tuple(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(id_):
    c = BUILDERS[id_]()
    c["id"] = id_
    return c


@functools.lru_cache(maxsize=None)
def oracle(id_, planner):
    """The oracle's plan_batch of a case, computed once and shared (read only)."""
    c = case(id_)
    if planner == "field":
        return Fo.plan_batch(c["occ"], ORIGIN, CELL, c["goal"], c["start"], c["r"], c["max_seg"], c["S_max"])
    return FR.plan_batch(c["ev"], T_FREE, T_OCC, ORIGIN, CELL, c["start"], c["r"], c["mu"], c["max_seg"], c["S_max"])


def rounds_to_settle(fld):
    """A budget that settles ``fld``, from the round guarantee: every cell's descent path is a least-cost path, so every value is
    final after (the most tile changes of any of them) + 1 rounds, and one more round, in which nothing falls, leaves no tile
    active."""
    changes = descent_changes(fld)
    return int(changes.max()) + 2


def guaranteed(fld, rounds):
    """The cells the round guarantee covers after ``rounds`` rounds, by their DESCENT path (one least-cost path): those that change
    tile at most rounds - 1 times.  A subset of what the guarantee covers ("some least-cost path"), so holding the device to it
    asks no more than the contract."""
    changes = descent_changes(fld)
    return (changes >= 0) & (changes <= rounds - 1)


@functools.lru_cache(maxsize=8)
def _descent_changes(key, shape):
    return _changes(np.frombuffer(key, np.uint32).reshape(shape))


def descent_changes(fld):
    """Per cell, how often its descent path changes tile; -1 on INF cells.  (Cached by the field's bytes.)"""
    fld = np.ascontiguousarray(fld, np.uint32)
    return _descent_changes(fld.tobytes(), fld.shape)


def _changes(fld):
    W, H = fld.shape
    changes = np.full((W, H), -1, np.int64)
    order = np.argsort(fld, axis=None, kind="stable")          # by cost: a cell's descent successor comes before it
    for flat in order:
        c = (int(flat) // H, int(flat) % H)
        if fld[c] == Fo.INF:
            break
        if fld[c] == 0:
            changes[c] = 0
            continue
        n = descent_step(fld, c)
        changes[c] = changes[n] + (tile_of(c) != tile_of(n))
    return changes


def descent_step(fld, c):
    """The contract's descent from c, one step (tests/field_oracle.py's descend walks to the end)."""
    W, H = fld.shape
    for di, dj in Fo.MOVES:
        a, b = c[0] + di, c[1] + dj
        if not (0 <= a < W and 0 <= b < H) or fld[a, b] == Fo.INF or (di and dj and (fld[a, c[1]] == Fo.INF or fld[c[0], b] == Fo.INF)):
            continue
        if int(fld[a, b]) + (Fo.DIAGONAL if di and dj else Fo.AXIAL) == int(fld[c]):
            return a, b
    raise AssertionError(f"no descent from {c}")
