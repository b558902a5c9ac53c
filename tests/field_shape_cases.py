"""Inputs of the grid planners' shape tests, shared by tests/test_field_shapes_oracle.py (CPU: do the inputs reach what they are
meant to reach?) and tests/test_field_shapes_gpu.py (the field planner and the frontier explorer against their oracles on the
same inputs).  numpy only.

A CASE is dict(id, shape (W, H), r, solid [n,2] (cells), goal [1,2] and occ [W,H] uint8 for the field planner, ev [W,H] int32 for
the frontier explorer, start [16,2], max_seg, S_max, inflation: bool).  Both planners read the same solid cells: ``occ`` marks
them, ``ev`` holds them at or above T_OCC, every other cell free at or below -T_FREE, and a 2 x 2 block of unknown cells in the
corner opposite cell (0, 0), so that the frontier lies where the field planner's goal does and a path from (0, 0) runs the
map's whole length either way.

THE MAPS.  Random occupancy does not serve here: 2 % of solid cells cut a strip 3 or 18 cells wide apart once they are inflated,
and at r_inflate = 16 they block a 64 x 96 map entirely.  So the solid cells are hand placed: BAFFLES across the short side, each
leaving a gap of GAP rows open after the inflation, the gap alternating between the two long edges, so that every path crosses
the strip between two baffles and is longer than the map's long side.  The inflation cases hold single cells on edges and in a
corner instead.
"""
import functools

import numpy as np

import field_oracle as Fo
import frontier_oracle as FR

ORIGIN, CELL = (-0.35, 0.2), (0.1, 0.125)                     # (anisotropic cells: the metric counts cells)
T_FREE, T_OCC = 1, 3
MAX_SEG, S_MAX = 200, 256                                     # a spacing cap: without one the oracle's string pulling is quadratic
MU = 2


def centre(c):
    return Fo.centre(c, ORIGIN, CELL)


def points(rng, W, H, n, origin=ORIGIN, cell=CELL, margin=0.0):
    """n world points over the grid's rectangle (+ a margin, in cells, that puts some outside)."""
    return np.stack([origin[0] + rng.uniform(-margin, W + margin, n) * cell[0], origin[1] + rng.uniform(-margin, H + margin, n) * cell[1]], 1)


# -- the LDS boundary, from the oracles' restatements of the two rules -----------------------------------------------------
def _boundary(fits, over_short_side):
    """(the widest strip W < H of the largest cell count that ``fits``, the shape of the first count over it that has
    ``over_short_side`` cells in its short side), both from Fo.lds_boundary: nothing here names a cell count."""
    (n, shapes), (n_over, over) = Fo.lds_boundary(fits)
    mine = [s for s in over if s[0] == over_short_side]
    assert mine, (f"the LDS rule has changed: the first cell count over it, {n_over} (after {n}), has no shape {over_short_side} cells "
                  f"across among {over}; choose another short side here")
    return max(s for s in shapes if s[0] < s[1]), mine[0]


# 18 x 2203 (39 654 cells, the most that fit) and 35 x 1133 (39 655); 22 x 1699 (37 378) and 60 x 623 (37 380: 37 379 has no shape
# with both sides <= 4096).  The first count over has several shapes; 35 and 60 cells across are the ones under test.
FIELD_FITS, FIELD_OVER = _boundary(Fo.field_fits_lds, 35)
FRONTIER_FITS, FRONTIER_OVER = _boundary(FR.field_fits_lds, 60)


def boundary_shapes():
    """[(W, H, planner the shape is a boundary of, fits?)] -- checked against Fo.lds_boundary by the CPU test."""
    t = lambda s: (s[1], s[0])
    return [(*FIELD_FITS, "field", True), (*t(FIELD_FITS), "field", True), (*FIELD_OVER, "field", False),
            (*FRONTIER_FITS, "frontier", True), (*t(FRONTIER_FITS), "frontier", True), (*FRONTIER_OVER, "frontier", False)]


# -- maps ----------------------------------------------------------------------------------------------------------------
def baffles(S, L, r, n):
    """Solid cells [k,2] of a strip of S x L cells (short side first): n baffles at even spacing along the long side, each a run of
    cells across the short side that leaves, after the inflation by r, ``gap`` rows open at one long edge, alternately."""
    gap = 1 if S <= 5 else 3
    run = S - gap - r                                         # solid rows 0 .. run - 1 block rows 0 .. run - 1 + r
    assert run >= 1
    cells = []
    for k in range(n):
        j = (k + 1) * L // (n + 1)
        rows = range(run) if k % 2 == 0 else range(S - run, S)
        cells += [(i, j) for i in rows]
    return np.array(cells)


def _oriented(cells, S, L, W, H):
    """Cells of the S x L strip in the (W, H) grid: as they are, or transposed when the long side comes first."""
    cells = np.asarray(cells).reshape(-1, 2)
    return cells if (W, H) == (S, L) else cells[:, ::-1]


def _maps(W, H, solid, seed):
    """(occ, ev) of the solid cells: ev with values on both sides of the thresholds and the unknown block in the far corner."""
    rng = np.random.default_rng(seed)
    occ = np.zeros((W, H), np.uint8)
    occ[solid[:, 0], solid[:, 1]] = 1
    ev = (-T_FREE - rng.integers(0, 4, (W, H))).astype(np.int32)
    ev[occ != 0] = T_OCC + rng.integers(0, 4, int(occ.sum()))
    ev[W - 2:, H - 2:] = rng.integers(-T_FREE + 1, T_OCC, (2, 2))
    return occ, ev


def _starts(W, H, solid, r, seed, snap_cells=()):
    """16 starts: cell (0, 0) -- the far end --, a solid cell, NaN, a point outside, the cells meant to snap, random points."""
    rng = np.random.default_rng(seed)
    fixed = [centre((0, 0)), centre(tuple(solid[0])), (float("nan"), 0.3), (ORIGIN[0] - 0.001, 0.3)] + [centre(c) for c in snap_cells]
    return np.concatenate([np.array(fixed), points(rng, W, H, 16 - len(fixed))])


def _case(id_, W, H, r, solid, inflation=False, snap_cells=()):
    seed = 1000 * W + H + r
    occ, ev = _maps(W, H, solid, seed)
    goal = np.array([centre((W - 1, H - 1)) + (0.01, -0.02)])
    return dict(id=id_, shape=(W, H), r=r, solid=solid, occ=occ, ev=ev, goal=goal, start=_starts(W, H, solid, r, seed, snap_cells),
                max_seg=MAX_SEG, S_max=S_MAX, inflation=inflation)


def strip_case(W, H, n_baffles=4, r=None):
    """A strip: r_inflate 0 on a short side of 2, 1 up to 5, else 2."""
    S, L = min(W, H), max(W, H)
    r = (0 if S == 2 else 1 if S <= 5 else 2) if r is None else r
    n = 12 if S == 2 else n_baffles                           # (a 2-wide strip: single cells, a diagonal step of + 0.4 cells each)
    return _case(f"{W}x{H}", W, H, r, _oriented(baffles(S, L, r, n), S, L, W, H))


def shape_cases():
    """The LDS boundary of either planner, rows longer than, equal to and just under the workgroup, strips 2 cells wide."""
    shapes = [(w, h) for w, h, _, _ in boundary_shapes()]
    shapes += [(5, 1023), (5, 1024), (5, 1025), (1023, 5), (1024, 5), (1025, 5), (2, 4096), (4096, 2)]
    return [strip_case(W, H) for W, H in shapes]


def cap_cases():
    """2^17 cells with a side at 4096: relaxed in global memory; 12 baffles of 27 cells."""
    return [strip_case(32, 4096, 12), strip_case(4096, 32, 12)]


INFLATION_R = (3, 7, 11, 16)
INFLATION_SHAPES = ((64, 96), (40, 67))


def inflation_cases():
    """Single solid cells in a corner ((W - 1, 0)) and on two edges ((0, H // 2), (W // 2, 0) up to r = 7), and one inside up to
    r = 7; starts r cells from the edge cell along both axes, which are blocked and snap to the first free cell beyond."""
    cases = []
    for W, H in INFLATION_SHAPES:
        for r in INFLATION_R:
            solid = [(0, H // 2), (W - 1, 0)] + ([(W // 2, 0), (W // 2, 3 * H // 4)] if r <= 7 else [])
            cases.append(_case(f"{W}x{H}r{r}", W, H, r, np.array(solid), inflation=True, snap_cells=((r, H // 2), (0, H // 2 - r))))
    return cases


def window_cases():
    """H = 64, r_inflate = 16, ONE solid cell: at (10, 63) the disc's own row around cell (10, 47) is the 33 cells j = 31 .. 63 --
    a window that starts at bit 31 of a bitmap word and needs all of its two words --, so (10, 47) is blocked and (10, 46) is not;
    at (10, 0) the row is clipped at its start: (10, 16) is blocked and (10, 17) is not."""
    out = []
    for j, blocked, free in ((63, (10, 47), (10, 46)), (0, (10, 16), (10, 17))):
        c = _case(f"window{j}", 72, 64, 16, np.array([(10, j)]), inflation=True, snap_cells=(blocked, free))
        c.update(blocked=blocked, free=free)
        out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    """Every case, built once (read only)."""
    return shape_cases() + cap_cases() + inflation_cases() + window_cases()


def case_ids(cases):
    return [c["id"] for c in cases]


@functools.lru_cache(maxsize=None)
def oracle(case_id, planner):
    """The oracle's plan_batch of a case, computed once and shared (read only)."""
    c = {c["id"]: c for c in all_cases()}[case_id]
    if planner == "field":
        return Fo.plan_batch(c["occ"], ORIGIN, CELL, c["goal"], c["start"], c["r"], c["max_seg"], c["S_max"])
    return FR.plan_batch(c["ev"], T_FREE, T_OCC, ORIGIN, CELL, c["start"], c["r"], MU, c["max_seg"], c["S_max"])


# -- many workgroups -----------------------------------------------------------------------------------------------------
def per_robot_maps(n=600, W=13, H=11, seed=31):
    """n maps of W x H, 6 % solid at random, and the evidence of the same cells with 20 % unknown; one goal and one start each,
    anywhere over the map and a margin around it."""
    rng = np.random.default_rng(seed)
    occ = (rng.random((n, W, H)) < 0.06).astype(np.uint8)
    ev = (-T_FREE - rng.integers(0, 4, (n, W, H))).astype(np.int32)
    unknown = rng.random((n, W, H)) < 0.2
    ev[unknown] = rng.integers(-T_FREE + 1, T_OCC, int(unknown.sum()))
    ev[occ != 0] = T_OCC + rng.integers(0, 4, int(occ.sum()))
    return occ, ev, points(rng, W, H, n, margin=0.3), points(rng, W, H, n, margin=0.3)


def field_fleet_case(n_random=118):
    """48 x 36, r_inflate = 2: a solid block with a one-cell pocket (inflated, nothing finite around it), a closed room (cut off),
    a wall to walk around; twelve special starts, then ``n_random`` random ones over the grid and a margin around it."""
    occ = np.zeros((48, 36), np.uint8)
    occ[4:13, 4:13] = 1
    occ[8, 8] = 0                                              # the pocket
    occ[20:31, 20] = occ[20:31, 30] = 1
    occ[20, 20:31] = occ[30, 20:31] = 1                        # the room: interior 9 x 9, its middle 5 x 5 unblocked
    occ[38, 6:] = 1
    rng = np.random.default_rng(9)
    special = [centre(c) for c in ((5, 5), (8, 8), (25, 25), (3, 8), (13, 8), (37, 20), (45, 30), (24, 26), (26, 24))]
    special += [(float("nan"), 0.3), (ORIGIN[0] - 0.001, 0.3), (ORIGIN[0] + 48 * CELL[0], 0.3)]
    start = np.concatenate([special, points(rng, 48, 36, n_random, margin=1.5)])
    return occ, np.array([centre((45, 30)) + (0.01, -0.02)]), start


def frontier_fleet_case(n_random=118):
    """48 x 36, r_inflate = 2: a solid block with a one-cell free pocket (inflated, nothing finite around it), a closed room
    (known, cut off from every frontier), an unknown block and an unknown band; special starts, then ``n_random`` random ones over
    the grid and a margin around it."""
    ev = np.full((48, 36), -1, np.int32)
    ev[4:13, 4:13] = 3
    ev[8, 8] = -1                                              # the pocket
    ev[20:31, 20] = ev[20:31, 30] = ev[20, 20:31] = ev[30, 20:31] = 4          # the room: walled in
    ev[38, 6:] = 3
    ev[44:, :] = 0                                             # the unknown band
    ev[14:18, 24:30] = 0                                       # the unknown block
    rng = np.random.default_rng(9)
    special = [centre(c) for c in ((5, 5), (8, 8), (25, 25), (3, 8), (43, 20), (15, 26), (47, 10), (24, 26), (13, 26))]
    special += [(float("nan"), 0.3), (ORIGIN[0] - 0.001, 0.3), (ORIGIN[0] + 48 * CELL[0], 0.3)]
    return ev, np.concatenate([special, points(rng, 48, 36, n_random, margin=1.5)])


# -- the worst case of chaotic relaxation -----------------------------------------------------------------------------------
def serpentine(W, H):
    """All solid but a one-cell corridor: rows 1, 3, 5, ... open from column 1 to H - 2, joined alternately at either end.  Returns
    (occ, the corridor's cells from (1, 1) to its far end)."""
    occ = np.ones((W, H), np.uint8)
    rows = list(range(1, W - 1, 2))
    cells = []
    for n, i in enumerate(rows):
        cols = list(range(1, H - 1))
        if n % 2:
            cols.reverse()
        cells += [(i, j) for j in cols]
        if i != rows[-1]:
            cells.append((i + 1, cols[-1]))                    # the join to the next row
    for c in cells:
        occ[c] = 0
    return occ, cells


# -- fields the kernel did not make -------------------------------------------------------------------------------------------
def moved_wall(a):
    """Map B of a fleet map A (occ, or evidence with solid = 3): the wall at i = 38 stands at i = 35 and leaves its gap at the
    other end."""
    b = a.copy()
    solid, free = a[38, 10], a[38, 0]
    b[38, 6:] = free
    b[35, :30] = solid
    return b


def foreign_fields(fld, path):
    """{name: a field that is no cost-to-go field of the map} from a valid field [W,H] and the cells of one path down it."""
    const = np.full_like(fld, 35)
    lifted = np.where(fld == Fo.INF, fld, fld + np.uint32(10)).astype(np.uint32)       # the goal is a strict minimum of 10, not 0
    for c in path[len(path) // 2:-1]:                          # (where the path has a twin of equal cost, the descent takes that)
        raised = fld.copy()
        raised[c] += 1
        if Fo.descend(raised, path[0], strict=False) is None:
            break
    else:
        raise AssertionError("every cell of the path has a twin")
    return dict(constant=const, local_minimum=lifted, raised=raised)
