"""Inputs of the soft-clearance tests, shared by tests/test_clearance_oracle.py (CPU: does every case reach what it claims?) and the
GPU tests tests/test_clearance_cost_gpu.py / tests/test_clearance_field_gpu.py.  numpy and the library's host-only
lipmpc_grid_tiled_info: shapes are derived from the tile sides TW x TH as tests/field_tiled_cases.py derives them.

A CASE is a case of tests/field_tiled_cases.py -- dict(id, occ, ev, goal, start, r, mu, max_seg, S_max) -- plus EITHER ``cost`` (a
uint8 layer of occ's shape, handed to the planners as ``cost=``) OR ``clear`` = (r_clear, w_clear) (the planners make the layer).
occ and ev hold the same solid cells, so both planners see the same clearance layer.  Oracles are computed once and shared, read
only."""
import functools

import numpy as np

import clearance_oracle as CO
import field_oracle as Fo
import field_shape_cases as S
import field_tiled_cases as T

ORIGIN, CELL, T_FREE, T_OCC = T.ORIGIN, T.CELL, T.T_FREE, T.T_OCC
TW, TH = T.TW, T.TH
ZERO_IDS = ("2x2", "spiral", "corner_goals", "corner_cuts", "disc16", "no_frontier")     # of field_tiled_cases: the zero-layer identity


# -- the two-door map of the issue ---------------------------------------------------------------------------------------
DOOR_ROW, NARROW, WIDE = 12, 4, range(20, 29)


def two_door_occ():
    occ = np.zeros((24, 40), np.uint8)
    occ[DOOR_ROW, :] = 1
    occ[DOOR_ROW, NARROW] = 0
    occ[DOOR_ROW, WIDE.start:WIDE.stop] = 0
    return occ


def two_door(r_clear=4, w_clear=40):
    """24 x 40 cells, a wall on row i = 12 with a one-cell door at j = 4 and a nine-cell door at j = 20..28; from (2, 4) to (21, 4)
    (the frontier map: the goal cell unknown, mu = 1 -- its neighbours are the frontier)."""
    c = T._case("two_door", two_door_occ(), (21, 4), [(2, 4), (2, 30)], unknown=[(21, 4)])
    c["goal"] = np.array([S.centre((21, 4))])
    c["clear"] = (r_clear, w_clear)
    return c


def door_of(cells):
    """The column in which a path of cells crosses the wall row."""
    (j,) = {c[1] for c in cells if c[0] == DOOR_ROW}
    return j


# -- layers ----------------------------------------------------------------------------------------------------------------
def random_layer(shape, seed):
    """Bytes that are constant on 8 x 8 blocks (whole regions are dear: a straight segment may cross one that the descent went
    round, while inside a block straightening costs nothing), with bytes 249..255 sprinkled in: the kernels read them as 248."""
    rng = np.random.default_rng(seed)
    W, H = shape[-2:]
    coarse = rng.integers(0, 200, shape[:-2] + (-(-W // 8), -(-H // 8)))
    layer = np.repeat(np.repeat(coarse, 8, -2), 8, -1)[..., :W, :H].copy()
    over = rng.random(shape) < 0.03
    layer[over] = rng.integers(249, 256, int(over.sum()))
    return layer.astype(np.uint8)


def random_case():
    """(2 TW + 5) x (TH + 7), two baffles, r_inflate 2, a random byte layer."""
    c = T._strip("random", 2 * TW + 5, TH + 7, 2)
    c["cost"] = random_layer(c["occ"].shape, 7)
    assert (c["cost"] > CO.COST_MAX).any()
    return c


def clear_strip(r):
    """A strip with baffles at r_inflate ``r``, the clearance layer r_clear 7, w_clear 60 made by the planner."""
    W, H = TW + 3, 2 * TH + 5
    s = S.strip_case(W, H, 3, r=r)
    return dict(occ=s["occ"], ev=s["ev"], goal=s["goal"], start=s["start"], r=r, mu=S.MU, max_seg=s["max_seg"], S_max=s["S_max"], clear=(7, 60))


def priced_cells_blocked():
    """r_clear <= r_inflate: every cell with a cost is blocked, so the weighted field is the unweighted one."""
    c = T._strip("", TW + 3, TH + 3, 2)
    assert c["r"] == 2
    c["clear"] = (2, 248)
    return c


def per_robot():
    """F = B = 4 maps of one shape, each with its own random layer."""
    W, H = TW + 3, TH + 3
    c = T._stack("", [T._strip("", W, H, n) for n in (1, 2, 3, 4)])
    c["cost"] = random_layer(c["occ"].shape, 11)
    return c


def many_starts():
    """One field, 130 starts."""
    c = T._strip("", TW + 3, TH + 3, 2)
    c["start"] = np.concatenate([c["start"], S.points(np.random.default_rng(130), TW + 3, TH + 3, 130 - len(c["start"]), margin=0.5)])
    c["cost"] = random_layer(c["occ"].shape, 13)
    return c


def snap_case():
    """Starts in cells that the inflation blocks (beside a baffle, r_inflate 2): the snap picks the cell the walk starts from."""
    c = T._strip("", TW + 3, TH + 3, 2)
    solid = np.argwhere(c["occ"] != 0)
    i, j = (int(v) for v in solid[len(solid) // 2])
    c["start"] = np.array([S.centre((i, j + 1)), S.centre((i, j - 2)), S.centre((i, j + 2))])
    c["snap_cells"] = [(i, j + 1), (i, j - 2), (i, j + 2)]
    c["cost"] = random_layer(c["occ"].shape, 17)
    return c


def overflow_case():
    """S_max = 2 where the walk sets more sub-goals: PATH_OVERFLOW, the cost still given."""
    c = random_case()
    c["S_max"] = 2
    return c


def all_248(max_seg):
    """A layer of 248 everywhere: field values pass max_seg long before lengths do."""
    c = T._strip("", TW + 3, TH + 3, 2)
    c["start"] = c["start"][:6]
    c["max_seg"] = max_seg
    c["cost"] = np.full(c["occ"].shape, 248, np.uint8)
    return c


def two_tiles():
    """TW x (TH + 9): two tiles, a clearance layer; rounds=1 leaves it unsettled."""
    c = T._strip("", TW, TH + 9, 2)
    c["clear"] = (5, 100)
    return c


def serpentine():
    """TW x 2 TH, two tiles.  A channel of columns TH - 7 .. TH + 6 between two walls, crossed by a wall every second row whose
    one-cell gap alternates between column TH - 5 (tile 0) and column TH + 4 (tile 1): every path down the channel changes tile once
    per wall, far more often than the map has tiles.  A random layer on top."""
    W, H = TW, 2 * TH
    occ = np.zeros((W, H), np.uint8)
    lo, hi = TH - 8, TH + 7
    occ[:, lo] = occ[:, hi] = 1
    for n, i in enumerate(range(2, W - 1, 2)):
        occ[i, lo:hi] = 1
        occ[i, TH - 5 if n % 2 == 0 else TH + 4] = 0
    c = T._case("serpentine", occ, (W - 1, TH), [(0, TH), (0, TH - 3)], unknown=[(W - 1, TH)], S_max=256)
    c["cost"] = random_layer(occ.shape, 19) // 4                # (small bytes: the walls decide the way)
    return c


BUILDERS = {"random": random_case, "two_door": two_door, "two_door_w16": lambda: two_door(4, 16), "clear_strip_r0": lambda: clear_strip(0),
            "clear_strip_r2": lambda: clear_strip(2), "priced_blocked": priced_cells_blocked, "per_robot": per_robot,
            "130_starts": many_starts, "snap": snap_case, "overflow": overflow_case, "all248_seg5": lambda: all_248(5),
            "all248_seg60": lambda: all_248(60), "all248_nocap": lambda: all_248(None), "two_tiles": two_tiles, "serpentine": serpentine}
IDS = tuple(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(id_):
    c = BUILDERS[id_]()
    c["id"] = id_
    return c


def layer(c):
    """The case's cost layer (occ's shape): the given one, or the clearance layer of its solid cells."""
    if "cost" in c:
        return c["cost"]
    solid = c["occ"] != 0
    maps = solid if solid.ndim == 3 else solid[None]
    out = np.stack([CO.clearance_cost(m, *c["clear"]) for m in maps])
    return out if solid.ndim == 3 else out[0]


def plan(c, kind, cost):
    """The weighted oracle's plan_batch of a case under ``cost``."""
    if kind == "field":
        return CO.plan_batch(c["occ"], cost, ORIGIN, CELL, c["goal"], c["start"], c["r"], c["max_seg"], c["S_max"])
    return CO.frontier_plan_batch(c["ev"], cost, T_FREE, T_OCC, ORIGIN, CELL, c["start"], c["r"], c["mu"], c["max_seg"], c["S_max"])


@functools.lru_cache(maxsize=None)
def oracle(id_, kind):
    c = case(id_)
    return plan(c, kind, layer(c))


@functools.lru_cache(maxsize=None)
def zero_oracle(id_, kind):
    """A case of tests/field_tiled_cases.py under the all-zero layer."""
    c = T.case(id_)
    return plan(c, kind, np.zeros(c["occ"].shape, np.uint8))


# -- rounds ----------------------------------------------------------------------------------------------------------------
def descent_changes(fld, k):
    """Per cell, how often its weighted descent path changes tile; -1 on INF cells (tests/field_tiled_cases.py's, weighted)."""
    W, H = fld.shape
    changes = np.full((W, H), -1, np.int64)
    for flat in np.argsort(fld, axis=None, kind="stable"):
        c = (int(flat) // H, int(flat) % H)
        if fld[c] == Fo.INF:
            break
        if fld[c] == 0:
            changes[c] = 0
            continue
        n = CO.descent_step(fld, k, c)
        changes[c] = changes[n] + (T.tile_of(c) != T.tile_of(n))
    return changes


def rounds_to_settle(fld, cost):
    """A budget that settles ``fld``, from the round guarantee in the weighted metric: every cell's descent path is a least-cost
    path, so every value is final after (the most tile changes of any of them) + 1 rounds; one more leaves no tile active."""
    return int(descent_changes(fld, CO.k_of(cost)).max()) + 2
