"""What the tests of the informed explorer share (tests/test_gain_oracle.py, tests/test_gain_gpu.py): the maps, one run of
InformedFrontierPlanner into poisoned buffers, and the comparison of EVERY output with tests/gain_oracle.py, bit for bit.  The maps
and the oracle side need no GPU; torch and the library are imported by the functions that run the device."""
import functools

import numpy as np

import field_oracle as FO
import frontier_oracle as FR
import gain_oracle as G
import lidar_oracle as L
import map_oracle as M

SENTINEL = -7.25
ORIGIN, CELL = (-0.35, 0.2), (0.1, 0.125)                     # tests/grid_checks.py's placement (anisotropic cells)
T_FREE, T_OCC = 1, 3
POISON_I32, POISON_WORD = 77, 0x5EEDBEEF

HAND_MADE = np.array([[-1, -1, -1, 0, 0, 3, -1],              # tests/test_frontier_gpu.py's 5 x 7
                      [-1, -2, -1, 0, 2, 3, -1],
                      [-1, -1, -1, -1, -1, 3, 0],
                      [3, -1, -5, -1, 0, 0, 0],
                      [3, 3, -1, -1, -1, 1, -3]], np.int32)

MAP_W, MAP_H, MAP_ORIGIN, MAP_CELL, MAP_RANGE = 92, 80, (1.0, 0.0), (0.05, 0.05), 1.5
SCAN_AT = ((1.6, 2.72), (2.6, 1.0), (4.3, 3.2))


@functools.lru_cache(maxsize=None)
def scanned_maps():
    """(shared [W,H], per robot [3,W,H]) int32: three scans of a U-shaped wall through tests/map_oracle.py (the map of
    tests/test_frontier_gpu.py)."""
    occ = np.zeros((MAP_W, MAP_H), np.uint8)
    for i0, j0, i1, j1 in ((48, 28, 51, 80), (36, 28, 48, 31), (36, 77, 48, 80)):
        occ[i0:i1, j0:j1] = 1
    table = L.ray_table(360)
    pos = np.array(SCAN_AT)
    hits = M.oracle_hits(pos, occ, MAP_ORIGIN, MAP_CELL, MAP_RANGE, table)
    per = M.update(np.zeros((3, MAP_W, MAP_H), np.int64), pos, hits, MAP_ORIGIN, MAP_CELL, MAP_RANGE, table)
    return per.sum(0).astype(np.int32), per.astype(np.int32)


def centres(cells, origin=ORIGIN, cell=CELL):
    return np.array([FO.centre(c, origin, cell) for c in cells]).reshape(-1, 2)


def points(rng, W, H, n, origin=ORIGIN, cell=CELL, margin=0.0):
    """n world points over the grid's rectangle (+ a margin, in cells, that puts some outside)."""
    return np.stack([origin[0] + rng.uniform(-margin, W + margin, n) * cell[0], origin[1] + rng.uniform(-margin, H + margin, n) * cell[1]], 1)


def speckled(rng, W, H, p_free=0.6, p_solid=0.1):
    """Evidence of all three classes cell by cell, the values spread over both sides of each threshold."""
    ev = rng.integers(-T_FREE + 1, T_OCC, (W, H)).astype(np.int32)
    free = rng.random((W, H)) < p_free
    ev[free] = -T_FREE - rng.integers(0, 4, int(free.sum()))
    solid = rng.random((W, H)) < p_solid
    ev[solid] = T_OCC + rng.integers(0, 4, int(solid.sum()))
    return ev


def one_free_cell(r):
    """An all-unknown (2 r + 3)^2 map with one free cell in the middle: the whole disc is seen."""
    ev = np.zeros((2 * r + 3, 2 * r + 3), np.int32)
    ev[r + 1, r + 1] = -T_FREE
    return ev


def rooms(W, H):
    """A large known area with walls, an unknown band along the far edge and an unknown block in the middle."""
    ev = np.full((W, H), -2, np.int32)
    ev[W // 4, : H - 9] = ev[W // 2, 7:] = 5
    ev[3 * W // 4, : H // 2] = ev[3 * W // 4, H // 2 + 9:] = 3
    ev[W - 6:, :] = 0
    ev[W // 3:W // 3 + 8, H // 2:H // 2 + 8] = 1
    return ev


@functools.lru_cache(maxsize=None)
def fleet_case():
    """tests/test_frontier_gpu.py's 48 x 36 map with a pocket, a sealed room, an unknown block and band; 130 starts: special ones
    (solid, pocket, walled in, inflated, on a frontier cell, unknown, NaN, outside), then random ones over the grid and a margin."""
    ev = np.full((48, 36), -1, np.int32)
    ev[4:13, 4:13] = 3
    ev[8, 8] = -1
    ev[20:31, 20] = ev[20:31, 30] = ev[20, 20:31] = ev[30, 20:31] = 4
    ev[38, 6:] = 3
    ev[44:, :] = 0
    ev[14:18, 24:30] = 0
    rng = np.random.default_rng(9)
    special = list(centres(((5, 5), (8, 8), (25, 25), (3, 8), (43, 20), (15, 26), (47, 10), (24, 26), (13, 26))))
    special += [(float("nan"), 0.3), (ORIGIN[0] - 0.001, 0.3), (ORIGIN[0] + 48 * CELL[0], 0.3)]
    return ev, np.concatenate([np.array(special), points(rng, 48, 36, 118, margin=1.5)])


# -- the hand-made corridor of the terminal test ---------------------------------------------------------------------------
CORRIDOR_A, CORRIDOR_B = (1, 3), (1, 8)


def corridor(gain_a, gain_b=100):
    """(evidence 3 x 12, gain): a one-cell free corridor between solid rows with two unknown cells in the wall, at j = 3 and j = 8.
    With r_inflate 0 and min_unknown 1 each makes three frontier cells; the hand-written gain is 0 on all but A = (1, 3) and
    B = (1, 8), so with min_gain 1 those two are the sources.  With w_gain 16 and g_cap 100 a seed is 100 - gain, and A is 25 cost
    units (five axial steps) from B: gain_a = 75 TIES the route through A, 74 leaves A dominated, 76 makes A strictly better."""
    ev = np.full((3, 12), T_OCC, np.int32)
    ev[1, :] = -T_FREE
    ev[0, 3] = ev[0, 8] = 0
    gain = np.zeros((3, 12), np.int32)
    gain[CORRIDOR_A], gain[CORRIDOR_B] = gain_a, gain_b
    return ev, gain


CORRIDOR_KW = dict(r_view=2, w_gain=16, g_cap=100, min_gain=1, r=0, mu=1)


# -- oracle and device ---------------------------------------------------------------------------------------------------------
def expected(ev, start, r_view, w_gain, g_cap, min_gain=0, r=2, mu=2, max_seg=None, S_max=64, t=(T_FREE, T_OCC), origin=ORIGIN, cell=CELL,
             gain=None, nearest=None):
    return G.plan_batch(ev, t[0], t[1], origin, cell, np.asarray(start, np.float64).reshape(-1, 2), r_view, w_gain, g_cap, min_gain, r, mu,
                        max_seg, S_max, gain=gain, nearest=nearest)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def buffers(B, F, W, H, S_max):
    """Every output poisoned: the sentinel in the sub-goal rows, patterns no call writes in the rest."""
    import torch
    import lipmpc
    out = {k: torch.empty(shape, dtype=dt, device="cuda") for k, (dt, shape, _) in lipmpc.planner.informed_outputs(B, F, W, H, S_max).items()}
    poison(out)
    return out


def poison(out):
    import torch
    for k in ("sub_goals", "path_cost", "target"):
        out[k].fill_(SENTINEL)
    for k in ("n_sub", "status", "target_cell", "target_gain", "n_frontier", "n_sources", "gain"):
        out[k].fill_(POISON_I32)
    out["frontier"].fill_(9)
    for k in ("field", "ufield"):
        out[k].view(torch.int32).fill_(POISON_WORD)


def host(out):
    import torch
    h = {k: v.cpu().numpy() for k, v in out.items() if k not in ("field", "ufield")}
    for k in ("field", "ufield"):
        h[k] = out[k].view(torch.int32).cpu().numpy().view(np.uint32)
    return h


def planner(r_view, w_gain, g_cap, min_gain=0, r=2, mu=2, max_seg=None, t=(T_FREE, T_OCC)):
    import lipmpc
    return lipmpc.InformedFrontierPlanner(r_view, w_gain, g_cap, min_gain, r_inflate=r, min_unknown=mu, t_free=t[0], t_occ=t[1],
                                          max_seg=max_seg)


def run(ev, start, r_view, w_gain, g_cap, min_gain=0, r=2, mu=2, max_seg=None, S_max=64, t=(T_FREE, T_OCC), origin=ORIGIN, cell=CELL,
        gain=None):
    """One plan through the Python class into poisoned buffers.  ``gain``: a hand-written gain in the place of the gain call's --
    then the class's own calls are made one by one, with the given array in out["gain"]."""
    import torch
    ev, start = np.ascontiguousarray(ev, np.int32), np.ascontiguousarray(np.asarray(start, np.float64).reshape(-1, 2))
    W, H = ev.shape[-2:]
    out = buffers(len(start), 1 if ev.ndim == 2 else len(ev), W, H, S_max)
    pl = planner(r_view, w_gain, g_cap, min_gain, r, mu, max_seg, t)
    d_ev, d_start = torch.as_tensor(ev, device="cuda"), torch.as_tensor(start, device="cuda")
    if gain is None:
        got = pl.plan(d_ev, d_start, origin=origin, cell=cell, S_max=S_max, out=out)
        assert got is out and pl.last is out
    else:
        ev3, t_free, t_occ, org, cs = pl._map(d_ev, origin, cell)
        org, cs, org_c, cell_c = pl._placement(org, cs)
        pl._field(ev3, t_free, t_occ, out)
        out["gain"].copy_(torch.as_tensor(np.ascontiguousarray(gain, np.int32).reshape(ev3.shape), device="cuda"))
        pl._ufield(ev3, out)
        pl._path(ev3, t_occ, d_start, org_c, cell_c, S_max, out)
        pl._target(out, org, cs, H)
    torch.cuda.synchronize()
    return host(out)


def same(got, want, S_max):
    """Every output of the device equals the oracle's, bit for bit; sub-goal rows from n_sub on still hold the sentinel."""
    for k in ("n_frontier", "frontier", "field", "gain", "n_sources", "ufield", "status", "n_sub", "target_cell", "target_gain"):
        assert np.array_equal(got[k], want[k]), (k, int((np.asarray(got[k]) != np.asarray(want[k])).sum()),
                                                 np.argwhere(np.asarray(got[k]) != np.asarray(want[k]))[:4].tolist())
    assert np.array_equal(bits(got["path_cost"]), bits(want["path_cost"]))             # (one NaN pattern: __builtin_nan = numpy's)
    found = want["target_cell"] >= 0
    assert np.array_equal(bits(got["target"][found]), bits(want["target"][found])) and np.isnan(got["target"][~found]).all()
    assert got["sub_goals"].shape[1] == S_max
    for b, sub in enumerate(want["sub_goals"]):
        n = len(sub)
        assert np.array_equal(bits(got["sub_goals"][b, :n]), bits(sub)), b
        assert (got["sub_goals"][b, n:] == SENTINEL).all(), b


def check(ev, start, r_view, w_gain, g_cap, min_gain=0, r=2, mu=2, max_seg=None, S_max=64, t=(T_FREE, T_OCC), origin=ORIGIN, cell=CELL,
          gain=None, want=None):
    if want is None:
        want = expected(ev, start, r_view, w_gain, g_cap, min_gain, r, mu, max_seg, S_max, t, origin, cell, gain)
    got = run(ev, start, r_view, w_gain, g_cap, min_gain, r, mu, max_seg, S_max, t, origin, cell, gain)
    same(got, want, S_max)
    return got, want
