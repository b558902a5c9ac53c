"""Inputs of the wave-per-robot path tests, shared by tests/test_path_wave_oracle.py (CPU: does every case reach what it claims?) and
tests/test_path_wave_gpu.py (the one-lane and the wave path calls against the oracles on the same inputs).  numpy and the case
modules of the tiled and the clearance tests.

A CASE is a case of tests/field_tiled_cases.py -- dict(id, occ, ev, goal, start, r, mu, max_seg, S_max) -- and may carry ``cost`` (a
uint8 layer of occ's shape) for the weighted form.  Oracles are computed once per case and kind and shared, read only.

What a wave walk can get wrong that a one-lane walk cannot is in the SIGHT TEST (64 cells a round by a closed form: the chunk
borders at 64 and 128 cells, the floor of a negative numerator), in the SNAP (a strided window, a wave minimum with ties) and in the
BATCH SHAPE (four robots a workgroup: B that is no multiple of 4, more than one workgroup).  ``replay`` restates the string pulling
of tests/field_oracle.py and records every sight test it makes, so that the CPU test can show which of these the cases reach."""
import functools
import math

import numpy as np

import clearance_cases as K
import field_oracle as Fo
import field_shape_cases as S
import field_tiled_cases as T
import frontier_oracle as FR

ORIGIN, CELL, T_FREE, T_OCC = T.ORIGIN, T.CELL, T.T_FREE, T.T_OCC
WAVE = 64
centre = S.centre


# -- the sight tests of a walk -------------------------------------------------------------------------------------------------
def sight(fld, a, b):
    """One sight test by the closed form of tests/field_oracle.py's los: dict(a, b after the swap, di, dj, m, cells = m + 1, blocked =
    the segment index of the first impassable cell or None, negative = some numerator 2 k dj + m is below 0)."""
    if tuple(b) < tuple(a):
        a, b = b, a
    di, dj = b[0] - a[0], b[1] - a[1]
    m = max(abs(di), abs(dj))
    out = dict(a=a, b=b, di=di, dj=dj, m=m, cells=m + 1, blocked=None, negative=False)
    if m == 0:
        out["blocked"] = None if fld[a] != Fo.INF else 0
        return out
    out["negative"] = any(2 * k * dj + m < 0 for k in range(m + 1))
    for k in range(m + 1):
        if fld[a[0] + (2 * k * di + m) // (2 * m), a[1] + (2 * k * dj + m) // (2 * m)] == Fo.INF:
            out["blocked"] = k
            break
    return out


def replay(fld, path, max_seg=None):
    """tests/field_oracle.py's string_pull, test for test: (the cells whose centres are sub-goals, every sight test made in order)."""
    max_seg = Fo.NO_CAP if max_seg is None else int(max_seg)
    out, tests, a, k, last = [], [], 0, 1, len(path) - 1
    while k <= last:
        t = sight(fld, path[a], path[k])
        tests.append(t)
        if t["blocked"] is not None or int(fld[path[a]]) - int(fld[path[k]]) >= max_seg:
            e = k - 1 if k - 1 > a else k
            if e == last:
                break
            out.append(path[e])
            a, k = e, e + 1
        else:
            k += 1
    assert out == Fo.string_pull(fld, path, max_seg)
    return out, tests


def read_counts(fld, path, max_seg=None):
    """What one pass of the walk down ``path`` reads: dict(path = its cells, tests = sight tests made, serial_sight = the cell reads of
    the one-lane sight tests (each stops at its first impassable cell), wave_sight = load rounds of ceil((m + 1) / 64) per test (a
    test stops after the chunk that holds an impassable cell), serial_descent = the most a one-lane descent reads (24 a step),
    wave_descent = one round a step)."""
    _, tests = replay(fld, path, max_seg)
    serial = sum(t["cells"] if t["blocked"] is None else t["blocked"] + 1 for t in tests)
    rounds = sum(math.ceil((t["cells"] if t["blocked"] is None else t["blocked"] + 1) / WAVE) for t in tests)
    steps = len(path) - 1
    return dict(path=len(path), tests=len(tests), serial_sight=serial, wave_sight=rounds, serial_descent=24 * steps, wave_descent=steps)


# -- 1. sight lengths around the wave width ---------------------------------------------------------------------------------
JOGS = (2, 124, 126, 128, 130, 254)          # a first impassable cell at segment index ceil(K / 2): 1, 62, 63, 64, 65, 127
JOG_H = 262


def jog_map(K_):
    """4 x JOG_H, all solid but a one-cell corridor along row 1 from column 0 to K_ that steps to row 2 there and runs on to the end.
    From the anchor (1, 0) every cell of row 1 is in sight -- tests of 2 .. K_ + 1 cells that pass --, and the first cell of row 2,
    (2, K_), is not: the segment changes row at index ceil(K_ / 2), where row 2 is still solid."""
    occ = np.ones((4, JOG_H), np.uint8)
    occ[1, :K_ + 1] = 0
    occ[2, K_:] = 0
    return occ


def sight_lengths():
    """F = B = 6 maps, one jog each; the goal at the far end of row 2 (the frontier maps: that cell unknown)."""
    goal = (2, JOG_H - 1)
    c = T._stack("sight_lengths", [T._case("", jog_map(k), goal, [(1, 0)], unknown=[goal], max_seg=None, S_max=8) for k in JOGS])
    c["cost"] = K.random_layer(c["occ"].shape, 41) // 8
    return c


# -- 2. all slopes and both orders -----------------------------------------------------------------------------------------------
ROOM = 71


def slopes():
    """An open room of 71 x 71 cells, the goal in the middle, the starts on a ring of radius 31 cells round it (every cell the
    circle crosses, once)."""
    g = ROOM // 2
    ring = sorted({(g + round(31 * math.cos(2 * math.pi * t / 720)), g + round(31 * math.sin(2 * math.pi * t / 720))) for t in range(720)})
    c = T._case("slopes", np.zeros((ROOM, ROOM)), (g, g), ring, unknown=[(g, g)], max_seg=None, S_max=4)
    return c


# -- 3. spacing and slots ----------------------------------------------------------------------------------------------------------
SPACINGS = (5, 35, None)


def _baffled():
    """The baffled strip of the tiled tests, plus a start in the goal's cell and one in a frontier cell: paths of one sub-goal."""
    c = T._strip("", T.TW + 3, T.TH + 3, 2)
    g = Fo.cell_of(c["goal"][0], ORIGIN, CELL, *c["occ"].shape)
    f = np.argwhere(FR.field(c["ev"], T_FREE, T_OCC, c["r"], c["mu"])[1] != 0)[0]
    c["start"] = np.concatenate([c["start"], [centre(g), centre((int(f[0]), int(f[1])))]])
    return c


@functools.lru_cache(maxsize=None)
def _counts(max_seg):
    """Per kind the most sub-goals of any robot of the baffled strip at this spacing (S_max large enough for all)."""
    c = dict(_baffled(), max_seg=max_seg, S_max=1024)
    return {kind: int(_plan(c, kind)["n_sub"].max()) for kind in ("field", "frontier")}


def spacing(max_seg, slots):
    """The baffled strip of the tiled tests at one spacing; ``slots``: "fit" = S_max is the longest path's count, "one_less" = one
    below it (that path overflows: nothing written, path_cost written), "one" = S_max 1."""
    c = _baffled()
    c["max_seg"] = max_seg
    n = _counts(max_seg)
    c["S_max_of"] = {kind: dict(fit=n[kind], one_less=n[kind] - 1, one=1)[slots] for kind in n}
    c["S_max"] = None                                          # (per kind: the two planners' paths differ)
    return c


# -- 4. the snap ---------------------------------------------------------------------------------------------------------------------
PILLAR, TIE_START, TIE = (10, 10), (10, 9), ((9, 9), (11, 9))
POCKET = (18, 32)


def snaps():
    """24 x 40, r_inflate 1.  A pillar at (10, 10) and the goal on its row: the start (10, 9) is inflated, and of the finite cells of
    its window (9, 9) and (11, 9) tie in (d^2, field) -- the lower index wins.  A solid cell at (1, 1): the starts (0, 1) and (1, 0) are
    inflated and their windows are clipped by the map's corner.  A 5 x 5 solid block with its middle (18, 32) free: that start's whole
    window is impassable, NO_PATH."""
    occ = np.zeros((24, 40), np.uint8)
    occ[PILLAR] = occ[1, 1] = 1
    occ[16:21, 30:35] = 1
    occ[POCKET] = 0
    return T._case("snaps", occ, (10, 30), [TIE_START, (0, 1), (1, 0), POCKET, (5, 5)], unknown=[(10, 30)], r=1, max_seg=None, S_max=8)


def wide_snap():
    """64 x 128, r_inflate 16 round one solid cell: the snap window is 35 x 35 = 1225 cells, more than 19 chunks of 64.  The starts
    are inflated cells beside the solid one and on the disc's rim."""
    occ = np.zeros((64, 128), np.uint8)
    occ[32, 64] = 1
    starts = [(32, 63), (31, 64), (33, 65), (32, 48), (20, 60), (45, 70)]
    return T._case("wide_snap", occ, (60, 120), starts, unknown=[(60, 120), (61, 120)], r=16, mu=1, max_seg=None, S_max=8)


# -- 5. batch shapes -----------------------------------------------------------------------------------------------------------------
BATCHES = (1, 3, 5, 65, 257)
BATCH_W, BATCH_H = 14, 19


def batch(B, per_robot):
    """B robots on 14 x 19 cells with two baffles and sprinkled solid cells: one shared map, field and layer (F = 1), or a map, a goal
    and a layer per robot (F = B)."""
    rng = np.random.default_rng(1000 + 2 * B + per_robot)
    F = B if per_robot else 1
    occ = (rng.random((F, BATCH_W, BATCH_H)) < 0.06).astype(np.uint8)
    occ[:, 4, :13] = occ[:, 9, 6:] = 1
    occ[:, :2, :2] = occ[:, -2:, -2:] = 0
    unknown = [(BATCH_W - 1, BATCH_H - 1), (BATCH_W - 2, BATCH_H - 1)]
    start = S.points(rng, BATCH_W, BATCH_H, B, margin=0.3)
    start[0] = centre((0, 0))
    ev = np.stack([T._ev(o, unknown) for o in occ])
    goal = np.array([centre((BATCH_W - 1, BATCH_H - 1)) + (0.01, -0.02)] * F)
    c = dict(occ=occ if per_robot else occ[0], ev=ev if per_robot else ev[0], goal=goal, start=start, r=0, mu=1, max_seg=35, S_max=16)
    c["cost"] = K.random_layer(c["occ"].shape, 50 + B)
    return c


BUILDERS = {"sight_lengths": sight_lengths, "slopes": slopes, "snaps": snaps, "wide_snap": wide_snap}
BUILDERS.update({f"seg{'_none' if m is None else m}_{s}": functools.partial(spacing, m, s) for m in SPACINGS for s in ("fit", "one_less", "one")})
BUILDERS.update({f"batch{B}_{'per_robot' if p else 'shared'}": functools.partial(batch, B, p) for B in BATCHES for p in (False, True)})
IDS = tuple(BUILDERS)
WEIGHTED_IDS = tuple(i for i in IDS if i == "sight_lengths" or i.startswith("batch"))


@functools.lru_cache(maxsize=None)
def case(id_):
    c = BUILDERS[id_]()
    c["id"] = id_
    return c


def s_max(c, kind):
    return c["S_max_of"][kind] if c.get("S_max") is None else c["S_max"]


def _plan(c, kind, cost=None):
    S_max = s_max(c, kind)
    if cost is not None:
        return K.plan(dict(c, S_max=S_max), kind, cost)
    if kind == "field":
        return Fo.plan_batch(c["occ"], ORIGIN, CELL, c["goal"], c["start"], c["r"], c["max_seg"], S_max)
    return FR.plan_batch(c["ev"], T_FREE, T_OCC, ORIGIN, CELL, c["start"], c["r"], c["mu"], c["max_seg"], S_max)


@functools.lru_cache(maxsize=None)
def oracle(id_, kind, weighted=False):
    """The oracle's plan_batch of a case (``weighted``: under the case's cost layer), computed once and shared (read only)."""
    c = case(id_)
    return _plan(c, kind, c["cost"] if weighted else None)


def tests_of(id_):
    """Every sight test the goal-field walks of a case make, robot by robot."""
    c, want = case(id_), oracle(id_, "field")
    out = []
    for b, cells in enumerate(want["cells"]):
        if cells:
            out += replay(want["field"][0 if len(want["field"]) == 1 else b], cells, c["max_seg"])[1]
    return out


# -- the map of the read counts ------------------------------------------------------------------------------------------------------
def walled(side=362, every=60, gap=4):
    """side x side cells, a wall across every ``every`` rows with a gap of ``gap`` cells alternately at either end."""
    occ = np.zeros((side, side), np.uint8)
    for n, i in enumerate(range(every, side - every // 2, every)):
        occ[i, :] = 1
        if n % 2 == 0:
            occ[i, side - 2 - gap:side - 2] = 0
        else:
            occ[i, 2:2 + gap] = 0
    return occ


@functools.lru_cache(maxsize=None)
def walled_counts(side=362):
    """read_counts of the walk from row 1 to row side - 3 of ``walled(side)`` at r_inflate 1, no spacing cap."""
    occ = walled(side)
    goal, start = centre((side - 3, side // 2)), centre((1, side // 2))
    fld, fs = Fo.field(occ, ORIGIN, CELL, goal, 1)
    p = Fo.plan(occ, ORIGIN, CELL, goal, start, 1, None, 4096, fld=fld, field_status=fs)
    assert p["status"] == Fo.FOUND
    return dict(read_counts(fld, p["cells"]), n_sub=p["n_sub"])
