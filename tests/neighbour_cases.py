"""Inputs of the neighbour LDCBF rows (lipmpc_neighbour_c_eta_batch) at the limits of the grid, the sort and the doubles: named
builders, numpy only.  tests/test_neighbour_cases_oracle.py shows on the oracle that every case is what it claims,
tests/test_neighbours_limits_gpu.py runs them on the device.

A builder returns a dict: the arguments of one call (state, radius, sense_range, k_rows, n_obs_max, share, group, first_slot),
``at`` (named robot indices), ``nonfinite`` (the robots whose rows hold a NaN or an infinity BY DESIGN; everywhere else a
non-finite row is a mistake of the case) and ``with_neighbours`` (False: the call is made without the `neighbours` output).

``cell_of`` and ``bucket_of`` restate two IMPLEMENTATION DETAILS of csrc/lipmpc_neighbours.hip -- the cell formula with its
clamp and floor, and the hash of the bucket table -- which the contract (include/lipmpc.h) does not promise: the cases use
them only to aim at the kernel's clamp and at colliding buckets, and the GPU test reads the kernel's own buckets back so
that a change of either shows as a failed comparison instead of as a case that quietly stopped aiming."""
import numpy as np

DBL_MAX = np.finfo(np.float64).max
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
CELL_CLAMP = 2.0 ** 30
CELL_FLOOR = 2.0 ** -500
NB_MIN = 1024


# ---- the restated implementation details ---------------------------------------------------------------------------------
def cell_width(R):
    with np.errstate(over="ignore"):
        return max(np.float64(R) * (1.0 + 2.0 ** -20), CELL_FLOOR)


def cell_unclamped(v, R):
    """floor(v / w) as a double: the cell coordinate before the clamp."""
    with np.errstate(over="ignore"):
        return np.floor(np.asarray(v, np.float64) / cell_width(R))


def cell_of(v, R):
    return np.clip(cell_unclamped(v, R), -CELL_CLAMP, CELL_CLAMP).astype(np.int64)


def n_buckets(B):
    nb = NB_MIN
    while nb < 2 * B:
        nb <<= 1
    return nb


def bucket_of(cx, cy, g, nb):
    u = lambda a: np.asarray(a, np.int64).astype(np.uint32)
    with np.errstate(over="ignore"):
        h = u(cx) * np.uint32(0x9E3779B1) ^ u(cy) * np.uint32(0x85EBCA77) ^ u(g) * np.uint32(0xC2B2AE3D)
        h ^= h >> np.uint32(15); h *= np.uint32(0x2C1B3C6D); h ^= h >> np.uint32(12); h *= np.uint32(0x297A2D39); h ^= h >> np.uint32(15)
    return (h & np.uint32(nb - 1)).astype(np.int64)


def buckets(case):
    """[B] the bucket of every robot of a case (-1: absent is not modelled here; the cases that use this have no absent robot)."""
    st, R = case["state"], case["sense_range"]
    g = np.zeros(len(st), np.int64) if case["group"] is None else case["group"]
    return bucket_of(cell_of(st[:, 0], R), cell_of(st[:, 2], R), g, n_buckets(len(st)))


# ---- building blocks -----------------------------------------------------------------------------------------------------
def states(x, y):
    st = np.zeros((len(x), 5))
    st[:, 0], st[:, 2] = x, y
    st[:, 1], st[:, 3], st[:, 4] = 0.3, -0.2, 0.7            # never read
    return st


class _Batch:
    """Robots collected under names; every ``add`` may put its robots into a group of their own, so that sub-cases that
    lie on top of each other do not see each other."""

    def __init__(self):
        self.x, self.y, self.g, self.at = [], [], [], {}

    def add(self, name, pts, group=0):
        self.at.setdefault(name, []).extend(range(len(self.x), len(self.x) + len(pts)))
        for p in pts:
            self.x.append(p[0]); self.y.append(p[1]); self.g.append(group)

    def case(self, R, **kw):
        g = np.array(self.g, np.int32)
        return _case(self.x, self.y, R, group=g if g.any() else None, at=self.at, **kw)


def _case(x, y, R, k_rows=4, n_obs_max=6, radius=0.1, share=0.5, group=None, first_slot=None, at=None, nonfinite=(),
          with_neighbours=True):
    return dict(state=states(x, y), radius=radius, sense_range=float(R), k_rows=k_rows, n_obs_max=n_obs_max, share=share,
                group=None if group is None else np.asarray(group, np.int32),
                first_slot=None if first_slot is None else np.asarray(first_slot, np.int32), at=at or {},
                nonfinite=sorted(nonfinite), with_neighbours=with_neighbours)


def call_args(case):
    """The oracle's keyword arguments of a case."""
    return {k: case[k] for k in ("state", "radius", "sense_range", "k_rows", "n_obs_max", "share", "group", "first_slot")}


# ---- ranges that are not 1 -----------------------------------------------------------------------------------------------
def range_edges(R):
    """The edge batch at a range whose square is not the square of a rounded distance: lattices on multiples of the cell width
    and of the range (negative ones included; the multiple 0 is left to ``small_doubles``, where one ulp is a subnormal), each
    lattice robot with partners one ulp across the cell boundary and 0.6 R / 0.5 R away; pairs exactly at the range and one
    ulp inside it along both axes and the diagonal, every pair in a group of its own; and a ring of 96 robots at distance R
    (to within a few ulps) around one at the origin.  On the ring `d2 < R * R` and `sqrt(d2) < R` part wherever they can:
    they can iff the double below R * R still has the root R, which holds for 0.7 and 1/3 and not for 1e-3 and 1e5 (there the
    two comparisons agree on every double)."""
    R = np.float64(R)
    w, inside = cell_width(R), np.nextafter(R, 0.0)
    b = _Batch()
    for name, pitch, y0, g in (("cell multiples", w, 0.0, 0), ("range multiples", R, 50.0 * R, 0)):
        pts = []
        for i in (-3, -2, -1, 1, 2):
            for j in range(-2, 3):
                px, py = i * pitch, y0 + j * pitch
                pts += [(px, py), (np.nextafter(px, -np.inf), py), (px - 0.6 * R, py), (px, py - 0.6 * R), (px - 0.5 * R, py - 0.5 * R)]
        b.add(name, pts, g)
    a = R / np.sqrt(2.0)
    g = 10
    for name, pairs in (("exactly at range", [((0.0, 0.0), (R, 0.0)), ((0.0, 0.0), (0.0, R)), ((-R, 0.0), (0.0, 0.0)), ((0.0, R), (0.0, 0.0))]),
                        ("one ulp inside", [((0.0, 0.0), (inside, 0.0)), ((0.0, 0.0), (0.0, -inside)), ((-inside, 3.0 * w), (0.0, 3.0 * w))]),
                        ("diagonal", [((0.0, 0.0), (s * a * (1.0 + k * 2.0 ** -52), a * (1.0 + k * 2.0 ** -52))) for s in (1.0, -1.0) for k in range(-3, 4)])):
        for p, q in pairs:
            b.add(name, [p, q], g)
            g += 1
    th = 0.1 + 2.0 * np.pi * np.arange(96) / 96.0
    b.add("ring centre", [(0.0, 0.0)], 5)
    r = R * (1.0 - (np.arange(96) % 4) * 2.0 ** -53)         # the radii a few ulps apart: part of the ring is in range
    b.add("ring", list(zip(r * np.cos(th), r * np.sin(th))), 5)
    return b.case(R, radius=0.1 * float(R))


# ---- the clamp -----------------------------------------------------------------------------------------------------------
def clamp_straddle(sign):
    """R = 1: 56 robots within +-3 of x = sign 2^30 w (y around 0) and 56 within +-3 of y = -sign 2^30 w (x around 0): cells
    on both sides of the clamp, in-range pairs across it (eight of them planted 0.4 apart, the others as they fall)."""
    rng = np.random.default_rng(30 + (sign > 0))
    w = cell_width(1.0)

    def cluster(s):
        edge = s * CELL_CLAMP * w                             # +-(2^30 + 2^10): a double; the last cell that is not clamped
        bound = edge + w if s > 0 else edge                   # begins (s < 0) or ends (s > 0) here
        free = list(zip(edge + rng.uniform(-3, 3, 40), rng.uniform(-1.2, 1.2, 40)))
        return free + [(bound + d, v) for v in np.linspace(-1.05, 1.05, 8) for d in (-0.2, 0.2)]

    b = _Batch()
    b.add("x", cluster(sign))
    b.add("y", [(v, u) for u, v in cluster(-sign)])
    return b.case(1.0, k_rows=16, n_obs_max=20)


def clamp_far():
    """R = 1, 48 robots near (2^40, -2^40): every cell coordinate is clamped, all robots in the one cell (2^30, -2^30)."""
    rng = np.random.default_rng(40)
    return _case(2.0 ** 40 + rng.uniform(-2.5, 2.5, 48), -2.0 ** 40 + rng.uniform(-2.5, 2.5, 48), 1.0)


def clamp_int32_edge():
    """R = 1, 48 robots within +-3 of (2^31 w, -2^31 w): quotients on both sides of the largest int32, all of them clamped."""
    rng = np.random.default_rng(31)
    edge = 2.0 ** 31 * cell_width(1.0)
    return _case(edge + rng.uniform(-3, 3, 48), -edge + rng.uniform(-3, 3, 48), 1.0)


def clamp_tiny_range():
    """R = 1e-12, 48 robots near (1, 1): ordinary coordinates, and 1 / w is beyond 2^30 all the same."""
    rng = np.random.default_rng(12)
    return _case(1.0 + 1e-12 * rng.uniform(-2.5, 2.5, 48), 1.0 + 1e-12 * rng.uniform(-2.5, 2.5, 48), 1e-12, radius=1e-13)


# ---- the floor and infinity ----------------------------------------------------------------------------------------------
def floored_cells():
    """R = 1e-151 < 2^-500: the cell width is the floor (about 3 R).  One robot in each of 6 x 6 floored cells with 0, 1 or 2
    partners 0.6 R from it, many of them across a cell boundary."""
    R, w = 1e-151, CELL_FLOOR
    rng = np.random.default_rng(151)
    x, y = [], []
    for i in range(-3, 3):
        for j in range(-3, 3):
            px, py = (i + rng.uniform(0.05, 0.95)) * w, (j + rng.uniform(0.05, 0.95)) * w
            x.append(px); y.append(py)
            for k in range((i + j) % 3):
                th = rng.uniform(0, 2 * np.pi)
                x.append(px + 0.6 * R * np.cos(th)); y.append(py + 0.6 * R * np.sin(th))
    return _case(x, y, R, radius=1e-152)


def infinite_cell(scale):
    """R = the largest double: w = inf, every quotient 0, one cell.  scale 1e153: every d2 is finite and all 24 robots see each
    other; scale 1e155: d2 overflows to infinity for all but the pairs planted 5e153 apart."""
    rng = np.random.default_rng(int(np.log10(scale)))
    x, y = list(scale * rng.uniform(-1, 1, 24)), list(scale * rng.uniform(-1, 1, 24))
    if scale > 1e154:
        for k in range(0, 24, 2):                             # partners (3, 4) 1e153 from every other robot, and one more for a few
            x.append(x[k] + 3e153); y.append(y[k] + 4e153)
            if k % 4 == 0:
                x.append(x[k] - 4e153); y.append(y[k] + 3e153)
    return _case(x, y, DBL_MAX, k_rows=16, n_obs_max=24)


# ---- small doubles -------------------------------------------------------------------------------------------------------
SMALL_SEPARATIONS = (1e-150, 1e-155, 1e-160, 1e-162, 5e-324)


def small_doubles():
    """R = 1.  23 robots within 1e-159 of each other around the origin (d2 is subnormal and eta visibly off unit length), and
    pairs in groups of their own at the separations of SMALL_SEPARATIONS along x, y and a diagonal: at 1e-162 d2 is 0 and the
    row is (-inf, NaN, ...), at 5e-324 (one ulp across the cell boundary at 0) the same."""
    rng = np.random.default_rng(159)
    b = _Batch()
    b.add("cluster", list(zip(1e-159 * rng.uniform(-0.5, 0.5, 23), 1e-159 * rng.uniform(-0.5, 0.5, 23))))
    g = 1
    for s in SMALL_SEPARATIONS:
        for d in ((s, 0.0), (0.0, -s), (-s, s)):
            b.add(f"pair {s:g}", [(0.0, 0.0), d], g)
            g += 1
    at = b.at
    return b.case(1.0, k_rows=16, n_obs_max=24, nonfinite=at["pair 1e-162"] + at["pair 4.94066e-324"])


# ---- ties in a full list -------------------------------------------------------------------------------------------------
OCTETS = ((0.25, 0.5), (0.125, 0.75), (0.375, 0.625))         # d2 = 0.3125, 0.578125, 0.53125: exact, equal within an octet
OCTET_K_ROWS = (1, 3, 4, 5, 15, 16)


def octets(k_rows):
    """A centre robot with three octets (+-a, +-b), (+-b, +-a) around it, the indices shuffled; room for every row."""
    pts = [(0.0, 0.0)]
    for a, c in OCTETS:
        pts += [(sx * p, sy * q) for p, q in ((a, c), (c, a)) for sx in (1, -1) for sy in (1, -1)]
    perm = np.random.default_rng(8).permutation(len(pts))     # robot perm[k] is point k
    x, y = np.zeros(len(pts)), np.zeros(len(pts))
    x[perm], y[perm] = np.array(pts).T
    at = dict(centre=[int(perm[0])], **{f"octet {o}": sorted(int(v) for v in perm[1 + 8 * o: 9 + 8 * o]) for o in range(3)})
    return _case(x, y, 1.0, k_rows=k_rows, n_obs_max=20, at=at)


# ---- colliding buckets ---------------------------------------------------------------------------------------------------
ADJACENT_IN_ONE_BUCKET = ((-35, 31), (-35, 32))               # two adjacent cells, one bucket of 1024 (group 0)
BETWEEN_TWO_IN_ONE_BUCKET = (-33, 26)                         # the cells left and right of this one share a bucket
GROUPS_IN_ONE_BUCKET = (2, 52)                                # in cell (0, 0)
BIG_GROUPS = (2 ** 31 - 1, 2 ** 30)


def collisions():
    """R = 1, 1024 buckets.  Robots in range of each other in two adjacent cells of one bucket (a robot of either walks the
    same run twice, for two of its nine cells), in three cells in a row of which the outer two share a bucket, in two groups
    that share the bucket of cell (0, 0), and in two groups with large ids."""
    w = cell_width(1.0)
    rng = np.random.default_rng(1024)
    b = _Batch()
    (ax, ay), (bx, by) = ADJACENT_IN_ONE_BUCKET
    assert ax == bx and by == ay + 1
    b.add("adjacent A", [((ax + u) * w, (ay + v) * w) for u, v in zip(rng.uniform(0.1, 0.9, 6), rng.uniform(0.6, 0.98, 6))])
    b.add("adjacent B", [((bx + u) * w, (by + v) * w) for u, v in zip(rng.uniform(0.1, 0.9, 6), rng.uniform(0.02, 0.4, 6))])
    cx, cy = BETWEEN_TWO_IN_ONE_BUCKET
    b.add("left", [((cx - 1 + u) * w, (cy + v) * w) for u, v in zip(rng.uniform(0.6, 0.98, 4), rng.uniform(0.3, 0.7, 4))])
    b.add("between", [((cx + u) * w, (cy + v) * w) for u, v in zip(rng.uniform(0.02, 0.98, 6), rng.uniform(0.3, 0.7, 6))])
    b.add("right", [((cx + 1 + u) * w, (cy + v) * w) for u, v in zip(rng.uniform(0.02, 0.4, 4), rng.uniform(0.3, 0.7, 4))])
    for g in GROUPS_IN_ONE_BUCKET + BIG_GROUPS:
        n = 6 if g != BIG_GROUPS[1] else 3
        b.add(f"group {g}", [(u * w, v * w) for u, v in zip(rng.uniform(0.05, 0.95, n), rng.uniform(0.05, 0.95, n))], g)
    return b.case(1.0, k_rows=8, n_obs_max=10)


# ---- first_slot and the lanes of the row kernel --------------------------------------------------------------------------
def slots(n_obs_max, k_rows=4, with_neighbours=True):
    """64 robots on 4 x 4 (about 10 in range of each), first_slot through every value outside 0..n_obs_max and its ends."""
    rng = np.random.default_rng(n_obs_max)
    first = np.resize(np.array([INT_MIN, -3, 0, n_obs_max, n_obs_max + 5, INT_MAX, 1, n_obs_max - 1], np.int64), 64)
    return _case(rng.uniform(0, 4, 64), rng.uniform(0, 4, 64), 1.0, k_rows=k_rows, n_obs_max=n_obs_max,
                 radius=rng.uniform(0.05, 0.3, 64), first_slot=first, at=dict(first_slot=first), with_neighbours=with_neighbours)


# ---- batch size ----------------------------------------------------------------------------------------------------------
def batch_4099():
    """4099 robots on 40 x 40, R = 1 (8 in range on average, 19 at most): 16384 buckets, 64 workgroups of nb_runs_kernel;
    k_rows = 8: the 16-entry search with fewer rows than entries."""
    rng = np.random.default_rng(4099)
    return _case(rng.uniform(0, 40, 4099), rng.uniform(0, 40, 4099), 1.0, k_rows=8, n_obs_max=10, radius=0.2,
                 first_slot=rng.integers(0, 4, 4099))


def batch_300():
    rng = np.random.default_rng(300)
    return _case(rng.uniform(0, 8, 300), rng.uniform(0, 8, 300), 1.0, k_rows=8, n_obs_max=10, radius=0.2,
                 first_slot=rng.integers(0, 4, 300))


ABSENT_WAYS = ("group < 0", "x NaN", "y infinite", "radius negative")


def large():
    """257^2 = 66049 robots (indices above 2^16) on a jittered lattice of pitch 0.55 R, three groups, one robot in 16 absent
    by each of the four ways in turn: 4128 absent robots, so that 16 trailing workgroups of the search have nothing to do."""
    n, R = 257, 1.0
    rng = np.random.default_rng(257)
    i, j = np.divmod(rng.permutation(n * n), n)               # lattice sites in shuffled order: index and place unrelated
    x = 0.55 * R * (i + rng.uniform(-0.3, 0.3, n * n))
    y = 0.55 * R * (j + rng.uniform(-0.3, 0.3, n * n))
    group = rng.integers(0, 3, n * n).astype(np.int32)
    radius = rng.uniform(0.05, 0.2, n * n)
    gone = np.arange(5, n * n, 16)
    way = np.arange(len(gone)) % 4
    group[gone[way == 0]] = -1 - (gone[way == 0] % 7)
    x[gone[way == 1]] = np.nan
    y[gone[way == 2]] = np.inf
    radius[gone[way == 3]] = -0.05
    return _case(x, y, R, k_rows=5, n_obs_max=6, radius=radius, group=group, first_slot=rng.integers(0, 3, n * n),
                 at=dict(absent=gone, way=way))


# ---- the list ------------------------------------------------------------------------------------------------------------
RANGES = (0.7, 1.0 / 3.0, 1e-3, 1e5)
EXTREME = {                                                   # the cases the oracle test holds to the density conditions
    **{f"range {R:.3g}": (lambda R=R: range_edges(R)) for R in RANGES},
    "clamp straddle +": lambda: clamp_straddle(+1.0),
    "clamp straddle -": lambda: clamp_straddle(-1.0),
    "clamp far": clamp_far,
    "clamp int32 edge": clamp_int32_edge,
    "clamp tiny range": clamp_tiny_range,
    "floored cells": floored_cells,
    "infinite cell, all in range": lambda: infinite_cell(1e153),
    "infinite cell, d2 overflows": lambda: infinite_cell(1e155),
    "small doubles": small_doubles,
}
CASES = {                                                     # every case but the large one
    **EXTREME,
    **{f"octets k_rows={k}": (lambda k=k: octets(k)) for k in OCTET_K_ROWS},
    "collisions": collisions,
    "slots n_obs_max=1": lambda: slots(1),
    "slots n_obs_max=50": lambda: slots(50),
    "16 rows into 3 slots, no neighbours output": lambda: slots(3, k_rows=16, with_neighbours=False),
    "batch 300": batch_300,
    "batch 4099": batch_4099,
}
