"""Inputs of the polygon-scan tests on large rings and long lists, shared by tests/test_lidar_ring_cases_oracle.py (CPU: does every
case reach the route it is named for?) and tests/test_lidar_rings_gpu.py (the kernel against oracle/lidar_oracle.py on the same
inputs).  numpy only.

A CASE is dict(id, rings, pos [B,2], lidar_range, resolution, noise [B,R,2] or None, n_obs_max, v_max, expect_overflow [B]) and may
carry ``per_robot`` (``rings`` is then one list of rings PER ROBOT: env_shared = 0) and ``oracle_rings`` (per robot the rings the
oracle is given, where the contract of include/lipmpc.h says that the kernel drops some: a ring of more than ECAP edges, the rings
behind the RMAX-th in range; or where the map is too long for the oracle and the rings left out are shown to be out of reach).
Oracle results are computed once per case and shared, read only.

The ray phase (csrc/lipmpc_lidar_rays.inc) is restated here from its constants -- which rings are candidates, how the candidate list
is cut into staging chunks -- so that the CPU module can show what each case reaches.  RMAX, NCC, VFAST and ECAP are the constants
of that name in csrc/lipmpc_lidar.hip; CHUNK is the wave width (one candidate a lane)."""
import functools
import math

import numpy as np

import lidar_oracle as L

RMAX = 384           # candidates a scan lists (and rays)
NCC = 64             # candidates with a cached bounding circle for the sector test
VFAST = 8            # v_env up to which a ring is fetched in one round of loads
ECAP = 152           # edges staged per chunk
CHUNK = 64           # candidates staged per chunk
MAX_CLUSTERS = 64    # clusters a scan keeps on record (csrc/lipmpc_lidar_hulls.inc)


# -- the kernel's rules, restated ----------------------------------------------------------------------------------------------------
def pack(rings):
    """(xy [n,v,2], nv [n]) of a list of rings, as LidarSensor lays them out."""
    n, v = len(rings), max([1] + [len(r) for r in rings])
    xy, nv = np.zeros((max(n, 1), v, 2)), np.zeros(max(n, 1), np.int64)
    for j, r in enumerate(rings):
        xy[j, :len(r)] = r
        nv[j] = len(r)
    return xy[:n], nv[:n]


def circles(xy, nv):
    """Centre (the vertex mean, summed in ring order) and radius of every ring's bounding circle, as the candidate pass forms them."""
    m, n = np.zeros((len(nv), 2)), np.maximum(nv, 1)[:, None]
    for e in range(xy.shape[1]):
        m += np.where((e < nv)[:, None], xy[:, e], 0.0)
    m /= n
    rad2 = np.zeros(len(nv))
    for e in range(xy.shape[1]):
        d = xy[:, e] - m
        rad2 = np.where(e < nv, np.maximum(rad2, d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]), rad2)
    return m, np.sqrt(rad2) * (1.0 + 1e-12)


def candidates(pos, xy, nv, lidar_range):
    """(indices of the rings that pass the candidate test, in list order; |distance - reach| / reach of EVERY ring with vertices):
    a ring is a candidate when its circle's centre lies within reach = (range + radius) (1 + 1e-9) + 1e-9 of the robot."""
    m, rad = circles(xy, nv)
    reach = (lidar_range + rad) * (1.0 + 1e-9) + 1e-9
    d2 = (m[:, 0] - pos[0]) ** 2 + (m[:, 1] - pos[1]) ** 2
    with np.errstate(invalid="ignore"):
        keep = (nv > 0) & (d2 <= reach * reach)
        margin = np.abs(np.sqrt(d2) - reach) / reach
    return np.nonzero(keep)[0], margin[nv > 0]


def chunks(edge_counts):
    """The staging chunks of a candidate list with these edge counts: [(first position, candidates, skipped)].  A chunk is the
    longest prefix of at most CHUNK candidates whose edges sum to at most ECAP; a ring of more than ECAP edges at the head of a chunk
    is skipped (a chunk of one, nothing staged)."""
    out, k, n = [], 0, len(edge_counts)
    while k < n:
        tot = fit = 0
        while fit < CHUNK and k + fit < n and tot + edge_counts[k + fit] <= ECAP:
            tot += edge_counts[k + fit]
            fit += 1
        out.append((k, max(fit, 1), fit == 0))
        k += max(fit, 1)
    return out


def slots(pts, labels, n_obs_max, v_max):
    """(rings, overflow) that the hull stage makes of clustered readings: more than MAX_CLUSTERS clusters, a hull beyond the
    n_obs_max-th or one of more than v_max vertices set the flag (that hull is dropped, later ones may still fit)."""
    n_cl = labels.max() + 1 if len(labels) else 0
    rings, overflow = [], int(n_cl > MAX_CLUSTERS)
    for k in range(n_cl):
        ring = L.hull_ring(pts[labels == k])
        if ring is None:
            continue
        if len(rings) >= n_obs_max or len(ring) > v_max:
            overflow = 1
            continue
        rings.append(ring)
    return rings, overflow


# -- shapes --------------------------------------------------------------------------------------------------------------------------
def gon(n, centre, radius, seed=0, phase=0.1):
    """A regular n-gon whose radius wobbles by a fraction of its sagitta: no three vertices in line."""
    u = np.random.default_rng(1000 * n + seed).uniform(-1.0, 1.0, n)
    r = radius * (1.0 + 0.2 * (1.0 - math.cos(2 * math.pi / n)) * u)
    t = phase + 2 * math.pi * np.arange(n) / n
    return np.asarray(centre, float) + np.stack([r * np.cos(t), r * np.sin(t)], 1)


def _noise(B, R, seed, quiet=()):
    n = L.NOISE_STD * np.random.default_rng(seed).standard_normal((B, R, 2))
    n[list(quiet)] = 0.0
    return n


def _case(rings, pos, lidar_range, resolution, seed, n_obs_max=16, v_max=64, quiet=(), **more):
    pos = np.asarray(pos, float)
    return dict(rings=rings, pos=pos, lidar_range=float(lidar_range), resolution=int(resolution),
                noise=_noise(len(pos), resolution, seed, quiet), n_obs_max=n_obs_max, v_max=v_max, **more)


# -- 1. ring sizes -------------------------------------------------------------------------------------------------------------------
GON_AT, GON_R = (2.0, 0.5), 1.2
GON_ROBOTS = [(0.0, 0.0), (2.1, 0.7), (-1.5, 0.5)]         # outside; inside the long ring; the long ring partly in range


def _small_rings():
    tri = np.array([[0.0, 0.0], [0.3, 0.05], [0.1, 0.3]])
    quad = np.array([[0.0, 0.0], [0.35, 0.0], [0.4, 0.3], [0.05, 0.35]])
    pent = np.array([[0.0, 0.0], [0.3, -0.05], [0.45, 0.2], [0.2, 0.4], [-0.05, 0.25]])
    return [tri + (1.0, -1.5), quad + (-1.0, 1.0)], [pent + (0.5, 2.0), tri + (3.9, 0.4), quad + (-2.5, -0.6)]


def gon_map(n, shift=(0.0, 0.0)):
    """3- to 5-vertex rings before and behind one n-gon in the list."""
    before, behind = _small_rings()
    rings = before + [gon(n, GON_AT, GON_R)] + behind
    return [r + np.asarray(shift, float) for r in rings]


def gon_case(n):
    c = _case(gon_map(n), GON_ROBOTS, 3.0, 360, seed=n)
    if n > ECAP:                                              # the contract: the ring is skipped and the scan flagged
        c["oracle_rings"] = [[r for r in c["rings"] if len(r) <= ECAP]] * len(GON_ROBOTS)
    return c


# -- 2. chunking ---------------------------------------------------------------------------------------------------------------------
def edges_160():
    """20 octagons round the robots: 19 fill the first chunk to exactly ECAP edges, the 20th -- which stands in front of the first
    -- makes a second."""
    rings = [gon(8, (2.0 * math.cos(2 * math.pi * k / 19), 2.0 * math.sin(2 * math.pi * k / 19)), 0.15, seed=k) for k in range(19)]
    rings.append(gon(8, (1.0, 0.0), 0.15, seed=19))
    return _case(rings, [(0.0, 0.0), (0.3, 0.2), (-0.4, 0.1)], 3.0, 129, seed=160, n_obs_max=24)


def two_hundreds():
    """Two 100-gons, the second between the robots and the first: it does not fit the first chunk's remaining 52 edges."""
    rings = [np.array([[0.0, 0.0], [0.3, 0.05], [0.1, 0.3]]) + (-1.0, -1.0), gon(100, (2.0, 0.0), 0.8), gon(100, (0.9, 0.2), 0.3),
             np.array([[0.0, 0.0], [0.35, 0.0], [0.4, 0.3], [0.05, 0.35]]) + (0.0, 1.5)]
    return _case(rings, [(0.0, 0.0), (0.2, -0.6), (2.0, 0.1)], 3.0, 180, seed=200)


# the exact tie: ray 7 of 65 from (0, 0) meets edge A and edge B at bit-identical distances and at points one rounding apart (found
# by search on the oracle's arithmetic; tests/test_lidar_ring_cases_oracle.py asserts it)
TIE_RAY, TIE_RES = 7, 65
_H = float.fromhex
TIE_A = np.array([[_H("0x1.c537bb3f09314p-2"), _H("0x1.aef4427f53cdfp-2")], [_H("0x1.ff680e98f75f3p-2"), _H("0x1.546c0cd35d069p-2")]])
TIE_B = np.array([[_H("0x1.dae230119713bp-2"), _H("0x1.b82e6539b82fap-2")], [_H("0x1.e8522925b354bp-2"), _H("0x1.4d675dde585fap-2")]])
TIE_POS, TIE_LATE = 3, 64                                 # their positions among the rings in range
# the mirror pair: images of each other about ray 0 from a robot on y = 0 (the same arithmetic up to signs: the same bits)
MIRROR_A = np.array([[0.5, -0.25], [0.75, 0.125], [0.75, -0.25]])
MIRROR_B = MIRROR_A * (1.0, -1.0)
MIRROR_POS, MIRROR_LATE = 5, 100
CAND_ROBOTS = [(0.0, 0.0), (0.09375, 0.046875)]
GOLDEN_ANGLE = math.pi * (3.0 - math.sqrt(5.0))


def _behind(edge, out=0.05):
    """The triangle on ``edge`` whose third vertex lies ``out`` farther from the origin."""
    mid = edge.mean(0)
    return np.vstack([edge, mid + out * mid / np.hypot(*mid)])


def cands(n_near, far_every=5):
    """``n_near`` small rings well within the range of both robots, far rings (beyond range + 10) between them in the list.  Those at
    positions below 64 stand 2.0 .. 2.4 from the origin, the later ones 1.0 .. 1.5: nearer on the same rays.  Most of the first 128
    are 2-vertex slivers (two edges: 64 of them fit a chunk, which then ends on the candidate count; 50 triangles fill a chunk's
    ECAP edges before that), every eighth a triangle; from 128 on all are triangles."""
    near = []
    for k in range(n_near):
        rho = (2.0 + 0.4 * ((k * 7) % 5) / 5.0) if k < CHUNK else (1.0 + 0.5 * ((k * 11) % 13) / 13.0)
        a = GOLDEN_ANGLE * k + 0.05
        c, t = rho * np.array([math.cos(a), math.sin(a)]), 0.04 * np.array([-math.sin(a), math.cos(a)])
        edge = np.array([c - t, c + t])
        near.append(_behind(edge) if (k % 8 == 3 or k >= 2 * CHUNK) else edge)
    near[TIE_POS] = _behind(TIE_A)
    near[TIE_LATE] = _behind(TIE_B)
    if n_near > MIRROR_LATE:
        near[MIRROR_POS], near[MIRROR_LATE] = MIRROR_A, MIRROR_B
    rings, is_near = [], []
    for k, r in enumerate(near):
        if k % far_every == 2:
            rings.append(np.array([[0.0, 0.0], [0.1, 0.0], [0.05, 0.1]]) + (40.0 + k, 30.0))
            is_near.append(False)
        rings.append(r)
        is_near.append(True)
    c = _case(rings, CAND_ROBOTS, 3.0, TIE_RES, seed=n_near, n_obs_max=32)
    c["near"] = np.array(is_near)
    if n_near > RMAX:                                         # the contract: the surplus is dropped, never read
        c["oracle_rings"] = [[r for r, nr in zip(rings, is_near) if nr][:RMAX]] * len(CAND_ROBOTS)
    return c


# -- 3. reach and indices ------------------------------------------------------------------------------------------------------------
def long_wall(v):
    """A wall 20 m long and 5 cm thick along y = 0.45 = 0.3 x range, from x = -1 to x = 19 (its centre 9 m = 6 x range from the first
    robot), as a ring of 4 vertices or -- with more vertices along its long sides -- of ``v``."""
    h = v // 2
    ring = np.array([(x, 0.45) for x in np.linspace(-1.0, 19.0, h)] + [(x, 0.5) for x in np.linspace(19.0, -1.0, v - h)])
    tri = np.array([[0.0, 0.0], [0.3, 0.05], [0.1, 0.3]])
    return _case([tri + (0.5, -1.0), ring, tri + (18.0, -0.9)], [(0.0, 0.0), (9.0, 0.0), (18.5, -0.2), (30.0, 0.0)], 1.5, 360, seed=v)


N_ENV_LONG = 65535
NEAR_SHARED = (0, 63, 64, 65533, 65534)
NEAR_PER_ROBOT = ((0, 63, 64, 65533, 65534), (1, 62, 65, 32768, 65534))
_SQ = np.array([[-0.1, -0.1], [0.1, -0.1], [0.1, 0.1], [-0.1, 0.1]])


def _long_list(near, lidar_range, pos):
    """N_ENV_LONG squares: those of ``near`` on a circle of radius 1.5 round the origin, every other one on a lattice beyond
    range + 10 of every robot -- asserted here by the distance of EVERY vertex, so that the oracle may leave them out."""
    j = np.arange(N_ENV_LONG)
    xy = (np.stack([100.0 + 0.5 * (j % 256), 100.0 + 0.5 * (j // 256)], 1)[:, None, :] + _SQ[None]).copy()
    for t, k in enumerate(near):
        a = 2 * math.pi * t / len(near) + 0.3
        xy[k] = _SQ * (1.0 + 0.1 * t) + (1.5 * math.cos(a), 1.5 * math.sin(a))
    far = np.ones(N_ENV_LONG, bool)
    far[list(near)] = False
    for p in pos:
        assert np.hypot(xy[far, :, 0] - p[0], xy[far, :, 1] - p[1]).min() > lidar_range + 10.0
    return xy


def n_env_65535(per_robot):
    if not per_robot:
        pos = [(0.0, 0.0), (0.4, -0.3), (-0.2, 0.5)]
        xy = _long_list(NEAR_SHARED, 3.0, pos)
        return _case(list(xy), pos, 3.0, 65, seed=65535, oracle_rings=[[xy[k] for k in NEAR_SHARED]] * len(pos))
    pos = [(0.0, 0.0), (0.4, -0.3)]
    maps = [_long_list(near, 3.0, pos) for near in NEAR_PER_ROBOT]
    return _case([list(m) for m in maps], pos, 3.0, 65, seed=65536, per_robot=True,
                 oracle_rings=[[m[k] for k in near] for m, near in zip(maps, NEAR_PER_ROBOT)])


# -- 4. the boundaries of the hit test -------------------------------------------------------------------------------------------------
SITE, BOUNDARY_RANGE = 16.0, 2.0
BOUNDARY_INPUTS = (("vertex", "collinear", "at_range", "on_edge", "on_vertex"), ("inside", "coincident", "two_vertex", "one_vertex", "gon40"))
BOUNDARY_RES = (4, 8, 360)
QUIET = ("on_edge", "on_vertex")                          # no noise: every reading is the robot's own position


def _site(name):
    """The rings of one input round a robot at the origin; every coordinate a multiple of 1/8 (but the 40-gon's), so that ray 0 --
    direction (1, 0) exactly -- meets the vertices and edges it is meant to meet."""
    sq = np.array([[0.0, 0.0], [0.5, 0.0], [0.5, 0.5], [0.0, 0.5]])
    back = np.array([[-1.0, -0.5], [-0.5, -0.5], [-0.5, 0.5], [-1.0, 0.5]])       # something to read behind the robot
    return {
        "vertex": [np.array([[1.0, 0.0], [1.5, -0.5], [1.75, 0.0], [1.5, 0.5]]), back],     # ray 0 through the vertex of edge 0 and the closing edge
        "collinear": [sq + (1.0, 0.0), back],                                              # ray 0 along edge 0
        "at_range": [sq * 2.0 + (2.0, -0.5), back],                                        # ray 0 meets the closing edge at exactly 2.0
        "on_edge": [np.array([[-0.5, -0.25], [0.5, 0.25], [0.25, 1.0], [-0.75, 0.5]])],      # the robot on edge 0 (no ray along it)
        "on_vertex": [np.array([[0.0, 0.0], [1.0, 0.5], [0.5, 1.0]])],                      # the robot on vertex 0
        "inside": [np.array([[-0.75, -0.5], [0.5, -0.75], [1.0, 0.25], [0.0, 1.0], [-1.0, 0.25]])],
        "coincident": [sq + (1.0, -0.25), sq + (1.0, -0.25), back],
        "two_vertex": [np.array([[1.0, -0.5], [1.0, 0.5]]), back],
        "one_vertex": [np.array([[1.0, 0.0]]), back],
        "gon40": [gon(40, (0.25, 0.125), 1.0)],
    }[name]


def boundaries(group, resolution):
    """Five inputs SITE apart on one map, one robot each."""
    rings, pos = [], []
    for s, name in enumerate(BOUNDARY_INPUTS[group]):
        rings += [r + (SITE * s, 0.0) for r in _site(name)]
        pos.append((SITE * s, 0.0))
    quiet = [s for s, name in enumerate(BOUNDARY_INPUTS[group]) if name in QUIET]
    return _case(rings, pos, BOUNDARY_RANGE, resolution, seed=10 * group + resolution, quiet=quiet, inputs=BOUNDARY_INPUTS[group])


# -- 5. resolutions and positions ------------------------------------------------------------------------------------------------------
RESOLUTIONS = (1, 2, 63, 64, 65, 128, 129, 383)


@functools.lru_cache(maxsize=None)
def crowded_map():
    """Hulls of five random points round centres at least 1.3 apart on [-1, 6]^2: a crowded map of 3- to 5-vertex rings."""
    rng = np.random.default_rng(77)
    rings, ctrs = [], []
    while len(rings) < 18:
        c = rng.uniform(-1.0, 6.0, 2)
        if all(np.hypot(*(c - o)) >= 1.3 for o in ctrs):
            ring = L.hull_ring(c + rng.uniform(-0.5, 0.5, (5, 2)))
            if ring is not None:
                rings.append(ring)
                ctrs.append(c)
    return rings


def res_case(R):
    pos = np.random.default_rng(R).uniform(-1.0, 6.0, (4, 2))
    return _case(crowded_map(), pos, 1.5, R, seed=5000 + R)


FAR = (2.0 ** 20, -2.0 ** 20)


def far_origin():
    return _case(gon_map(40, FAR), np.array(GON_ROBOTS) + FAR, 3.0, 360, seed=40)


ODD = {1: (math.nan, 0.0), 3: (0.5, math.inf), 4: (-math.inf, 0.3)}


def odd_positions():
    pos = [(0.0, 0.0), None, (2.1, 0.7), None, None, (-1.5, 0.5)]
    return _case(gon_map(40), [ODD.get(b, p) for b, p in enumerate(pos)], 3.0, 360, seed=41, odd=tuple(ODD))


BUILDERS = {f"gon{n}": functools.partial(gon_case, n) for n in (9, 40, 152, 153)}
BUILDERS.update(edges_160=edges_160, two_hundreds=two_hundreds)
BUILDERS.update({f"cands_{n}": functools.partial(cands, n) for n in (65, 128, 129, 384, 385)})
BUILDERS.update(long_wall=functools.partial(long_wall, 4), long_wall_12=functools.partial(long_wall, 12))
BUILDERS.update(n_env_65535=functools.partial(n_env_65535, False), n_env_65535_per_robot=functools.partial(n_env_65535, True))
BUILDERS.update({f"boundaries_{'ab'[g]}_{R}": functools.partial(boundaries, g, R) for g in (0, 1) for R in BOUNDARY_RES})
BUILDERS.update({f"res{R}": functools.partial(res_case, R) for R in RESOLUTIONS})
BUILDERS.update(far_origin=far_origin, odd_positions=odd_positions)
IDS = tuple(BUILDERS)
GOLDEN_IDS = tuple(i for i in IDS if i.startswith("boundaries")) + ("gon9", "gon40", "long_wall")


def rings_of(c, b):
    """The true map of robot ``b``."""
    return c["rings"][b] if c.get("per_robot") else c["rings"]


@functools.lru_cache(maxsize=None)
def _built(id_):
    c = BUILDERS[id_]()
    c["id"] = id_
    return c


@functools.lru_cache(maxsize=None)
def route(id_):
    """Per robot what the ray phase does with the case: dict(cand = the candidates' ring indices in list order, listed = those the
    list holds (RMAX), margin = the least |distance - reach| / reach of any ring, edges = the listed rings' edge counts, chunks,
    skipped = listed rings of more than ECAP edges, in_ovf = the flag the ray phase raises)."""
    c, out, packed = _built(id_), [], None
    for b, p in enumerate(c["pos"]):
        if packed is None or c.get("per_robot"):
            packed = pack(rings_of(c, b))
        xy, nv = packed
        cand, margin = candidates(p, xy, nv, c["lidar_range"])
        listed = cand[:RMAX]
        edges = [int(nv[j]) for j in listed]
        ch = chunks(edges)
        skipped = [int(listed[k]) for k, _, skip in ch if skip]
        out.append(dict(cand=cand, listed=listed, margin=float(margin[np.isfinite(margin)].min()) if np.isfinite(margin).any() else math.inf, edges=edges,
                        chunks=ch, skipped=skipped, in_ovf=int(len(cand) > RMAX or bool(skipped)), v_env=int(xy.shape[1])))
    return out


@functools.lru_cache(maxsize=None)
def oracle(id_):
    """oracle/lidar_oracle.py::range_finder per robot: [dict(hits [R,2] with NaN where no reading, valid, labels [R] with -2 where no
    reading, rings, overflow = the hull stage's flag)], computed once and shared (read only)."""
    return scan(_built(id_), _built(id_)["noise"])


def scan(c, noise):
    """``oracle`` under another noise sample [B,R,2] (the golden vectors carry the reference's own)."""
    tab, out = L.ray_table(c["resolution"]), []
    for b, p in enumerate(c["pos"]):
        rings = c["oracle_rings"][b] if "oracle_rings" in c else rings_of(c, b)
        with np.errstate(invalid="ignore"):                   # (a robot at NaN or inf)
            hits, valid, labels, _ = L.range_finder(p, rings, c["lidar_range"], noise=None if noise is None else noise[b], table=tab)
        inferred, overflow = slots(hits[valid], labels, c["n_obs_max"], c["v_max"])
        full = np.full(len(valid), -2)
        full[valid] = labels
        out.append(dict(hits=np.where(valid[:, None], hits, np.nan), valid=valid, labels=full, rings=inferred, overflow=overflow))
    return out


@functools.lru_cache(maxsize=None)
def case(id_):
    """The case with ``expect_overflow`` [B]: the ray phase's flag (``route``) or the hull stage's (``oracle``)."""
    c = dict(_built(id_))
    c["expect_overflow"] = np.array([r["in_ovf"] | o["overflow"] for r, o in zip(route(id_), oracle(id_))])
    return c


# -- which hits the chunks hand on -----------------------------------------------------------------------------------------------------
def ring_scan(pos, ring, lidar_range, table):
    """Per ray the nearest hit of ONE ring as oracle/lidar_oracle.py::lidar_hits finds it: (distance [R], inf where none; point [R,2])."""
    x, y = float(pos[0]), float(pos[1])
    dist, pts, n = np.full(len(table), math.inf), np.zeros((len(table), 2)), len(ring)
    for i in range(len(table)):
        end = (x + lidar_range * table[i, 0], y + lidar_range * table[i, 1])
        best = lidar_range
        for e in range(n):
            p = L._segment_hit((x, y), end, ring[e], ring[(e + 1) % n])
            if p is None:
                continue
            d = math.sqrt((p[0] - x) * (p[0] - x) + (p[1] - y) * (p[1] - y))
            if d < best:
                best, dist[i], pts[i] = d, d, p
    return dist, pts


@functools.lru_cache(maxsize=None)
def handovers(id_, b=0):
    """Robot ``b``'s listed candidates walked chunk by chunk: dict(overwritten = rays on which a ring of a LATER chunk takes the hit
    from a ring of an earlier one, ties = [(ray, earlier position, later position, distinct)] where a later ring (of another chunk)
    meets the ray at the bit-identical distance of the hit that stands and loses -- ``distinct``: at another point)."""
    c, r = _built(id_), route(id_)[b]
    tab = L.ray_table(c["resolution"])
    chunk_of = np.zeros(len(r["listed"]), int)
    for n, (k, cnt, _) in enumerate(r["chunks"]):
        chunk_of[k:k + cnt] = n
    R = c["resolution"]
    best, best_pt, owner = np.full(R, c["lidar_range"]), np.zeros((R, 2)), np.full(R, -1)
    overwritten, ties = set(), []
    for k, j in enumerate(r["listed"]):
        ring = rings_of(c, b)[j]
        if len(ring) > ECAP:
            continue
        dist, pts = ring_scan(c["pos"][b], ring, c["lidar_range"], tab)
        for i in np.nonzero(dist < math.inf)[0]:
            if dist[i] < best[i]:
                if owner[i] >= 0 and chunk_of[k] > chunk_of[owner[i]]:
                    overwritten.add(int(i))
                best[i], best_pt[i], owner[i] = dist[i], pts[i], k
            elif dist[i] == best[i] and chunk_of[k] > chunk_of[owner[i]]:
                ties.append((int(i), int(owner[i]), k, bool(np.any(pts[i] != best_pt[i]))))
    ties = [t for t in ties if owner[t[0]] == t[1]]            # the earlier ring's hit is the ray's final reading
    return dict(overwritten=sorted(overwritten), ties=ties, owner=owner, best=best, best_pt=best_pt)
