"""CPU: the inputs of tests/lidar_ring_cases.py reach what they are named for, shown on the ray phase's rules as that module restates
them from the kernel's constants (csrc/lipmpc_lidar.hip: RMAX, NCC, VFAST, ECAP) and on oracle/lidar_oracle.py -- how many candidates
every robot has, how many staging chunks they make and whether a chunk ends on the candidate count or on the edge count, whether a
candidate sits at a position without a cached circle, whether the rings go through the serial vertex loop, on how many rays a later
chunk takes a hit from an earlier one, and the exact tie.  ``expect_overflow`` comes from these counts and from the oracle's clusters
and hulls, never from a device run.  The oracle itself is pinned to vectors of the reference (tests/golden/lidar_golden_edges.npz,
made by tests/golden/make_lidar_golden_edges.py).  No GPU: tests/test_lidar_rings_gpu.py runs the same inputs through the kernel."""
import math
import os

import numpy as np
import pytest

import lidar_oracle as L
import lidar_ring_cases as C

# id -> per robot (candidates, chunks)
ROUTES = {
    "gon9": [(5, 1), (5, 1), (4, 1)], "gon40": [(5, 1), (5, 1), (4, 1)], "gon152": [(5, 3), (5, 3), (4, 3)],
    "gon153": [(5, 3), (5, 3), (4, 3)], "edges_160": [(20, 2)] * 3, "two_hundreds": [(4, 2)] * 3,
    "cands_65": [(65, 2)] * 2, "cands_128": [(128, 2)] * 2, "cands_129": [(129, 3)] * 2, "cands_384": [(384, 8)] * 2,
    "cands_385": [(385, 8)] * 2, "long_wall": [(2, 1), (1, 1), (2, 1), (0, 0)], "long_wall_12": [(2, 1), (1, 1), (2, 1), (0, 0)],
    "n_env_65535": [(5, 1)] * 3, "n_env_65535_per_robot": [(5, 1)] * 2,
    "boundaries_a": [(2, 1), (2, 1), (2, 1), (1, 1), (1, 1)], "boundaries_b": [(1, 1), (3, 1), (2, 1), (2, 1), (1, 1)],
    "far_origin": [(5, 1), (5, 1), (4, 1)], "odd_positions": [(5, 1), (0, 0), (5, 1), (0, 0), (0, 0), (4, 1)],
}
V_ENV = {"gon9": 9, "gon40": 40, "gon152": 152, "gon153": 153, "edges_160": 8, "two_hundreds": 100, "long_wall": 4, "long_wall_12": 12,
         "n_env_65535": 4, "n_env_65535_per_robot": 4, "boundaries_a": 4, "boundaries_b": 40, "far_origin": 40, "odd_positions": 40,
         "cands_65": 3, "cands_128": 3, "cands_129": 3, "cands_384": 3, "cands_385": 3}
def _key(id_):
    return id_.rsplit("_", 1)[0] if id_.startswith("boundaries") else id_


SLOW = {i for i in C.IDS if V_ENV.get(_key(i), 5) > C.VFAST}          # the serial vertex loop


def test_the_chunk_rule():
    """A chunk is a prefix of at most 64 candidates whose edges sum to at most ECAP; a longer ring is a chunk of its own, skipped."""
    assert C.chunks([]) == []
    assert C.chunks([3] * 64) == [(0, 50, False), (50, 14, False)]             # 50 triangles are 150 edges
    assert C.chunks([2] * 65) == [(0, 64, False), (64, 1, False)]              # 64 slivers are 128: the candidate count ends the chunk
    assert C.chunks([8] * 20) == [(0, 19, False), (19, 1, False)]              # exactly ECAP fits
    assert C.chunks([100, 100]) == [(0, 1, False), (1, 1, False)]
    assert C.chunks([4, 152, 3]) == [(0, 1, False), (1, 1, False), (2, 1, False)]
    assert C.chunks([4, 153, 3]) == [(0, 1, False), (1, 1, True), (2, 1, False)]
    assert C.chunks([153]) == [(0, 1, True)]


@pytest.mark.parametrize("id_", C.IDS)
def test_case_shape_and_route(id_):
    """Every case: at most 8 robots, its candidate and chunk counts, the fetch route, no ring near the edge of the reach, and the
    expected flag from the counts."""
    c, route, want = C.case(id_), C.route(id_), C.oracle(id_)
    B = len(c["pos"])
    assert B <= 8 and c["noise"].shape == (B, c["resolution"], 2) and 1 <= c["resolution"] <= C.RMAX and c["v_max"] <= 64
    assert len(c["expect_overflow"]) == B == len(route) == len(want)
    got = [(len(r["cand"]), len(r["chunks"])) for r in route]
    print(id_, "candidates, chunks:", got, "least margin of the reach: %.2g" % min(r["margin"] for r in route),
          "readings:", [int(o["valid"].sum()) for o in want], "rings:", [len(o["rings"]) for o in want])
    if _key(id_) in ROUTES:
        assert got == ROUTES[_key(id_)]
        assert route[0]["v_env"] == V_ENV[_key(id_)]
    else:
        assert id_.startswith("res") and all(1 <= n <= 5 and k == 1 for n, k in got) and route[0]["v_env"] == 5
    assert (route[0]["v_env"] > C.VFAST) == (id_ in SLOW)
    # membership is never decided by a rounding: the kernel may contract the test's products, the restatement does not
    assert min(r["margin"] for r in route) > (1e-2 if id_.startswith(("cands_38", "n_env")) else 5e-5)
    for b, (r, o) in enumerate(zip(route, want)):
        late = len(r["listed"]) > C.NCC
        assert late == (id_.startswith("cands_")), (b, len(r["listed"]))
        assert r["in_ovf"] == int(len(r["cand"]) > C.RMAX or any(n > C.ECAP for n in r["edges"]))
        assert c["expect_overflow"][b] == (r["in_ovf"] | o["overflow"])
    if id_ not in ("gon153", "cands_385"):
        assert not c["expect_overflow"].any()                  # every ring of every other case is compared


def test_ring_size_cases():
    """gon9 / 40 / 152: the long ring shares its map with 3- to 5-vertex rings (and, up to 40 vertices, its chunk); one robot
    outside it, one inside, one with the ring partly in range.  gon153: the ring is a candidate of every robot, skipped and flagged;
    the oracle gets the map without it."""
    import lipmpc_oracle as O
    for n in (9, 40, 152, 153):
        c, route = C.case(f"gon{n}"), C.route(f"gon{n}")
        ring = c["rings"][2]
        assert len(ring) == n and sorted({len(r) for r in c["rings"]}) == [3, 4, 5, n]
        assert [bool(O.point_in_ring(p, ring)) for p in c["pos"]] == [False, True, False]
        d = np.hypot(*(ring - c["pos"][2]).T)
        assert d.min() < c["lidar_range"] < d.max()
        # no three consecutive vertices in line
        a, b, d3 = ring, np.roll(ring, -1, 0), np.roll(ring, -2, 0)
        assert np.all((b - a)[:, 0] * (d3 - b)[:, 1] - (b - a)[:, 1] * (d3 - b)[:, 0] != 0.0)
        for r in route:
            assert 2 in r["listed"]
            assert r["skipped"] == ([2] if n > C.ECAP else [])
        if n <= 40:
            assert all(len(r["chunks"]) == 1 for r in route)      # long and short rings in one chunk
    assert C.case("gon153")["expect_overflow"].tolist() == [1, 1, 1]
    assert all(len(r) <= C.ECAP for rings in C.case("gon153")["oracle_rings"] for r in rings)
    assert all(o["overflow"] == 0 for o in C.oracle("gon153"))    # the flag is the skipped ring's alone
    # the inside robot of gon9 .. gon152 reads on every ray, and its one hull fits the slots
    for n in (9, 40, 152):
        o = C.oracle(f"gon{n}")[1]
        assert o["valid"].all() and len(o["rings"]) == 1


def test_chunking_cases():
    """edges_160 and two_hundreds split on the edge count below 64 candidates; the cands cases have chunks that end on the
    candidate count (64 rings of two edges) and, from 128 on, chunks of 50 triangles; a later chunk takes hits from an earlier one."""
    sizes = lambda id_, b=0: [n for _, n, _ in C.route(id_)[b]["chunks"]]
    assert sizes("edges_160") == [19, 1] and sum(C.route("edges_160")[0]["edges"][:19]) == C.ECAP
    assert sizes("two_hundreds") == [2, 2] and C.route("two_hundreds")[0]["edges"] == [3, 100, 100, 4]
    assert sizes("gon152") == [2, 1, 2]
    assert sizes("cands_65") == [64, 1] and sizes("cands_128") == [64, 64] and sizes("cands_129") == [64, 64, 1]
    assert sizes("cands_384") == sizes("cands_385") == [64, 64, 50, 50, 50, 50, 50, 6]
    over = {id_: [len(C.handovers(id_, b)["overwritten"]) for b in range(len(C.case(id_)["pos"]))]
            for id_ in ("gon152", "edges_160", "two_hundreds", "cands_65", "cands_128", "cands_129", "cands_384", "cands_385")}
    print("rays on which a later chunk takes the hit from an earlier one, per robot:", over)
    assert over == {"gon152": [0, 14, 0], "edges_160": [3, 5, 3], "two_hundreds": [15, 5, 0], "cands_65": [0, 1],
                    "cands_128": [12, 13], "cands_129": [12, 13], "cands_384": [50, 44], "cands_385": [50, 44]}
    # the cands cases read from rings at positions 64 and above, which have no cached circle (cands_65 has one such ring: it loses
    # the tie on robot 0's ray and is read by robot 1)
    for id_ in ("cands_65", "cands_128", "cands_129", "cands_384", "cands_385"):
        late = [int((C.handovers(id_, b)["owner"] >= C.NCC).sum()) for b in range(2)]
        assert late == [0, 1] if id_ == "cands_65" else min(late) >= 10, (id_, late)


@pytest.mark.parametrize("id_", ["cands_65", "cands_128", "cands_129", "cands_384", "cands_385"])
def test_the_exact_tie(id_):
    """Ray 7 of robot 0 meets the ring at position 3 and the ring at position 64 -- another chunk -- at bit-identical distances and
    at points one rounding apart: the oracle keeps the earlier ring's point, and only `strictly nearer` does.  From 128 rings on,
    ray 0 also meets a mirror pair (positions 5 and 100) at the same distance and the same point."""
    c, h = C.case(id_), C.handovers(id_, 0)
    assert (C.TIE_RAY, C.TIE_POS, C.TIE_LATE, True) in h["ties"]
    near = [r for r, nr in zip(c["rings"], c["near"]) if nr]
    tab = L.ray_table(c["resolution"])
    da, pa = C.ring_scan(c["pos"][0], near[C.TIE_POS], c["lidar_range"], tab)
    db, pb = C.ring_scan(c["pos"][0], near[C.TIE_LATE], c["lidar_range"], tab)
    i = C.TIE_RAY
    assert da[i] == db[i] and da[i].tobytes() == db[i].tobytes() and not np.array_equal(pa[i], pb[i])
    assert np.max(np.abs(pa[i] - pb[i])) < 1e-15
    o = C.oracle(id_)[0]
    assert o["valid"][i] and np.array_equal(o["hits"][i], pa[i] + c["noise"][0, i]) and not np.array_equal(o["hits"][i], pb[i] + c["noise"][0, i])
    if len(near) > C.MIRROR_LATE:
        assert (0, C.MIRROR_POS, C.MIRROR_LATE, False) in h["ties"]
        assert c["pos"][0, 1] == 0.0 and np.array_equal(near[C.MIRROR_LATE], near[C.MIRROR_POS] * (1.0, -1.0))


def test_list_length_cases():
    """cands_384 / 385: exactly RMAX rings in range and one more, each ring clearly in (every vertex within 0.9 x range of both robots)
    or clearly out (beyond range + 10); the oracle of 385 gets the first RMAX in list order."""
    for n in (65, 128, 129, 384, 385):
        c, route = C.case(f"cands_{n}"), C.route(f"cands_{n}")
        assert int(c["near"].sum()) == n and (~c["near"]).sum() > n // 6
        for p, r in zip(c["pos"], route):
            assert np.array_equal(r["cand"], np.nonzero(c["near"])[0])          # the restated test agrees with the construction
            for ring, nr in zip(c["rings"], c["near"]):
                d = np.hypot(*(ring - p).T)
                assert d.max() < 0.9 * c["lidar_range"] if nr else d.min() > c["lidar_range"] + 10.0
    c = C.case("cands_385")
    assert c["expect_overflow"].tolist() == [1, 1] and C.case("cands_384")["expect_overflow"].tolist() == [0, 0]
    first = [r for r, nr in zip(c["rings"], c["near"]) if nr][:C.RMAX]
    assert len(c["oracle_rings"][0]) == C.RMAX and all(a is b for a, b in zip(c["oracle_rings"][0], first))
    assert all(o["overflow"] == 0 for o in C.oracle("cands_385"))


def test_reach_and_index_cases():
    """long_wall: the wall's centre lies beyond 5 x range of a robot that one of its edges passes at 0.3 x range.  n_env_65535: the
    rings in range sit at the list positions the case names, every other ring beyond range + 10."""
    for id_ in ("long_wall", "long_wall_12"):
        c, route, want = C.case(id_), C.route(id_), C.oracle(id_)
        wall = c["rings"][1]
        assert len(wall) == (4 if id_ == "long_wall" else 12) and np.ptp(wall[:, 0]) == 20.0
        assert np.hypot(*(wall.mean(0) - c["pos"][0])) > 5 * c["lidar_range"] and abs(wall[:, 1].min() - 0.3 * c["lidar_range"]) < 1e-15
        assert 1 in route[0]["cand"] and int(want[0]["valid"].sum()) > 100
        assert len(route[3]["cand"]) == 0 and not want[3]["valid"].any()          # beyond the wall's reach
    c, route = C.case("n_env_65535"), C.route("n_env_65535")
    assert len(c["rings"]) == 65535
    for r in route:
        assert r["cand"].tolist() == list(C.NEAR_SHARED)
    c, route = C.case("n_env_65535_per_robot"), C.route("n_env_65535_per_robot")
    assert c["per_robot"] and [len(m) for m in c["rings"]] == [65535, 65535]
    assert [r["cand"].tolist() for r in route] == [list(n) for n in C.NEAR_PER_ROBOT]
    assert all(int(o["valid"].sum()) > 5 for id_ in ("n_env_65535", "n_env_65535_per_robot") for o in C.oracle(id_))


@pytest.mark.parametrize("R", C.BOUNDARY_RES)
def test_boundary_cases(R):
    """What the oracle reads at the boundaries of the hit test."""
    a, b = C.case(f"boundaries_a_{R}"), C.case(f"boundaries_b_{R}")
    wa, wb = C.oracle(f"boundaries_a_{R}"), C.oracle(f"boundaries_b_{R}")
    assert a["inputs"] + b["inputs"] == ("vertex", "collinear", "at_range", "on_edge", "on_vertex", "inside", "coincident",
                                         "two_vertex", "one_vertex", "gon40")
    tab = L.ray_table(R)
    assert tuple(tab[0]) == (1.0, 0.0)
    clean = lambda c, o, s: o["hits"][0] - c["noise"][s, 0]
    # ray 0 through a vertex: read at the vertex; along an edge: read at the edge's near end
    for s in (0, 1):
        assert wa[s]["valid"][0] and np.allclose(clean(a, wa[s], s), (C.SITE * s + 1.0, 0.0), atol=1e-15)
    # a hit at exactly the range is no reading
    assert not wa[2]["valid"][0]
    # the robot on an edge or on a vertex: every ray reads the robot's own position -- one cluster, no hull
    for s in (3, 4):
        assert wa[s]["valid"].all() and np.all(wa[s]["hits"] == a["pos"][s]) and not a["noise"][s].any()
        assert wa[s]["rings"] == [] and wa[s]["overflow"] == 0 and (np.all(wa[s]["labels"] == 0) if R >= 3 else True)
    assert wb[0]["valid"].all() and wb[4]["valid"].all()                        # inside a pentagon, inside the 40-gon
    # coincident rings, the 2-vertex ring: read on ray 0 at x = 1; the 1-vertex ring is never read (ray 0 passes the ring behind)
    for s in (1, 2):
        assert wb[s]["valid"][0] and np.allclose(clean(b, wb[s], s), (C.SITE * s + 1.0, 0.0), atol=1e-15)
    assert not wb[3]["valid"][0] and wb[3]["valid"].any()
    for c in (a, b):
        for ring in c["rings"]:
            if len(ring) != 40:
                assert np.array_equal(ring * 8.0, np.round(ring * 8.0))           # exactly representable
    assert not a["expect_overflow"].any() and not b["expect_overflow"].any()


def test_resolution_and_position_cases():
    for R in C.RESOLUTIONS:
        c = C.case(f"res{R}")
        assert c["resolution"] == R and len(c["pos"]) == 4 and c["noise"].any() and {len(r) for r in c["rings"]} <= {3, 4, 5}
    assert sum(int(o["valid"].sum()) for R in C.RESOLUTIONS for o in C.oracle(f"res{R}")) > 1000
    far, near = C.case("far_origin"), C.case("gon40")
    assert np.max(np.abs(far["pos"] - C.FAR - near["pos"])) < 2.0 ** -32        # (translated up to the spacing of doubles at 2^20)
    for a, b in zip(C.oracle("far_origin"), C.oracle("gon40")):
        assert np.array_equal(a["valid"], b["valid"]) and np.nanmax(np.abs(a["hits"] - C.FAR - b["hits"])) < 0.05
    c, want = C.case("odd_positions"), C.oracle("odd_positions")
    assert c["odd"] == (1, 3, 4) and [bool(np.isfinite(p).all()) for p in c["pos"]] == [True, False, True, False, False, True]
    for b in c["odd"]:
        assert not want[b]["valid"].any() and want[b]["rings"] == [] and want[b]["overflow"] == 0
    for b, g in ((0, 0), (2, 1), (5, 2)):
        assert int(want[b]["valid"].sum()) == int(C.oracle("gon40")[g]["valid"].sum())


# -- the oracle against the reference's own readings -----------------------------------------------------------------------------------
def _same_ring(a, b):
    if len(a) != len(b):
        return False
    k = int(np.argmin(np.abs(b - a[0]).sum(1)))
    return np.array_equal(np.roll(b, -k, axis=0), a)


@pytest.mark.parametrize("id_", C.GOLDEN_IDS)
def test_oracle_matches_the_reference_on_the_edge_cases(golden_dir, id_):
    """lidar_golden_edges.npz: compute_lidar_readings and range_finder of the reference on these cases (made by importing it,
    tests/golden/make_lidar_golden_edges.py) -- readings bit for bit, scikit-learn's labels, Qhull's rings up to rotation."""
    d = np.load(os.path.join(golden_dir, "lidar_golden_edges.npz"))
    c = C.case(id_)
    noise = d[id_ + "/noise"]
    want = C.scan(dict(c, n_obs_max=1 << 20, v_max=1 << 20), noise)
    for b, o in enumerate(want):
        valid = d[id_ + "/valid"][b]
        assert np.array_equal(o["valid"], valid), b
        assert np.array_equal(o["hits"][valid], (d[id_ + "/clean"][b] + noise[b])[valid]), b
        assert np.array_equal(np.isnan(o["hits"][:, 0]), ~valid)
        if not d[id_ + "/clustered"][b]:
            continue
        assert np.array_equal(o["labels"], d[id_ + "/labels"][b]), b
        nv = d[id_ + "/inf_nv"][b]
        assert len(o["rings"]) == int((nv > 0).sum()), b
        for j, ring in enumerate(o["rings"]):
            assert _same_ring(ring, d[id_ + "/inf_xy"][b][j][: nv[j]]), (b, j)
