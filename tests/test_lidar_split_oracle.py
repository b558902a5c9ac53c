"""CPU: the sector-split rule (include/lipmpc.h, lipmpc_lidar_c_eta_split_batch) as tests/lidar_split_oracle.py restates it, on its
own: the pieces partition every cluster, no piece spans more than split_rays rays, a split that is no smaller than every extent is
the identity, the anchor and its tie rule on hand-made ray sets, and -- the point of it all -- no piece's hull contains the
robot on noise-free grid readings."""
import numpy as np
import pytest

import grid_lidar_oracle as G
import lidar_oracle as L
import lidar_split_oracle as S


def _span(rays, R):
    """Consecutive rays the set covers, cyclically: R less the largest gap, plus one."""
    rays = sorted(int(r) for r in rays)
    if len(rays) == 1:
        return 1
    return R - max((rays[t] - rays[t - 1]) % R for t in range(len(rays))) + 1


def _random_scan(rng, R):
    """Rays with a reading and labels: runs of rays dealt to clusters (a cluster may own several runs, one may wrap), some noise."""
    valid = np.zeros(R, bool)
    labels = np.full(R, -1)
    pos = int(rng.integers(0, R))
    n_cl = int(rng.integers(1, 9))
    for _ in range(int(rng.integers(1, 14))):
        length = int(rng.integers(1, R // 2))
        k = int(rng.integers(-1, n_cl))
        for t in range(length):
            if rng.random() < 0.85:
                valid[(pos + t) % R], labels[(pos + t) % R] = True, k
        pos += length + int(rng.integers(0, 30))
    rays = np.nonzero(valid)[0]
    lab = labels[rays]
    _, lab2 = np.unique(lab[lab >= 0], return_inverse=True)          # labels 0..n-1 without holes
    lab = lab.copy(); lab[lab >= 0] = lab2
    return rays, lab


@pytest.mark.parametrize("R", [360, 384, 90, 7])
def test_pieces_partition_clusters_and_span_at_most_split_rays(R):
    rng = np.random.default_rng(R)
    n_split = 0
    for _ in range(100):
        rays, labels = _random_scan(rng, R)
        for split in sorted({1, 2, 7, 30, 45, max(R // 2, 1)}):
            if split > max(R // 2, 1):
                continue
            pieces, n_pieces = S.piece_ids(rays, labels, split, R)
            assert np.all((pieces == -1) == (labels == -1))
            base = 0
            for k in range(labels.max() + 1 if len(labels) else 0):
                mine = pieces[labels == k]
                ids = np.unique(mine)
                # numbered cluster by cluster, without holes inside the count the rule gives, nobody else's numbers
                _, n_p, _ = S.cluster_pieces(rays[labels == k], split, R)
                assert ids.min() >= base and ids.max() < base + n_p
                assert not np.isin(pieces[labels != k], np.arange(base, base + n_p)).any()
                for i in ids:
                    assert _span(rays[pieces == i], R) <= split, (R, split, rays[pieces == i])
                n_split += n_p > 1
                base += n_p
            assert base == n_pieces
    assert n_split > 100


@pytest.mark.parametrize("R", [360, 90])
def test_identity_when_split_rays_covers_every_extent(R):
    rng = np.random.default_rng(5 + R)
    for _ in range(200):
        rays, labels = _random_scan(rng, R)
        spans = [_span(rays[labels == k], R) for k in range(labels.max() + 1 if len(labels) else 0)]
        off, n_off = S.piece_ids(rays, labels, 0, R)
        assert np.array_equal(off, labels)                            # off: a cluster is one piece, numbered by its label
        if spans and max(spans) <= R // 2:
            on, n_on = S.piece_ids(rays, labels, R // 2, R)
            assert np.array_equal(on, labels) and n_on == n_off
        big = max(spans + [1])
        on, n_on = S.piece_ids(rays, labels, big, R)                  # (the library caps split_rays at R / 2; the rule does not)
        assert np.array_equal(on, labels) and n_on == n_off


def test_anchor_and_tie_rule_by_hand():
    R = 360
    # a wrap across ray 0: rays 350..359 and 0..9 -- the largest gap (340) lies in front of ray 350
    rays = list(range(0, 10)) + list(range(350, 360))
    p, n_p, a = S.cluster_pieces(rays, 10, R)
    assert a == 350 and n_p == 2
    assert p == [1] * 10 + [0] * 10                                    # offsets 0..9 -> piece 0 are rays 350..359
    p, n_p, a = S.cluster_pieces(rays, 20, R)
    assert a == 350 and n_p == 1 and set(p) == {0}
    # a full circle: every gap is 1, the tie goes to the smallest ray
    p, n_p, a = S.cluster_pieces(range(R), 45, R)
    assert a == 0 and n_p == 8 and p == [t * 8 // 360 for t in range(R)]
    assert [p.count(i) for i in range(8)] == [45] * 8
    # two equal largest gaps: {10, 11, 190, 191} -- gaps 179 in front of 10 and of 190: the anchor is 10
    p, n_p, a = S.cluster_pieces([10, 11, 190, 191], 100, R)
    assert a == 10 and n_p == 2 and p == [0, 0, 1, 1]                  # extent 182, offsets 0, 1, 180, 181
    # ... the same pair of gaps across ray 0: the smallest ray with the largest gap, not the first in cyclic order
    p, n_p, a = S.cluster_pieces([0, 1, 180, 181], 100, R)
    assert a == 0
    # n = 1: the gap is R, the extent 1, one piece
    p, n_p, a = S.cluster_pieces([123], 1, R)
    assert (p, n_p, a) == ([0], 1, 123)
    # balanced: an extent of 91 at 45 rays per piece is three pieces of 31, 30, 30 rays, not 45 + 45 + 1
    p, n_p, a = S.cluster_pieces(range(100, 191), 45, R)
    assert n_p == 3 and [p.count(i) for i in range(3)] == [31, 30, 30]
    # piece_ids: noise keeps -1, clusters in label order
    pieces, n = S.piece_ids([3, 4, 5, 6, 200, 201], [1, 1, -1, 1, 0, 0], 2, R)
    assert pieces.tolist() == [1, 1, -1, 2, 0, 0] and n == 3


def _strictly_inside(ring, q):
    """q strictly inside the CCW convex ring."""
    a, b = ring, np.roll(ring, -1, axis=0)
    cr = (b[:, 0] - a[:, 0]) * (q[1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (q[0] - a[:, 0])
    return bool(np.all(cr > 0))


@pytest.mark.parametrize("R", [360, 90])
def test_no_piece_hull_contains_the_robot_on_noise_free_grid_readings(R):
    """split_rays <= R / 2: a piece's rays lie in an open half-plane through the robot, the robot is an extreme point of the cone
    that holds the readings, so it is not in their hull -- in the three rooms and on the fixture's boxes; and the defect this
    mends: one hull per cluster DOES contain a robot standing in a room."""
    tab = L.ray_table(R)
    occ, origin, cell = S.rooms_scene()
    fx = G.fixture()
    rng = np.random.default_rng(1)
    rooms = [p for p in rng.uniform((0.3, 0.3), (6.1, 5.3), (200, 2)) if not occ[int(p[0] / 0.1) - 1:int(p[0] / 0.1) + 2, int(p[1] / 0.1) - 1:int(p[1] / 0.1) + 2].any()][:12]
    cases = [(p, occ, origin, cell, 3.0) for p in rooms] + [(p, fx["occ"], fx["origin"], fx["cell"], 1.5) for p in fx["pos"][:12]]
    n_hulls = n_inside_unsplit = 0
    for pos, oc, org, cl, rng_ in cases:
        hits, valid = G.grid_hits(pos, oc, org, cl, rng_, tab)
        for split in (1, 7, 30, 45, R // 2):
            if split > R // 2:
                continue
            sc = S.split_scan(hits, valid, split, 64, 64)
            if sc["rings"] is None:
                continue
            for ring in sc["rings"]:
                assert not _strictly_inside(ring, pos), (pos, split)
                n_hulls += 1
        for ring in S.split_scan(hits, valid, 0, 64, 64)["rings"]:
            n_inside_unsplit += _strictly_inside(ring, pos)
    assert n_hulls > 100 and n_inside_unsplit >= len(rooms) // 2
