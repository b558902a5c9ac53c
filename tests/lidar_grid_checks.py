"""What the GPU tests of the grid scan share (tests/test_lidar_grid_gpu.py, tests/test_gpu_poison.py): the device's hits against
tests/grid_lidar_oracle.py bit for bit, and everything behind the hits against the oracle chain of the polygon front end fed the
device's own hits.  numpy and the oracles only."""
import numpy as np

import grid_lidar_oracle as G
import lidar_oracle as L


def same_ring(a, b):
    if len(a) != len(b):
        return False
    k = int(np.argmin(np.abs(b - a[0]).sum(1)))
    return np.array_equal(np.roll(b, -k, axis=0), a)


def check_hits(g, pos, occ_of, origin, cell, lidar_range, table, noise, scan_of=None):
    """Device hits == oracle hits (+ noise), bit for bit; a robot in a solid cell: no reading, overflow, nothing inferred.
    ``scan_of(b)``: robot b's (hits, valid) by G.grid_hits on these very inputs, where a caller has computed them already."""
    n_hits = n_solid = 0
    for b in range(len(pos)):
        hits, valid = G.grid_hits(pos[b], occ_of(b), origin, cell, lidar_range, table) if scan_of is None else scan_of(b)
        if noise is not None:
            hits = hits + np.where(valid[:, None], noise[b], 0.0)
        gv = ~np.isnan(g["hits"][b, :, 0])
        assert np.array_equal(gv, valid), (b, int(gv.sum()), int(valid.sum()))
        assert np.array_equal(g["hits"][b][valid], hits[valid]), b
        n_hits += int(valid.sum())
        if G.in_solid_cell(pos[b], occ_of(b), origin, cell):
            n_solid += 1
            assert g["overflow"][b] == 1 and g["n_inferred"][b] == 0 and not gv.any(), b
            assert not g["c_eta"][b].any() and not g["obs_nv"][b].any()
    return n_hits, n_solid


def check_chain(g, pos, eps=L.DBSCAN_EPS, min_samples=L.DBSCAN_MIN_SAMPLES):
    """Labels, rings, n_inferred and (c, eta) of the launch against the oracle chain fed the device's own hits: the rule of the
    polygon front end's fuzz (labels equal, rings equal, c / eta within 1e-12), with and without noise.  (Readings on one face
    of a wall lie ON that face's boundary coordinate -- the contract places them there -- so a noise-free cluster on one face
    is exactly collinear for the kernel and for the oracle's rank test alike: no ring.)  Returns the rings compared."""
    import lipmpc_oracle as O
    n_rings = 0
    for b in range(len(pos)):
        valid = ~np.isnan(g["hits"][b, :, 0])
        assert np.all(g["labels"][b][~valid] == -2)
        pts = g["hits"][b][valid]
        if len(pts) == 0:
            assert g["n_inferred"][b] == 0
            continue
        labels = L.dbscan_labels(pts, eps, min_samples)
        assert np.array_equal(g["labels"][b][valid], labels), (b, len(pts))
        if g["overflow"][b]:
            continue
        want = [r for r in (L.hull_ring(pts[labels == k]) for k in range(labels.max() + 1)) if r is not None]
        assert g["n_inferred"][b] == len(want), (b, g["n_inferred"][b], len(want))
        for j, ring in enumerate(want):
            assert same_ring(g["obs_xy"][b, j, : g["obs_nv"][b, j]], ring), (b, j)
            c, eta, _, degen = O.closest_point_and_normal(pos[b], ring)
            if not degen:
                assert np.max(np.abs(g["c_eta"][b, j, :2] - c)) < 1e-12 and np.max(np.abs(g["c_eta"][b, j, 2:] - eta)) < 1e-12
            n_rings += 1
    return n_rings
