"""Golden vectors for the LiDAR front end at the EDGES of the hit test and on long rings, produced by IMPORTING the reference (build
container):

    PYTHONPATH=<reference checkout>:tests:oracle MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_lidar_golden_edges.py

The inputs are cases of tests/lidar_ring_cases.py (GOLDEN_IDS): the ten boundary inputs at 4, 8 and 360 rays -- a ray through a
vertex, along an edge, a hit at exactly the range, the robot on an edge, on a vertex and inside a ring, coincident rings, rings of
two vertices and of one, a 40-gon -- and gon9, gon40 and long_wall.  Per case and robot: the reference's compute_lidar_readings,
then its range_finder with numpy's global generator seeded, so that the noise it drew is recovered by subtraction (the robots on an
edge and on a vertex are scanned with noisy=False: their readings are to stay identical), scikit-learn's clusters and Qhull's rings.
Where range_finder raises on an input, that robot's readings are recorded alone (``clustered`` = False).  On these inputs it raises
for none.  Output: lidar_golden_edges.npz (data only; keys "<case id>/<array>").
"""
import os

import numpy as np

from HumanoidNavigation.RangeFinder import range_finder_wth_polygons_dbscan as rf

import lidar_ring_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_INF, VMAX_INF = 8, 64


def main():
    out, raised = {}, []
    for n, id_ in enumerate(C.GOLDEN_IDS):
        c = C.case(id_)
        B, R = len(c["pos"]), c["resolution"]
        clean = np.zeros((B, R, 2)); valid = np.zeros((B, R), bool); noise = np.zeros((B, R, 2))
        labels = np.full((B, R), -2, np.int32)                      # -2 = no reading, -1 = DBSCAN noise
        inf_xy = np.zeros((B, MAX_INF, VMAX_INF, 2)); inf_nv = np.zeros((B, MAX_INF), np.int32)
        clustered = np.zeros(B, bool)
        for b, pos in enumerate(c["pos"]):
            rings, pos = [np.asarray(r, float) for r in c["rings"]], tuple(float(v) for v in pos)
            cl = rf.compute_lidar_readings(pos, rings, lidar_range=c["lidar_range"], resolution=R)
            for k in range(R):
                if cl[k] is not None:
                    valid[b, k] = True; clean[b, k] = cl[k]
            np.random.seed(7000 + 10 * n + b)
            try:
                no, clusters, local = rf.range_finder(pos, rings, lidar_range=c["lidar_range"], resolution=R, noisy=bool(c["noise"][b].any()))
            except Exception as e:                                  # a degenerate input: the readings alone
                raised.append((id_, b, repr(e)))
                continue
            clustered[b] = True
            for k in range(R):
                if cl[k] is not None:
                    noise[b, k] = np.array(no[k]) - np.array(cl[k])
            # a reading's label: the cluster that holds its point (identical points share their cluster)
            labels[b][valid[b]] = -1
            for lab, cpts in enumerate(clusters):
                held = {tuple(q) for q in np.asarray(cpts)}
                for k in range(R):
                    if no[k] is not None and (float(no[k][0]), float(no[k][1])) in held:
                        labels[b, k] = lab
            assert len(local) <= MAX_INF
            for j, ring in enumerate(local):
                ring = ring[:-1]                                    # build_local_obstacles appends the first vertex again
                assert len(ring) <= VMAX_INF
                inf_xy[b, j, :len(ring)] = ring; inf_nv[b, j] = len(ring)
        for k, v in dict(clean=clean, valid=valid, noise=noise, labels=labels, inf_xy=inf_xy, inf_nv=inf_nv, clustered=clustered).items():
            out[f"{id_}/{k}"] = v
        print(id_, "readings", valid.sum(1).tolist(), "rings", (inf_nv > 0).sum(1).tolist(), "max hull vertices", int(inf_nv.max()))
    print("range_finder raised on:", raised)
    np.savez_compressed(os.path.join(HERE, "lidar_golden_edges.npz"), **out)


if __name__ == "__main__":
    main()
