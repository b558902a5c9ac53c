"""Arrival table of the RRT* planner (tests/golden/RRT_PLANNER.md, tests/test_rrt_gpu.py::test_end_to_end_class):

    python tests/golden/make_rrt_arrival.py

For SimulationRRT, SimulationMaze1 and SimulationMaze2 of pdf_scenarios.npz and seeds 0..15: the oracle plan
(tests/rrt_oracle.py, default parameters, start at the origin), then the sub-goals walked one after the other with the
oracle closed loop (oracle/lipmpc_oracle.py run_closed_loop: interior mode, tol_interior 1e-6, N = 3, 300 samples,
sampling time 0.4, each run started from the last state of the previous one, as HumanoidMPCWithRRT.py:155-181 chains
them).  A seed ARRIVES if the final CoM is within 0.2 m of the goal cell.  Prints the table; the first two arriving seeds
per scene are the seeds of the GPU end-to-end test.
"""
import os
import sys
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
import lipmpc_oracle as O  # noqa: E402
import rrt_oracle as R  # noqa: E402

SCENES = ("SimulationRRT", "SimulationMaze1", "SimulationMaze2")


def scene(name):
    sc = np.load(os.path.join(HERE, "pdf_scenarios.npz"))
    rings = [sc[name + "/rings"][j][: sc[name + "/nv"][j]] for j in range(len(sc[name + "/nv"]))]
    return rings, np.asarray(sc[name + "/goal"], float)


def arrival(args):
    name, seed = args
    rings, goal = scene(name)
    res = R.plan(rings, goal, seed=seed)
    if res["status"] != R.FOUND:
        return name, seed, res["status"], 0, float("nan")
    st = np.zeros(5)
    for sg in res["sub_goals"]:
        X, _ = O.run_closed_loop(sg, rings, N_horizon=3, N_mpc_timesteps=300, sampling_time=0.4, init_state=tuple(st),
                                 params=O.Params(tol_interior=1e-6), exact=False)
        st = X[:, -1]
    dist = float(np.hypot(st[0] - res["sub_goals"][-1][0], st[2] - res["sub_goals"][-1][1]))
    return name, seed, res["status"], res["n_sub"], dist


def main():
    jobs = [(n, s) for n in SCENES for s in range(16)]
    with Pool(min(16, os.cpu_count() or 1)) as pool:
        rows = pool.map(arrival, jobs)
    for name in SCENES:
        r = [x for x in rows if x[0] == name]
        ok = [x[1] for x in r if x[4] <= 0.2]
        print(f"{name}: {len(ok)} of 16 arrive: {ok}; n_sub {[x[3] for x in r]}; "
              f"final distance {[round(x[4], 3) for x in r]}")


if __name__ == "__main__":
    main()
