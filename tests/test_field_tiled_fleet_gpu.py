"""GPU: the exploring fleet with a tiled FrontierPlanner on the recorded open-field scene of tests/test_frontier_fleet_gpu.py
(tests/golden/exploration.npz): with rounds=None every tensor of the run is bit-identical to the run with tiled=False, and with a
budget of one round -- replans that come back RRT_FIELD_UNSETTLED -- the run still ends, such a robot parked and never ``done``."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import lipmpc  # noqa: E402
import test_frontier_fleet_gpu as base  # noqa: E402


def _explorer(d, **kw):
    return lipmpc.FrontierPlanner(r_inflate=int(d["r_inflate"]), min_unknown=int(d["min_unknown"]), **kw)


def test_gpu_tiled_exploring_run_is_bit_identical():
    d, occ, _ = base._scene()
    seed = d["seeds"].tolist()[0]
    fleet, mapper, plain = base._fleet(d, occ)
    want = base._explore(d, fleet, mapper, plain, seed)
    got = base._explore(d, fleet, mapper, _explorer(d, tiled=True), seed)
    assert set(got) == set(want)
    for k, v in want.items():
        if isinstance(v, np.ndarray):
            same = np.array_equal(v.view(np.int64) if v.dtype == np.float64 else v, got[k].view(np.int64) if v.dtype == np.float64 else got[k])
            assert same, k
        else:
            assert v == got[k], k
    assert want["n_frontier"][0, 0] > 0 and (want["n_steps"] > 0).all()


def test_gpu_unsettled_replans_park_robots_and_never_end_the_fleet():
    """rounds=1 on a map of more than one tile: a replan is settled only if nothing fell on a tile's rim in its one round.  Whatever
    each replan came to, the run ends after k_max samples; a robot whose closing plan is RRT_FIELD_UNSETTLED is parked and not
    ``done`` (``done`` reads RRT_NO_PATH only)."""
    d, occ, _ = base._scene()
    (W, H) = d["grid"].tolist()
    tw, th, _ = lipmpc.tiled_info()
    assert -(-W // tw) * -(-H // th) >= 2
    fleet, mapper, _ = base._fleet(d, occ)
    r = base._explore(d, fleet, mapper, _explorer(d, tiled=True, rounds=1), d["seeds"].tolist()[0])
    K, every = int(d["k_max"]), int(d["replan_every"])
    assert r["n_replans"] == (K + every - 1) // every and r["X_pred"].shape[1] == K + 1
    unsettled = r["explore_status"] == lipmpc.RRT_FIELD_UNSETTLED
    print("closing plan", r["explore_status"].tolist(), "done", r["done"].tolist(), "frontier cells per replan", r["n_frontier"][:, 0].tolist())
    assert not r["done"][unsettled].any() and not r["walking"][unsettled].any()
    assert set(r["explore_status"].tolist()) <= {lipmpc.RRT_FOUND, lipmpc.RRT_NO_PATH, lipmpc.RRT_FIELD_UNSETTLED, lipmpc.RRT_PATH_OVERFLOW}
    assert np.array_equal(r["done"], (r["walking"] == 0) & np.isin(r["last_status"], base.SOLVED) & (r["explore_status"] == lipmpc.RRT_NO_PATH))
