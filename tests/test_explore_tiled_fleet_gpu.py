"""GPU: the exploring fleet with the two large-map explorers on the recorded open-field scene of tests/test_frontier_fleet_gpu.py
(tests/golden/exploration.npz): with rounds=None every tensor of a run with TiledCoordinatedFrontierPlanner or
TiledInformedFrontierPlanner is bit-identical to the run with its one-workgroup parent class."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import lipmpc  # noqa: E402
import test_frontier_fleet_gpu as base  # noqa: E402

PAIRS = {
    "coordinated": (lipmpc.CoordinatedFrontierPlanner, lipmpc.TiledCoordinatedFrontierPlanner, dict(r_claim=12, max_claims=8)),
    "informed": (lipmpc.InformedFrontierPlanner, lipmpc.TiledInformedFrontierPlanner, dict(r_view=10, w_gain=16, g_cap=120, min_gain=2)),
}


@pytest.mark.parametrize("kind", list(PAIRS))
def test_gpu_tiled_exploring_run_is_bit_identical(kind):
    parent, tiled, args = PAIRS[kind]
    d, occ, _ = base._scene()
    (W, H) = d["grid"].tolist()
    tw, th, _ = lipmpc.tiled_info()
    assert -(-W // tw) * -(-H // th) >= 2                      # more than one tile
    seed = d["seeds"].tolist()[0]
    kw = dict(args, r_inflate=int(d["r_inflate"]), min_unknown=int(d["min_unknown"]))
    fleet, mapper, _ = base._fleet(d, occ)
    want = base._explore(d, fleet, mapper, parent(**kw), seed)
    explorer = tiled(**kw)
    got = base._explore(d, fleet, mapper, explorer, seed)
    assert isinstance(explorer, parent) and set(got) == set(want) and ("n_claims" in want) == (kind == "coordinated")
    for k, v in want.items():
        if isinstance(v, np.ndarray):
            same = np.array_equal(v.view(np.int64) if v.dtype == np.float64 else v, got[k].view(np.int64) if v.dtype == np.float64 else got[k])
            assert same, k
        else:
            assert v == got[k], k
    assert want["n_frontier"][0, 0] > 0 and (want["n_steps"] > 0).all()
    if kind == "coordinated":
        assert want["n_claims"].max() >= 1 and int(explorer.last["claims_settled"][0]) == 1
    else:
        assert explorer.last["usettled"].tolist() == [1]
