"""GPU: the exploring fleet on the recorded open field (`field` of tests/golden/exploration_informed.npz) with
InformedFrontierPlanner(None, w_gain, g_cap, min_gain, gain_from="region", target="representative"): two runs give identical bits,
the first replan's dict is what the oracles say on the map and the positions it was planned on, and n_regions comes back per replan.
Nothing here asserts "sooner"."""
import functools
import os

import numpy as np
import pytest

import frontier_oracle as FR
import gain_oracle as G
import regions_oracle as RO

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import lipmpc  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SCENE = "field"
PLAN_KEYS = ("gain", "n_sources", "status", "n_sub", "target_cell", "target_gain", "n_frontier", "frontier", "label", "rep", "n_regions")


@functools.lru_cache(maxsize=None)
def _scene():
    d = np.load(os.path.join(HERE, "golden", "exploration_informed.npz"))
    (W, H) = d["grid"].tolist()
    occ = np.zeros((W, H), np.uint8)
    for i0, j0, i1, j1 in d["walls"]:
        occ[i0:i1, j0:j1] = 1
    return d, occ


def _explore(seed):
    d, occ = _scene()
    (W, H), origin, cell = d["grid"].tolist(), tuple(d["origin"].tolist()), tuple(d["cell"].tolist())
    w_hit, w_miss = (int(v) for v in d["weights"])
    rng = float(d["lidar_range"])
    mapper = lipmpc.OccupancyMapper(W, H, origin, cell, rng, w_hit=w_hit, w_miss=w_miss)
    fleet = lipmpc.UnknownEnvFleet(grid=lipmpc.GridMap(occ, origin, cell), N_horizon=3, lidar_range=rng, mapper=mapper,
                                   recover=int(d["max_recover"]))
    explorer = lipmpc.InformedFrontierPlanner(None, int(d["w_gain"]), int(d["g_cap"]), int(d["min_gain"]), gain_from="region",
                                              target="representative", r_inflate=int(d["r_inflate"]), min_unknown=int(d["min_unknown"]))
    first, plan = {}, explorer.plan

    def recording(m, pos, **kw):                              # the first replan's dict, with what it was planned on
        out = plan(m, pos, **kw)
        if not first:
            first.update({k: v.clone() for k, v in out.items()}, evidence=m.evidence.clone(), pos=pos.clone())
        return out
    explorer.plan = recording
    starts, K = d[f"{SCENE}/starts"], int(d[f"{SCENE}/k_max"])
    B = len(starts)
    st = np.zeros((B, 5)); st[:, 0] = starts[:, 0]; st[:, 2] = starts[:, 1]
    noise = torch.as_tensor(float(d["noise_std"]) * np.random.default_rng(seed).standard_normal((K, B, 360, 2)), device="cuda")
    r = fleet.run_exploring(torch.as_tensor(st, device="cuda"), torch.ones((B,), dtype=torch.int8, device="cuda"), K, explorer,
                            int(d["replan_every"]), float(d["lookahead"]), noise=noise)
    torch.cuda.synchronize()
    out = {k: (v.cpu().numpy().copy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}
    out["evidence"] = mapper.evidence.cpu().numpy().copy()
    out["closing"] = {k: explorer.last[k].cpu().numpy().copy() for k in PLAN_KEYS}
    out["first"] = {k: (v.view(torch.int32) if v.dtype == torch.uint32 else v).cpu().numpy().copy() for k, v in first.items()}
    return out


@functools.lru_cache(maxsize=None)
def _runs():
    seed = _scene()[0][f"{SCENE}/seeds"].tolist()[0]
    return _explore(seed), _explore(seed)


def test_gpu_two_runs_give_the_same_bits():
    a, b = _runs()
    same = lambda x, y: np.array_equal(x.view(np.int64) if x.dtype == np.float64 else x, y.view(np.int64) if y.dtype == np.float64 else y)
    assert set(a) == set(b)
    for k, v in a.items():
        if isinstance(v, np.ndarray):
            assert same(v, b[k]), k
        elif isinstance(v, dict):
            assert all(same(x, b[k][j]) for j, x in v.items()), k
        else:
            assert v == b[k], k


def test_gpu_the_first_replan_is_the_oracles():
    d, _ = _scene()
    r, _ = _runs()
    f = r["first"]
    origin, cell = tuple(d["origin"].tolist()), tuple(d["cell"].tolist())
    w_hit, w_miss = (int(v) for v in d["weights"])
    w_gain, g_cap, min_gain = int(d["w_gain"]), int(d["g_cap"]), int(d["min_gain"])
    ri, mu = int(d["r_inflate"]), int(d["min_unknown"])
    near = FR.plan_batch(f["evidence"], w_miss, w_hit, origin, cell, f["pos"], ri, mu, None, 64)
    reg = RO.regions_batch(near["frontier"], max(min_gain, 1), 1024)
    want = G.plan_batch(f["evidence"], w_miss, w_hit, origin, cell, f["pos"], 1, w_gain, g_cap, min_gain, ri, mu, None, 64, gain=reg["size"],
                        nearest=dict(near, frontier=reg["rep"]))
    want = dict(want, frontier=near["frontier"], label=reg["label"], rep=reg["rep"], n_regions=reg["n_regions"])
    assert reg["n_regions"][0, 1] >= 1 and (want["status"] == G.FOUND).any()
    for k in PLAN_KEYS:
        assert np.array_equal(f[k], want[k]), k
    assert np.array_equal(f["ufield"].view(np.uint32), want["ufield"]) and np.array_equal(f["field"].view(np.uint32), near["field"])
    assert np.array_equal(f["table"][0, :len(reg["table"][0])], reg["table"][0])
    assert np.array_equal(f["path_cost"].view(np.int64), want["path_cost"].view(np.int64))
    for b, sub in enumerate(want["sub_goals"]):
        assert np.array_equal(f["sub_goals"][b, :len(sub)].view(np.int64), np.ascontiguousarray(sub).view(np.int64)), b
    found = np.isin(f["status"], (G.FOUND, G.PATH_OVERFLOW))
    assert set(f["target_cell"][found].tolist()) <= set(reg["table"][0][:, 3].tolist())
    assert np.array_equal(r["n_regions"][0], reg["n_regions"])                   # the first row of the run's record


def test_gpu_n_regions_per_replan_and_none_kept_when_the_run_stops():
    d, _ = _scene()
    r, _ = _runs()
    K, every = int(d[f"{SCENE}/k_max"]), int(d["replan_every"])
    n = r["n_regions"]
    assert r["n_replans"] == (K + every - 1) // every and n.shape == (r["n_replans"], 1, 3) and n.dtype == np.int32
    assert (n[:, 0, 0] >= n[:, 0, 1]).all() and (n[:, 0, 1] >= 0).all() and (n[:, 0, 2] == np.maximum(n[:, 0, 1] - 1024, 0)).all()
    assert (n[:, 0, 0] <= r["n_frontier"][:, 0]).all() and ((n[:, 0, 0] > 0) == (r["n_frontier"][:, 0] > 0)).all()
    closing = r["closing"]
    print("kept regions per replan", n[:, 0, 1].tolist(), "closing", closing["n_regions"].tolist(), "done", r["done"].tolist(),
          "last status", r["last_status"].tolist(), "(recorded, not asserted: no test asserts sooner)")
    # every representative is a frontier cell, hence passable, and its gain is its region's size >= min_size: a tabled region is a source
    assert closing["n_sources"][0] == min(closing["n_regions"][0, 1], 1024)
    # this recorded seed's run stops for every robot within k_max, and no kept region is left no later than that: the kept count
    # reaches 0 at some replan, stays 0 from there on, and is 0 at the closing plan
    assert r["done"].all() and closing["n_regions"][0, 1] == 0
    zero = np.flatnonzero(n[:, 0, 1] == 0)
    assert len(zero) and (n[zero[0]:, 0, 1] == 0).all()
    assert "n_claims" not in r                                 # (not a coordinated explorer: nothing else is new)
