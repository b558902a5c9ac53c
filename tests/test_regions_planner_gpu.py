"""GPU: the planners with gain_from="region" / target="representative" on the scanned U-wall map (92 x 80) of tests/gain_checks.py:
the gain is the size of a direct regions call, and every plan output is what tests/gain_oracle.py, tests/assign_utility_oracle.py
and tests/assign_keep_utility_oracle.py say when fed tests/regions_oracle.py's size (and rep, for representatives), bit for bit --
the one-workgroup classes and their tiled twins alike."""
import functools

import numpy as np
import pytest

import assign_keep_utility_oracle as AKU
import assign_utility_checks as AK
import assign_utility_oracle as AU
import frontier_oracle as FR
import gain_checks as K
import gain_oracle as G
import regions_oracle as RO

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import lipmpc  # noqa: E402

STARTS = AK.UWALL_STARTS
R_CLAIM, S_MAX = AK.UWALL_R_CLAIM, 64
SETS = ((16, 40, 0), (16, 40, 3), (64, 12, 6))               # (w_gain, g_cap, min_gain): sizes below, around and above the cap
KEEP = dict(r_keep=4, keep_ratio16=24, keep_slack=4)
TARGETS = ("cell", "representative")
PLAN_KEYS = ("gain", "n_sources", "status", "n_sub", "target_cell", "target_gain", "n_frontier")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


@functools.lru_cache(maxsize=None)
def _nearest(per_robot=False):
    shared, per = K.scanned_maps()
    starts = np.array(K.SCAN_AT) if per_robot else STARTS
    return FR.plan_batch(per if per_robot else shared, K.T_FREE, K.T_OCC, K.MAP_ORIGIN, K.MAP_CELL, starts, 2, 2, None, S_MAX)


@functools.lru_cache(maxsize=None)
def _regions(min_gain, per_robot=False):
    return RO.regions_batch(_nearest(per_robot)["frontier"], max(min_gain, 1), 1024)


@functools.lru_cache(maxsize=None)
def _informed(w_gain, g_cap, min_gain, target, per_robot=False):
    """tests/gain_oracle.py fed the regions oracle's size as the gain and, for representatives, its rep as the frontier."""
    shared, per = K.scanned_maps()
    near, reg = _nearest(per_robot), _regions(min_gain, per_robot)
    src = reg["rep"] if target == "representative" else near["frontier"]
    starts = np.array(K.SCAN_AT) if per_robot else STARTS
    return G.plan_batch(per if per_robot else shared, K.T_FREE, K.T_OCC, K.MAP_ORIGIN, K.MAP_CELL, starts, 1, w_gain, g_cap, min_gain, 2, 2,
                        None, S_MAX, gain=reg["size"], nearest=dict(near, frontier=src))


def _host(out):
    h = {k: v.cpu().numpy() for k, v in out.items() if k not in ("field", "ufield", "work")}
    for k in ("field", "ufield"):
        h[k] = out[k].view(torch.int32).cpu().numpy().view(np.uint32)
    return h


def _same(got, want, keys, min_gain, per_robot=False):
    near, reg = _nearest(per_robot), _regions(min_gain, per_robot)
    for k in keys:
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])
    assert np.array_equal(got["ufield"], want["ufield"]) and np.array_equal(got["field"], near["field"])
    assert np.array_equal(got["frontier"], near["frontier"])              # the real frontier stays in the dict
    assert np.array_equal(_bits(got["path_cost"]), _bits(want["path_cost"]))
    found = want["target_cell"] >= 0
    assert np.array_equal(_bits(got["target"][found]), _bits(want["target"][found])) and np.isnan(got["target"][~found]).all()
    for b, sub in enumerate(want["sub_goals"]):
        assert np.array_equal(_bits(got["sub_goals"][b, :len(sub)]), _bits(sub)), b
    # the dict gains the regions call's outputs
    for k in ("label", "rep", "n_regions"):
        assert np.array_equal(got[k], reg[k]), k
    for f, rows in enumerate(reg["table"]):
        assert np.array_equal(got["table"][f, :len(rows)], rows) and not got["table"][f, len(rows):].any()


def _make(cls, w_gain, g_cap, min_gain, target, **kw):
    common = dict(r_inflate=2, min_unknown=2, t_free=K.T_FREE, t_occ=K.T_OCC, gain_from="region", target=target)
    if issubclass(cls, lipmpc.InformedFrontierPlanner):
        return cls(None, w_gain, g_cap, min_gain, **common, **kw)
    return cls(R_CLAIM, 64, r_view=None, w_gain=w_gain, g_cap=g_cap, min_gain=min_gain, **common, **kw)


def _plan(pl, per_robot=False, **kw):
    shared, per = K.scanned_maps()
    ev = torch.as_tensor(np.ascontiguousarray(per if per_robot else shared), device="cuda")
    starts = torch.as_tensor(np.array(K.SCAN_AT) if per_robot else STARTS, device="cuda")
    call = pl.replan if "prev_target" in kw else pl.plan
    out = call(ev, starts, origin=K.MAP_ORIGIN, cell=K.MAP_CELL, S_max=S_MAX, **kw)
    torch.cuda.synchronize()
    return _host(out)


@pytest.mark.parametrize("target", TARGETS)
@pytest.mark.parametrize("w_gain,g_cap,min_gain", SETS)
def test_gpu_informed_by_region(w_gain, g_cap, min_gain, target):
    want = _informed(w_gain, g_cap, min_gain, target)
    reg = _regions(min_gain)
    assert reg["n_regions"][0, 1] >= 2 and (want["status"] == G.FOUND).sum() >= 3
    got = _plan(_make(lipmpc.InformedFrontierPlanner, w_gain, g_cap, min_gain, target))
    tiled = _plan(_make(lipmpc.TiledInformedFrontierPlanner, w_gain, g_cap, min_gain, target))
    wave = _plan(_make(lipmpc.InformedFrontierPlanner, w_gain, g_cap, min_gain, target, paths="wave"))
    for g in (got, tiled, wave):
        _same(g, want, PLAN_KEYS, min_gain)
        assert np.array_equal(g["gain"], reg["size"])
    assert tiled["settled"].tolist() == [1] and tiled["usettled"].tolist() == [1]
    assert all(np.array_equal(_bits(got[k]), _bits(tiled[k])) for k in got)          # the twins are identical to each other
    # gain equals size of a direct call on the planner's frontier
    direct = lipmpc.frontier_regions(torch.as_tensor(got["frontier"], device="cuda"), max(min_gain, 1), 1024)
    torch.cuda.synchronize()
    assert np.array_equal(direct["size"].cpu().numpy(), got["gain"]) and np.array_equal(direct["rep"].cpu().numpy(), got["rep"])
    if target == "representative":
        found = np.isin(got["status"], (G.FOUND, G.PATH_OVERFLOW))
        assert set(got["target_cell"][found].tolist()) <= set(reg["table"][0][:, 3].tolist())


@pytest.mark.parametrize("target", TARGETS)
def test_gpu_informed_by_region_on_per_robot_maps(target):
    w_gain, g_cap, min_gain = SETS[1]
    want = _informed(w_gain, g_cap, min_gain, target, True)
    for cls in (lipmpc.InformedFrontierPlanner, lipmpc.TiledInformedFrontierPlanner):
        _same(_plan(_make(cls, w_gain, g_cap, min_gain, target), True), want, PLAN_KEYS, min_gain, True)


@pytest.mark.parametrize("target", TARGETS)
@pytest.mark.parametrize("w_gain,g_cap,min_gain", SETS[:2])
def test_gpu_claims_by_region(w_gain, g_cap, min_gain, target):
    shared, _ = K.scanned_maps()
    informed = _informed(w_gain, g_cap, min_gain, target)
    want = AU.plan_batch(shared, K.T_FREE, K.T_OCC, K.MAP_ORIGIN, K.MAP_CELL, STARTS, R_CLAIM, 1, w_gain, g_cap, min_gain, 64, 2, 2, None,
                         S_MAX, informed=informed)
    assert want["n_claims"] >= 2
    got = _plan(_make(lipmpc.CoordinatedFrontierPlanner, w_gain, g_cap, min_gain, target))
    tiled = _plan(_make(lipmpc.TiledCoordinatedFrontierPlanner, w_gain, g_cap, min_gain, target))
    for g in (got, tiled):
        _same(g, want, PLAN_KEYS + ("claim_round",), min_gain)
        assert g["n_claims"].tolist() == [want["n_claims"]]
    assert tiled["claims_settled"].tolist() == [1]
    assert all(np.array_equal(_bits(got[k]), _bits(tiled[k])) for k in tiled if k in got)
    if target == "representative":
        reg = _regions(min_gain)
        reps = reg["table"][0][:, 3].tolist()
        found = np.isin(got["status"], (G.FOUND, G.PATH_OVERFLOW))
        assert set(got["target_cell"][found].tolist()) <= set(reps)             # every FOUND robot's target is a tabled rep_cell ...
        winners = got["target_cell"][got["claim_round"] >= 0]
        labels = reg["label"][0].reshape(-1)[winners]
        assert len(set(labels.tolist())) == len(winners)                          # ... and two winners never share a region


@pytest.mark.parametrize("target", TARGETS)
def test_gpu_kept_claims_by_region(target):
    w_gain, g_cap, min_gain = SETS[1]
    shared, _ = K.scanned_maps()
    informed = _informed(w_gain, g_cap, min_gain, target)
    first = AKU.plan_batch(shared, K.T_FREE, K.T_OCC, K.MAP_ORIGIN, K.MAP_CELL, STARTS, R_CLAIM, 1, w_gain, g_cap, np.full(len(STARTS), -1, np.int32), KEEP["r_keep"],
                           KEEP["keep_ratio16"], KEEP["keep_slack"], min_gain, 64, 2, 2, None, S_MAX, informed=informed)
    prev = np.where(first["status"] == G.FOUND, first["target_cell"], -1).astype(np.int32)
    again = AKU.plan_batch(shared, K.T_FREE, K.T_OCC, K.MAP_ORIGIN, K.MAP_CELL, STARTS, R_CLAIM, 1, w_gain, g_cap, prev, KEEP["r_keep"],
                           KEEP["keep_ratio16"], KEEP["keep_slack"], min_gain, 64, 2, 2, None, S_MAX, informed=informed)
    assert again["n_kept"] >= 1
    outs = []
    for cls in (lipmpc.GainKeepFrontierPlanner, lipmpc.TiledGainKeepFrontierPlanner):
        pl = _make(cls, w_gain, g_cap, min_gain, target, **KEEP)
        for want, kw in ((first, {}), (again, dict(prev_target=torch.as_tensor(prev, device="cuda")))):
            got = _plan(pl, **kw)
            _same(got, want, PLAN_KEYS + ("claim_round", "kept"), min_gain)
            assert got["n_claims"].tolist() == [want["n_claims"]] and got["n_kept"].tolist() == [want["n_kept"]]
        outs.append(got)
    assert all(np.array_equal(_bits(outs[0][k]), _bits(outs[1][k])) for k in outs[1] if k in outs[0])


def test_gpu_view_and_cell_give_the_defaults_bits():
    shared, _ = K.scanned_maps()
    ev, starts = torch.as_tensor(shared, device="cuda"), torch.as_tensor(STARTS, device="cuda")
    kw = dict(r_inflate=2, min_unknown=2, t_free=K.T_FREE, t_occ=K.T_OCC)
    gain = dict(r_view=10, w_gain=16, g_cap=120, min_gain=2)
    pairs = [(lambda **o: lipmpc.InformedFrontierPlanner(10, 16, 120, 2, **kw, **o), "plan"),
             (lambda **o: lipmpc.TiledInformedFrontierPlanner(10, 16, 120, 2, **kw, **o), "plan"),
             (lambda **o: lipmpc.CoordinatedFrontierPlanner(R_CLAIM, **gain, **kw, **o), "plan"),
             (lambda **o: lipmpc.TiledCoordinatedFrontierPlanner(R_CLAIM, **gain, **kw, **o), "plan"),
             (lambda **o: lipmpc.GainKeepFrontierPlanner(R_CLAIM, **gain, **KEEP, **kw, **o), "plan"),
             (lambda **o: lipmpc.TiledGainKeepFrontierPlanner(R_CLAIM, **gain, **KEEP, **kw, **o), "plan")]
    for make, method in pairs:
        base = getattr(make(), method)(ev, starts, origin=K.MAP_ORIGIN, cell=K.MAP_CELL, S_max=S_MAX)
        for options in (dict(gain_from="view"), dict(target="cell"), dict(gain_from="view", target="cell")):
            got = getattr(make(**options), method)(ev, starts, origin=K.MAP_ORIGIN, cell=K.MAP_CELL, S_max=S_MAX)
            torch.cuda.synchronize()
            assert set(got) == set(base) and not {"label", "rep", "table", "n_regions"} & set(got)
            for k in base:
                a, b = base[k], got[k]
                assert k == "work" or torch.equal(a.view(torch.uint8), b.view(torch.uint8)), k
