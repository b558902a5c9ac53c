"""GPU: the exploring loop's kernels above the 2^17 cells the one-workgroup planners stop at, on the shapes of
tests/large_map_cases.py (363 x 362, (TW + 1) x 4096, 4096 x (TW + 1); tests/test_large_map_oracle.py shows on the CPU what each
reaches): a. the grid scan, b. the map update, c. one sample kernel by kernel -- scan, update, plan with the three tiled explorers
-- and d. UnknownEnvFleet.run_exploring on a map that only the tiled classes accept.

Every device buffer starts poisoned; everything is compared with the numpy oracles bit for bit or integer for integer (the one
tolerance is the 1e-12 on c / eta inside tests/lidar_grid_checks.py's check_chain)."""
import functools

import numpy as np
import pytest

import assign_checks as AC
import frontier_oracle as FR
import gain_checks as GC
import grid_lidar_oracle as G
import large_map_cases as LC
import lidar_oracle as L
from grid_checks import SENTINEL, bits, same_frontier
from lidar_grid_checks import check_chain, check_hits

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import lipmpc  # noqa: E402

N_OBS_MAX, V_MAX = 24, 64
POISON = -0x01010102                                          # int32 of the bytes FE FE FE FE: not a status, a count or a flag
POISON_WORD = 0x5EEDBEEF
UNSETTLED = lipmpc.RRT_FIELD_UNSETTLED
SOLVED = (0, 4)                                               # STATUS_SOLVED, STATUS_UNCERTIFIED
KINDS = ("frontier", "informed", "claims")
E_UNSUPPORTED = -2


def _states(pos):
    st = np.zeros((len(pos), 5)); st[:, 0] = pos[:, 0]; st[:, 2] = pos[:, 1]
    return torch.as_tensor(st, device="cuda")


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _sensor(s, occ=None):
    return lipmpc.LidarSensor.from_grid(lipmpc.GridMap(s["occ"] if occ is None else occ, s["origin"], s["cell"]), lidar_range=LC.RANGE,
                                        resolution=LC.RESOLUTION, n_obs_max=N_OBS_MAX, v_max=V_MAX)


def _scan(s, occ=None, noise=None):
    """One scan of every station into poisoned buffers: the outputs as numpy."""
    sensor = _sensor(s, occ)
    out = sensor.alloc_outputs(len(LC.STATIONS), with_debug=True, c_eta=True)
    for k in ("hits", "labels", "n_inferred", "overflow", "c_eta"):      # (written whole by every scan; ring slots beyond obs_nv are not)
        out[k].fill_(-7.5 if out[k].dtype == torch.float64 else -5)
    got = sensor.sense(_states(LC.positions(s)), None if noise is None else _dev(noise), with_debug=True, c_eta=True, out=out)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in got.items()}


def _mapper(s, per_robot=None):
    return lipmpc.OccupancyMapper(s["W"], s["H"], s["origin"], s["cell"], LC.RANGE, LC.RESOLUTION, per_robot=per_robot, w_hit=LC.W_HIT,
                                  w_miss=LC.W_MISS)


# -- a. the grid scan ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noisy", [False, True])
@pytest.mark.parametrize("per_robot", [False, True])
@pytest.mark.parametrize("id_", LC.IDS)
def test_grid_scan(id_, per_robot, noisy):
    """Hits bit for bit (check_hits, the solid-cell rule included), labels / rings / (c, eta) by check_chain, on a shared map and
    on one map per robot; the station outside the grid reads the grid, the far one reads nothing."""
    s = LC.shape(id_)
    occ = LC.per_robot_occ(s) if per_robot else None
    noise = LC.noise(s) if noisy else None
    g = _scan(s, occ, noise)
    oracle = LC.scan_oracle(id_, per_robot)
    pos = LC.positions(s)
    n_hits, n_solid = check_hits(g, pos, (lambda b: occ[b]) if per_robot else (lambda b: s["occ"]), s["origin"], s["cell"], LC.RANGE,
                                 L.ray_table(LC.RESOLUTION), noise, scan_of=lambda b: oracle[b])
    n_rings = check_chain(g, pos)
    print(f"{id_} per_robot={per_robot} noisy={noisy}: {n_hits} hits, {n_solid} in a solid cell, {n_rings} rings")
    assert n_hits == sum(int(v.sum()) for _, v in oracle) and n_solid >= (0 if per_robot else 1)
    b = LC.index("solid")
    if G.in_solid_cell(pos[b], occ[b] if per_robot else s["occ"], s["origin"], s["cell"]):
        assert g["overflow"][b] == 1 and np.isnan(g["hits"][b]).all() and (g["labels"][b] == -2).all()
    b = LC.index("far")
    assert np.isnan(g["hits"][b]).all() and g["overflow"][b] == 0 and g["n_inferred"][b] == 0 and not g["c_eta"][b].any()
    assert (g["labels"][b] == -2).all()
    b = LC.index("outside")
    assert (~np.isnan(g["hits"][b, :, 0])).sum() == oracle[b][1].sum() > 0 and g["overflow"][b] == 0


# -- b. the map update --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _device_hits(id_):
    """hits [B,R,2] (numpy) of the device's own scan of the shared map with the given noise (held to the oracle by test_grid_scan)."""
    s = LC.shape(id_)
    return _scan(s, None, LC.noise(s))["hits"]


@pytest.mark.parametrize("source", ["device", "hand_made"])
@pytest.mark.parametrize("id_", LC.IDS)
def test_map_update(id_, source):
    """A shared mapper (atomics on one map) and per_robot = B, from a random evidence pattern: one update that skips two stations,
    then one of all -- after each the WHOLE array equals tests/map_oracle.py's on the same readings."""
    s = LC.shape(id_)
    B, W, H = len(LC.STATIONS), s["W"], s["H"]
    pos = LC.positions(s)
    hits = _device_hits(id_) if source == "device" else LC.hand_made_hits(s)
    assert np.isnan(hits).all(2).any()
    ev0 = LC.random_evidence(s, 11)
    st, d_hits = _states(pos), _dev(hits)
    sh, per = _mapper(s), _mapper(s, B)
    sh.evidence.copy_(_dev(ev0))
    per.evidence.copy_(_dev(ev0).expand(B, W, H))
    want_sh, want_per = ev0.astype(np.int64), np.repeat(ev0[None].astype(np.int64), B, 0)
    for mask in (LC.mask(), None):
        d_mask = None if mask is None else _dev(mask)
        e_sh, e_per = sh.update(st, d_hits, d_mask), per.update(st, d_hits, d_mask)
        torch.cuda.synchronize()
        LC.update(s, want_sh, pos, hits, mask)
        LC.update(s, want_per, pos, hits, mask)
        got_sh, got_per = e_sh.cpu().numpy(), e_per.cpu().numpy()
        assert got_sh.shape == (W, H) and got_per.shape == (B, W, H) and got_sh.dtype == np.int32
        bad = np.argwhere(got_sh != want_sh)
        assert len(bad) == 0, ("shared", mask is None, len(bad), bad[:5].tolist())
        bad = np.argwhere(got_per != want_per)
        assert len(bad) == 0, ("per robot", mask is None, len(bad), bad[:5].tolist())
    delta = want_per - ev0[None]
    touched = np.nonzero((want_sh != ev0).ravel())[0]
    print(f"{id_} {source}: {len(touched)} cells changed, largest flat index {int(touched.max())}, per robot {delta.any((1, 2)).tolist()}")
    assert touched.max() > LC.OLD_CAP and touched.min() < H and not delta[LC.index("far")].any()
    assert delta[LC.index("outside")].any() and (delta[LC.index("far_corner")][W - 1].any() or delta[LC.index("far_corner")][:, H - 1].any())


# -- c. one sample, kernel by kernel ------------------------------------------------------------------------------------------
def _planner(kind, rounds=None, **over):
    kw = dict(dict(r_inflate=LC.R_INFLATE, min_unknown=LC.MIN_UNKNOWN, max_seg=LC.MAX_SEG, rounds=rounds), **over)
    if kind == "frontier":
        return lipmpc.FrontierPlanner(tiled=True, **kw)
    if kind == "informed":
        return lipmpc.TiledInformedFrontierPlanner(**LC.INFORMED, **kw)
    return lipmpc.TiledCoordinatedFrontierPlanner(**LC.CLAIMS, **kw)


def _parent(kind):
    kw = dict(r_inflate=LC.R_INFLATE, min_unknown=LC.MIN_UNKNOWN, max_seg=LC.MAX_SEG)
    if kind == "frontier":
        return lipmpc.FrontierPlanner(**kw)
    if kind == "informed":
        return lipmpc.InformedFrontierPlanner(**LC.INFORMED, **kw)
    return lipmpc.CoordinatedFrontierPlanner(**LC.CLAIMS, **kw)


SETTLED_KEYS = {"frontier": ("settled",), "informed": ("settled", "usettled"), "claims": ("settled", "claims_settled")}


def _poison(out):
    for k, v in out.items():
        if k in ("settled", "usettled", "claims_settled"):
            v.fill_(POISON)
        elif v.dtype == torch.float64:
            v.fill_(SENTINEL)
        elif v.dtype == torch.uint32:
            v.view(torch.int32).fill_(POISON_WORD)
        elif v.dtype == torch.uint8:
            v.fill_(9)
        else:
            v.fill_(77)
    return out


def _buffers(kind, B, F, W, H):
    P = lipmpc.planner
    table = {"frontier": lambda: P.frontier_outputs(B, F, W, H, LC.S_MAX), "informed": lambda: P.informed_outputs(B, F, W, H, LC.S_MAX),
             "claims": lambda: P.tiled_assign_outputs(B, W, H, LC.S_MAX)}[kind]()
    out = {k: torch.empty(shape, dtype=dt, device="cuda") for k, (dt, shape, _) in table.items()}
    for k in SETTLED_KEYS[kind]:
        out[k] = torch.empty((F,), dtype=torch.int32, device="cuda")
    return _poison(out)


def _host(out):
    h = {k: v.cpu().numpy() for k, v in out.items() if v.dtype != torch.uint32}
    for k, v in out.items():
        if v.dtype == torch.uint32:
            h[k] = v.view(torch.int32).cpu().numpy().view(np.uint32)
    return h


def _same(kind, got, want):
    for k in SETTLED_KEYS[kind]:
        assert (got[k] == 1).all(), (k, got[k])
    if kind == "frontier":
        same_frontier(got, want, LC.S_MAX)
    elif kind == "informed":
        GC.same(got, want, LC.S_MAX)
    else:
        AC.same(got, want, LC.S_MAX)


def _same_in_a_run(kind, got, want):
    """``_same`` for the plan buffers of a run: run_exploring lets its first plan make them (zeros, no sentinel) and every later
    plan reuses them, so the sub-goal rows that a plan does not write -- those behind n_sub, and behind the nearest-frontier plan's
    n_sub for a robot that claimed -- hold an earlier replan's.  They are set to the sentinel here; every written row and every
    other output is compared as everywhere."""
    keep = np.maximum(want["n_sub"], want["nearest"]["n_sub"]) if kind == "claims" else want["n_sub"]
    got = dict(got, sub_goals=got["sub_goals"].copy())
    for b, n in enumerate(keep):
        got["sub_goals"][b, n:] = SENTINEL
    _same(kind, got, want)


def _same_bits(a, b):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(bits(a[k]), bits(b[k])), k


def _plan(kind, mapper, pos, rounds=None, **over):
    """One plan on the mapper into poisoned buffers."""
    ev = mapper.evidence
    F, (W, H) = (1 if ev.dim() == 2 else ev.shape[0]), ev.shape[-2:]
    pl, out = _planner(kind, rounds, **over), _buffers(kind, len(pos), F, W, H)
    got = pl.plan(mapper, _dev(pos), S_max=LC.S_MAX, out=out)
    torch.cuda.synchronize()
    assert got is out and pl.last is out
    return _host(out)


def _unsettled(kind, got, B):
    """rounds = 1: no field settled, every robot RRT_FIELD_UNSETTLED and nothing else written."""
    for k in SETTLED_KEYS[kind]:
        assert (got[k] == 0).all(), (k, got[k])
    assert got["status"].tolist() == [UNSETTLED] * B and got["n_sub"].tolist() == [0] * B
    assert np.isnan(got["path_cost"]).all() and (got["sub_goals"] == SENTINEL).all()
    assert got["target_cell"].tolist() == [-1] * B and np.isnan(got["target"]).all()
    if kind == "informed":
        assert got["target_gain"].tolist() == [-1] * B
    if kind == "claims":
        assert got["n_claims"].tolist() == [0] and (got["claim_round"] == -1).all()


@functools.lru_cache(maxsize=None)
def _sampled_mapper(id_):
    """A shared mapper that holds the preset and one device scan + device update of every station: held to the oracle's evidence
    by every test that uses it."""
    s = LC.shape(id_)
    mapper = _mapper(s)
    mapper.evidence.copy_(_dev(LC.preset(s)))
    sensor = _sensor(s)
    st = _states(LC.positions(s))
    hits = sensor.sense(st, None, with_debug=True, c_eta=True)["hits"]
    mapper.update(st, hits)
    torch.cuda.synchronize()
    return mapper


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("id_", LC.IDS)
def test_one_sample_scan_update_plan(id_, kind):
    s = LC.shape(id_)
    mapper, pos = _sampled_mapper(id_), LC.positions(s)
    B = len(pos)
    ev = mapper.evidence.cpu().numpy()
    bad = np.argwhere(ev != LC.sample_evidence(id_))
    assert len(bad) == 0, (len(bad), bad[:5].tolist())          # the evidence first: the plan below is on the oracle's map
    want = LC.plan_oracle(id_, kind)
    got = _plan(kind, mapper, pos)                             # rounds=None: resumed until settled
    _same(kind, got, want)
    budget = LC.budgets(id_, kind)                             # a fixed budget from the round guarantee: settles, the same bits
    fixed = _plan(kind, mapper, pos, rounds=budget)
    _same(kind, fixed, want)
    _same_bits(got, fixed)
    _unsettled(kind, _plan(kind, mapper, pos, rounds=1), B)
    assert np.array_equal(mapper.evidence.cpu().numpy(), ev)    # no plan writes the map
    with pytest.raises(RuntimeError) as e:                      # and the one-workgroup parent refuses it
        _parent(kind).plan(mapper, _dev(pos), S_max=LC.S_MAX)
    assert e.value.code == E_UNSUPPORTED
    print(f"{id_} {kind}: budget {budget} rounds, statuses {got['status'].tolist()}, n_sub {got['n_sub'].tolist()}")


@pytest.mark.parametrize("kind", ["frontier", "informed"])
def test_one_sample_on_per_robot_maps_of_363_x_362(kind):
    """F = B: one evidence map per station -- the preset and the station's own scan -- through the two classes that take it."""
    id_ = "first_refused"
    s = LC.shape(id_)
    pos = LC.positions(s)
    B = len(pos)
    mapper = _mapper(s, B)
    mapper.evidence.copy_(_dev(LC.preset(s)).expand(B, s["W"], s["H"]))
    st = _states(pos)
    mapper.update(st, _sensor(s).sense(st, None, with_debug=True, c_eta=True)["hits"])
    torch.cuda.synchronize()
    bad = np.argwhere(mapper.evidence.cpu().numpy() != LC.per_robot_sample_evidence(id_))
    assert len(bad) == 0, (len(bad), bad[:5].tolist())
    want = LC.per_robot_plan_oracle(kind)
    got = _plan(kind, mapper, pos)
    _same(kind, got, want)
    _unsettled(kind, _plan(kind, mapper, pos, rounds=1), B)
    with pytest.raises(ValueError, match="ONE shared map"):
        _planner("claims").plan(mapper, _dev(pos), S_max=LC.S_MAX)


@pytest.mark.parametrize("kind", ["frontier", "claims"])
def test_a_corner_cell_s_fall_wakes_the_diagonal_tile(kind):
    """tests/large_map_cases.py's corner_wake, 3 x 2 tiles: the last cell of tile (0, 0) gets its value through the diagonal from the
    first cell of tile (1, 1), a round after every rim cell of the two side tiles is final -- only the corner flag of a round tells
    tile (0, 0) to relax again."""
    c, near = LC.corner_wake(), LC.corner_wake_oracle()
    W, H = c["ev"].shape
    mapper = lipmpc.OccupancyMapper(W, H, c["origin"], c["cell"], LC.RANGE, LC.RESOLUTION, w_hit=LC.W_HIT, w_miss=LC.W_MISS)
    mapper.evidence.copy_(_dev(c["ev"]))
    over = dict(r_inflate=c["r"], min_unknown=c["mu"], max_seg=None)
    want = near if kind == "frontier" else AC.expected(c["ev"], c["start"], LC.CLAIMS["r_claim"], LC.CLAIMS["max_claims"], c["r"], c["mu"],
                                                       None, LC.S_MAX, origin=c["origin"], cell=c["cell"])
    got = _plan(kind, mapper, c["start"], **over)
    _same(kind, got, want)
    D = c["cells"]["D"]
    assert got["field"][0][D] == near["field"][0][c["cells"]["C"]] + 7
    budget = LC.T.rounds_to_settle(near["field"][0]) if kind == "frontier" else max(LC.T.rounds_to_settle(f) for f in [near["field"][0]] + LC.claim_fields(want))
    _same(kind, _plan(kind, mapper, c["start"], rounds=budget, **over), want)


# -- d. the run ---------------------------------------------------------------------------------------------------------------
K_MAX, REPLAN_EVERY, LOOKAHEAD, CUT = 12, 3, 0.3, 6


def _fleet(per_robot=None):
    s = LC.shape("first_refused")
    mapper = _mapper(s, per_robot)
    fleet = lipmpc.UnknownEnvFleet(grid=lipmpc.GridMap(s["occ"], s["origin"], s["cell"]), N_horizon=3, lidar_range=LC.RANGE, mapper=mapper)
    return s, fleet, mapper


def _explore(s, fleet, mapper, explorer, k_max=K_MAX, **kw):
    """One exploring run of the four runners from the preset evidence with the given noise: every result on the host."""
    pre = _dev(LC.preset(s))
    mapper.evidence.copy_(pre if mapper.evidence.dim() == 2 else pre.expand_as(mapper.evidence))
    start = LC.positions(s, LC.RUNNERS)
    noise = _dev(LC.noise(s, K_MAX, LC.RUNNERS)[:k_max])
    r = fleet.run_exploring(_states(start), torch.ones((len(start),), dtype=torch.int8, device="cuda"), k_max, explorer, REPLAN_EVERY, LOOKAHEAD,
                            noise=noise, S_max=LC.S_MAX, **kw)
    torch.cuda.synchronize()
    out = {k: (v.cpu().numpy().copy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}
    out["evidence"] = mapper.evidence.cpu().numpy().copy()
    out["last"] = {k: v.copy() for k, v in _host(explorer.last).items()}
    return out


@functools.lru_cache(maxsize=None)
def _runs(kind):
    """The long run of a tiled explorer, the same run again, the run without a graph, and the run cut at CUT samples."""
    s, fleet, mapper = _fleet()
    explorer = _planner(kind)
    long_ = _explore(s, fleet, mapper, explorer)
    again = _explore(s, fleet, mapper, explorer)
    eager = _explore(s, fleet, mapper, explorer, use_graph=False)
    cut = _explore(s, fleet, mapper, explorer, k_max=CUT)
    return s, long_, again, eager, cut


def _final_plan(s, kind, r):
    """The oracle's plan on a run's final evidence and positions (the coordinated one with the run's claimants)."""
    pos = r["X_pred"][:, -1][:, (0, 2)]
    if kind == "frontier":
        return LC.frontier_plan(s, r["evidence"], pos)
    if kind == "informed":
        return LC.informed_plan(s, r["evidence"], pos)
    return LC.claim_plan(s, r["evidence"], pos, may_claim=np.isin(r["last_status"], SOLVED))


def _bookkeeping(s, r, want, k_max=K_MAX, shared=True):
    assert r["n_replans"] == (k_max + REPLAN_EVERY - 1) // REPLAN_EVERY
    assert r["n_frontier"].shape == (r["n_replans"], len(want["n_frontier"])) and r["known_free"].shape == r["n_frontier"].shape
    assert np.array_equal(r["explore_status"], want["status"]), (r["explore_status"], want["status"])
    failed = ~np.isin(r["last_status"], SOLVED)
    assert np.array_equal(r["done"], (want["status"] == FR.NO_PATH) & ~failed)
    assert not r["walking"][r["done"]].any() and not r["walking"][want["status"] != FR.FOUND].any()
    assert (r["n_frontier"][:, :] > 0).all()
    # known_free does not fall on the shared map.  On a robot's OWN map it may, by the update rule: a robot that stands beside a
    # block adds nothing new, and a noisy reading pushed past the block's corner gives a free cell + w_hit, which makes it unknown
    # again (tests/test_large_map_oracle.py shows such cells on the oracle) -- there the fleet's total must not fall
    rows = r["known_free"] if shared else r["known_free"].sum(1, keepdims=True)
    assert (np.diff(rows, axis=0) >= 0).all() and rows[-1].sum() > rows[0].sum(), r["known_free"].tolist()
    ev = r["evidence"] if r["evidence"].ndim == 3 else r["evidence"][None]
    assert (r["known_free"][-1] <= (ev <= -LC.T_FREE).sum((1, 2))).all()


def _within_the_windows(s, r):
    """Every cell whose evidence differs from the preset lies within the update's window of some position of the run."""
    nx, ny = LC.map_half(s)
    allowed = np.zeros((s["W"], s["H"]), bool)
    for p in r["X_pred"][:, :, (0, 2)].reshape(-1, 2):
        c = G.robot_cell(p, s["origin"], s["cell"])
        allowed[max(c[0] - nx, 0):max(c[0] + nx + 1, 0), max(c[1] - ny, 0):max(c[1] + ny + 1, 0)] = True
    ev = r["evidence"] if r["evidence"].ndim == 3 else r["evidence"][None]
    changed = (ev != LC.preset(s)[None]).any(0)
    assert changed.any() and not (changed & ~allowed).any(), np.argwhere(changed & ~allowed)[:5].tolist()
    return int(changed.sum())


@pytest.mark.parametrize("kind", KINDS)
def test_the_one_workgroup_explorers_refuse_the_run(kind):
    s, fleet, mapper = _fleet()
    with pytest.raises(RuntimeError) as e:
        _explore(s, fleet, mapper, _parent(kind))
    assert e.value.code == E_UNSUPPORTED


@pytest.mark.parametrize("kind", KINDS)
def test_exploring_run_on_363_x_362(kind):
    s, r, again, eager, cut = _runs(kind)
    want = _final_plan(s, kind, r)
    _same_in_a_run(kind, r["last"], want)                      # the closing plan: every output, not just the status
    _bookkeeping(s, r, want)
    assert r["n_replans"] == 4 and (r["n_steps"] > 0).any()
    if kind == "claims":
        assert (r["n_claims"] >= 1).all() and r["last"]["claims_settled"].tolist() == [1]
    n_changed = _within_the_windows(s, r)
    print(f"{kind}: steps {r['n_steps'].tolist()}, last status {r['last_status'].tolist()}, explore status {r['explore_status'].tolist()}, "
          f"n_frontier {r['n_frontier'][:, 0].tolist()}, known_free {r['known_free'][:, 0].tolist()}, {n_changed} cells changed"
          + (f", n_claims {r['n_claims'].tolist()}" if kind == "claims" else ""))


@pytest.mark.parametrize("kind", KINDS)
def test_exploring_runs_are_deterministic(kind):
    s, r, again, eager, cut = _runs(kind)
    for other in (again, eager):
        assert set(other) == set(r)
        for k, v in r.items():
            if k == "last":
                _same_bits(v, other[k])
            elif isinstance(v, np.ndarray):
                assert np.array_equal(bits(v), bits(other[k])), k
            else:
                assert v == other[k], k


@pytest.mark.parametrize("kind", KINDS)
def test_a_run_cut_at_the_third_replan_is_the_long_run_s_row_2(kind):
    s, r, again, eager, cut = _runs(kind)
    want = _final_plan(s, kind, cut)
    _same_in_a_run(kind, cut["last"], want)
    _bookkeeping(s, cut, want, CUT)
    row = CUT // REPLAN_EVERY
    assert cut["n_replans"] == row and np.array_equal(cut["X_pred"], r["X_pred"][:, :CUT + 1])
    assert want["n_frontier"].tolist() == r["n_frontier"][row].tolist() == cut["last"]["n_frontier"].tolist()
    assert [int((cut["evidence"] <= -LC.T_FREE).sum())] == r["known_free"][row].tolist()
    assert np.array_equal(cut["n_frontier"], r["n_frontier"][:row]) and np.array_equal(cut["known_free"], r["known_free"][:row])


def test_exploring_run_with_one_map_per_robot():
    """The tiled FrontierPlanner on a per_robot mapper: F = B maps of 131k cells through run_exploring."""
    s, fleet, mapper = _fleet(per_robot=len(LC.RUNNERS))
    explorer = _planner("frontier")
    r = _explore(s, fleet, mapper, explorer)
    pos = r["X_pred"][:, -1][:, (0, 2)]
    want = LC.frontier_plan(s, r["evidence"], pos)
    _same_in_a_run("frontier", r["last"], want)
    _bookkeeping(s, r, want, shared=False)
    assert r["n_replans"] == 4 and (r["n_steps"] > 0).any() and r["n_frontier"].shape == (4, len(LC.RUNNERS))
    assert len({e.tobytes() for e in r["evidence"]}) == len(LC.RUNNERS)
    _within_the_windows(s, r)
