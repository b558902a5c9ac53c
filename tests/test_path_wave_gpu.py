"""GPU: the wave-per-robot path calls (include/lipmpc.h, WAVE-PER-ROBOT PATH CALLS) against the one-lane calls and the numpy oracles,
bit for bit -- status, n_sub, the bits of path_cost and of sub_goals[:n_sub], the sentinel behind n_sub, target_cell and target_gain --
on the inputs of tests/path_wave_cases.py (tests/test_path_wave_oracle.py shows on the CPU what each reaches) and on cases of
tests/field_tiled_cases.py, tests/clearance_cases.py, tests/field_shape_cases.py and tests/large_map_cases.py; all three entry points
in all their nullable forms, through the planners' keyword ``paths`` and through the C calls."""
import ctypes as C

import numpy as np
import pytest

import clearance_cases as K
import field_oracle as Fo
import field_shape_cases as S
import field_tiled_cases as T
import frontier_oracle as FR
import gain_oracle as GO
import large_map_cases as LC
import path_wave_cases as P

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import gain_checks as GC  # noqa: E402
import lipmpc  # noqa: E402
from grid_checks import SENTINEL, bits, field_buffers, frontier_buffers, host, same_field, same_frontier, same_paths  # noqa: E402
from helpers import raw_call  # noqa: E402

KINDS = ("field", "frontier")
POISON = -0x01010102
FORMS = ("plain", "tiled", "weighted")          # the nullable forms: cost and settled null; settled given; both given
INFORMED = dict(r_view=8, w_gain=16, g_cap=120, min_gain=1)
TILED_IDS = ("2x2", "spiral", "corner_cuts", "disc16", "no_frontier", "bad_goals", "three_maps", "130_robots")
CLEARANCE_IDS = ("two_door", "random", "snap", "overflow", "all248_seg5", "all248_seg60", "all248_nocap", "per_robot")


def _dims(c, kind):
    F = len(c["goal"]) if kind == "field" else 1 if c["ev"].ndim == 2 else len(c["ev"])
    return (len(c["start"]), F) + c["occ"].shape[-2:]


def _planner(c, kind, form, paths, **kw):
    kw = dict(kw, paths=paths)
    if form != "plain":
        kw["tiled"] = True
    if form == "weighted" and "clear" in c:
        kw.update(r_clear=c["clear"][0], w_clear=c["clear"][1])
    if kind == "field":
        return lipmpc.GridFieldPlanner(r_inflate=c["r"], max_seg=c["max_seg"], **kw)
    return lipmpc.FrontierPlanner(r_inflate=c["r"], min_unknown=c["mu"], t_free=T.T_FREE, t_occ=T.T_OCC, max_seg=c["max_seg"], **kw)


def _buffers(c, kind, form):
    B, F, W, H = _dims(c, kind)
    out = (field_buffers if kind == "field" else frontier_buffers)(B, F, W, H, P.s_max(c, kind))
    if form != "plain":
        out["settled"] = torch.full((F,), POISON, dtype=torch.int32, device="cuda")
    return out


def _inputs(c, kind, form):
    inp = dict(start=torch.as_tensor(c["start"], device="cuda"))
    if kind == "field":
        inp.update(goal=torch.as_tensor(c["goal"], device="cuda"), grid=lipmpc.GridMap(c["occ"], T.ORIGIN, T.CELL).to("cuda"))
    else:
        inp.update(ev=torch.as_tensor(np.ascontiguousarray(c["ev"]), device="cuda"))
    if form == "weighted" and "cost" in c:
        inp["cost"] = torch.as_tensor(np.ascontiguousarray(c["cost"]), device="cuda")
    return inp


def _plan(pl, kind, inp, out, S_max):
    more = dict(cost=inp["cost"]) if "cost" in inp else {}
    if kind == "field":
        return pl.plan_grid_batch(inp["goal"], inp["grid"], inp["start"], S_max=S_max, out=out, **more)
    return pl.plan(inp["ev"], inp["start"], origin=T.ORIGIN, cell=T.CELL, S_max=S_max, out=out, **more)


def _run(c, kind, form, paths, **kw):
    out, pl = _buffers(c, kind, form), _planner(c, kind, form, paths, **kw)
    got = _plan(pl, kind, _inputs(c, kind, form), out, P.s_max(c, kind))
    torch.cuda.synchronize()
    assert got is out and pl.last is out and pl.paths == paths
    return host(out)


def _same_bits(a, b):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(bits(a[k]), bits(b[k])), k


def _three_way(c, kind, form, want):
    """The oracle, the one-lane call and the wave call: every output, bit for bit, the sentinel behind n_sub."""
    lane, wave = _run(c, kind, form, "lane"), _run(c, kind, form, "wave")
    if form != "plain":
        assert (lane["settled"] == 1).all() and (wave["settled"] == 1).all()
    wave.pop("cost", None), lane.pop("cost", None)
    _same_bits(wave, lane)
    (same_field if kind == "field" else same_frontier)(wave, want, P.s_max(c, kind))
    (same_field if kind == "field" else same_frontier)(lane, want, P.s_max(c, kind))


# -- the cases, three ways -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("id_", P.IDS)
def test_wave_cases_equal_the_lane_calls_and_the_oracle(id_, kind):
    c = P.case(id_)
    for form in FORMS if id_ in P.WEIGHTED_IDS else FORMS[:2]:
        want = P.oracle(id_, kind, form == "weighted")
        if form == "plain":
            print(id_, kind, "status", np.bincount(want["status"], minlength=9).tolist(), "most sub-goals", int(want["n_sub"].max()))
        _three_way(c, kind, form, want)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("id_", TILED_IDS)
def test_tiled_cases_equal_the_lane_calls_and_the_oracle(id_, kind):
    c = T.case(id_)
    for form in FORMS[:2]:
        _three_way(c, kind, form, T.oracle(id_, kind))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("id_", CLEARANCE_IDS)
def test_clearance_cases_equal_the_lane_calls_and_the_oracle(id_, kind):
    _three_way(K.case(id_), kind, "weighted", K.oracle(id_, kind))


def test_an_empty_batch_is_no_call():
    c = dict(P.case("batch5_shared"))
    c["start"] = c["start"][:0]
    for kind in KINDS:
        for form in FORMS:
            out = _plan(_planner(c, kind, form, "wave"), kind, _inputs(c, kind, form), _buffers(c, kind, form), c["S_max"])
            torch.cuda.synchronize()
            assert out["sub_goals"].shape == (0, c["S_max"], 2) and out["status"].shape == (0,)


# -- the utility paths -----------------------------------------------------------------------------------------------------------------
def _informed_case(id_):
    return T.case(id_) if id_ in T.IDS else P.case(id_)


def _informed_oracle(id_, _cache={}):
    if id_ not in _cache:
        c = _informed_case(id_)
        nearest = T.oracle(id_, "frontier") if id_ in T.IDS else P.oracle(id_, "frontier")
        _cache[id_] = GO.plan_batch(c["ev"], T.T_FREE, T.T_OCC, T.ORIGIN, T.CELL, c["start"], INFORMED["r_view"], INFORMED["w_gain"],
                                    INFORMED["g_cap"], INFORMED["min_gain"], c["r"], c["mu"], c["max_seg"], P.s_max(c, "frontier"), nearest=nearest)
    return _cache[id_]


def _informed(c, tiled, paths, **kw):
    cls = lipmpc.TiledInformedFrontierPlanner if tiled else lipmpc.InformedFrontierPlanner
    pl = cls(**INFORMED, r_inflate=c["r"], min_unknown=c["mu"], t_free=T.T_FREE, t_occ=T.T_OCC, max_seg=c["max_seg"], paths=paths, **kw)
    B, F, W, H = _dims(c, "frontier")
    S_max = P.s_max(c, "frontier")
    out = GC.buffers(B, F, W, H, S_max)
    if tiled:
        out.update({k: torch.full((F,), POISON, dtype=torch.int32, device="cuda") for k in ("settled", "usettled")})
    got = pl.plan(torch.as_tensor(np.ascontiguousarray(c["ev"]), device="cuda"), torch.as_tensor(c["start"], device="cuda"), origin=T.ORIGIN,
                  cell=T.CELL, S_max=S_max, out=out)
    torch.cuda.synchronize()
    assert got is out
    h = GC.host({k: v for k, v in out.items() if k not in ("settled", "usettled")})
    h.update({k: out[k].cpu().numpy() for k in ("settled", "usettled") if k in out})
    return h


@pytest.mark.parametrize("id_", ["2x2", "corner_cuts", "disc16", "no_frontier", "three_maps", "130_robots", "snaps", "seg5_one_less",
                                 "batch5_shared", "batch65_per_robot"])
def test_utility_paths_equal_the_lane_calls_and_the_oracle(id_):
    """lipmpc_grid_frontier_utility_path_wave_batch with settled null (the one-workgroup utility field) and given (the tiled one)."""
    c, want = _informed_case(id_), _informed_oracle(id_)
    print(id_, "status", np.bincount(want["status"], minlength=9).tolist(), "sources", want["n_sources"].tolist()[:4])
    for tiled in (False, True):
        lane, wave = _informed(c, tiled, "lane"), _informed(c, tiled, "wave")
        _same_bits(wave, lane)
        GC.same(wave, want, P.s_max(c, "frontier"))
        if tiled:
            assert (wave["settled"] == 1).all() and (wave["usettled"] == 1).all()


# -- an unsettled field ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS + ("informed",))
def test_an_unsettled_field_is_reported_as_the_lane_call_reports_it(kind):
    """rounds=1 on a map of several tiles: RRT_FIELD_UNSETTLED for every robot, before any other rule, and nothing else written --
    whatever the one-lane call leaves, the wave call leaves."""
    c = T.case("baffles")
    B = len(c["start"])
    if kind == "informed":
        lane, wave = _informed(c, True, "lane", rounds=1), _informed(c, True, "wave", rounds=1)
        assert (wave["usettled"] == 0).all() and wave["target_gain"].tolist() == [-1] * B
    else:
        for form in FORMS[1:]:
            cw = dict(c, cost=K.random_layer(c["occ"].shape, 3))
            lane, wave = _run(cw, kind, form, "lane", rounds=1), _run(cw, kind, form, "wave", rounds=1)
            wave.pop("cost", None), lane.pop("cost", None)
            _same_bits(wave, lane)
        assert (wave["settled"] == 0).all()
    _same_bits(wave, lane)
    assert wave["status"].tolist() == [lipmpc.RRT_FIELD_UNSETTLED] * B and wave["n_sub"].tolist() == [0] * B
    assert np.isnan(wave["path_cost"]).all() and (wave["sub_goals"] == SENTINEL).all()
    if kind != "field":
        assert wave["target_cell"].tolist() == [-1] * B


# -- fields the field call did not make ------------------------------------------------------------------------------------------
def _dev(a, dt):
    return torch.as_tensor(np.ascontiguousarray(a).view(np.int32) if a.dtype == np.uint32 else np.ascontiguousarray(a), dtype=dt, device="cuda")


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _placement():
    org, cs = (C.c_double * 2)(*S.ORIGIN), (C.c_double * 2)(*S.CELL)
    return dict(origin=C.cast(org, C.c_void_p), cell=C.cast(cs, C.c_void_p)), (org, cs)


def _prefilled(out):
    for k in ("n_sub", "status", "target_cell"):
        if k in out:
            out[k].fill_(-9)
    out["path_cost"].fill_(SENTINEL)
    return out


def _batch(plans, extra=()):
    want = {k: np.array([p[k] for p in plans], np.int32) for k in ("n_sub", "status") + tuple(extra)}
    want.update(path_cost=np.array([p["path_cost"] for p in plans]), sub_goals=[p["sub_goals"] for p in plans])
    return want


@pytest.mark.parametrize("name", ["stale", "constant", "local_minimum", "raised"])
def test_goal_paths_down_a_field_the_field_call_did_not_make(name):
    """tests/test_field_shapes_gpu.py's four foreign fields -- a stale field after a wall moved, a constant field, a field whose only
    minimum is 10, a field with one raised value -- are ordinary data: the wave call returns, and ends every robot exactly as the
    oracle and the one-lane call do (the descent takes strictly falling words only: every walk ends within W * H steps)."""
    occ, goal, start = S.field_fleet_case()
    fld, fs = Fo.field(occ, S.ORIGIN, S.CELL, goal[0], 2)
    path = Fo.plan(occ, S.ORIGIN, S.CELL, goal[0], start[3], 2, fld=fld, field_status=fs)["cells"]
    fld = dict(S.foreign_fields(fld, path), stale=fld)[name]
    occ_b = S.moved_wall(occ) if name == "stale" else occ
    B, (W, H), S_max = len(start), occ.shape, 64
    want = _batch([Fo.plan(occ_b, S.ORIGIN, S.CELL, goal[0], s, 2, None, S_max, fld=fld, field_status=fs, strict=False) for s in start])
    place, keep = _placement()
    d = dict(occ=_dev(occ_b, torch.uint8), field=_dev(fld, torch.int32), field_status=_dev(np.array([fs], np.int32), torch.int32),
             goal=_dev(goal, torch.float64), start=_dev(start, torch.float64))
    got = {}
    for call in ("lipmpc_grid_path_batch", "lipmpc_grid_path_wave_batch"):
        out = _prefilled(field_buffers(B, 1, W, H, S_max))
        rc = raw_call(call, device=0, B=B, F=1, W=W, H=H, grid_shared=1, r_inflate=2, max_seg=lipmpc.planner.FIELD_NO_CAP, S_max=S_max,
                      **place, **{k: _ptr(v) for k, v in d.items()}, **{k: _ptr(out[k]) for k in ("sub_goals", "n_sub", "status", "path_cost")},
                      hip_stream=C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert rc == 0
        got[call] = {k: out[k].cpu().numpy() for k in ("sub_goals", "n_sub", "status", "path_cost")}
        same_paths(got[call], want, S_max)
    _same_bits(*got.values())


@pytest.mark.parametrize("name", ["stale", "constant", "local_minimum", "raised"])
def test_frontier_paths_down_a_field_the_field_call_did_not_make(name):
    ev, start = S.frontier_fleet_case()
    fld, _, n_front = FR.field(ev, S.T_FREE, S.T_OCC, 2, S.MU)
    path = FR.plan(ev, S.T_OCC, fld, n_front, S.ORIGIN, S.CELL, start[3], 2)["cells"]
    fld = dict(S.foreign_fields(fld, path), stale=fld)[name]
    ev_b = S.moved_wall(ev) if name == "stale" else ev
    B, (W, H), S_max = len(start), ev.shape, 64
    want = _batch([FR.plan(ev_b, S.T_OCC, fld, n_front, S.ORIGIN, S.CELL, s, 2, None, S_max, strict=False) for s in start], ("target_cell",))
    place, keep = _placement()
    d = dict(evidence=_dev(ev_b, torch.int32), field=_dev(fld, torch.int32), n_frontier=_dev(np.array([n_front], np.int32), torch.int32),
             start=_dev(start, torch.float64))
    names, got = ("sub_goals", "n_sub", "status", "path_cost", "target_cell"), {}
    for call in ("lipmpc_grid_frontier_path_batch", "lipmpc_grid_frontier_path_wave_batch"):
        out = _prefilled(frontier_buffers(B, 1, W, H, S_max))
        rc = raw_call(call, device=0, B=B, F=1, W=W, H=H, t_occ=S.T_OCC, r_inflate=2, max_seg=lipmpc.planner.FIELD_NO_CAP, S_max=S_max,
                      **place, **{k: _ptr(v) for k, v in d.items()}, **{k: _ptr(out[k]) for k in names},
                      hip_stream=C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert rc == 0
        got[call] = {k: out[k].cpu().numpy() for k in names}
        assert np.array_equal(got[call]["target_cell"], want["target_cell"])
        same_paths(got[call], want, S_max)
    _same_bits(*got.values())


# -- above 2^17 cells ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["frontier", "informed"])
@pytest.mark.parametrize("id_", ["first_refused", "long_j"])
def test_large_maps(id_, kind):
    """363 x 362 and (TW + 1) x 4096 cells: field offsets in 64 bits, rows 4096 cells long, against tests/large_map_cases.py's oracle."""
    s, want = LC.shape(id_), LC.plan_oracle(id_, kind)
    kw = dict(r_inflate=LC.R_INFLATE, min_unknown=LC.MIN_UNKNOWN, max_seg=LC.MAX_SEG, t_free=LC.T_FREE, t_occ=LC.T_OCC, paths="wave")
    pl = lipmpc.FrontierPlanner(tiled=True, **kw) if kind == "frontier" else lipmpc.TiledInformedFrontierPlanner(**LC.INFORMED, **kw)
    pos = LC.positions(s)
    B, W, H = len(pos), s["W"], s["H"]
    out = frontier_buffers(B, 1, W, H, LC.S_MAX) if kind == "frontier" else GC.buffers(B, 1, W, H, LC.S_MAX)
    for k in ("settled",) + (("usettled",) if kind == "informed" else ()):
        out[k] = torch.full((1,), POISON, dtype=torch.int32, device="cuda")
    pl.plan(torch.as_tensor(LC.sample_evidence(id_), device="cuda"), torch.as_tensor(pos, device="cuda"), origin=s["origin"], cell=s["cell"],
            S_max=LC.S_MAX, out=out)
    torch.cuda.synchronize()
    settled = {k: out.pop(k).cpu().numpy() for k in ("settled", "usettled") if k in out}
    assert all((v == 1).all() for v in settled.values())
    if kind == "frontier":
        same_frontier(host(out), want, LC.S_MAX)
    else:
        GC.same(GC.host(out), want, LC.S_MAX)


# -- capture, reused buffers ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_graph_replay_equals_the_eager_call(kind):
    c, id_ = T.case("baffles"), "baffles"
    want = T.oracle(id_, kind)
    rounds = T.rounds_to_settle(want["field"][0])             # from the round guarantee, not measured
    eager = _run(c, kind, "tiled", "wave", rounds=rounds)
    pl, inp, out = _planner(c, kind, "tiled", "wave", rounds=rounds), _inputs(c, kind, "tiled"), _buffers(c, kind, "tiled")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _plan(pl, kind, inp, out, c["S_max"])                 # warm-up outside the capture: the workspace grows here
    torch.cuda.current_stream().wait_stream(side)
    works = len(pl._works)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _plan(pl, kind, inp, out, c["S_max"])
    assert len(pl._works) == works
    for k, v in out.items():
        if v.dtype == torch.float64:
            v.fill_(SENTINEL)
        elif k == "field":
            v.view(torch.int32).fill_(12345)
        else:
            v.fill_(77)
    graph.replay()
    torch.cuda.synchronize()
    got = host(out)
    _same_bits(got, eager)
    (same_field if kind == "field" else same_frontier)(got, want, c["S_max"])


def test_a_smaller_batch_on_the_same_buffers_leaves_the_other_rows():
    """A second wave call with B = 5 on the buffers of a call with B = 65: rows 5 .. 64 of every output are untouched (poisoned
    between the calls), rows 0 .. 4 are written as before."""
    c = P.case("batch65_shared")
    pl, inp, out = _planner(c, "field", "plain", "wave"), _inputs(c, "field", "plain"), _buffers(c, "field", "plain")
    _plan(pl, "field", inp, out, c["S_max"])
    torch.cuda.synchronize()
    first = host(out)
    names = ("sub_goals", "n_sub", "status", "path_cost")
    out["sub_goals"].fill_(SENTINEL), out["path_cost"].fill_(SENTINEL), out["n_sub"].fill_(-9), out["status"].fill_(-9)
    B, (W, H) = 5, c["occ"].shape
    lipmpc._lib.call("lipmpc_grid_path_wave_batch", device=0, B=B, F=1, **inp["grid"]._args(1, torch.device("cuda", 0)), cost=None,
                     field=out["field"], field_status=out["field_status"], settled=None, goal=inp["goal"], start=inp["start"], r_inflate=c["r"],
                     max_seg=c["max_seg"], S_max=c["S_max"], **{k: out[k] for k in names}, hip_stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    second = host(out)
    for k in names:
        assert np.array_equal(bits(second[k][:B]), bits(first[k][:B])), k
    assert (second["sub_goals"][B:] == SENTINEL).all() and (second["path_cost"][B:] == SENTINEL).all()
    assert (second["n_sub"][B:] == -9).all() and (second["status"][B:] == -9).all()
    want = P.oracle("batch65_shared", "field")
    for b in range(B):                                       # (and behind n_sub inside the batch: the sentinel)
        assert (second["sub_goals"][b, want["n_sub"][b]:] == SENTINEL).all()


# -- the planner classes -------------------------------------------------------------------------------------------------------------
CLASSES = [("GridFieldPlanner", {}), ("GridFieldPlanner", dict(tiled=True)), ("GridFieldPlanner", dict(tiled=True, r_clear=4, w_clear=40)),
           ("FrontierPlanner", {}), ("FrontierPlanner", dict(tiled=True)), ("FrontierPlanner", dict(tiled=True, r_clear=4, w_clear=40)),
           ("CoordinatedFrontierPlanner", dict(r_claim=6)), ("TiledCoordinatedFrontierPlanner", dict(r_claim=6)), ("InformedFrontierPlanner", INFORMED), ("TiledInformedFrontierPlanner", INFORMED)]


@pytest.mark.parametrize("name,kw", CLASSES, ids=[f"{n}-{'-'.join(k) or 'plain'}" for n, k in CLASSES])
def test_every_accepting_class_gives_the_same_dict_either_way(name, kw):
    c = T.case("one_tile")
    got = {}
    for paths in ("lane", "wave"):
        if name == "GridFieldPlanner":
            pl = lipmpc.GridFieldPlanner(r_inflate=c["r"], max_seg=c["max_seg"], paths=paths, **kw)
            out = pl.plan_grid_batch(torch.as_tensor(c["goal"], device="cuda"), lipmpc.GridMap(c["occ"], T.ORIGIN, T.CELL).to("cuda"),
                                     torch.as_tensor(c["start"], device="cuda"), S_max=c["S_max"])
        else:
            pl = getattr(lipmpc, name)(**kw, r_inflate=c["r"], min_unknown=c["mu"], t_free=T.T_FREE, t_occ=T.T_OCC, max_seg=c["max_seg"], paths=paths)
            out = pl.plan(torch.as_tensor(c["ev"], device="cuda"), torch.as_tensor(c["start"], device="cuda"), origin=T.ORIGIN, cell=T.CELL,
                          S_max=c["S_max"])
        torch.cuda.synchronize()
        assert pl.paths == paths
        got[paths] = {k: (v.view(torch.int32) if v.dtype == torch.uint32 else v).cpu().numpy() for k, v in out.items()
                      if k != "work"}            # (the one-workgroup claim call's scratch field: no output)
    _same_bits(got["wave"], got["lane"])
    assert (got["wave"]["status"] == lipmpc.RRT_FOUND).any()


def test_the_exploring_fleet_runs_the_same_either_way():
    """UnknownEnvFleet.run_exploring on the recorded open-field scene cut to a dozen samples: a FrontierPlanner with paths="wave"
    reproduces the run with paths="lane", every tensor bit for bit."""
    import test_frontier_fleet_gpu as base
    d, occ, _ = base._scene()
    d = dict({k: d[k] for k in d.files}, k_max=np.int64(12))
    seed = d["seeds"].tolist()[0]
    fleet, mapper, _ = base._fleet(d, occ)
    runs = {paths: base._explore(d, fleet, mapper, lipmpc.FrontierPlanner(r_inflate=int(d["r_inflate"]), min_unknown=int(d["min_unknown"]),
                                                                         paths=paths), seed) for paths in ("lane", "wave")}
    want, got = runs["lane"], runs["wave"]
    assert set(got) == set(want)
    for k, v in want.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(bits(v), bits(got[k])), k
        else:
            assert v == got[k], k
    assert want["n_replans"] >= 2 and want["n_frontier"][0, 0] > 0
