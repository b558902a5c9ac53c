"""The informed explorer: C ABI, Python signatures and compiled resources (no GPU needed)."""
import ctypes as C
import inspect

import pytest

import lipmpc
from code_object import kernel_resources
from helpers import raw_call

E_ARG, E_UNSUPPORTED = -1, -2
GAIN, UFIELD, UPATH = "lipmpc_grid_frontier_gain_batch", "lipmpc_grid_frontier_utility_field_batch", "lipmpc_grid_frontier_utility_path_batch"
ARGS = {
    GAIN: ["device", "F", "W", "H", "evidence", "t_free", "t_occ", "frontier", "r_view", "gain", "hip_stream"],
    UFIELD: ["device", "F", "W", "H", "frontier", "field", "gain", "w_gain", "g_cap", "min_gain", "ufield", "n_sources", "hip_stream"],
    UPATH: ["device", "B", "F", "W", "H", "origin", "cell", "evidence", "t_occ", "frontier", "gain", "ufield", "n_sources", "w_gain", "g_cap",
            "min_gain", "start", "r_inflate", "max_seg", "S_max", "sub_goals", "n_sub", "status", "path_cost", "target_cell", "target_gain",
            "hip_stream"],
}
POINTERS = {
    GAIN: ("evidence", "frontier", "gain"),
    UFIELD: ("frontier", "field", "gain", "ufield", "n_sources"),
    UPATH: ("evidence", "frontier", "gain", "ufield", "n_sources", "start", "sub_goals", "n_sub", "status", "path_cost", "target_cell",
            "target_gain"),
}
ONE = C.c_void_p(8)                                           # device pointers: never dereferenced


def test_gain_symbols_are_exported_and_bound():
    lib = lipmpc._lib.load()
    for name, args in ARGS.items():
        assert name in lipmpc._lib.EXPORTS and name in lipmpc._lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == [t for _, t in lipmpc._lib.SIGNATURES[name][1]]
        assert [n for n, _ in lipmpc._lib.SIGNATURES[name][1]] == args
    assert lib.lipmpc_version() == 5                       # a backward-compatible addition
    assert lipmpc.InformedFrontierPlanner is lipmpc.planner.InformedFrontierPlanner
    assert issubclass(lipmpc.InformedFrontierPlanner, lipmpc.FrontierPlanner)


def test_gain_kernels_code_object():
    """From the built library's gfx950 code objects: each new kernel exists once, uses no scratch and spills nothing; its static LDS
    is the workgroup reduction's words, within the slack the LDS rules keep."""
    res = kernel_resources(lipmpc._lib.LIB_PATH)
    for k in ("frontier_gain_kernel", "frontier_utility_lds_kernel", "frontier_utility_global_kernel", "frontier_utility_path_kernel"):
        mine = {name: r for name, r in res.items() if k in name}
        assert len(mine) == 1, (k, sorted(mine))
        (name, r), = mine.items()
        print(k, {f: r.get(f) for f in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")})
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r.get("sgpr_spill_count", 0) == 0, (name, r)
        assert r["group_segment_fixed_size"] <= 256, (name, r)


def _caps(rc):
    """An argument error comes before the caps, the caps before "nothing to do" (the cases of lipmpc_grid_frontier_field_batch)."""
    assert rc(W=1) == E_ARG and rc(H=1) == E_ARG and rc(W=0) == E_ARG and rc(H=-3) == E_ARG and rc(W=2, H=2) == 0
    assert rc(W=4097, H=2) == E_UNSUPPORTED and rc(W=2, H=4097) == E_UNSUPPORTED and rc(W=4096, H=32) == 0
    assert rc(W=363, H=362) == E_UNSUPPORTED and rc(W=512, H=256) == 0 and rc(W=512, H=257) == E_UNSUPPORTED
    assert rc(W=4097, H=2, **{rc.count: 3}) == E_UNSUPPORTED
    assert rc(**{rc.count: -1}) == E_ARG and rc(**{rc.count: 1 << 31}) == E_ARG


def _gain_ranges(rc):
    assert rc(w_gain=-1) == E_ARG and rc(w_gain=65536) == E_ARG and rc(w_gain=0) == 0 and rc(w_gain=65535) == 0
    assert rc(g_cap=0) == E_ARG and rc(g_cap=16385) == E_ARG and rc(g_cap=1) == 0 and rc(g_cap=16384) == 0
    assert rc(min_gain=-1) == E_ARG and rc(min_gain=16385) == E_ARG and rc(min_gain=0) == 0 and rc(min_gain=16384) == 0
    assert rc(W=4097, H=2, w_gain=-1) == E_ARG and rc(W=4097, H=2, g_cap=0) == E_ARG and rc(W=4097, H=2, min_gain=16385) == E_ARG


def test_gain_call_refusals_reach_no_device():
    def rc(drop=(), **kw):
        args = dict(device=0, F=0, W=92, H=80, t_free=1, t_occ=3, r_view=10)
        args.update(kw)
        return raw_call(GAIN, **{n: ONE for n in POINTERS[GAIN] if n not in drop}, **args)
    rc.count = "F"
    assert rc() == 0                                       # the same arguments pass: F = 0 enqueues nothing
    _caps(rc)
    assert rc(r_view=0) == E_ARG and rc(r_view=65) == E_ARG and rc(r_view=-1) == E_ARG and rc(r_view=1) == 0 and rc(r_view=64) == 0
    for t in ("t_free", "t_occ"):
        assert rc(**{t: 0}) == E_ARG and rc(**{t: (1 << 30) + 1}) == E_ARG and rc(**{t: -1}) == E_ARG
        assert rc(**{t: 1}) == 0 and rc(**{t: 1 << 30}) == 0
    for missing in POINTERS[GAIN]:
        assert rc(drop=(missing,)) == E_ARG and rc(F=3, drop=(missing,)) == E_ARG and rc(W=4097, H=2, drop=(missing,)) == E_ARG, missing
    assert rc(W=4097, H=2, r_view=0) == E_ARG and rc(W=4097, H=2, t_occ=0) == E_ARG


def test_utility_field_refusals_reach_no_device():
    def rc(drop=(), **kw):
        args = dict(device=0, F=0, W=92, H=80, w_gain=16, g_cap=174, min_gain=0)
        args.update(kw)
        return raw_call(UFIELD, **{n: ONE for n in POINTERS[UFIELD] if n not in drop}, **args)
    rc.count = "F"
    assert rc() == 0
    _caps(rc)
    _gain_ranges(rc)
    for missing in POINTERS[UFIELD]:
        assert rc(drop=(missing,)) == E_ARG and rc(F=3, drop=(missing,)) == E_ARG and rc(W=4097, H=2, drop=(missing,)) == E_ARG, missing


def test_utility_path_refusals_reach_no_device():
    org, cs = (C.c_double * 2)(0.0, 0.0), (C.c_double * 2)(0.1, 0.1)

    def rc(drop=(), cell=cs, origin=org, **kw):
        args = dict(device=0, B=0, F=0, W=92, H=80, t_occ=3, w_gain=16, g_cap=174, min_gain=0, r_inflate=2, max_seg=5, S_max=1)
        args.update(kw)
        if "B" in kw and "F" not in kw:
            args["F"] = kw["B"]
        q = dict({n: ONE for n in POINTERS[UPATH]}, origin=C.cast(origin, C.c_void_p), cell=C.cast(cell, C.c_void_p))
        return raw_call(UPATH, **{k: v for k, v in q.items() if k not in drop}, **args)
    rc.count = "B"
    assert rc() == 0 and rc(B=0, F=1) == 0                 # B = 0 enqueues nothing
    _caps(rc)
    _gain_ranges(rc)
    assert rc(B=3, F=2, W=4097, H=2) == E_ARG and rc(B=3, F=1, W=4097, H=2) == E_UNSUPPORTED          # F is 1 or B
    assert rc(cell=(C.c_double * 2)(0.0, 0.1)) == E_ARG and rc(cell=(C.c_double * 2)(0.1, float("inf"))) == E_ARG
    assert rc(cell=(C.c_double * 2)(-0.1, 0.1)) == E_ARG and rc(cell=(C.c_double * 2)(0.1, float("nan"))) == E_ARG
    assert rc(origin=(C.c_double * 2)(float("nan"), 0.0)) == E_ARG and rc(origin=(C.c_double * 2)(0.0, float("-inf"))) == E_ARG
    assert rc(r_inflate=-1) == E_ARG and rc(r_inflate=17) == E_ARG and rc(r_inflate=16) == 0 and rc(r_inflate=0) == 0
    assert rc(t_occ=0) == E_ARG and rc(t_occ=(1 << 30) + 1) == E_ARG and rc(t_occ=1) == 0 and rc(t_occ=1 << 30) == 0
    assert rc(max_seg=4) == E_ARG and rc(max_seg=0) == E_ARG and rc(max_seg=0x7FFFFFFF) == 0
    assert rc(S_max=0) == E_ARG and rc(S_max=-1) == E_ARG
    assert rc(drop=("origin",)) == E_ARG and rc(drop=("cell",)) == E_ARG
    for missing in POINTERS[UPATH]:
        assert rc(drop=(missing,)) == E_ARG and rc(B=3, drop=(missing,)) == E_ARG and rc(W=4097, H=2, drop=(missing,)) == E_ARG, missing
    assert rc(W=4097, H=2, max_seg=4) == E_ARG and rc(W=4097, H=2, t_occ=0) == E_ARG and rc(W=4097, H=2, drop=("cell",)) == E_ARG


def test_gain_python_signatures():
    """(The constructor needs a device to finish: what it refuses before it asks for one is checked here.)"""
    cls = lipmpc.InformedFrontierPlanner
    sig = inspect.signature(cls.__init__)
    assert [p for p in sig.parameters][1:] == ["r_view", "w_gain", "g_cap", "min_gain", "frontier_planner_kwargs"]
    assert sig.parameters["min_gain"].default == 0
    assert all(sig.parameters[p].default is inspect.Parameter.empty for p in ("r_view", "w_gain", "g_cap"))
    assert sig.parameters["frontier_planner_kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    sig = inspect.signature(cls.plan)
    assert sig == inspect.signature(lipmpc.FrontierPlanner.plan)
    assert [p for p in sig.parameters][1:] == ["mapper_or_evidence", "start", "origin", "cell", "S_max", "out"] and sig.parameters["S_max"].default == 64
    for m in (cls.gain, cls.field):
        assert [p for p in inspect.signature(m).parameters][1:] == ["mapper_or_evidence", "out"]
    ok = dict(r_view=10, w_gain=16, g_cap=174)
    for bad in (dict(r_view=0), dict(r_view=65), dict(w_gain=-1), dict(w_gain=65536), dict(g_cap=0), dict(g_cap=16385), dict(min_gain=-1),
                dict(min_gain=16385), dict(r_inflate=17), dict(min_unknown=0), dict(max_seg=4), dict(t_occ=0)):
        with pytest.raises(ValueError):
            cls(**dict(ok, **bad))
    for missing in ok:
        with pytest.raises(TypeError):
            cls(**{k: v for k, v in ok.items() if k != missing})       # no gain parameter has a default
    # the parents' own signatures stay as they are
    sig = inspect.signature(lipmpc.FrontierPlanner.__init__)
    assert [p for p in sig.parameters][1:] == ["r_inflate", "min_unknown", "t_free", "t_occ", "max_seg", "device"]
    assert [p for p in inspect.signature(lipmpc.FrontierPlanner.field).parameters][1:] == ["mapper_or_evidence", "out"]
    sig = inspect.signature(lipmpc.CoordinatedFrontierPlanner.plan)
    assert [p for p in sig.parameters][1:] == ["mapper_or_evidence", "start", "origin", "cell", "S_max", "out", "may_claim"]
    sig = inspect.signature(lipmpc.UnknownEnvFleet.run_exploring)
    assert [p for p in sig.parameters][1:] == ["state0", "first_foot", "k_max", "explorer", "replan_every", "lookahead", "noise", "noise_seed",
                                                "delta", "stop_obj", "use_graph", "S_max"]
    table = lipmpc.planner.informed_outputs(3, 1, 20, 24, 64)
    near = lipmpc.planner.frontier_outputs(3, 1, 20, 24, 64)
    assert set(table) == set(near) | {"gain", "ufield", "n_sources", "target_gain"} and all(table[k] == near[k] for k in near)
    assert table["gain"][1] == table["ufield"][1] == (1, 20, 24) and table["n_sources"][1] == (1,) and table["target_gain"][1] == (3,)
    assert set(lipmpc.planner.assign_outputs(3, 20, 24, 64)) == set(near) | {"claim_round", "n_claims", "work"}
