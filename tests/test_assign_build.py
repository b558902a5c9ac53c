"""The coordinated claim: C ABI, Python signatures and compiled resources (no GPU needed)."""
import ctypes as C
import inspect

import pytest

import lipmpc
from code_object import kernel_resources
from helpers import raw_call

E_ARG, E_UNSUPPORTED = -1, -2
ASSIGN = "lipmpc_grid_frontier_assign_batch"
POINTERS = ("frontier", "field", "start", "may_claim", "work", "sub_goals", "n_sub", "status", "path_cost", "target_cell", "claim_round",
            "n_claims")


def test_assign_symbol_is_exported_and_bound():
    lib = lipmpc._lib.load()
    assert ASSIGN in lipmpc._lib.EXPORTS and ASSIGN in lipmpc._lib.SIGNATURES and hasattr(lib, ASSIGN)
    assert getattr(lib, ASSIGN).argtypes == [t for _, t in lipmpc._lib.SIGNATURES[ASSIGN][1]]
    assert [n for n, _ in lipmpc._lib.SIGNATURES[ASSIGN][1]] == [
        "device", "B", "W", "H", "origin", "cell", "frontier", "field", "start", "may_claim", "r_inflate", "r_claim", "max_claims", "max_seg",
        "S_max", "work", "sub_goals", "n_sub", "status", "path_cost", "target_cell", "claim_round", "n_claims", "hip_stream"]
    assert lib.lipmpc_version() == 5                       # a backward-compatible addition
    assert lipmpc.CoordinatedFrontierPlanner is lipmpc.planner.CoordinatedFrontierPlanner
    assert issubclass(lipmpc.CoordinatedFrontierPlanner, lipmpc.FrontierPlanner)


def test_assign_kernels_code_object():
    """From the built library's gfx950 code objects: the two assign kernels (round field in LDS / in ``work``) exist once each, use
    no scratch and spill nothing; their static LDS is the workgroup reduction's words, within the slack the LDS rule keeps."""
    res = kernel_resources(lipmpc._lib.LIB_PATH)
    for k in ("frontier_assign_lds_kernel", "frontier_assign_global_kernel"):
        mine = {name: r for name, r in res.items() if k in name}
        assert len(mine) == 1, (k, sorted(mine))
        (name, r), = mine.items()
        print(k, {f: r.get(f) for f in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")})
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r.get("sgpr_spill_count", 0) == 0, (name, r)
        assert r["group_segment_fixed_size"] <= 256, (name, r)


def test_assign_refusals_reach_no_device():
    """Every refusal is decided on the host before anything is enqueued."""
    one = C.c_void_p(8)                                    # device pointers: never dereferenced
    ptrs = {n: one for n in POINTERS}
    org, cs = (C.c_double * 2)(0.0, 0.0), (C.c_double * 2)(0.1, 0.1)

    def rc(drop=(), cell=cs, origin=org, **kw):
        args = dict(device=0, B=0, W=92, H=80, r_inflate=0, r_claim=15, max_claims=64, max_seg=5, S_max=1)
        args.update(kw)
        q = {k: v for k, v in dict(ptrs, origin=C.cast(origin, C.c_void_p), cell=C.cast(cell, C.c_void_p)).items() if k not in drop}
        return raw_call(ASSIGN, **q, **args)

    assert rc() == 0                                       # the same arguments pass: B = 0 enqueues nothing
    assert rc(drop=("may_claim",)) == 0                    # (optional)
    assert rc(B=-1) == E_ARG and rc(B=1 << 31) == E_ARG
    assert rc(W=1) == E_ARG and rc(H=1) == E_ARG and rc(W=0) == E_ARG and rc(H=-3) == E_ARG and rc(W=2, H=2) == 0
    assert rc(cell=(C.c_double * 2)(0.0, 0.1)) == E_ARG and rc(cell=(C.c_double * 2)(0.1, float("inf"))) == E_ARG
    assert rc(cell=(C.c_double * 2)(-0.1, 0.1)) == E_ARG and rc(cell=(C.c_double * 2)(0.1, float("nan"))) == E_ARG
    assert rc(origin=(C.c_double * 2)(float("nan"), 0.0)) == E_ARG and rc(origin=(C.c_double * 2)(0.0, float("-inf"))) == E_ARG
    assert rc(r_inflate=-1) == E_ARG and rc(r_inflate=17) == E_ARG and rc(r_inflate=16) == 0
    assert rc(r_claim=-1) == E_ARG and rc(r_claim=4097) == E_ARG and rc(r_claim=0) == 0 and rc(r_claim=4096) == 0
    assert rc(max_claims=-1) == E_ARG and rc(max_claims=4097) == E_ARG and rc(max_claims=0) == 0 and rc(max_claims=4096) == 0
    assert rc(max_seg=4) == E_ARG and rc(max_seg=0) == E_ARG and rc(max_seg=0x7FFFFFFF) == 0
    assert rc(S_max=0) == E_ARG and rc(S_max=-1) == E_ARG
    assert rc(drop=("origin",)) == E_ARG and rc(drop=("cell",)) == E_ARG
    for missing in POINTERS:
        if missing != "may_claim":
            assert rc(drop=(missing,)) == E_ARG and rc(B=3, drop=(missing,)) == E_ARG, missing
    # an argument error comes before the caps, the caps before "nothing to do"
    assert rc(W=4097, H=2) == E_UNSUPPORTED and rc(W=2, H=4097) == E_UNSUPPORTED and rc(W=4096, H=32) == 0
    assert rc(W=363, H=362) == E_UNSUPPORTED and rc(W=512, H=256) == 0 and rc(W=512, H=257) == E_UNSUPPORTED
    assert rc(W=4097, H=2, r_claim=-1) == E_ARG and rc(W=4097, H=2, drop=("work",)) == E_ARG and rc(W=4097, H=2, B=3) == E_UNSUPPORTED


def test_assign_python_signatures():
    """(The constructor needs a device to finish: what it refuses before it asks for one is checked here.)"""
    sig = inspect.signature(lipmpc.CoordinatedFrontierPlanner.__init__)
    assert [p for p in sig.parameters][1:] == ["r_claim", "max_claims", "frontier_planner_kwargs"]
    assert sig.parameters["max_claims"].default == 64 and sig.parameters["r_claim"].default is inspect.Parameter.empty
    assert sig.parameters["frontier_planner_kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    sig = inspect.signature(lipmpc.CoordinatedFrontierPlanner.plan)
    assert [p for p in sig.parameters][1:] == ["mapper_or_evidence", "start", "origin", "cell", "S_max", "out", "may_claim"]
    assert sig.parameters["S_max"].default == 64 and sig.parameters["may_claim"].default is None
    for bad in (dict(r_claim=-1), dict(r_claim=4097), dict(r_claim=5, max_claims=-1), dict(r_claim=5, max_claims=4097),
                dict(r_claim=5, r_inflate=17), dict(r_claim=5, min_unknown=0), dict(r_claim=5, max_seg=4), dict(r_claim=5, t_occ=0)):
        with pytest.raises(ValueError):
            lipmpc.CoordinatedFrontierPlanner(**bad)
    with pytest.raises(TypeError):
        lipmpc.CoordinatedFrontierPlanner()                # the claim radius has no default
    # the parent's own signatures stay as they are
    sig = inspect.signature(lipmpc.FrontierPlanner.plan)
    assert [p for p in sig.parameters][1:] == ["mapper_or_evidence", "start", "origin", "cell", "S_max", "out"]
    sig = inspect.signature(lipmpc.UnknownEnvFleet.run_exploring)
    assert [p for p in sig.parameters][1:] == ["state0", "first_foot", "k_max", "explorer", "replan_every", "lookahead", "noise", "noise_seed",
                                                "delta", "stop_obj", "use_graph", "S_max"]
    table = lipmpc.planner.assign_outputs(3, 20, 24, 64)
    assert set(table) == set(lipmpc.planner.frontier_outputs(3, 1, 20, 24, 64)) | {"claim_round", "n_claims", "work"}
    assert table["work"][1] == (20, 24) and table["claim_round"][1] == (3,) and table["n_claims"][1] == (1,)
