"""Claim hysteresis: C ABI, Python signatures and compiled resources (no GPU needed)."""
import ctypes as C
import inspect
import os

import pytest

import lipmpc
from code_object import kernel_resources
from helpers import raw_call

E_ARG, E_UNSUPPORTED = -1, -2
ASSIGN, KEEP = "lipmpc_grid_frontier_assign_batch", "lipmpc_grid_frontier_assign_keep_batch"
TILED, TILED_KEEP = "lipmpc_grid_frontier_assign_tiled_batch", "lipmpc_grid_frontier_assign_keep_tiled_batch"
TILED_KEEP_BYTES = "lipmpc_grid_frontier_assign_keep_tiled_workspace_bytes"
NEW = ("prev_target", "r_keep", "keep_ratio16", "keep_slack", "kept", "n_kept")
POINTERS = ("frontier", "field", "start", "may_claim", "prev_target", "work", "sub_goals", "n_sub", "status", "path_cost", "target_cell",
            "claim_round", "n_claims", "kept", "n_kept")


def _names(name):
    return [n for n, _ in lipmpc._lib.SIGNATURES[name][1]]


def test_keep_symbol_is_exported_and_bound():
    lib = lipmpc._lib.load()
    assert KEEP in lipmpc._lib.EXPORTS and KEEP in lipmpc._lib.SIGNATURES and hasattr(lib, KEEP)
    assert getattr(lib, KEEP).argtypes == [t for _, t in lipmpc._lib.SIGNATURES[KEEP][1]]
    # the existing call's argument list, in its order, plus the six new ones
    assert [n for n in _names(KEEP) if n not in NEW] == _names(ASSIGN) and set(NEW) < set(_names(KEEP))
    assert len(_names(KEEP)) == len(_names(ASSIGN)) + 6
    assert lib.lipmpc_version() == 5                       # a backward-compatible addition


def test_keep_kernels_code_object():
    """From the built library's gfx950 code objects: the two keep kernels (slot field in LDS / in ``work``) exist once each, use no
    scratch and spill nothing, as tests/test_assign_build.py reports for the assign kernels -- whose report is still that."""
    res = kernel_resources(lipmpc._lib.LIB_PATH)
    for k in ("frontier_assign_keep_lds_kernel", "frontier_assign_keep_global_kernel", "frontier_assign_lds_kernel",
              "frontier_assign_global_kernel"):
        mine = {name: r for name, r in res.items() if k in name}
        assert len(mine) == 1, (k, sorted(mine))
        (name, r), = mine.items()
        print(k, {f: r.get(f) for f in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")})
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r.get("sgpr_spill_count", 0) == 0, (name, r)
        assert r["group_segment_fixed_size"] <= 256, (name, r)


def test_keep_refusals_reach_no_device():
    """Every refusal is decided on the host before anything is enqueued."""
    one = C.c_void_p(8)                                    # device pointers: never dereferenced
    ptrs = {n: one for n in POINTERS}
    org, cs = (C.c_double * 2)(0.0, 0.0), (C.c_double * 2)(0.1, 0.1)

    def rc(drop=(), **kw):
        args = dict(device=0, B=0, W=92, H=80, r_inflate=0, r_claim=15, r_keep=3, keep_ratio16=24, keep_slack=4, max_claims=64, max_seg=5,
                    S_max=1)
        args.update(kw)
        q = {k: v for k, v in dict(ptrs, origin=C.cast(org, C.c_void_p), cell=C.cast(cs, C.c_void_p)).items() if k not in drop}
        return raw_call(KEEP, **q, **args)

    assert rc() == 0 and rc(drop=("may_claim",)) == 0      # B = 0 enqueues nothing; may_claim is optional
    assert rc(r_keep=-1) == E_ARG and rc(r_keep=65) == E_ARG and rc(r_keep=0) == 0 and rc(r_keep=64) == 0
    assert rc(keep_ratio16=15) == E_ARG and rc(keep_ratio16=1025) == E_ARG and rc(keep_ratio16=16) == 0 and rc(keep_ratio16=1024) == 0
    assert rc(keep_slack=-1) == E_ARG and rc(keep_slack=4097) == E_ARG and rc(keep_slack=0) == 0 and rc(keep_slack=4096) == 0
    # what the existing call refuses
    assert rc(B=-1) == E_ARG and rc(W=1) == E_ARG and rc(r_inflate=17) == E_ARG and rc(r_claim=4097) == E_ARG
    assert rc(max_claims=-1) == E_ARG and rc(max_claims=4097) == E_ARG and rc(max_seg=4) == E_ARG and rc(S_max=0) == E_ARG
    assert rc(drop=("origin",)) == E_ARG and rc(drop=("cell",)) == E_ARG
    for missing in POINTERS:
        if missing != "may_claim":
            assert rc(drop=(missing,)) == E_ARG and rc(B=3, drop=(missing,)) == E_ARG, missing
    # an argument error comes before the caps, the caps before "nothing to do"
    assert rc(W=363, H=362) == E_UNSUPPORTED and rc(W=512, H=256) == 0 and rc(W=4097, H=2, B=3) == E_UNSUPPORTED
    assert rc(W=4097, H=2, r_keep=65) == E_ARG and rc(W=4097, H=2, drop=("kept",)) == E_ARG


def test_tiled_keep_symbols_kernels_and_refusals():
    lib = lipmpc._lib.load()
    assert [n for n in _names(TILED_KEEP) if n not in NEW] == _names(TILED) and len(_names(TILED_KEEP)) == len(_names(TILED)) + 6
    for name in (TILED_KEEP, TILED_KEEP_BYTES):
        assert name in lipmpc._lib.EXPORTS and hasattr(lib, name)
    res = kernel_resources(lipmpc._lib.LIB_PATH)
    for k in ("keep_robots_kernel", "keep_mode_kernel", "keep_seed_kernel", "keep_pick_kernel", "keep_take_kernel", "keep_finish_kernel"):
        mine = {name: r for name, r in res.items() if k in name}
        assert len(mine) == 1, (k, sorted(mine))
        (name, r), = mine.items()
        print(k, {f: r.get(f) for f in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")})
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r.get("sgpr_spill_count", 0) == 0, (name, r)
    # the workspace: the tiled claim call's and eight more control words
    size, old = getattr(lib, TILED_KEEP_BYTES), lib.lipmpc_grid_frontier_assign_tiled_workspace_bytes
    for W, H in ((2, 2), (33, 72), (363, 362), (4096, 4096)):
        assert size(W, H) == old(W, H) + 32
    assert size(1, 5) == E_ARG and size(4097, 2) == E_UNSUPPORTED
    one = C.c_void_p(8)
    ptrs = {n: one for n in POINTERS + ("settled", "claims_settled")}
    org, cs = (C.c_double * 2)(0.0, 0.0), (C.c_double * 2)(0.1, 0.1)

    def rc(drop=(), **kw):
        args = dict(device=0, B=0, W=92, H=80, r_inflate=0, r_claim=15, r_keep=3, keep_ratio16=24, keep_slack=4, max_claims=64, max_seg=5,
                    S_max=1, max_rounds=8, work_bytes=1 << 30)
        args.update(kw)
        q = {k: v for k, v in dict(ptrs, origin=C.cast(org, C.c_void_p), cell=C.cast(cs, C.c_void_p)).items() if k not in drop}
        return raw_call(TILED_KEEP, **q, **args)

    assert rc() == 0 and rc(drop=("may_claim",)) == 0
    assert rc(r_keep=65) == E_ARG and rc(keep_ratio16=15) == E_ARG and rc(keep_slack=4097) == E_ARG and rc(max_rounds=0) == E_ARG
    assert rc(max_claims=4096, max_rounds=257) == E_ARG and rc(max_claims=4096, max_rounds=256) == 0      # the 2^20 launch cap stays
    assert rc(work_bytes=size(92, 80) - 1) == E_ARG and rc(work_bytes=size(92, 80)) == 0
    for missing in POINTERS + ("settled", "claims_settled"):
        if missing != "may_claim":
            assert rc(drop=(missing,)) == E_ARG, missing
    # the launch count is stated as one formula in the header and in the class (counted on the device, as the kernel nodes of a
    # captured call, by tests/test_assign_keep_tiled_gpu.py)
    formula = "max_claims * (max_rounds + 5) + 3"
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lipmpc.h")) as f:
        assert formula in f.read()
    assert "(budget + 5) + 3" in " ".join(lipmpc.TiledCoordinatedFrontierPlanner.__doc__.split())


def test_keep_python_signatures():
    """(The constructor needs a device to finish: what it refuses before it asks for one is checked here.)"""
    P = lipmpc.CoordinatedFrontierPlanner
    sig = inspect.signature(P.replan)
    assert [p for p in sig.parameters][1:] == ["mapper_or_evidence", "start", "origin", "cell", "S_max", "out", "may_claim", "prev_target"]
    assert sig.parameters["prev_target"].default is None and sig.parameters["S_max"].default == 64
    for bad in (dict(r_keep=3), dict(r_keep=3, keep_ratio16=24), dict(r_keep=3, keep_slack=4), dict(keep_ratio16=24), dict(keep_slack=4),
                dict(r_keep=-1, keep_ratio16=24, keep_slack=4), dict(r_keep=65, keep_ratio16=24, keep_slack=4),
                dict(r_keep=3, keep_ratio16=15, keep_slack=4), dict(r_keep=3, keep_ratio16=1025, keep_slack=4),
                dict(r_keep=3, keep_ratio16=24, keep_slack=-1), dict(r_keep=3, keep_ratio16=24, keep_slack=4097)):
        with pytest.raises(ValueError):
            P(5, **bad)
    with pytest.raises(TypeError, match="r_keep, keep_ratio16 and keep_slack"):
        P(5, r_keep=3, keep_ratio=24, keep_slack=4)        # a misspelt keyword is named here, not by the parent's __init__
    with pytest.raises(ValueError):
        lipmpc.TiledCoordinatedFrontierPlanner(5, r_keep=3, keep_ratio16=24)
    tiled = lipmpc.planner.tiled_assign_keep_outputs(3, 20, 24, 64)
    assert set(tiled) == set(lipmpc.planner.tiled_assign_outputs(3, 20, 24, 64)) | {"kept", "n_kept"} and "work" not in tiled
    table = lipmpc.planner.assign_keep_outputs(3, 20, 24, 64)
    assert set(table) == set(lipmpc.planner.assign_outputs(3, 20, 24, 64)) | {"kept", "n_kept"}
    assert table["kept"][:2] == (lipmpc.planner.torch.int8, (3,)) and table["n_kept"][1] == (1,)
