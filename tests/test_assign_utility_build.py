"""The gain-seeded claims: C ABI, Python signatures and compiled resources (no GPU needed)."""
import ctypes as C
import inspect
import os
import re

import pytest

import lipmpc
from code_object import kernel_resources
from helpers import raw_call

E_ARG, E_UNSUPPORTED = -1, -2
ASSIGN, CALL = "lipmpc_grid_frontier_assign_batch", "lipmpc_grid_frontier_assign_utility_batch"
NEW = ["gain", "w_gain", "g_cap", "min_gain", "target_gain"]
POINTERS = ("frontier", "field", "start", "may_claim", "work", "sub_goals", "n_sub", "status", "path_cost", "target_cell", "claim_round",
            "n_claims", "gain", "target_gain")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lipmpc.h")


def test_symbol_is_exported_and_bound():
    lib = lipmpc._lib.load()
    assert CALL in lipmpc._lib.EXPORTS and CALL in lipmpc._lib.SIGNATURES and hasattr(lib, CALL)
    assert getattr(lib, CALL).argtypes == [t for _, t in lipmpc._lib.SIGNATURES[CALL][1]]
    assert lib.lipmpc_version() == 5                       # a backward-compatible addition


def test_argument_list_is_the_assign_calls_plus_the_new_ones():
    """The assign call's list in its order, then gain, w_gain, g_cap, min_gain, target_gain, ahead of the stream (which closes
    every list) -- in the binding and in the header's prototype."""
    old, new = (lipmpc._lib.SIGNATURES[n][1] for n in (ASSIGN, CALL))
    assert old[-1][0] == new[-1][0] == "hip_stream"
    assert list(new[:len(old) - 1]) == list(old[:-1]) and [n for n, _ in new[len(old) - 1:-1]] == NEW
    assert [t for _, t in new[len(old) - 1:-1]] == [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    text = open(HEADER).read()
    proto = re.search(r"\bint " + CALL + r"\(([^;]*)\);", text).group(1)
    assert [p.split()[-1].lstrip("*") for p in proto.replace("\n", " ").split(",")] == [n for n, _ in new]
    assert "two calls give identical bits" in text and "4 (2 (2 ceil(W H / 64) + 2) + 34 + W H) + 256 <= 163840" in text


def test_kernels_code_object():
    """From the built library's gfx950 code objects: the two kernels (round field in LDS / in ``work``) exist once each, use no
    scratch and spill nothing; their static LDS is the workgroup reduction's words, within the slack the LDS rule keeps."""
    res = kernel_resources(lipmpc._lib.LIB_PATH)
    for k in ("frontier_assign_utility_lds_kernel", "frontier_assign_utility_global_kernel"):
        mine = {name: r for name, r in res.items() if k in name}
        assert len(mine) == 1, (k, sorted(mine))
        (name, r), = mine.items()
        print(k, {f: r.get(f) for f in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")})
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r.get("sgpr_spill_count", 0) == 0, (name, r)
        assert r["group_segment_fixed_size"] <= 256, (name, r)


def test_refusals_reach_no_device():
    """Every refusal is decided on the host before anything is enqueued: ARG, then UNSUPPORTED, then B = 0."""
    one = C.c_void_p(8)                                    # device pointers: never dereferenced
    ptrs = {n: one for n in POINTERS}
    org, cs = (C.c_double * 2)(0.0, 0.0), (C.c_double * 2)(0.1, 0.1)

    def rc(drop=(), cell=cs, origin=org, **kw):
        args = dict(device=0, B=0, W=92, H=80, r_inflate=0, r_claim=15, max_claims=64, max_seg=5, S_max=1, w_gain=16, g_cap=120, min_gain=0)
        args.update(kw)
        q = {k: v for k, v in dict(ptrs, origin=C.cast(origin, C.c_void_p), cell=C.cast(cell, C.c_void_p)).items() if k not in drop}
        return raw_call(CALL, **q, **args)

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
    assert rc(w_gain=-1) == E_ARG and rc(w_gain=65536) == E_ARG and rc(w_gain=0) == 0 and rc(w_gain=65535) == 0
    assert rc(g_cap=0) == E_ARG and rc(g_cap=16385) == E_ARG and rc(g_cap=1) == 0 and rc(g_cap=16384) == 0
    assert rc(min_gain=-1) == E_ARG and rc(min_gain=16385) == E_ARG and rc(min_gain=16384) == 0
    assert rc(drop=("origin",)) == E_ARG and rc(drop=("cell",)) == E_ARG
    for missing in POINTERS:
        if missing != "may_claim":
            assert rc(drop=(missing,)) == E_ARG and rc(B=3, drop=(missing,)) == E_ARG, missing
    # an argument error comes before the caps, the caps before "nothing to do"
    assert rc(W=4097, H=2) == E_UNSUPPORTED and rc(W=2, H=4097) == E_UNSUPPORTED and rc(W=4096, H=32) == 0
    assert rc(W=363, H=362) == E_UNSUPPORTED and rc(W=512, H=256) == 0 and rc(W=512, H=257) == E_UNSUPPORTED
    assert rc(W=4097, H=2, g_cap=0) == E_ARG and rc(W=4097, H=2, drop=("gain",)) == E_ARG and rc(W=4097, H=2, B=3) == E_UNSUPPORTED
    assert rc(W=363, H=362, min_gain=-1) == E_ARG and rc(W=363, H=362, drop=("target_gain",)) == E_ARG


GAIN = dict(r_view=15, w_gain=16, g_cap=120)


@pytest.mark.parametrize("P", [lipmpc.CoordinatedFrontierPlanner, lipmpc.TiledCoordinatedFrontierPlanner])
def test_python_keywords(P):
    """(The constructor needs a device to finish: what it refuses before it asks for one is checked here.)"""
    sig = inspect.signature(P.__init__)
    assert [p for p in sig.parameters][1:] == ["r_claim", "max_claims", "frontier_planner_kwargs"]          # keyword-only, opt-in
    sig = inspect.signature(P.plan)
    assert [p for p in sig.parameters][1:] == ["mapper_or_evidence", "start", "origin", "cell", "S_max", "out", "may_claim"]
    for bad in (dict(r_view=15), dict(w_gain=16, g_cap=120), dict(r_view=15, w_gain=16), dict(min_gain=3),          # all or none
                dict(GAIN, r_view=0), dict(GAIN, r_view=65), dict(GAIN, w_gain=-1), dict(GAIN, w_gain=65536), dict(GAIN, g_cap=0),
                dict(GAIN, g_cap=16385), dict(GAIN, min_gain=-1), dict(GAIN, min_gain=16385),
                dict(GAIN, r_keep=3, keep_ratio16=24, keep_slack=4), dict(GAIN, r_keep=3),                           # no hysteresis
                dict(GAIN, r_clear=3, w_clear=40), dict(GAIN, r_clear=3, w_clear=40, tiled=True)):                   # no clearance
        with pytest.raises(ValueError):
            P(5, **bad)
    for misspelt in (dict(GAIN, mingain=3), dict(r_veiw=15, w_gain=16, g_cap=120), dict(r_view=15, wgain=16, g_cap=120),
                     dict(r_view=15, w_gain=16, gcap=120)):
        with pytest.raises(TypeError, match="r_view, w_gain, g_cap and min_gain"):
            P(5, **misspelt)
    if lipmpc.planner.torch.cuda.is_available():
        assert P(5, **GAIN, min_gain=8, t_free=1, t_occ=3).min_gain == 8 and P(5, **GAIN).min_gain == 0
    else:
        with pytest.raises(RuntimeError, match="HIP device"):
            P(5, **GAIN, min_gain=8, t_free=1, t_occ=3)    # every check passed: only the device is missing
    pl = object.__new__(P)                                 # (no device: the refusals below come before any attribute is read)
    pl.r_view, pl.r_keep = 15, None
    with pytest.raises(ValueError, match="hysteresis"):
        pl.replan(None, None, prev_target=[1])
    with pytest.raises(ValueError, match="cost="):
        pl.plan(None, None, cost=object())
    table = lipmpc.planner.assign_utility_outputs(3, 20, 24, 64)
    assert set(table) == set(lipmpc.planner.assign_outputs(3, 20, 24, 64)) | {"gain", "ufield", "n_sources", "target_gain"}
    assert table["gain"][1] == table["ufield"][1] == (1, 20, 24) and table["n_sources"][1] == (1,) and table["target_gain"][1] == (3,)


# -- the tiled call ----------------------------------------------------------------------------------------------------------------
TILED, TILED_OLD = "lipmpc_grid_frontier_assign_utility_tiled_batch", "lipmpc_grid_frontier_assign_tiled_batch"
TILED_BYTES = "lipmpc_grid_frontier_assign_utility_tiled_workspace_bytes"


def test_tiled_symbols_and_argument_list():
    lib = lipmpc._lib.load()
    for name in (TILED, TILED_BYTES):
        assert name in lipmpc._lib.EXPORTS and hasattr(lib, name)
        assert getattr(lib, name).argtypes == [t for _, t in lipmpc._lib.SIGNATURES[name][1]]
    old, new = (lipmpc._lib.SIGNATURES[n][1] for n in (TILED_OLD, TILED))
    assert list(new[:len(old) - 1]) == list(old[:-1]) and [n for n, _ in new[len(old) - 1:]] == NEW + ["hip_stream"]
    text = open(HEADER).read()
    proto = re.search(r"\bint " + TILED + r"\(([^;]*)\);", text).group(1)
    assert [p.split()[-1].lstrip("*") for p in proto.replace("\n", " ").split(",")] == [n for n, _ in new]
    doc = text[text.index("lipmpc_grid_frontier_assign_utility_tiled_batch (backward-compatible addition)"):text.index("int64_t " + TILED_BYTES)]
    assert "max_claims * (max_rounds + 4) + 3" in doc      # the fixed launch count, unchanged
    for W, H in ((33, 72), (363, 362), (4096, 4096)):
        assert getattr(lib, TILED_BYTES)(W, H) == lib.lipmpc_grid_frontier_assign_tiled_workspace_bytes(W, H) > 4 * W * H
    assert getattr(lib, TILED_BYTES)(1, 9) == E_ARG and getattr(lib, TILED_BYTES)(4097, 2) == E_UNSUPPORTED


def test_tiled_kernels_code_object():
    """The three kernels of the tiled call's own exist once each, with no scratch and no spills; the kernels it shares with the
    tiled claim call are still there once each."""
    res = kernel_resources(lipmpc._lib.LIB_PATH)
    for k in ("utility_assign_setup_kernel", "utility_assign_seed_kernel", "utility_assign_take_kernel", "claim_robots_kernel",
              "claim_pick_kernel", "claim_finish_kernel", "claim_setup_kernel", "claim_seed_kernel", "claim_take_kernel"):
        mine = {name: r for name, r in res.items() if k in name}
        assert len(mine) == 1, (k, sorted(mine))
        (name, r), = mine.items()
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r.get("sgpr_spill_count", 0) == 0, (name, r)


def test_tiled_refusals_reach_no_device():
    aligned = C.c_void_p(64)                               # device pointers: never dereferenced
    names = POINTERS + ("settled", "claims_settled")
    ptrs = {n: aligned for n in names}
    org, cs = (C.c_double * 2)(0.0, 0.0), (C.c_double * 2)(0.1, 0.1)
    need = lambda W, H: lipmpc._lib.load().lipmpc_grid_frontier_assign_utility_tiled_workspace_bytes(W, H)

    def rc(drop=(), **kw):
        args = dict(device=0, B=0, W=363, H=362, r_inflate=0, r_claim=15, max_claims=64, max_seg=5, S_max=1, w_gain=16, g_cap=120, min_gain=0,
                    max_rounds=8)
        args.update(kw)
        args.setdefault("work_bytes", max(need(args["W"], args["H"]), 0))
        q = {k: v for k, v in dict(ptrs, origin=C.cast(org, C.c_void_p), cell=C.cast(cs, C.c_void_p)).items() if k not in drop}
        return raw_call(TILED, **q, **args)

    assert rc() == 0 and rc(drop=("may_claim",)) == 0      # 363 x 362 is accepted here; B = 0 enqueues nothing
    assert rc(B=-1) == E_ARG and rc(W=1) == E_ARG and rc(r_claim=4097) == E_ARG and rc(max_claims=4097) == E_ARG and rc(max_seg=4) == E_ARG
    assert rc(w_gain=-1) == E_ARG and rc(w_gain=65536) == E_ARG and rc(w_gain=0) == 0 and rc(w_gain=65535) == 0
    assert rc(g_cap=0) == E_ARG and rc(g_cap=16385) == E_ARG and rc(g_cap=1) == 0 and rc(g_cap=16384) == 0
    assert rc(min_gain=-1) == E_ARG and rc(min_gain=16385) == E_ARG and rc(min_gain=16384) == 0
    assert rc(max_rounds=0) == E_ARG and rc(max_rounds=65537) == E_ARG and rc(max_claims=1, max_rounds=65536) == 0
    assert rc(max_claims=4096, max_rounds=256) == 0 and rc(max_claims=4096, max_rounds=257) == E_ARG          # the 2^20 launch cap
    for missing in names:
        if missing != "may_claim":
            assert rc(drop=(missing,)) == E_ARG and rc(B=3, drop=(missing,)) == E_ARG, missing
    assert rc(W=4096, H=4096) == 0 and rc(W=4097, H=2) == E_UNSUPPORTED and rc(W=2, H=4097) == E_UNSUPPORTED
    assert rc(W=4097, H=2, g_cap=0) == E_ARG and rc(W=4097, H=2, drop=("gain",)) == E_ARG and rc(W=4097, H=2, B=3) == E_UNSUPPORTED
    assert rc(work_bytes=need(363, 362) - 1) == E_ARG and rc(W=4097, H=2, work_bytes=0) == E_UNSUPPORTED
