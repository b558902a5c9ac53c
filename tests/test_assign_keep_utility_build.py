"""Claim hysteresis for the gain-seeded claims: C ABI, Python signatures and compiled resources (no GPU needed)."""
import ctypes as C
import inspect
import os
import re

import pytest

import lipmpc
from code_object import kernel_resources
from helpers import raw_call

E_ARG, E_UNSUPPORTED = -1, -2
KEEP, CALL = "lipmpc_grid_frontier_assign_keep_batch", "lipmpc_grid_frontier_assign_keep_utility_batch"
TILED_KEEP, TILED = "lipmpc_grid_frontier_assign_keep_tiled_batch", "lipmpc_grid_frontier_assign_keep_utility_tiled_batch"
TILED_BYTES = "lipmpc_grid_frontier_assign_keep_utility_tiled_workspace_bytes"
NEW = ["gain", "ufield", "w_gain", "g_cap", "min_gain", "target_gain"]
TILED_NEW = ["gain", "ufield", "usettled", "w_gain", "g_cap", "min_gain", "target_gain"]
POINTERS = ("frontier", "field", "start", "may_claim", "prev_target", "work", "sub_goals", "n_sub", "status", "path_cost", "target_cell",
            "claim_round", "n_claims", "kept", "n_kept", "gain", "ufield", "target_gain")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lipmpc.h")
GAIN = dict(r_view=15, w_gain=16, g_cap=120)
KEEPS = dict(r_keep=6, keep_ratio16=24, keep_slack=8)


def test_symbols_are_exported_and_bound():
    lib = lipmpc._lib.load()
    for name in (CALL, TILED, TILED_BYTES):
        assert name in lipmpc._lib.EXPORTS and name in lipmpc._lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == [t for _, t in lipmpc._lib.SIGNATURES[name][1]]
    assert lib.lipmpc_version() == 5                       # a backward-compatible addition


@pytest.mark.parametrize("old,new,added", [(KEEP, CALL, NEW), (TILED_KEEP, TILED, TILED_NEW)])
def test_argument_list_is_the_keep_calls_plus_the_new_ones(old, new, added):
    """The keep call's list in its order, then the new names, ahead of the stream (which closes every list) -- in the binding and in
    the header's prototype."""
    was, now = (lipmpc._lib.SIGNATURES[n][1] for n in (old, new))
    assert was[-1][0] == now[-1][0] == "hip_stream"
    assert list(now[:len(was) - 1]) == list(was[:-1]) and [n for n, _ in now[len(was) - 1:-1]] == added
    ints = {"w_gain", "g_cap", "min_gain"}
    assert [t for _, t in now[len(was) - 1:-1]] == [C.c_int32 if n in ints else C.c_void_p for n in added]
    text = open(HEADER).read()
    proto = re.search(r"\bint " + new + r"\(([^;]*)\);", text).group(1)
    assert [p.split()[-1].lstrip("*") for p in proto.replace("\n", " ").split(",")] == [n for n, _ in now]


def test_the_header_states_the_consequences_the_lds_rule_and_the_launch_count():
    text = open(HEADER).read()
    doc = text[text.index(CALL + " (backward-compatible addition)"):text.index("int " + CALL + "(")]
    flat = " ".join(" ".join(re.sub(r"^\s*/?\*", "", line) for line in doc.splitlines()).split())
    for sentence in ("16 * keepfield[s_b] <= keep_ratio16 * near_b + 80 * keep_slack", "two calls give identical bits",
                     "every output the calls share equals lipmpc_grid_frontier_assign_utility_batch's, bit for bit",
                     "every output equals lipmpc_grid_frontier_assign_keep_batch's, bit for bit, kept and n_kept included",
                     "are more than r_claim apart", "No addition wraps",
                     "4 (2 (2 ceil(W H / 64) + 2) + 48 + W H) + 256 <= 163840", "tests/assign_keep_utility_oracle.py"):
        assert sentence in flat, sentence
    tiled = text[text.index(TILED + " (backward-compatible addition)"):text.index("int64_t " + TILED_BYTES)]
    assert "max_claims * (max_rounds + 5) + 3" in tiled and "usettled[0] == 0" in " ".join(tiled.split())
    assert "no hysteresis for these claims" in text and text.index("no hysteresis for these claims") < text.index(CALL) < \
        text.index("no hysteresis for these claims") + 200      # the sentence of the memoryless call points to this one


def test_kernels_code_object():
    """From the built library's gfx950 code objects: the new kernels exist once each, use no scratch and spill nothing; the
    one-workgroup pair's static LDS is the workgroup reduction's words, within the slack the LDS rule keeps; the kernels the tiled
    call shares with the tiled keep call, and the sibling calls' own, are still there once each."""
    res = kernel_resources(lipmpc._lib.LIB_PATH)
    new = ("frontier_assign_keep_utility_lds_kernel", "frontier_assign_keep_utility_global_kernel", "keep_utility_setup_kernel",
           "keep_utility_seed_kernel", "keep_utility_take_kernel")
    shared = ("keep_robots_kernel", "keep_mode_kernel", "keep_pick_kernel", "keep_finish_kernel", "keep_seed_kernel", "keep_take_kernel",
              "claim_setup_kernel", "frontier_assign_keep_lds_kernel", "frontier_assign_keep_global_kernel",
              "frontier_assign_utility_lds_kernel", "frontier_assign_utility_global_kernel", "utility_assign_setup_kernel",
              "utility_assign_seed_kernel", "utility_assign_take_kernel")
    for k in new + shared:
        mine = {name: r for name, r in res.items() if re.search(r"\d" + k + "E", name)}
        assert len(mine) == 1, (k, sorted(mine))
        (name, r), = mine.items()
        if k in new:
            print(k, {f: r.get(f) for f in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")})
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r.get("sgpr_spill_count", 0) == 0, (name, r)
        if k.startswith("frontier_assign_keep_utility"):
            assert r["group_segment_fixed_size"] <= 256, (name, r)


def test_refusals_reach_no_device():
    """Every refusal is decided on the host before anything is enqueued: ARG, then UNSUPPORTED, then B = 0."""
    one = C.c_void_p(8)                                    # device pointers: never dereferenced
    ptrs = {n: one for n in POINTERS}
    org, cs = (C.c_double * 2)(0.0, 0.0), (C.c_double * 2)(0.1, 0.1)

    def rc(drop=(), cell=cs, origin=org, **kw):
        args = dict(device=0, B=0, W=92, H=80, r_inflate=0, r_claim=15, r_keep=3, keep_ratio16=24, keep_slack=4, max_claims=64, max_seg=5,
                    S_max=1, w_gain=16, g_cap=120, min_gain=0)
        args.update(kw)
        q = {k: v for k, v in dict(ptrs, origin=C.cast(origin, C.c_void_p), cell=C.cast(cell, C.c_void_p)).items() if k not in drop}
        return raw_call(CALL, **q, **args)

    assert rc() == 0 and rc(drop=("may_claim",)) == 0      # B = 0 enqueues nothing; may_claim is optional
    # what the keep call refuses
    assert rc(r_keep=-1) == E_ARG and rc(r_keep=65) == E_ARG and rc(r_keep=0) == 0 and rc(r_keep=64) == 0
    assert rc(keep_ratio16=15) == E_ARG and rc(keep_ratio16=1025) == E_ARG and rc(keep_ratio16=16) == 0 and rc(keep_ratio16=1024) == 0
    assert rc(keep_slack=-1) == E_ARG and rc(keep_slack=4097) == E_ARG and rc(keep_slack=0) == 0 and rc(keep_slack=4096) == 0
    # what the gain-seeded call refuses
    assert rc(w_gain=-1) == E_ARG and rc(w_gain=65536) == E_ARG and rc(w_gain=0) == 0 and rc(w_gain=65535) == 0
    assert rc(g_cap=0) == E_ARG and rc(g_cap=16385) == E_ARG and rc(g_cap=1) == 0 and rc(g_cap=16384) == 0
    assert rc(min_gain=-1) == E_ARG and rc(min_gain=16385) == E_ARG and rc(min_gain=16384) == 0
    # what the assign call refuses
    assert rc(B=-1) == E_ARG and rc(B=1 << 31) == E_ARG and rc(W=1) == E_ARG and rc(H=1) == E_ARG and rc(W=2, H=2) == 0
    assert rc(r_inflate=-1) == E_ARG and rc(r_inflate=17) == E_ARG and rc(r_claim=-1) == E_ARG and rc(r_claim=4097) == E_ARG
    assert rc(max_claims=-1) == E_ARG and rc(max_claims=4097) == E_ARG and rc(max_claims=0) == 0 and rc(max_seg=4) == E_ARG and rc(S_max=0) == E_ARG
    assert rc(cell=(C.c_double * 2)(0.0, 0.1)) == E_ARG and rc(origin=(C.c_double * 2)(float("nan"), 0.0)) == E_ARG
    assert rc(drop=("origin",)) == E_ARG and rc(drop=("cell",)) == E_ARG
    for missing in POINTERS:
        if missing != "may_claim":
            assert rc(drop=(missing,)) == E_ARG and rc(B=3, drop=(missing,)) == E_ARG, missing
    # an argument error comes before the caps, the caps before "nothing to do"
    assert rc(W=363, H=362) == E_UNSUPPORTED and rc(W=512, H=256) == 0 and rc(W=512, H=257) == E_UNSUPPORTED
    assert rc(W=4097, H=2, B=3) == E_UNSUPPORTED and rc(W=4097, H=2, r_keep=65) == E_ARG and rc(W=4097, H=2, g_cap=0) == E_ARG
    assert rc(W=4097, H=2, drop=("ufield",)) == E_ARG and rc(W=363, H=362, drop=("target_gain",)) == E_ARG


def test_tiled_refusals_and_workspace_reach_no_device():
    lib = lipmpc._lib.load()
    size, old = getattr(lib, TILED_BYTES), lib.lipmpc_grid_frontier_assign_keep_tiled_workspace_bytes
    for W, H in ((2, 2), (33, 72), (363, 362), (4096, 4096)):
        assert size(W, H) == old(W, H) > 4 * W * H          # the tiled keep call's layout
    assert size(1, 5) == E_ARG and size(4097, 2) == E_UNSUPPORTED
    aligned = C.c_void_p(64)                               # device pointers: never dereferenced
    names = POINTERS + ("settled", "usettled", "claims_settled")
    ptrs = {n: aligned for n in names}
    org, cs = (C.c_double * 2)(0.0, 0.0), (C.c_double * 2)(0.1, 0.1)

    def rc(drop=(), **kw):
        args = dict(device=0, B=0, W=363, H=362, r_inflate=0, r_claim=15, r_keep=3, keep_ratio16=24, keep_slack=4, max_claims=64, max_seg=5,
                    S_max=1, w_gain=16, g_cap=120, min_gain=0, max_rounds=8)
        args.update(kw)
        args.setdefault("work_bytes", max(size(args["W"], args["H"]), 0))
        q = {k: v for k, v in dict(ptrs, origin=C.cast(org, C.c_void_p), cell=C.cast(cs, C.c_void_p)).items() if k not in drop and k not in args}
        return raw_call(TILED, **q, **args)

    assert rc() == 0 and rc(drop=("may_claim",)) == 0      # 363 x 362 is accepted here; B = 0 enqueues nothing
    assert rc(B=-1) == E_ARG and rc(W=1) == E_ARG and rc(r_claim=4097) == E_ARG and rc(max_claims=4097) == E_ARG and rc(max_seg=4) == E_ARG
    assert rc(r_keep=65) == E_ARG and rc(keep_ratio16=15) == E_ARG and rc(keep_slack=4097) == E_ARG
    assert rc(w_gain=65536) == E_ARG and rc(g_cap=0) == E_ARG and rc(min_gain=16385) == E_ARG and rc(w_gain=65535, g_cap=16384, min_gain=16384) == 0
    assert rc(max_rounds=0) == E_ARG and rc(max_rounds=65537) == E_ARG and rc(max_claims=1, max_rounds=65536) == 0
    assert rc(max_claims=4096, max_rounds=256) == 0 and rc(max_claims=4096, max_rounds=257) == E_ARG          # the 2^20 launch cap
    assert rc(work=C.c_void_p(68)) == E_ARG                # 8-byte aligned
    for missing in names:
        if missing != "may_claim":
            assert rc(drop=(missing,)) == E_ARG and rc(B=3, drop=(missing,)) == E_ARG, missing
    assert rc(W=4096, H=4096) == 0 and rc(W=4097, H=2) == E_UNSUPPORTED and rc(W=2, H=4097) == E_UNSUPPORTED
    assert rc(W=4097, H=2, g_cap=0) == E_ARG and rc(W=4097, H=2, drop=("usettled",)) == E_ARG and rc(W=4097, H=2, B=3) == E_UNSUPPORTED
    assert rc(work_bytes=size(363, 362) - 1) == E_ARG and rc(W=4097, H=2, work_bytes=0) == E_UNSUPPORTED
    assert "(budget + 5) + 3" in " ".join(lipmpc.TiledGainKeepFrontierPlanner.__doc__.split())


@pytest.mark.parametrize("P", [lipmpc.GainKeepFrontierPlanner, lipmpc.TiledGainKeepFrontierPlanner])
def test_python_keywords(P):
    """(The constructor needs a device to finish: what it refuses before it asks for one is checked here.)"""
    sig = inspect.signature(P.__init__)
    assert [p for p in sig.parameters][1:] == ["r_claim", "max_claims", "r_view", "w_gain", "g_cap", "min_gain", "r_keep", "keep_ratio16",
                                               "keep_slack", "frontier_planner_kwargs"]
    for name, p in sig.parameters.items():
        if name in dict(GAIN, **KEEPS, min_gain=0):
            assert p.kind is inspect.Parameter.KEYWORD_ONLY
            assert (p.default == 0) if name == "min_gain" else (p.default is inspect.Parameter.empty), name      # no default but min_gain's
    assert sig.parameters["max_claims"].default == 64
    every = dict(GAIN, **KEEPS)
    for missing in every:                                      # all or none -- and "none" is the parent class
        with pytest.raises(TypeError, match=missing):
            P(5, **{k: v for k, v in every.items() if k != missing})
        with pytest.raises(ValueError, match="no defaults"):
            P(5, **dict(every, **{missing: None}))
    for bad in (dict(r_view=0), dict(r_view=65), dict(w_gain=-1), dict(w_gain=65536), dict(g_cap=0), dict(g_cap=16385), dict(min_gain=-1),
                dict(min_gain=16385), dict(r_keep=-1), dict(r_keep=65), dict(keep_ratio16=15), dict(keep_ratio16=1025), dict(keep_slack=-1),
                dict(keep_slack=4097), dict(r_clear=3, w_clear=40)):                                               # ranges; no clearance
        with pytest.raises(ValueError):
            P(5, **dict(every, **bad))
    with pytest.raises(ValueError):
        P(4097, **every)
    for misspelt, names in ((dict(every, keep_ratio=24), "r_keep, keep_ratio16 and keep_slack"),
                            (dict(every, mingain=3), "r_view, w_gain, g_cap and min_gain"),
                            (dict(every, gcap=3), "r_view, w_gain, g_cap and min_gain")):
        with pytest.raises(TypeError, match=names):
            P(5, **misspelt)
    if lipmpc.planner.torch.cuda.is_available():
        pl = P(5, **every, min_gain=8, t_free=1, t_occ=3)
        assert (pl.min_gain, pl.r_keep, pl.r_view) == (8, 6, 15) and P(5, **every).min_gain == 0
    else:
        with pytest.raises(RuntimeError, match="HIP device"):
            P(5, **every, min_gain=8, t_free=1, t_occ=3)   # every check passed: only the device is missing
    pl = object.__new__(P)                                 # (no device: the refusal below comes before any attribute is read)
    with pytest.raises(ValueError, match="cost="):
        pl.plan(None, None, cost=object())
    assert [p for p in inspect.signature(P.replan).parameters][1:] == ["mapper_or_evidence", "start", "origin", "cell", "S_max", "out", "may_claim",
                                                                       "prev_target"]


def test_output_tables():
    planner = lipmpc.planner
    table = planner.assign_keep_utility_outputs(3, 20, 24, 64)
    assert set(table) == set(planner.assign_utility_outputs(3, 20, 24, 64)) | {"kept", "n_kept"}
    assert table["kept"][:2] == (planner.torch.int8, (3,)) and table["n_kept"][1] == (1,) and table["target_gain"][1] == (3,)
    tiled = planner.tiled_assign_keep_utility_outputs(3, 20, 24, 64)
    assert set(tiled) == set(planner.tiled_assign_utility_outputs(3, 20, 24, 64)) | {"kept", "n_kept"} and "work" not in tiled
    assert "claims_settled" in tiled


@pytest.mark.parametrize("P,points_to", [(lipmpc.CoordinatedFrontierPlanner, "GainKeepFrontierPlanner"),
                                         (lipmpc.TiledCoordinatedFrontierPlanner, "TiledGainKeepFrontierPlanner")])
def test_the_parents_still_refuse_and_point_to_the_new_classes(P, points_to):
    with pytest.raises(ValueError, match=r"the class with both is " + points_to):
        P(5, **GAIN, **KEEPS)
    with pytest.raises(ValueError, match="hysteresis"):
        P(5, **GAIN, r_keep=3)
    pl = object.__new__(P)
    pl.r_view, pl.r_keep = 15, None
    with pytest.raises(ValueError, match=r"hysteresis.*the class with both is " + points_to):
        pl.replan(None, None, prev_target=[1])
    assert issubclass(getattr(lipmpc, points_to), P) and points_to in P.__doc__
