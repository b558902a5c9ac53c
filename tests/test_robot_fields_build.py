"""Claims from per-robot fields: C ABI, Python signatures and compiled resources (no GPU needed)."""
import ctypes as C
import inspect
import os
import re

import pytest

import lipmpc
import robot_fields_checks as RC
from code_object import kernel_resources
from helpers import raw_call

E_ARG, E_UNSUPPORTED = -1, -2
CALL, BYTES = "lipmpc_grid_frontier_assign_robot_fields_batch", "lipmpc_grid_frontier_assign_robot_fields_workspace_bytes"
KEEP_TILED = "lipmpc_grid_frontier_assign_keep_tiled_batch"
POINTERS = ("frontier", "field", "settled", "start", "may_claim", "prev_target", "work", "sub_goals", "n_sub", "status", "path_cost",
            "target_cell", "claim_round", "n_claims", "kept", "n_kept", "claims_settled")
OPTIONAL = ("may_claim", "prev_target")
KERNELS = ("robot_setup_kernel", "robot_entry_kernel", "robot_fill_kernel", "robot_all_settled_kernel", "robot_claim_kernel",
           "robot_walk_kernel", "robot_finish_kernel")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lipmpc.h")


def _names(name):
    return [n for n, _ in lipmpc._lib.SIGNATURES[name][1]]


def test_symbols_are_exported_and_bound():
    lib = lipmpc._lib.load()
    for name in (CALL, BYTES):
        assert name in lipmpc._lib.EXPORTS and name in lipmpc._lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == [t for _, t in lipmpc._lib.SIGNATURES[name][1]]
    # the keep call's argument list in its order, with `resume` after max_rounds
    old = _names(KEEP_TILED)
    at = old.index("max_rounds") + 1
    assert _names(CALL) == old[:at] + ["resume"] + old[at:] and _names(BYTES) == ["B", "W", "H"]
    assert lib.lipmpc_version() == 5                       # a backward-compatible addition
    assert lipmpc.planner.tiled_info()[:2] == (RC.TW, RC.TH)


def test_the_header_prototype_names_the_bindings_arguments_and_states_the_launch_count():
    with open(HEADER) as f:
        text = f.read()
    proto = re.search(r"\nint " + CALL + r"\((.*?)\);", text, re.S).group(1)
    assert [p.split()[-1].lstrip("*") for p in proto.replace("\n", " ").split(",")] == _names(CALL)
    proto = re.search(r"\nint64_t " + BYTES + r"\((.*?)\);", text, re.S).group(1)
    assert [p.split()[-1] for p in proto.split(",")] == ["B", "W", "H"]
    flat = " ".join(text.split()).replace(" * ", " ")
    assert "max_rounds + 8 launches" in flat and "max_rounds + 5" in flat
    assert "+ 8 launches" in " ".join(lipmpc.RobotFieldsFrontierPlanner.__doc__.split())


def test_kernels_code_object():
    """From the built library's gfx950 code objects: the seven new kernels exist once each, use no scratch and spill nothing; the
    rounds and the settle kernel they are launched with are still there once each."""
    res = kernel_resources(lipmpc._lib.LIB_PATH)
    for k in KERNELS + ("tiled_round_kernel", "tiled_settle_kernel"):
        mine = {name: r for name, r in res.items() if k in name}
        assert len(mine) == 1, (k, sorted(mine))
        (name, r), = mine.items()
        print(k, {f: r.get(f) for f in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")})
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r.get("sgpr_spill_count", 0) == 0, (name, r)


def test_the_workspace_is_monotone_and_below_twice_the_fields():
    size = getattr(lipmpc._lib.load(), BYTES)
    shapes = [(2, 2), (16, 16), (33, 72), (40, 44), (363, 362), (1024, 1024)]
    for B in (0, 1, 4, 64, 300):
        for W, H in shapes:
            n = size(B, W, H)
            assert n > 0 and n % 4 == 0
            assert size(B + 1, W, H) > n and size(B, W + 1, H) >= n and size(B, W, H + 1) >= n and size(B, W + 32, H + 64) > n
            if B and W * H >= 256:
                assert 4 * B * W * H < n < 8 * B * W * H, (B, W, H, n)
    assert size(64, 362, 362) < 2 * 33.6e6                   # 33.5 MB of fields for 64 robots on 362 x 362
    assert size(-1, 8, 8) == E_ARG and size(1, 1, 8) == E_ARG and size(1, 4097, 2) == E_UNSUPPORTED and size(1, 4096, 4097) == E_UNSUPPORTED
    # B * (W * H + 64) <= 2^31
    assert size(128, 4096, 4096) == E_UNSUPPORTED and size(127, 4096, 4096) > 0
    assert size(16384, 362, 362) == E_UNSUPPORTED and size(16000, 362, 362) > 0


def test_refusals_reach_no_device_in_order():
    """Every refusal is decided on the host before anything is enqueued: ARG, then UNSUPPORTED, then the work size, then B = 0."""
    size = getattr(lipmpc._lib.load(), BYTES)
    one = C.c_void_p(8)                                    # device pointers: never dereferenced
    ptrs = {n: one for n in POINTERS}
    org, cs = (C.c_double * 2)(0.0, 0.0), (C.c_double * 2)(0.1, 0.1)

    def rc(drop=(), **kw):
        args = dict(device=0, B=0, W=92, H=80, r_inflate=0, r_claim=15, r_keep=3, keep_ratio16=24, keep_slack=4, max_claims=64, max_seg=5,
                    S_max=1, max_rounds=8, resume=0, work_bytes=1 << 30)
        args.update(kw)
        q = {k: v for k, v in dict(ptrs, origin=C.cast(org, C.c_void_p), cell=C.cast(cs, C.c_void_p)).items() if k not in drop}
        return raw_call(CALL, **dict(q, **args))

    assert rc() == 0 and rc(drop=("may_claim",)) == 0 and rc(resume=1) == 0
    # prev_target may be NULL, and then kept and n_kept too; the three keep parameters are range-checked all the same
    assert rc(drop=("prev_target",)) == 0 and rc(drop=("prev_target", "kept", "n_kept")) == 0
    assert rc(drop=("kept",)) == E_ARG and rc(drop=("n_kept",)) == E_ARG
    for drop in ((), ("prev_target", "kept", "n_kept")):
        assert rc(drop, r_keep=-1) == E_ARG and rc(drop, r_keep=65) == E_ARG and rc(drop, r_keep=0) == 0 and rc(drop, r_keep=64) == 0
        assert rc(drop, keep_ratio16=15) == E_ARG and rc(drop, keep_ratio16=1025) == E_ARG and rc(drop, keep_ratio16=1024) == 0
        assert rc(drop, keep_slack=-1) == E_ARG and rc(drop, keep_slack=4097) == E_ARG and rc(drop, keep_slack=4096) == 0
    assert rc(B=-1) == E_ARG and rc(W=1) == E_ARG and rc(r_inflate=17) == E_ARG and rc(r_claim=4097) == E_ARG and rc(r_claim=-1) == E_ARG
    assert rc(max_claims=-1) == E_ARG and rc(max_claims=4097) == E_ARG and rc(max_seg=4) == E_ARG and rc(S_max=0) == E_ARG
    assert rc(max_rounds=0) == E_ARG and rc(max_rounds=65537) == E_ARG and rc(max_rounds=65536, max_claims=4096) == 0      # no launch cap
    assert rc(resume=2) == E_ARG and rc(resume=-1) == E_ARG
    assert rc(drop=("origin",)) == E_ARG and rc(drop=("cell",)) == E_ARG and rc(work=C.c_void_p(12)) == E_ARG      # 8-byte aligned
    for missing in POINTERS:
        if missing not in OPTIONAL:
            assert rc(drop=(missing,)) == E_ARG and rc(B=3, drop=(missing,)) == E_ARG, missing
    # an argument error comes before the caps, the caps before the work size, the work size before "nothing to do"
    assert rc(W=4097, H=2) == E_UNSUPPORTED and rc(W=4097, H=2, r_keep=65) == E_ARG and rc(W=4097, H=2, drop=("n_sub",)) == E_ARG
    assert rc(B=16384, W=362, H=362, work_bytes=0) == E_UNSUPPORTED and rc(B=128, W=4096, H=4096) == E_UNSUPPORTED
    assert rc(W=4097, H=2, work_bytes=0) == E_UNSUPPORTED
    assert rc(work_bytes=size(0, 92, 80) - 1) == E_ARG and rc(work_bytes=size(0, 92, 80)) == 0
    assert rc(B=3, work_bytes=size(3, 92, 80) - 1) == E_ARG and rc(B=3, W=363, H=362, work_bytes=size(3, 92, 80)) == E_ARG


def test_constructor_refusals_that_need_no_device():
    P = lipmpc.RobotFieldsFrontierPlanner
    assert issubclass(P, lipmpc.TiledCoordinatedFrontierPlanner) and "RobotFieldsFrontierPlanner" in dir(lipmpc)
    sig = inspect.signature(P.__init__)
    assert [p for p in sig.parameters][1:3] == ["r_claim", "max_claims"] and sig.parameters["max_claims"].default == 64
    for k in ("r_keep", "keep_ratio16", "keep_slack"):
        assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[k].default is None
    for bad, word in ((dict(tiled=False), "tiled=False"), (dict(r_view=3, w_gain=1, g_cap=4), "r_view"), (dict(min_gain=1), "min_gain"),
                      (dict(r_clear=2, w_clear=3), "r_clear"), (dict(r_keep=3), "go together"), (dict(keep_ratio16=24, keep_slack=4), "go together"),
                      (dict(r_keep=65, keep_ratio16=24, keep_slack=4), "r_keep"), (dict(r_keep=3, keep_ratio16=15, keep_slack=4), "keep_ratio16"),
                      (dict(r_keep=3, keep_ratio16=24, keep_slack=4097), "keep_slack"), (dict(rounds=0), "rounds"), (dict(rounds=65537), "rounds"),
                      (dict(paths="lanes"), "paths")):
        with pytest.raises(ValueError, match=word):
            P(5, **bad)
    for bad in (dict(r_claim=-1), dict(r_claim=4097), dict(r_claim=5, max_claims=4097)):
        with pytest.raises(ValueError):
            P(**bad)
    with pytest.raises(TypeError, match="r_keep, keep_ratio16 and keep_slack"):
        P(5, keep_ratio=24)
    assert inspect.signature(P.replan) == inspect.signature(lipmpc.TiledCoordinatedFrontierPlanner.replan)
    assert inspect.signature(P.plan) == inspect.signature(lipmpc.TiledCoordinatedFrontierPlanner.plan)
