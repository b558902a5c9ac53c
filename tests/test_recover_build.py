"""Recovery from a failed solve (lipmpc_fleet_recover_update_batch): C ABI, compiled resources and parameter validation (no
GPU needed)."""
import ctypes as C
import inspect

import pytest

import lipmpc
from code_object import kernel_resources
from helpers import raw_call

E_ARG = -1
NAME, PLAIN = "lipmpc_fleet_recover_update_batch", "lipmpc_fleet_update_batch"
NEW = ["goal", "c_eta", "delta", "max_recover", "recover_run", "n_recover", "recover_margin"]


def test_recover_symbol_is_exported_and_bound():
    lib = lipmpc._lib.load()
    assert NAME in lipmpc._lib.EXPORTS and NAME in lipmpc._lib.SIGNATURES and hasattr(lib, NAME)
    assert getattr(lib, NAME).argtypes == [t for _, t in lipmpc._lib.SIGNATURES[NAME][1]]
    names = [n for n, _ in lipmpc._lib.SIGNATURES[NAME][1]]
    plain = [n for n, _ in lipmpc._lib.SIGNATURES[PLAIN][1]]
    assert names == plain[:-1] + NEW + ["hip_stream"]          # every argument of the plain update, then the new ones
    assert dict(lipmpc._lib.SIGNATURES[NAME][1])["max_recover"] is C.c_int32
    assert lib.lipmpc_version() == 5                           # a backward-compatible addition


def test_recover_kernel_code_object():
    """From the built library's gfx950 code object: the kernel exists once, uses no scratch, spills nothing, needs no LDS."""
    res = kernel_resources(lipmpc._lib.LIB_PATH)
    mine = {name: r for name, r in res.items() if "fleet_recover_update_kernel" in name}
    assert len(mine) == 1, sorted(mine)
    (name, r), = mine.items()
    print({f: r.get(f) for f in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")})
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r.get("sgpr_spill_count", 0) == 0, (name, r)
    assert r["group_segment_fixed_size"] == 0, (name, r)


def test_recover_refusals_reach_no_device():
    """Every refusal is decided on the host before anything is enqueued -- and before the handle is looked at: the handle
    here is an address that is never dereferenced, like the device pointers."""
    required = ("state", "first_foot", "walking", "last_obj", "n_steps", "last_status", "sample", "X_pred", "U_pred", "U", "theta",
                "omega", "obj", "status", "goal", "recover_run", "n_recover", "recover_margin")
    optional = ("n_overflow", "overflow", "c_eta", "delta")
    one = C.c_void_p(8)
    ptrs = {n: one for n in required + optional + ("h",)}

    def rc(drop=(), **kw):
        args = dict(B=0, k_max=4, stop_obj=0.05, max_recover=6)
        args.update(kw)
        return raw_call(NAME, **{k: v for k, v in ptrs.items() if k not in drop}, **args)

    assert rc() == 0 and rc(max_recover=0) == 0                # B = 0 enqueues nothing
    assert rc(drop=optional) == 0
    assert rc(max_recover=-1) == E_ARG and rc(max_recover=-(1 << 31)) == E_ARG and rc(B=3, max_recover=-1) == E_ARG
    assert rc(B=-1) == E_ARG and rc(k_max=0) == E_ARG and rc(k_max=-2) == E_ARG and rc(drop=("h",)) == E_ARG
    for missing in required:
        assert rc(B=3, drop=(missing,)) == E_ARG and rc(B=300, drop=(missing,)) == E_ARG, missing
    assert rc(B=3, drop=("n_overflow",)) == E_ARG              # overflow flags without their counter: as the plain update


def test_fleet_parameters_are_validated():
    sig = inspect.signature(lipmpc.UnknownEnvFleet.__init__)
    assert list(sig.parameters)[-1] == "recover" and sig.parameters["recover"].default == 0
    for bad in (-1, 1.5, "6", True, None):
        with pytest.raises(ValueError):
            lipmpc.UnknownEnvFleet(env_rings=[], recover=bad)
    sig = inspect.signature(lipmpc.BatchedLipMpc.fleet_update)
    assert list(sig.parameters)[1:] == ["fleet", "out", "overflow", "stop_obj", "recover"] and sig.parameters["recover"].default is None
    assert tuple(lipmpc.solver.recover_state(3)) == ("recover_run", "n_recover", "recover_margin")
    assert tuple(lipmpc.solver.fleet_state(3, 4)) == ("state", "first_foot", "walking", "last_obj", "n_steps", "last_status", "n_overflow",
                                                      "sample", "X_pred", "U_pred")                              # unchanged


def test_fleet_update_validates_the_recover_dict():
    """(A handle needs a device: the checks that come before the C call are run on an object without one, on CPU tensors.)"""
    torch = pytest.importorskip("torch")
    S = lipmpc.solver
    B, k_max = 3, 4
    sv = object.__new__(lipmpc.BatchedLipMpc)
    sv.device, sv.params, sv._h = torch.device("cpu"), lipmpc.LipMpcParams(N=3, n_obs_max=2, v_max=5), None
    new = lambda table: {k: torch.zeros(s, dtype=dt) for k, (dt, s, _) in table.items()}
    fleet, rec = new(S.fleet_state(B, k_max)), new(S.recover_state(B))
    out = {k: v for k, v in new(S.step_outputs(B, sv.params)).items() if S.step_outputs(B, sv.params)[k][2]}
    good = dict(rec, goal=torch.zeros((B, 2), dtype=torch.float64), c_eta=torch.zeros((B, 2, 4), dtype=torch.float64), delta=None, max_recover=6)
    bad = [dict(good, max_recover=-1), dict(good, max_recover=1.0), dict(good, max_recover=True), {k: v for k, v in good.items() if k != "max_recover"},
           dict(good, goal=None), dict(good, goal=torch.zeros((B, 3), dtype=torch.float64)), dict(good, c_eta=torch.zeros((B, 3, 4), dtype=torch.float64)),
           dict(good, delta=torch.zeros((B,), dtype=torch.float32)), dict(good, recover_run=torch.zeros((B,), dtype=torch.int64)),
           {k: v for k, v in good.items() if k != "n_recover"}, dict(good, recover_margin=torch.zeros((B + 1,), dtype=torch.float64)),
           dict(good, walking=fleet["walking"]), (6,)]
    for r in bad:
        with pytest.raises(ValueError):
            sv.fleet_update(fleet, out, recover=r)
