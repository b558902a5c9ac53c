"""Neighbour LDCBF rows: C ABI and compiled resources (no GPU needed)."""
import lipmpc
from code_object import kernel_resources
from helpers import raw_call

KERNELS = ("nb_clear_kernel", "nb_bin_kernel", "nb_runs_kernel", "nb_scatter_kernel", "nb_search_kernelILi4E", "nb_search_kernelILi16E",
           "nb_rows_kernel")
E_ARG = -1


def test_neighbour_symbols_are_exported_and_bound():
    lib = lipmpc._lib.load()
    for name in ("lipmpc_neighbour_workspace_bytes", "lipmpc_neighbour_c_eta_batch"):
        assert name in lipmpc._lib.EXPORTS and name in lipmpc._lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == [t for _, t in lipmpc._lib.SIGNATURES[name][1]]
    assert lib.lipmpc_version() == 5
    assert lipmpc.NeighbourRows is lipmpc.neighbours.NeighbourRows


def test_neighbour_workspace_is_monotone_in_B():
    lib = lipmpc._lib.load()
    sizes = [lib.lipmpc_neighbour_workspace_bytes(B) for B in (0, 1, 2, 63, 64, 257, 511, 512, 513, 4096, 4097, 32768, 1 << 20, 1 << 22)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
    assert sizes[-1] > sizes[0]
    assert lib.lipmpc_neighbour_workspace_bytes(-1) < 0 and lib.lipmpc_neighbour_workspace_bytes((1 << 22) + 1) < 0


def test_neighbour_refusals_need_no_device():
    """Every refusal is decided before the device is touched."""
    good = dict(device=0, B=4, n_obs_max=6, k_rows=4, sense_range=1.0, share=0.5)
    ptrs = dict(state=8, radius=8, workspace=8, c_eta=8, n_rows=8, n_near=8)              # never dereferenced: refused first
    for bad in (dict(k_rows=0), dict(k_rows=17), dict(n_obs_max=0), dict(n_obs_max=51), dict(sense_range=0.0),
                dict(sense_range=-1.0), dict(sense_range=float("inf")), dict(sense_range=float("nan")), dict(share=-0.1),
                dict(share=1.1), dict(share=float("nan")), dict(B=-1), dict(B=(1 << 22) + 1)):
        assert raw_call("lipmpc_neighbour_c_eta_batch", **{**good, **bad}, **ptrs) == E_ARG, bad
    for missing in ptrs:
        assert raw_call("lipmpc_neighbour_c_eta_batch", **good, **{k: v for k, v in ptrs.items() if k != missing}) == E_ARG, missing
    assert raw_call("lipmpc_neighbour_c_eta_batch", **{**good, "B": 0}, **ptrs) == 0       # nothing to do


def test_neighbour_kernels_use_no_scratch():
    """The kernels of the built library, from its gfx950 code objects: no scratch (the search keeps its best 4 / 16
    candidates in registers: insertion with static indices), the run allocator's partial sums are the only LDS."""
    res = kernel_resources(lipmpc._lib.LIB_PATH)
    for k in KERNELS:
        mine = {name: r for name, r in res.items() if k in name}
        assert len(mine) == 1, (k, sorted(mine))
        (name, r), = mine.items()
        print(k, {f: r.get(f) for f in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")})
        assert r["private_segment_fixed_size"] == 0, (name, r)
        assert (0 < r["group_segment_fixed_size"] <= 2048) if k == "nb_runs_kernel" else r["group_segment_fixed_size"] == 0, (name, r)
