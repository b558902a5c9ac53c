"""GPU: lipmpc_grid_frontier_regions_batch against tests/regions_oracle.py on the masks of tests/regions_cases.py: label, size, rep,
the written rows of table and n_regions bit for bit, every run into poisoned outputs and a poisoned workspace, every case twice."""
import numpy as np
import pytest

import regions_cases as RC
import regions_oracle as RO

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import lipmpc  # noqa: E402

DEV = "cuda:0"
POISON = (0x5A, 0xA5)           # the bytes every output and the workspace hold before the two runs of a case
PLAIN = ("label", "size", "rep", "n_regions")


def _poisoned(F, W, H, R_max, byte, rep=True, table=True):
    """The call's dict (lipmpc.frontier_regions' ``out``) filled with one byte; ``rep`` / ``table`` False: None = NULL."""
    need = int(lipmpc._lib.load().lipmpc_grid_frontier_regions_workspace_bytes(F, W, H, R_max))
    table_ = dict(lipmpc.regions_outputs(F, W, H, R_max), work=(torch.uint8, (need,), True))
    out = {}
    for k, (dt, shape, _) in table_.items():
        n = int(np.prod(shape)) * torch.empty(0, dtype=dt).element_size()
        out[k] = torch.full((n,), byte, dtype=torch.uint8, device=DEV).view(dt).view(shape)
    if not rep:
        out["rep"] = None
    if not table:
        out["table"] = None
    return out


def _compare(got, want, byte, R_max):
    for k in PLAIN:
        if got[k] is not None:
            assert np.array_equal(got[k].cpu().numpy(), want[k]), k
    if got["table"] is not None:
        tab = got["table"].cpu().numpy()
        for f, rows in enumerate(want["table"]):
            assert np.array_equal(tab[f, :len(rows)], rows), f
            # the rows from min(kept, R_max) on are untouched
            assert (tab[f, len(rows):].view(np.uint8) == byte).all(), f


def _run(masks, min_size, R_max, want, **null):
    fr = torch.as_tensor(np.ascontiguousarray(masks), device=DEV)
    F, W, H = fr.shape
    first = None
    for byte in POISON:
        out = _poisoned(F, W, H, R_max, byte, **null)
        got = lipmpc.frontier_regions(fr, min_size, R_max, out=out)
        torch.cuda.synchronize()
        _compare(got, want, byte, R_max)
        bits = {k: got[k].cpu().numpy().copy() for k in PLAIN if got[k] is not None}
        if first is not None:
            assert all(np.array_equal(bits[k], first[k]) for k in bits)              # two calls: identical bits
        first = bits
    return got


@pytest.mark.parametrize("id_", RC.IDS)
def test_gpu_case_equals_the_oracle(id_):
    masks, min_size, R_max = RC.case(id_)
    _run(masks, min_size, R_max, RC.want(id_))


@pytest.mark.parametrize("id_", ["three_maps", "checkerboard_sparse", "comb"])
def test_gpu_rep_and_table_may_be_null(id_):
    masks, min_size, R_max = RC.case(id_)
    want = RC.want(id_)
    _run(masks, min_size, R_max, want, rep=False)
    # no table: R_max = 0, nothing tabled, nobody's representative marked
    none = RO.regions_batch(masks, min_size, 0)
    assert np.array_equal(none["label"], want["label"]) and not none["rep"].any()
    _run(masks, min_size, 0, none, table=False)
    _run(masks, min_size, 0, none, table=False, rep=False)


def test_gpu_fresh_dict_and_two_dimensional_mask():
    m = RC.case("rings")[0][0]
    got = lipmpc.frontier_regions(torch.as_tensor(m, device=DEV), R_max=8)
    torch.cuda.synchronize()
    want = RC.want("rings")
    assert all(np.array_equal(got[k].cpu().numpy(), want[k]) for k in PLAIN)
    tab = got["table"].cpu().numpy()
    assert np.array_equal(tab[0, :3], want["table"][0]) and not tab[0, 3:].any()
    for bad in (dict(min_size=0), dict(R_max=-1), dict(R_max=(1 << 20) + 1), dict(min_size=(1 << 24) + 1)):
        with pytest.raises(ValueError):
            lipmpc.frontier_regions(torch.as_tensor(m, device=DEV), **bad)
    with pytest.raises(ValueError):
        lipmpc.frontier_regions(torch.as_tensor(m.astype(np.int32), device=DEV))


@pytest.mark.parametrize("W,H", [RC.BIG, RC.BIGGER])
def test_gpu_full_rectangle_in_closed_form(W, H):
    """One launch sequence on 2^22 / 2^23 frontier cells in one region: label 0, size W * H, centroid and representative by formula
    (tests/regions_oracle.full_rectangle), not by the flood fill.  On 2048 x 2048 the sum of i is past 2^31 and the centroid's
    numerator past 2^32; on 4096 x 2048 the sum itself is 2^34 - 2^22: a 32-bit accumulator of either sign fails it."""
    root, n, cen, rep_cell = RO.full_rectangle(W, H)
    fr = torch.ones((1, W, H), dtype=torch.uint8, device=DEV)
    out = _poisoned(1, W, H, 4, POISON[0])
    got = lipmpc.frontier_regions(fr, 1, 4, out=out)
    torch.cuda.synchronize()
    assert bool((got["label"] == root).all()) and bool((got["size"] == n).all())
    assert got["n_regions"].cpu().tolist() == [[1, 1, 0]]
    assert got["table"][0, 0].cpu().tolist() == [root, n, cen, rep_cell, 0]
    assert (got["table"][0, 1:].cpu().numpy().view(np.uint8) == POISON[0]).all()
    assert int(got["rep"].sum()) == 1 and int(got["rep"].view(-1)[rep_cell]) == 1


def test_gpu_captured_graph_replayed_after_the_mask_changed():
    a, _, R_max = RC.case("comb")
    b = np.ascontiguousarray(RC.case("serpentine")[0])
    assert a.shape == b.shape
    fr = torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    out = _poisoned(*fr.shape, R_max, POISON[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        lipmpc.frontier_regions(fr, 1, R_max, out=out)                            # once before the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            lipmpc.frontier_regions(fr, 1, R_max, out=out)
    torch.cuda.current_stream().wait_stream(side)
    for masks, want in ((a, RC.want("comb")), (b, RC.want("serpentine")), (a, RC.want("comb"))):
        fr.copy_(torch.as_tensor(np.ascontiguousarray(masks), device=DEV))
        for k in ("label", "size", "rep", "table", "n_regions", "work"):
            out[k].view(torch.uint8).fill_(POISON[1])
        graph.replay()
        torch.cuda.synchronize()
        _compare(out, want, POISON[1], R_max)


def test_gpu_two_streams_on_two_buffer_sets():
    ids = ("real_frontier", "checkerboard_sparse")
    streams = [torch.cuda.Stream() for _ in ids]
    jobs = []
    for id_, s in zip(ids, streams):
        masks, min_size, R_max = RC.case(id_)
        fr = torch.as_tensor(np.ascontiguousarray(masks), device=DEV)
        jobs.append((id_, fr, min_size, R_max, _poisoned(*fr.shape, R_max, POISON[0])))
    torch.cuda.synchronize()
    for _ in range(3):
        for (id_, fr, min_size, R_max, out), s in zip(jobs, streams):
            with torch.cuda.stream(s):
                lipmpc.frontier_regions(fr, min_size, R_max, out=out)
    torch.cuda.synchronize()
    for id_, fr, min_size, R_max, out in jobs:
        _compare(out, RC.want(id_), POISON[0], R_max)


def test_gpu_planner_regions_method():
    """FrontierPlanner.regions = field() then the call on its frontier, one-workgroup and tiled alike; every subclass inherits it."""
    import frontier_oracle as FR
    import gain_checks as K
    shared, _ = K.scanned_maps()
    mask = FR.masks(shared, K.T_FREE, K.T_OCC, 2, 2)[1].astype(np.uint8)
    want = RO.regions(mask, 2, 64)
    ev = torch.as_tensor(shared, device=DEV)
    outs = []
    for make in (lambda: lipmpc.FrontierPlanner(t_free=K.T_FREE, t_occ=K.T_OCC),
                 lambda: lipmpc.FrontierPlanner(t_free=K.T_FREE, t_occ=K.T_OCC, tiled=True),
                 lambda: lipmpc.InformedFrontierPlanner(5, 16, 40, t_free=K.T_FREE, t_occ=K.T_OCC),
                 lambda: lipmpc.TiledCoordinatedFrontierPlanner(5, t_free=K.T_FREE, t_occ=K.T_OCC)):
        planner = make()
        got = planner.regions(ev, min_size=2, R_max=64)
        torch.cuda.synchronize()
        assert {"frontier", "label", "size", "rep", "table", "n_regions", "field", "n_frontier"} <= set(got)
        assert ("settled" in got) == planner.tiled
        assert np.array_equal(got["frontier"][0].cpu().numpy() != 0, mask != 0) and want["n_regions"][1] >= 2
        for k in PLAIN:
            assert np.array_equal(got[k][0].cpu().numpy(), want[k]), k
        assert np.array_equal(got["table"][0, :len(want["table"])].cpu().numpy(), want["table"]) and not got["table"][0, len(want["table"]):].any()
        again = planner.regions(ev, min_size=2, R_max=64, out=dict(got))
        torch.cuda.synchronize()
        assert all(again[k] is got[k] for k in got) and len(planner._region_works) == 1      # grow-only: no second buffer
        outs.append(got)
    assert all(torch.equal(outs[0][k], o[k]) for o in outs[1:] for k in ("label", "size", "rep", "table", "n_regions", "field"))
