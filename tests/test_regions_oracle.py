"""tests/regions_oracle.py held to a second method (no GPU): the transitive closure of adjacency on small maps, scipy's labelling
where scipy imports, and hand-written expectations for the cases with a closed form."""
import numpy as np
import pytest

import regions_cases as RC
import regions_oracle as RO


def closure_labels(mask):
    """label [W,H] by brute force: adjacency matrix, transitive closure by repeated squaring, the least index of each class."""
    W, H = mask.shape
    n = W * H
    assert n <= 64
    on = mask.reshape(-1) != 0
    ii, jj = np.divmod(np.arange(n), H)
    adj = (np.abs(ii[:, None] - ii[None, :]) <= 1) & (np.abs(jj[:, None] - jj[None, :]) <= 1) & on[:, None] & on[None, :]
    reach = adj.copy()
    for _ in range(7):                                       # paths of up to 2^7 > 64 steps
        reach = reach | ((reach.astype(np.int32) @ reach.astype(np.int32)) > 0)
    lab = np.where(on, np.where(reach, np.arange(n)[None, :], n).min(axis=1), -1)
    return lab.reshape(W, H).astype(np.int32), reach


def test_small_maps_against_the_transitive_closure():
    masks = RC.small_masks()
    assert len(masks) > 500
    for m in masks:
        lab, reach = closure_labels(m)
        got = RO.regions(m, 1, 64)
        assert np.array_equal(got["label"], lab), m
        assert np.array_equal(got["size"], np.where(lab >= 0, reach.sum(axis=1).reshape(m.shape), 0)), m
        roots = np.unique(lab[lab >= 0])
        assert got["n_regions"].tolist() == [len(roots), len(roots), 0] and got["table"][:, 0].tolist() == roots.tolist()
        assert np.array_equal(got["table"][:, 1], [(lab == r).sum() for r in roots])
        assert got["rep"].sum() == len(roots) and np.all(lab.reshape(-1)[got["table"][:, 3]] == roots)


@pytest.mark.parametrize("id_", [i for i in RC.IDS if not i.startswith("real")])
def test_cases_against_scipy(id_):
    ndi = pytest.importorskip("scipy.ndimage")
    masks, min_size, R_max = RC.case(id_)
    want = RC.want(id_)
    for f, m in enumerate(masks):
        lab, n = ndi.label(m != 0, structure=np.ones((3, 3), int))
        assert n == want["n_regions"][f, 0]
        flat = np.arange(m.size).reshape(m.shape)
        roots = ndi.minimum(flat, lab, np.arange(1, n + 1)).astype(np.int64) if n else np.zeros(0, np.int64)
        sizes = np.bincount(lab.reshape(-1), minlength=n + 1)
        assert np.array_equal(want["label"][f], np.where(lab > 0, np.concatenate([[-1], roots])[lab], -1))
        assert np.array_equal(want["size"][f], np.where(lab > 0, sizes[lab], 0))
        kept = np.sort(roots[sizes[1:] >= min_size])
        assert want["n_regions"][f].tolist() == [n, len(kept), max(len(kept) - R_max, 0)]
        assert want["table"][f][:, 0].tolist() == kept[:R_max].tolist()
        ci = ndi.sum(flat // m.shape[1], lab, np.arange(1, n + 1)) if n else []
        for row in want["table"][f]:
            k = int(np.nonzero(roots == row[0])[0][0])
            assert row[1] == sizes[k + 1] and row[2] // m.shape[1] == (2 * int(ci[k]) + row[1]) // (2 * row[1]) and row[4] == 0
            assert want["label"][f].reshape(-1)[row[3]] == row[0] and want["rep"][f].reshape(-1)[row[3]] == 1
        assert want["rep"][f].sum() == len(want["table"][f])


def test_closed_form_cases_by_hand():
    H = RC.TH + 1
    w = RC.want("ones_2x2")
    assert w["label"].reshape(-1).tolist() == [0] * 4 and w["size"].reshape(-1).tolist() == [4] * 4
    # sums 2 and 2 of 4 cells: (2 * 2 + 4) // 8 = 1 both ways: the centroid cell is (1, 1) = 3, a cell of the region
    assert w["table"][0].tolist() == [[0, 4, 3, 3, 0]] and w["n_regions"].tolist() == [[1, 1, 0]]
    w = RC.want("zeros_2x2")
    assert w["n_regions"].tolist() == [[0, 0, 0]] and len(w["table"][0]) == 0 and not w["rep"].any() and (w["label"] == -1).all()
    # (0, 0) and (1, 1): the centroid (2 * 1 + 2) // 4 = 1 is (1, 1) itself
    assert RC.want("diagonal_2x2")["table"][0].tolist() == [[0, 2, 3, 3, 0]]
    # (0, 1) and (1, 0): ci = 1, cj = 1: cell 3 is off the region; both cells are at distance 1: the lower index, 1
    assert RC.want("antidiagonal_2x2")["table"][0].tolist() == [[1, 2, 3, 1, 0]]
    a, b = (RC.TW - 1) * H + RC.TH - 1, RC.TW * H + RC.TH
    assert RC.want("corner_diagonal")["table"][0].tolist() == [[a, 2, b, b, 0]]
    a, b = (RC.TW - 1) * H + RC.TH, RC.TW * H + RC.TH - 1
    assert RC.want("corner_antidiagonal")["table"][0].tolist() == [[a, 2, RC.TW * H + RC.TH, a, 0]]
    assert RC.want("border_columns_joined")["n_regions"].tolist() == [[1, 1, 0]]
    assert RC.want("border_columns_apart")["n_regions"].tolist() == [[2, 2, 0]]
    assert RC.want("border_rows_joined")["n_regions"].tolist() == [[1, 1, 0]] and RC.want("border_rows_apart")["n_regions"].tolist() == [[2, 2, 0]]
    for id_ in ("serpentine", "comb", "checkerboard_full", "tile_exactly", "line_4096x2", "line_2x4096"):
        w, m = RC.want(id_), RC.case(id_)[0]
        assert w["n_regions"].tolist() == [[1, 1, 0]] and w["table"][0][0, 1] == (m != 0).sum(), id_
        assert w["table"][0][0, 0] == np.flatnonzero(m.reshape(-1))[0]
    assert RC.want("tile_exactly")["table"][0].tolist() == [list(RO.full_rectangle(RC.TW, RC.TH)) + [0]]
    # 4096 cells of column 1: ci = (2 * 4095 * 4096 / 2 + 4096) // 8192 = 2048, cj = 1
    assert RC.want("line_4096x2")["table"][0].tolist() == [[1, 4096, 2048 * 2 + 1, 2048 * 2 + 1, 0]]
    assert RC.want("line_2x4096")["table"][0].tolist() == [[0, 4096, 2048, 2048, 0]]
    w = RC.want("checkerboard_sparse")
    assert w["n_regions"].tolist() == [[1056, 1056, 56]] and len(w["table"][0]) == 1000 and w["rep"].sum() == 1000
    cells = np.flatnonzero(RC.case("checkerboard_sparse")[0].reshape(-1))
    assert np.array_equal(w["table"][0], np.stack([cells[:1000], np.ones(1000, int), cells[:1000], cells[:1000], np.zeros(1000, int)], 1))
    # the rings: centroid (50, 50) for each, off the region; the nearest cells are the four side midpoints, the least index wins
    w = RC.want("rings")
    assert w["n_regions"].tolist() == [[3, 3, 0]]
    assert sorted(w["table"][0].tolist()) == sorted([(50 - r) * 100 + 50 - r, 8 * r, 5050, (50 - r) * 100 + 50, 0] for r in (10, 25, 40))


def test_label_and_size_do_not_depend_on_min_size_or_r_max():
    ref = RC.want(RC.SAME_LABELS[0])
    for id_ in RC.SAME_LABELS[1:]:
        w = RC.want(id_)
        assert np.array_equal(w["label"], ref["label"]) and np.array_equal(w["size"], ref["size"]) and w["n_regions"][0, 0] == ref["n_regions"][0, 0]
    kept = [int(RC.want(i)["n_regions"][0, 1]) for i in ("min_size_1", "min_size_3", "min_size_above_all")]
    assert kept[0] > kept[1] > kept[2] == 0
    assert RC.want("table_overflow")["n_regions"][0, 2] == kept[0] - 5 and len(RC.want("no_table")["table"][0]) == 0
    for b in ("byte_2", "byte_255", "bytes_mixed"):
        assert all(np.array_equal(RC.want(b)[k], ref[k]) for k in ("label", "size")) and RC.want(b)["n_regions"][0, 1] == kept[0]


def test_the_real_frontier_is_many_regions_over_many_tiles():
    m = RC.case("real_frontier")[0][0]
    w = RC.want("real_frontier")
    assert m.shape == (363, 362) and m.any()
    tiles = {(c // 362 // RC.TW, c % 362 // RC.TH) for c in np.flatnonzero(m.reshape(-1))}
    assert len(tiles) >= 4 and w["n_regions"][0, 0] >= 2
    assert RC.want("real_frontier_min_4")["n_regions"][0, 1] < w["n_regions"][0, 1]


def test_the_full_rectangle_in_closed_form_needs_64_bit_sums():
    W, H = RC.BIG
    root, n, cen, rep = RO.full_rectangle(W, H)
    # the sum of i is 2^32 - 2^21: past a signed 32-bit word, and the centroid's numerator 2 * sum + n is past an unsigned one
    sum_i = H * (W * (W - 1) // 2)
    assert (root, n) == (0, 1 << 22) and sum_i == (1 << 32) - (1 << 21) and 2 * sum_i + n > 1 << 32
    W2, H2 = RC.BIGGER
    assert H2 * (W2 * (W2 - 1) // 2) == (1 << 34) - (1 << 22) and RO.full_rectangle(W2, H2) == (0, 1 << 23, 2048 * H2 + 1024, 2048 * H2 + 1024)
    assert cen == rep == 1024 * H + 1024                     # (2 * 2047 * 2^21 + 2^22) // 2^23 = 1024
    # and the formula is the flood fill's on a size the flood fill can do
    assert RO.regions(np.ones((20, 31), np.uint8))["table"].tolist() == [list(RO.full_rectangle(20, 31)) + [0]]
