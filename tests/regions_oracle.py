"""Frontier regions (lipmpc_grid_frontier_regions_batch, include/lipmpc.h) restated in plain numpy / Python: a flood fill, sums and
the representative's key.  Shares nothing with the device code (no union-find, no tiles, no ranks by scan)."""
import numpy as np

NEIGHBOURS = [(di, dj) for di in (-1, 0, 1) for dj in (-1, 0, 1) if (di, dj) != (0, 0)]


def components(mask):
    """[[flat index, ...], ...] of the maximal 8-connected sets of non-zero cells of mask [W,H], each list in the order the flood
    fill met its cells, the lists in ascending order of their least cell."""
    W, H = mask.shape
    on = mask != 0
    seen = np.zeros((W, H), bool)
    out = []
    for i, j in zip(*np.nonzero(on)):              # row-major: the first cell met of a region is its least
        if seen[i, j]:
            continue
        seen[i, j] = True
        stack, cells = [(int(i), int(j))], []
        while stack:
            a, b = stack.pop()
            cells.append(a * H + b)
            for di, dj in NEIGHBOURS:
                p, q = a + di, b + dj
                if 0 <= p < W and 0 <= q < H and on[p, q] and not seen[p, q]:
                    seen[p, q] = True
                    stack.append((p, q))
        out.append(cells)
    return out


def centroid(sum_i, sum_j, n):
    """(ci, cj) by the contract's integer division (Python integers: no width to overflow)."""
    return (2 * int(sum_i) + n) // (2 * n), (2 * int(sum_j) + n) // (2 * n)


def regions(mask, min_size=1, R_max=1024):
    """One map.  label, size [W,H] int32, rep [W,H] uint8, table [min(kept, R_max), 5] int32, n_regions [3] int32."""
    mask = np.asarray(mask)
    W, H = mask.shape
    label = np.full(W * H, -1, np.int32)
    size = np.zeros(W * H, np.int32)
    rep = np.zeros(W * H, np.uint8)
    rows, kept = [], 0
    comps = components(mask)
    for cells in comps:
        cells = np.array(cells, np.int64)
        root, n = int(cells.min()), len(cells)
        label[cells] = root
        size[cells] = n
        if n < min_size:
            continue
        kept += 1
        if kept > R_max:
            continue
        ii, jj = cells // H, cells % H
        ci, cj = centroid(ii.sum(), jj.sum(), n)
        d2 = (ii - ci) ** 2 + (jj - cj) ** 2
        best = min(zip(d2.tolist(), cells.tolist()))[1]
        rep[best] = 1
        rows.append((root, n, ci * H + cj, best, 0))
    assert [r[0] for r in rows] == sorted(r[0] for r in rows)
    return dict(label=label.reshape(W, H), size=size.reshape(W, H), rep=rep.reshape(W, H),
                table=np.array(rows, np.int32).reshape(-1, 5),
                n_regions=np.array([len(comps), kept, max(kept - R_max, 0)], np.int32))


def regions_batch(masks, min_size=1, R_max=1024):
    """[F,W,H] masks: the outputs stacked, `table` as a list of per-map arrays (the rows the call writes)."""
    outs = [regions(m, min_size, R_max) for m in masks]
    return {k: ([o[k] for o in outs] if k == "table" else np.stack([o[k] for o in outs])) for k in outs[0]}


def full_rectangle(W, H):
    """The all-ones W x H mask in closed form: (root, size, centroid_cell, rep_cell).  One region; sum of i = H * W (W - 1) / 2; the
    centroid cell is a cell of the region, so it is its own nearest cell."""
    n = W * H
    ci, cj = centroid(H * (W * (W - 1) // 2), W * (H * (H - 1) // 2), n)
    return 0, n, ci * H + cj, ci * H + cj
