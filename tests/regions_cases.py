"""Masks of the frontier regions tests, shared by tests/test_regions_oracle.py (CPU: the oracle against a second method) and
tests/test_regions_gpu.py (the device call against the oracle): the smallest shapes at which the kernels can go wrong.  The tiles
are the tiled field's TW x TH = 32 x 64 cells (along i, along j); the ranking passes cut the flat index into chunks of 2048.

A CASE is (masks [F,W,H] uint8, min_size, R_max); ``case(id)`` builds it (cached, read only)."""
import functools

import numpy as np

TW, TH, CHUNK = 32, 64, 2048


def _m(W, H, cells=(), value=1):
    m = np.zeros((W, H), np.uint8)
    for i, j in cells:
        m[i, j] = value
    return m


def serpentine(W=130, H=130):
    """A one-cell-wide path: every fourth row full, joined to the next at alternating ends.  One region through every tile, its
    root (0, 0) far from most cells."""
    m = np.zeros((W, H), np.uint8)
    for k, i in enumerate(range(0, W, 4)):
        m[i, :] = 1
        if i + 4 < W:
            m[i:i + 4, H - 1 if k % 2 == 0 else 0] = 1
    return m


def comb(W=130, H=130):
    """Teeth along i on every other column, joined only along the LAST row: each tooth's least cell is in row 0, so the teeth's roots
    merge late, through the border unions of the last tile row."""
    m = np.zeros((W, H), np.uint8)
    m[:, ::2] = 1
    m[W - 1, :] = 1
    return m


def rings(W=100, H=100):
    """Three nested square rings round (50, 50), not touching: each one's centroid is the centre, outside the region, and four
    cells (at least) tie for the nearest: the lower index wins."""
    m = np.zeros((W, H), np.uint8)
    for r in (10, 25, 40):
        m[50 - r:50 + r + 1, 50 - r] = m[50 - r:50 + r + 1, 50 + r] = 1
        m[50 - r, 50 - r:50 + r + 1] = m[50 + r, 50 - r:50 + r + 1] = 1
    return m


def checkerboard(W=64, H=66, sparse=False):
    i, j = np.meshgrid(np.arange(W), np.arange(H), indexing="ij")
    return (((i % 2 == 0) & (j % 2 == 0)) if sparse else ((i + j) % 2 == 0)).astype(np.uint8)


def mixed(W=45, H=70, seed=5):
    """Blobs of several sizes: 1, 2, 3, 5 and more cells, so that min_size 1, 3 and 1000 keep different sets."""
    rng = np.random.default_rng(seed)
    m = (rng.random((W, H)) < 0.22).astype(np.uint8)
    m[20:23, :] = 0                                          # two halves that cannot join
    m[30, 10:40] = 1
    return m


def real_frontier():
    """The 363 x 362 frontier of tests/large_map_cases.py's first_refused sample: 12 x 6 tiles, the last ones cut."""
    import frontier_oracle as FR
    import large_map_cases as L
    return FR.masks(L.sample_evidence("first_refused"), L.T_FREE, L.T_OCC, L.R_INFLATE, L.MIN_UNKNOWN)[1].astype(np.uint8)


def _three_maps():
    a = np.zeros((3, 40, 70), np.uint8)
    a[0] = mixed(40, 70, seed=9)
    a[2, 5:35, 63:66] = 1                                    # over the tile border along j
    a[2, 31:34, :10] = 1                                     # over the tile border along i
    a[2, 0, 0] = 1
    return a


_BUILDERS = {
    "ones_2x2": lambda: (np.ones((2, 2), np.uint8), 1, 4),
    "zeros_2x2": lambda: (np.zeros((2, 2), np.uint8), 1, 4),
    "diagonal_2x2": lambda: (_m(2, 2, [(0, 0), (1, 1)]), 1, 4),
    "antidiagonal_2x2": lambda: (_m(2, 2, [(0, 1), (1, 0)]), 1, 4),
    "tile_exactly": lambda: (np.ones((TW, TH), np.uint8), 1, 8),
    "tile_exactly_sparse": lambda: (checkerboard(TW, TH, sparse=True), 1, 600),
    "corner_diagonal": lambda: (_m(TW + 1, TH + 1, [(TW - 1, TH - 1), (TW, TH)]), 1, 4),
    "corner_antidiagonal": lambda: (_m(TW + 1, TH + 1, [(TW - 1, TH), (TW, TH - 1)]), 1, 4),
    "border_columns_joined": lambda: (_cols(TW + 8, TH + 8, (TH - 1, TH)), 1, 4),
    "border_columns_apart": lambda: (_cols(TW + 8, TH + 8, (TH - 1, TH + 1)), 1, 4),
    "border_rows_joined": lambda: (np.ascontiguousarray(_cols(TH + 8, TW + 8, (TW - 1, TW)).T), 1, 4),
    "border_rows_apart": lambda: (np.ascontiguousarray(_cols(TH + 8, TW + 8, (TW - 1, TW + 1)).T), 1, 4),
    "serpentine": lambda: (serpentine(), 1, 4),
    "comb": lambda: (comb(), 1, 4),
    "checkerboard_full": lambda: (checkerboard(), 1, 4),
    "checkerboard_sparse": lambda: (checkerboard(sparse=True), 1, 1000),
    "rings": lambda: (rings(), 1, 8),
    "line_4096x2": lambda: (_line(4096, 2), 1, 4),
    "line_2x4096": lambda: (_line(2, 4096), 1, 4),
    "three_maps": lambda: (_three_maps(), 2, 16),
    "byte_2": lambda: (mixed() * np.uint8(2), 1, 64),
    "byte_255": lambda: (mixed() * np.uint8(255), 1, 64),
    "bytes_mixed": lambda: (mixed() * np.random.default_rng(1).integers(1, 256, mixed().shape).astype(np.uint8), 1, 64),
    "min_size_1": lambda: (mixed(), 1, 256),
    "min_size_3": lambda: (mixed(), 3, 256),
    "min_size_above_all": lambda: (mixed(), 1000, 256),
    "table_overflow": lambda: (mixed(), 1, 5),
    "no_table": lambda: (mixed(), 1, 0),
    "real_frontier": lambda: (real_frontier(), 1, 1024),
    "real_frontier_min_4": lambda: (real_frontier(), 4, 1024),
}
IDS = tuple(_BUILDERS)
SMALL = ("ones_2x2", "zeros_2x2", "diagonal_2x2", "antidiagonal_2x2")          # <= 64 cells: the transitive closure
SAME_LABELS = ("min_size_1", "min_size_3", "min_size_above_all", "table_overflow", "no_table")     # one mask: label and size equal
BIG = (2048, 2048)                                        # the closed-form case: all ones
BIGGER = (4096, 2048)                                     # ... and the one whose sum of i, 2^34 - 2^22, is past every 32-bit word


def _cols(W, H, cols):
    m = np.zeros((W, H), np.uint8)
    for j in cols:
        m[:, j] = 1
    return m


def _line(W, H):
    m = np.zeros((W, H), np.uint8)
    if W > H:
        m[:, 1] = 1
    else:
        m[0, :] = 1
    return m


@functools.lru_cache(maxsize=None)
def case(id_):
    masks, min_size, R_max = _BUILDERS[id_]()
    masks = np.ascontiguousarray(masks if masks.ndim == 3 else masks[None])
    masks.setflags(write=False)
    return masks, min_size, R_max


@functools.lru_cache(maxsize=None)
def want(id_):
    """The oracle's outputs of a case (computed once, read only)."""
    import regions_oracle as RO
    masks, min_size, R_max = case(id_)
    return RO.regions_batch(masks, min_size, R_max)


def small_masks():
    """Every mask of up to 3 x 3 cells with a few set, and some random ones of up to 64 cells: for the transitive closure."""
    rng = np.random.default_rng(3)
    out = [case(i)[0][0] for i in SMALL]
    for W, H in ((2, 2), (3, 3), (2, 5)):
        for bits in range(1 << (W * H)):
            out.append(np.array([(bits >> k) & 1 for k in range(W * H)], np.uint8).reshape(W, H))
    for W, H, p in ((8, 8, 0.3), (8, 8, 0.5), (4, 16, 0.4), (16, 4, 0.45), (7, 9, 0.35)):
        for _ in range(6):
            out.append((rng.random((W, H)) < p).astype(np.uint8))
    return out
