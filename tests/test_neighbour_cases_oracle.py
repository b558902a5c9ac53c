"""tests/neighbour_cases.py on the oracle: every case is what it claims, so that no GPU test of
tests/test_neighbours_limits_gpu.py passes vacuously; and the sweep oracle equals the brute-force one bit for bit."""
import time

import numpy as np
import pytest

import neighbour_cases as NC
import neighbour_oracle as NO
from neighbour_checks import assert_equals_oracle


@pytest.fixture(scope="module")
def solved():
    """name -> (case, oracle outputs), every case of the module but the large one."""
    out = {}
    for name, build in NC.CASES.items():
        case = build()
        out[name] = (case, NO.neighbour_rows(**NC.call_args(case)))
    return out


def _nonfinite_robots(ref):
    return np.nonzero(~np.isfinite(ref["c_eta"]).all((1, 2)))[0].tolist()


def _in_range_pairs(ref):
    """(i, j) of every row the oracle wrote."""
    return [(i, int(j)) for i in range(len(ref["neighbours"])) for j in ref["neighbours"][i] if j >= 0]


@pytest.mark.parametrize("name", list(NC.EXTREME))
def test_an_extreme_case_has_neighbours_and_no_stray_nan(solved, name):
    case, ref = solved[name]
    n_near = ref["n_near"]
    print(name, "B", len(n_near), "n_near", n_near.min(), "..", n_near.max(), "with a neighbour", int((n_near >= 1).sum()))
    assert 4 * (n_near >= 1).sum() >= len(n_near)
    if name == "infinite cell, all in range":
        assert (n_near == len(n_near) - 1).all()
    else:
        assert len(set(n_near.tolist())) > 1
    assert _nonfinite_robots(ref) == case["nonfinite"]           # NaN and infinite rows where the case names them, nowhere else


@pytest.mark.parametrize("R", NC.RANGES)
def test_a_range_case_tells_the_root_from_the_square(R):
    """Among the present pairs of the case some have d2 < R * R but not sqrt(d2) < R: a kernel that compares squares gives
    another n_near.  That needs a double below R * R whose root rounds to R: there is one for R = 0.7 and 1/3; for 1e-3 and
    1e5 there is none, the two comparisons agree on every double and the case cannot tell them apart (nor can anything).
    Exactly at the range is out, one ulp inside is in."""
    case = NC.range_edges(R)
    st, g, at = case["state"], case["group"], case["at"]
    dx, dy = st[:, 0][:, None] - st[:, 0][None, :], st[:, 2][:, None] - st[:, 2][None, :]
    d2 = dx * dx + dy * dy
    same = (g[:, None] == g[None, :]) & ~np.eye(len(st), dtype=bool)
    R = np.float64(R)
    differ = same & ((np.sqrt(d2) < R) != (d2 < R * R))
    print("R", R, "pairs on which the root and the square part:", int(differ.sum()) // 2)
    can_part = np.sqrt(np.nextafter(R * R, 0.0)) == R
    assert can_part == (R in (np.float64(0.7), np.float64(1.0 / 3.0)))
    assert differ.sum() >= 8 if can_part else not differ.any()
    ref = NO.neighbour_rows(**NC.call_args(case))
    assert not ref["n_near"][at["exactly at range"]].any()
    assert (ref["n_near"][at["one ulp inside"]] == 1).all()
    assert set(ref["n_near"][at["diagonal"]].tolist()) == {0, 1}                 # the diagonal pairs lie on both sides
    for name in ("cell multiples", "range multiples"):
        assert (ref["n_near"][at[name]] >= 1).all()
    assert 10 <= ref["n_near"][at["ring centre"][0]] <= 86                       # the ring lies on both sides of the range


@pytest.mark.parametrize("name", ["clamp straddle +", "clamp straddle -"])
def test_a_clamp_straddle_has_robots_and_pairs_on_both_sides(solved, name):
    case, ref = solved[name]
    st, at = case["state"], case["at"]
    for axis, col in (("x", 0), ("y", 2)):
        idx = np.array(at[axis])
        clamped = np.abs(NC.cell_unclamped(st[idx, col], 1.0)) > NC.CELL_CLAMP
        beyond = dict(zip(idx.tolist(), clamped.tolist()))
        spanning = sum(1 for i, j in _in_range_pairs(ref) if i in beyond and i < j and beyond[i] != beyond[j])
        print(name, axis, "clamped", int(clamped.sum()), "of", len(idx), "in-range pairs across the bound", spanning)
        assert clamped.sum() >= 8 and (~clamped).sum() >= 8 and spanning >= 4
        assert (np.abs(NC.cell_of(st[idx, col], 1.0)) >= NC.CELL_CLAMP - 4).all()


@pytest.mark.parametrize("name", ["clamp far", "clamp int32 edge", "clamp tiny range"])
def test_everything_is_clamped_into_one_cell(solved, name):
    case, _ = solved[name]
    st, R = case["state"], case["sense_range"]
    for col in (0, 2):
        assert (np.abs(NC.cell_unclamped(st[:, col], R)) > NC.CELL_CLAMP).all()
        assert len(set(NC.cell_of(st[:, col], R).tolist())) == 1
    if name == "clamp int32 edge":
        q = NC.cell_unclamped(st[:, 0], R)
        assert (q > 2.0 ** 31 - 1).sum() >= 8 and (q < 2.0 ** 31 - 1).sum() >= 8


def test_the_floor_case_spreads_over_floored_cells(solved):
    case, _ = solved["floored cells"]
    st, R = case["state"], case["sense_range"]
    assert R < NC.CELL_FLOOR and NC.cell_width(R) == NC.CELL_FLOOR
    cells = set(zip(NC.cell_of(st[:, 0], R).tolist(), NC.cell_of(st[:, 2], R).tolist()))
    print("floored cells:", len(cells))
    assert len(cells) >= 16


def test_the_infinite_cell_is_one_cell_and_its_d2_overflows(solved):
    for name in ("infinite cell, all in range", "infinite cell, d2 overflows"):
        case, ref = solved[name]
        st = case["state"]
        assert np.isinf(NC.cell_width(case["sense_range"])) and not NC.cell_of(st[:, 0], case["sense_range"]).any()
    with np.errstate(over="ignore"):
        dx, dy = st[:, 0][:, None] - st[:, 0][None, :], st[:, 2][:, None] - st[:, 2][None, :]
        assert np.isinf(dx * dx + dy * dy).sum() > len(st) ** 2 // 2


def test_small_doubles_are_subnormal_and_off_unit_length(solved):
    case, ref = solved["small doubles"]
    st, at = case["state"], case["at"]
    c = at["cluster"]
    dx, dy = st[c, 0][:, None] - st[c, 0][None, :], st[c, 2][:, None] - st[c, 2][None, :]
    d2 = (dx * dx + dy * dy)[~np.eye(len(c), dtype=bool)]
    assert (d2 > 0).all() and (d2 < np.finfo(np.float64).tiny).all()             # subnormal, every one
    assert (ref["n_near"][c] == len(c) - 1).all()
    eta = ref["c_eta"][c, : ref["n_rows"][c[0]], 2:]
    off = np.abs(np.hypot(eta[..., 0], eta[..., 1]) - 1.0).max()
    print("subnormal d2: |eta| off unit length by up to", off)
    assert off > 1e-9
    for s in NC.SMALL_SEPARATIONS:
        rows = ref["c_eta"][at[f"pair {s:g}"], 0]
        assert (ref["n_rows"][at[f"pair {s:g}"]] == 1).all()
        assert np.isfinite(rows).all() == (s >= 1e-160), (s, rows)
    assert np.isinf(ref["c_eta"][at["pair 1e-162"][0], 0, 0]) and np.isnan(ref["c_eta"][at["pair 1e-162"][0], 0, 3])


@pytest.mark.parametrize("k_rows", NC.OCTET_K_ROWS)
def test_octets_are_cut_by_index(solved, k_rows):
    case, ref = solved[f"octets k_rows={k_rows}"]
    at = case["at"]
    centre = at["centre"][0]
    want = (at["octet 0"] + at["octet 2"] + at["octet 1"])[:k_rows]             # d2 = 0.3125 < 0.53125 < 0.578125, index order inside
    assert ref["n_near"][centre] == 24 and ref["neighbours"][centre].tolist() == want
    if k_rows == 15:
        assert want[-1] == at["octet 2"][6] and at["octet 2"][7] > want[-1]      # the last row is inside the second-nearest octet


def test_the_collision_cases_collide(solved):
    case, ref = solved["collisions"]
    at, nb = case["at"], NC.n_buckets(len(case["state"]))
    assert nb == 1024
    bk = NC.buckets(case)
    st = case["state"]
    cells = np.stack([NC.cell_of(st[:, 0], 1.0), NC.cell_of(st[:, 2], 1.0)], 1)
    (a, b), c = NC.ADJACENT_IN_ONE_BUCKET, NC.BETWEEN_TWO_IN_ONE_BUCKET
    assert (cells[at["adjacent A"]] == a).all() and (cells[at["adjacent B"]] == b).all()
    assert (cells[at["left"]] == (c[0] - 1, c[1])).all() and (cells[at["between"]] == c).all() and (cells[at["right"]] == (c[0] + 1, c[1])).all()
    assert len(set(bk[at["adjacent A"] + at["adjacent B"]].tolist())) == 1
    assert len(set(bk[at["left"] + at["right"]].tolist())) == 1 and bk[at["between"][0]] != bk[at["left"][0]]
    g0, g1 = (at[f"group {g}"] for g in NC.GROUPS_IN_ONE_BUCKET)
    assert not cells[g0 + g1].any() and len(set(bk[g0 + g1].tolist())) == 1
    # the example pair is one of 30 such pairs of adjacent cells among (-40..39)^2
    cx, cy = np.meshgrid(np.arange(-40, 40), np.arange(-40, 40), indexing="ij")
    h = NC.bucket_of(cx, cy, 0, 1024)
    assert int((h[:, :-1] == h[:, 1:]).sum() + (h[:-1, :] == h[1:, :]).sum() + (h[:-1, :-1] == h[1:, 1:]).sum()
               + (h[:-1, 1:] == h[1:, :-1]).sum()) == 30             # (along the axes and the diagonals)
    # pairs across the shared buckets are in range of each other, and the groups do not see each other
    pairs = _in_range_pairs(ref)
    for p, q in (("adjacent A", "adjacent B"), ("left", "between"), ("between", "right")):
        assert sum(1 for i, j in pairs if i in at[p] and j in at[q]) >= 4, (p, q)
    for g in NC.GROUPS_IN_ONE_BUCKET + NC.BIG_GROUPS:
        mine = at[f"group {g}"]
        assert (ref["n_near"][mine] == len(mine) - 1).all()


def test_slots_bind_at_both_ends(solved):
    for n_obs_max in (1, 50):
        case, ref = solved[f"slots n_obs_max={n_obs_max}"]
        first = case["at"]["first_slot"]
        assert (ref["n_near"] >= 4).sum() > 32
        assert not ref["n_rows"][first >= n_obs_max].any()
        assert (ref["n_rows"][first <= 0] == np.minimum(np.minimum(4, n_obs_max), ref["n_near"][first <= 0])).all()
    case, ref = solved["16 rows into 3 slots, no neighbours output"]
    assert not case["with_neighbours"] and ref["n_rows"].max() == 3 and (ref["n_near"] > 3).sum() > 32


def test_the_batches_fill_their_tables(solved):
    case, ref = solved["batch 4099"]
    assert NC.n_buckets(4099) == 16384                       # 2 B at least: 64 workgroups of nb_runs_kernel
    print("batch 4099: mean n_near", ref["n_near"].mean(), "max", ref["n_near"].max())
    assert (ref["n_near"] > 8).sum() > 1000 and (ref["n_near"] < 8).sum() > 1000         # k_rows = 8 binds and does not


@pytest.mark.parametrize("name", list(NC.CASES))
def test_the_sweep_equals_brute_force(solved, name):
    case, ref = solved[name]
    before = np.full((len(case["state"]), case["n_obs_max"], 4), -7.25)
    assert_equals_oracle(NO.neighbour_rows_sweep(**NC.call_args(case), c_eta=before),
                         NO.neighbour_rows(**NC.call_args(case), c_eta=before), name)
    assert_equals_oracle(NO.neighbour_rows_sweep(**NC.call_args(case), pairs_per_chunk=50), ref, name + ", small chunks")


def test_the_large_case_is_large_and_the_sweep_is_quick():
    """257^2 robots: 4128 absent (more than a workgroup of 256 robots, by each of the four ways), three groups, indices above
    2^16 among the neighbours.  The sweep oracle takes 1.6 - 2.0 s on it (one CPU core); brute force would take a minute."""
    case = NC.large()
    B = len(case["state"])
    t = time.perf_counter()
    ref = NO.neighbour_rows_sweep(**NC.call_args(case))
    print("sweep oracle on", B, "robots:", round(time.perf_counter() - t, 2), "s; mean n_near", ref["n_near"].mean())
    gone, way = case["at"]["absent"], case["at"]["way"]
    assert B == 257 * 257 > 1 << 16 and len(gone) > 16 * 256 and all((way == k).sum() > 1000 for k in range(4))
    assert not NO.present(case["state"], case["radius"], case["group"])[gone].any()
    assert NO.present(case["state"], case["radius"], case["group"]).sum() == B - len(gone)
    assert not ref["n_near"][gone].any() and not np.isin(ref["neighbours"], gone).any()
    assert (ref["neighbours"] >= 1 << 16).sum() > 1000
    assert (ref["n_near"] > 5).sum() > 1000 and (ref["n_near"] == 0).sum() > len(gone)       # k_rows binds; lone robots too
    assert len(set(case["group"][case["group"] >= 0].tolist())) == 3
    # a sample of the robots against brute force, with no window: all present robots as candidates
    some = np.random.default_rng(0).choice(B, 200, replace=False)
    st, R = case["state"], case["sense_range"]
    ok = NO.present(st, case["radius"], case["group"])
    for i in some:
        with np.errstate(invalid="ignore"):
            dx, dy = st[i, 0] - st[:, 0], st[i, 2] - st[:, 2]
            near = ok & ok[i] & (case["group"] == case["group"][i]) & (np.sqrt(dx * dx + dy * dy) < R)
        near[i] = False
        assert ref["n_near"][i] == near.sum(), i
        assert set(ref["neighbours"][i][ref["neighbours"][i] >= 0].tolist()) <= set(np.nonzero(near)[0].tolist())
