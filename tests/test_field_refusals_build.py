"""What every entry point of the field planner's translation unit refuses, and in which order (no GPU needed).

tests/golden/field_refusals.json (written by tests/golden/make_field_refusals.py) holds, per entry point, a base call with every
scalar legal and changes to it -- a scalar at a probe value, a pointer dropped, a shape, a placement, a workspace size, and
crossings of those with shapes beyond the caps -- each with the value the library returned when the table was recorded.  A
change is a row [values of `keys`..., returned...] of a table [keys, fixed, rows]: the arguments named by `keys` take the row's
values and those of `fixed` theirs; rows that start with "probes" take the values of the file's probe set in its order.
This test replays every row through helpers.raw_call and requires the same value: E_ARG, E_UNSUPPORTED, OK, E_HIP or a
workspace size.  What a call decides FIRST is part of its contract, and the table pins it for every call alike.

No row reaches a device.  A device pointer is the dummy value 8 (12: misaligned) and is never dereferenced; a row with a zero
count passes device 0 and returns before the device is selected; a row with a non-zero count passes device -1, so that a call
which accepts its arguments fails in the device selection -- its first HIP call -- with E_HIP and enqueues nothing.
"""
import ctypes as C
import glob
import json
import os
import re

import pytest

import lipmpc
from helpers import raw_call

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE = os.path.join(HERE, "golden", "field_refusals.json")
CSRC = os.path.join(os.path.dirname(lipmpc._lib.LIB_PATH), "csrc")

COUNTS = (0, 3)
# origin and cell are read on the host: real arrays, named here so that the table holds names and integers only
INF, NAN = float("inf"), float("nan")
PLACEMENTS = {
    "ok": ((0.0, 0.0), (0.1, 0.1)),
    "origin_null": (None, (0.1, 0.1)), "cell_null": ((0.0, 0.0), None),
    "dx_zero": ((0.0, 0.0), (0.0, 0.1)), "dy_zero": ((0.0, 0.0), (0.1, 0.0)),
    "dx_negative": ((0.0, 0.0), (-0.1, 0.1)), "dy_negative": ((0.0, 0.0), (0.1, -0.1)),
    "dx_inf": ((0.0, 0.0), (INF, 0.1)), "dy_inf": ((0.0, 0.0), (0.1, INF)),
    "dx_nan": ((0.0, 0.0), (NAN, 0.1)), "dy_nan": ((0.0, 0.0), (0.1, NAN)),
    "ox_inf": ((INF, 0.0), (0.1, 0.1)), "oy_inf": ((0.0, -INF), (0.1, 0.1)),
    "ox_nan": ((NAN, 0.0), (0.1, 0.1)), "oy_nan": ((0.0, NAN), (0.1, 0.1)),
}
HOST_OUTPUTS = ("tile_w", "tile_h", "max_cells")          # written by lipmpc_grid_tiled_info: real words where not dropped


def field_entry_points():
    """The binding's entry points that the field translation unit (lipmpc_field.hip and its sections) defines, in the binding's order."""
    text = "".join(open(p).read() for p in sorted(glob.glob(os.path.join(CSRC, "lipmpc_field*"))))
    defined = set(re.findall(r'^extern "C" \w+ (lipmpc_\w+)\(', text, re.M))
    assert defined and defined <= set(lipmpc._lib.SIGNATURES), defined - set(lipmpc._lib.SIGNATURES)
    return [n for n in lipmpc._lib.SIGNATURES if n in defined]


def is_pointer(t):
    return t is C.c_void_p or issubclass(t, C._Pointer)


def count_of(name):
    """The parameter that counts a call's work items (B, else F, else M), or None."""
    names = [n for n, _ in lipmpc._lib.SIGNATURES[name][1]]
    return next((c for c in ("B", "F", "M") if c in names), None)


def call_case(name, base, change):
    """One call: `base` with `change` applied; every pointer not named is 8, hip_stream NULL, the device by the count."""
    params = lipmpc._lib.SIGNATURES[name][1]
    given = dict(base)
    given.update(change)
    origin, cell = PLACEMENTS[given.pop("placement", "ok")]
    keep = [(C.c_double * 2)(*v) if v is not None else None for v in (origin, cell)] + [C.c_int64()]
    count = count_of(name)
    args = {}
    for n, t in params:
        if n == "device":
            args[n] = 0 if given[count] == 0 else -1
        elif n == "hip_stream":
            args[n] = None
        elif n in ("origin", "cell"):
            a = keep[n == "cell"]
            args[n] = C.cast(a, C.c_void_p) if a is not None else None
        elif is_pointer(t):
            v = given.get(n, 8)
            args[n] = None if v is None else C.c_void_p(C.addressof(keep[2]) if n in HOST_OUTPUTS else v)
        else:
            args[n] = given[n]
    return raw_call(name, **args)


def rows_of(entry):
    """[change, returned...] of every row of an entry point's tables."""
    for keys, fixed, rows in entry["tables"]:
        if rows[0] == "probes":
            assert len(keys) == 1 and len(rows) == 1 + len(PROBES), keys
            rows = [[v] + r for v, r in zip(PROBES, rows[1:])]
        for r in rows:
            yield [dict(zip(keys, r[:len(keys)]), **fixed)] + r[len(keys):]


def replay(name, entry):
    """Every row of an entry point's tables as (change, count, recorded, returned)."""
    count = count_of(name)
    for change, *recorded in rows_of(entry):
        if count is None or count in change:
            assert len(recorded) == 1, (name, change)
            yield change, change.get(count), recorded[0], call_case(name, entry["base"], change)
        else:
            assert len(recorded) == len(COUNTS), (name, change)
            for k, rec in zip(COUNTS, recorded):
                yield change, k, rec, call_case(name, entry["base"], dict(change, **{count: k}))


PROBES, RECORDED = [], {}                                  # (empty only while the generator writes the first table)
if os.path.exists(TABLE):
    with open(TABLE) as fh:
        _table = json.load(fh)
    PROBES, RECORDED = _table["probes"], _table["calls"]


def test_the_table_holds_every_field_entry_point():
    names = field_entry_points()
    assert sorted(RECORDED) == sorted(names), set(names) ^ set(RECORDED)
    for name, entry in RECORDED.items():
        rows = [json.dumps(r[0], sort_keys=True) for r in rows_of(entry)]
        assert rows and len(set(rows)) == len(rows), name                  # no empty table and no row twice
        assert "{}" in rows, name                                          # the base call itself


@pytest.mark.parametrize("name", sorted(set(RECORDED) | set(field_entry_points())))
def test_field_refusals_are_as_recorded(name):
    assert name in RECORDED, name
    wrong, n = [], 0
    for change, count, recorded, returned in replay(name, RECORDED[name]):
        n += 1
        if returned != recorded:
            wrong.append((change, count, recorded, returned))
    print(name, n, "calls")
    assert not wrong, (len(wrong), wrong[:10])
