"""What every entry point of the field planner's translation unit refuses, recorded from the built library (run by hand):

    python tests/golden/make_field_refusals.py

writes tests/golden/field_refusals.json, which tests/test_field_refusals_build.py replays.  Per entry point (the list is that
test's field_entry_points(): the binding's SIGNATURES met with what lipmpc_field.hip and its sections define) a base call with every
scalar legal, and per change the value returned at count 0 and at count 3 -- or one value where the change names the count itself
or the entry point has none -- in the tables that the test's docstring describes:
  - the base call;
  - every integer scalar alone at every value of PROBES (all of which an int32 holds); on a path call also B and F together;
  - every device pointer alone dropped, and alone at the misaligned value 12;
  - the shapes of SHAPES;
  - every placement of the test's PLACEMENTS;
  - work_bytes at 0, need - 1, need and 2^40, need from the call's own *_workspace_bytes;
  - every dropped pointer, every scalar value that the base shape refuses as E_ARG and every placement so refused, crossed with a shape
    beyond the side cap (4097 x 2) and one beyond the one-workgroup calls' cell cap alone (363 x 362): which of E_ARG and
    E_UNSUPPORTED wins;
  - the pairs and the either-or pointers of EXTRA.
No call reaches a device: see the test's docstring.  The table is recorded ONCE, from the library before the host layer's
refusals were restated; to regenerate it is to give up what it pins.
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
import lipmpc  # noqa: E402
import test_field_refusals_build as T  # noqa: E402

E_ARG = -1
PROBES = [-1, 0, 1, 2, 4, 5, 8, 9, 16, 17, 64, 65, 4096, 4097, 65536, 65537, 1 << 30, (1 << 30) + 1, (1 << 31) - 1]
SHAPES = [(1, 8), (8, 1), (2, 2), (92, 80), (363, 362), (4096, 4096), (4097, 2), (2, 4097), (65281, 257)]
CROSSED = [(4097, 2), (363, 362)]
BIG = 1 << 40
# a legal value of every scalar of the field calls (F of a path call: one shared field)
LEGAL = dict(W=92, H=80, F=1, grid_shared=1, r_inflate=0, t_free=1, t_occ=3, min_unknown=2, max_seg=5, S_max=1, r_claim=4, max_claims=2,
             r_keep=2, keep_ratio16=16, keep_slack=0, r_view=8, w_gain=16, g_cap=64, min_gain=0, max_rounds=1, resume=0, r_clear=2,
             w_clear=8, work_bytes=BIG)
# the clearance call takes occ or evidence, never both: the base call has occ
BASE_POINTERS = {"lipmpc_grid_clearance_cost_batch": {"evidence": None}}
# limits that one scalar alone cannot reach, and pointers that are required only beside another
LAUNCH_PAIRS = [dict(max_claims=a, max_rounds=b) for a, b in ((4096, 256), (4096, 257), (16, 65536), (17, 65536), (0, 65536))]
EXTRA = {
    "lipmpc_grid_clearance_cost_batch": [dict(occ=None, evidence=8), dict(occ=None), dict(evidence=8)]
                                        + [dict(occ=None, evidence=8, t_occ=v) for v in PROBES],
    "lipmpc_grid_path_wave_batch": [dict(cost=None, settled=None)],
    "lipmpc_grid_frontier_path_wave_batch": [dict(cost=None, settled=None)],
    "lipmpc_grid_frontier_assign_robot_fields_batch": [dict(prev_target=None, kept=None), dict(prev_target=None, n_kept=None),
                                                       dict(prev_target=None, kept=None, n_kept=None)],
}


def bytes_call(name):
    own = name.replace("_batch", "_workspace_bytes")
    return own if own in lipmpc._lib.SIGNATURES else "lipmpc_grid_tiled_workspace_bytes"


def changes_of(name):
    """The changes of one entry point, without the crossings."""
    params = lipmpc._lib.SIGNATURES[name][1]
    names = [n for n, _ in params]
    count = T.count_of(name)
    scalars = [n for n, t in params if not T.is_pointer(t) and n != "device"]
    pointers = [n for n, t in params if T.is_pointer(t) and n not in ("origin", "cell", "hip_stream")]
    probes = [{n: v} for n in scalars for v in PROBES]
    if "B" in names and "F" in names:
        probes += [dict(B=v, F=v) for v in PROBES]
    drops = [{p: None} for p in pointers if BASE_POINTERS.get(name, {}).get(p, 8) is not None]
    misaligned = [{p: 12} for p in pointers if p not in T.HOST_OUTPUTS]
    shapes = [dict(W=w, H=h) for w, h in SHAPES] if "W" in names else []
    placements = [dict(placement=p) for p in T.PLACEMENTS if p != "ok"] if "origin" in names else []
    extra = list(EXTRA.get(name, [])) + (LAUNCH_PAIRS if "max_claims" in names and "max_rounds" in names else [])
    sizes = []
    if "work_bytes" in names:
        size_params = [n for n, _ in lipmpc._lib.SIGNATURES[bytes_call(name)][1]]
        for k in T.COUNTS:
            need = T.raw_call(bytes_call(name), **{n: k if n == count else LEGAL[n] for n in size_params})
            assert need > 0, (name, need)
            sizes += [{count: k, "work_bytes": v} for v in (0, need - 1, need, BIG)]
    return probes, drops, misaligned, shapes, placements, extra, sizes


def record(name):
    params = lipmpc._lib.SIGNATURES[name][1]
    count = T.count_of(name)
    base = {n: LEGAL[n] for n, t in params if not T.is_pointer(t) and n not in ("device", count)}
    base.update(BASE_POINTERS.get(name, {}))
    if "origin" in [n for n, _ in params]:
        base["placement"] = "ok"

    def returned(change):
        if count is None or count in change:
            return [T.call_case(name, base, change)]
        return [T.call_case(name, base, dict(change, **{count: k})) for k in T.COUNTS]

    probes, drops, misaligned, shapes, placements, extra, sizes = changes_of(name)
    by_change = {}                                          # (in the order added: a change is recorded once)

    def add(change):
        return by_change.setdefault(json.dumps(change, sort_keys=True), [change] + returned(change))

    add({})
    refused = []
    for change in probes + placements:
        if E_ARG in add(change)[1:]:
            refused.append(change)
    for change in drops:
        add(change)
        refused.append(change)
    for change in misaligned + shapes + extra + sizes:
        add(change)
    if "W" in base:
        for change in refused:
            if "W" not in change and "H" not in change:
                for w, h in CROSSED:
                    add(dict(change, W=w, H=h))
    return {"base": base, "tables": tables_of(by_change.values())}


def tables_of(rows):
    """Rows [change, returned...] as tables [keys, fixed, rows]: one table per set of changed arguments, a crossing's shape in `fixed`."""
    tables = {}
    for change, *returned in rows:
        fixed = {"W": change["W"], "H": change["H"]} if len(change) > 2 and "W" in change and "H" in change else {}
        keys = [k for k in change if k not in fixed]
        tables.setdefault(json.dumps([keys, fixed]), [keys, fixed, []])[2].append([change[k] for k in keys] + returned)
    for t in tables.values():
        if len(t[0]) == 1 and [r[0] for r in t[2]] == PROBES and len({len(r) for r in t[2]}) == 1:
            t[2] = ["probes"] + [r[1:] for r in t[2]]
    return list(tables.values())


def main():
    table = {name: record(name) for name in T.field_entry_points()}
    with open(T.TABLE, "w") as fh:
        fh.write('{"probes": ' + json.dumps(PROBES) + ', "calls": {\n' + ",\n".join(
            json.dumps(name) + ': {"base": ' + json.dumps(e["base"]) + ', "tables": [\n'
            + ",\n".join(json.dumps(t, separators=(",", ":")) for t in e["tables"]) + "\n]}" for name, e in table.items()) + "\n}}\n")
    print(f"{len(table)} entry points, {os.path.getsize(T.TABLE)} bytes")


if __name__ == "__main__":
    main()
