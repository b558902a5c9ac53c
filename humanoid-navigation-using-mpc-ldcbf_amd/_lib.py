"""ctypes binding of liblipmpc.so (C ABI: include/lipmpc.h).  There is no CPU fallback: if the
HIP library is missing this module raises at import of the solver."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblipmpc.so")


class LipmpcRrtParamsC(C.Structure):
    """struct lipmpc_rrt_params (include/lipmpc.h)"""
    _fields_ = [("width", C.c_int32), ("n_samples", C.c_int32), ("r_rewire", C.c_int32), ("max_cells", C.c_int32),
                ("margin", C.c_double)]


class LipmpcParamsC(C.Structure):
    """struct lipmpc_params (include/lipmpc.h)"""
    _fields_ = [
        ("N", C.c_int32), ("n_obs_max", C.c_int32), ("v_max", C.c_int32), ("max_iter", C.c_int32),
        ("flags", C.c_int32), ("finish_rounds", C.c_int32),
        ("dt", C.c_double), ("g", C.c_double), ("h_com", C.c_double), ("alpha", C.c_double),
        ("l_max", C.c_double * 2), ("l_min", C.c_double * 2), ("v_min", C.c_double * 2),
        ("v_max_xy", C.c_double * 2),
        ("omega_max", C.c_double), ("ell", C.c_double), ("sampling_time", C.c_double),
        ("tol", C.c_double), ("tol_interior", C.c_double), ("k0_tol", C.c_double),
    ]


_TYPES = {"ptr": C.c_void_p, "int": C.c_int, "i32": C.c_int32, "i64": C.c_int64, "f64": C.c_double,
          "params": C.POINTER(LipmpcParamsC), "rrt_params": C.POINTER(LipmpcRrtParamsC), "handle_out": C.POINTER(C.c_void_p)}


def _sig(restype, params):
    """(restype, ((name, ctype), ...)) from 'name name:type ...' in the order of the prototype: a bare name is a pointer
    (c_void_p: a handle, a device buffer, the stream), ':type' a key of _TYPES."""
    return restype, tuple((n, _TYPES[t or "ptr"]) for n, _, t in (p.partition(":") for p in params.split()))


_STEP_OUT = "U X theta omega obj status iters active working"
_GRID_SCAN = "resolution:i32 W:i32 H:i32 grid_shared:i32 origin cell lidar_range:f64 eps:f64 min_samples:i32"
_SCAN = "resolution:i32 n_env:i32 v_env:i32 env_shared:i32 lidar_range:f64 eps:f64 min_samples:i32"
_ASSIGN = ("device:int B:i64 W:i32 H:i32 origin cell frontier field start may_claim r_inflate:i32 r_claim:i32 max_claims:i32 max_seg:i32 "
           "S_max:i32 work sub_goals n_sub status path_cost target_cell claim_round n_claims")
_ASSIGN_TILED = ("device:int B:i64 W:i32 H:i32 origin cell frontier field settled start may_claim r_inflate:i32 r_claim:i32 max_claims:i32 "
                 "max_seg:i32 S_max:i32 work work_bytes:i64 max_rounds:i32 sub_goals n_sub status path_cost target_cell claim_round n_claims "
                 "claims_settled")
_ASSIGN_KEEP = ("device:int B:i64 W:i32 H:i32 origin cell frontier field start may_claim prev_target r_inflate:i32 r_claim:i32 r_keep:i32 "
                "keep_ratio16:i32 keep_slack:i32 max_claims:i32 max_seg:i32 S_max:i32 work sub_goals n_sub status path_cost target_cell "
                "claim_round n_claims kept n_kept")
_ASSIGN_KEEP_TILED = ("device:int B:i64 W:i32 H:i32 origin cell frontier field settled start may_claim prev_target r_inflate:i32 r_claim:i32 "
                      "r_keep:i32 keep_ratio16:i32 keep_slack:i32 max_claims:i32 max_seg:i32 S_max:i32 work work_bytes:i64 max_rounds:i32 "
                      "sub_goals n_sub status path_cost target_cell claim_round n_claims kept n_kept claims_settled")

# Every export of include/lipmpc.h with the header's own parameter names: the ONE statement of each argument list on the
# Python side.  load() binds restype / argtypes from it, call() takes its arguments by these names, and
# tests/test_abi_and_c_oracle.py holds it to the prototypes (return type, count, names, order, type of every parameter).
SIGNATURES = {
    "lipmpc_default_params": _sig(C.c_int, "p:params"),
    "lipmpc_create": _sig(C.c_int, "p:params device:int out:handle_out"),
    "lipmpc_destroy": _sig(None, "h"),
    "lipmpc_num_rows": _sig(C.c_int64, "p:params"),
    "lipmpc_active_words": _sig(C.c_int64, "p:params"),
    "lipmpc_plan_step_batch": _sig(C.c_int, f"h B:i64 state goal first_foot delta obs_xy obs_nv {_STEP_OUT} c_eta diag bounds hip_stream"),
    "lipmpc_set_schedule": _sig(C.c_int, "h schedule capacity:i64"),
    "lipmpc_schedule_words": _sig(C.c_int64, "B:i64"),
    "lipmpc_set_warm_start": _sig(C.c_int, "h record capacity:i64"),
    "lipmpc_warm_words": _sig(C.c_int64, "p:params"),
    "lipmpc_workspace_bytes": _sig(C.c_int64, "h capacity:i64"),
    "lipmpc_set_workspace": _sig(C.c_int, "h workspace capacity:i64"),
    "lipmpc_plan_step_batch_c_eta": _sig(C.c_int, f"h B:i64 state goal first_foot delta c_eta_in overflow {_STEP_OUT} diag bounds hip_stream"),
    "lipmpc_advance_batch": _sig(C.c_int, "h B:i64 state first_foot U theta status hip_stream"),
    "lipmpc_fleet_update_batch": _sig(C.c_int, "h B:i64 k_max:i32 stop_obj:f64 state first_foot walking last_obj n_steps last_status n_overflow "
                                               "sample X_pred U_pred U theta omega obj status overflow hip_stream"),
    "lipmpc_fleet_recover_update_batch": _sig(C.c_int, "h B:i64 k_max:i32 stop_obj:f64 state first_foot walking last_obj n_steps last_status "
                                                       "n_overflow sample X_pred U_pred U theta omega obj status overflow goal c_eta delta "
                                                       "max_recover:i32 recover_run n_recover recover_margin hip_stream"),
    "lipmpc_rollout_batch": _sig(C.c_int, "h B:i64 k_max:i32 mpc_step:i32 stop_obj:f64 state0 goal first_foot delta obs_xy obs_nv "
                                          "X_pred U_pred n_steps last_status total_iters bounds hip_stream"),
    "lipmpc_lidar_sense_batch": _sig(C.c_int, f"device:int B:i64 {_SCAN} n_obs_max:i32 v_max:i32 state env_xy env_nv ray_table noise "
                                              "obs_xy obs_nv n_inferred overflow hits labels hip_stream"),
    "lipmpc_lidar_c_eta_batch": _sig(C.c_int, f"device:int B:i64 {_SCAN} n_obs_max:i32 v_max:i32 state env_xy env_nv ray_table noise "
                                              "c_eta n_inferred overflow obs_xy obs_nv hits labels schedule hip_stream"),
    "lipmpc_lidar_schedule_words": _sig(C.c_int64, "B:i64"),
    "lipmpc_sense_plan_step_batch": _sig(C.c_int, f"h B:i64 {_SCAN} state goal first_foot delta env_xy env_nv ray_table noise "
                                                  f"c_eta n_inferred overflow schedule {_STEP_OUT} diag bounds hip_stream"),
    "lipmpc_lidar_grid_c_eta_batch": _sig(C.c_int, f"device:int B:i64 {_GRID_SCAN} n_obs_max:i32 v_max:i32 state occ ray_table noise "
                                                   "c_eta n_inferred overflow obs_xy obs_nv hits labels hip_stream"),
    "lipmpc_lidar_c_eta_split_batch": _sig(C.c_int, f"device:int B:i64 {_SCAN} n_obs_max:i32 v_max:i32 state env_xy env_nv ray_table noise "
                                                    "c_eta n_inferred overflow obs_xy obs_nv hits labels schedule split_rays:i32 pieces hip_stream"),
    "lipmpc_lidar_grid_c_eta_split_batch": _sig(C.c_int, f"device:int B:i64 {_GRID_SCAN} n_obs_max:i32 v_max:i32 state occ ray_table noise "
                                                         "c_eta n_inferred overflow obs_xy obs_nv hits labels split_rays:i32 pieces hip_stream"),
    "lipmpc_sense_grid_plan_step_batch": _sig(C.c_int, f"h B:i64 {_GRID_SCAN} state goal first_foot delta occ ray_table noise "
                                                       f"c_eta n_inferred overflow {_STEP_OUT} diag bounds hip_stream"),
    "lipmpc_rrt_default_params": _sig(C.c_int, "p:rrt_params"),
    "lipmpc_rrt_workspace_bytes": _sig(C.c_int64, "p:rrt_params B:i64"),
    "lipmpc_rrt_plan_batch": _sig(C.c_int, "device:int p:rrt_params B:i64 obs_xy obs_nv n_obs_max:i32 v_max:i32 start goal seed workspace "
                                           "sub_goals n_sub status path_cost grid_dims occ_d2 cost_grid tree S_max:i32 hip_stream"),
    "lipmpc_rrt_plan_grid_batch": _sig(C.c_int, "device:int p:rrt_params B:i64 W:i32 H:i32 grid_shared:i32 origin cell occ start goal seed workspace "
                                                "sub_goals n_sub status path_cost grid_dims occ_d2 cost_grid tree S_max:i32 hip_stream"),
    "lipmpc_grid_field_batch": _sig(C.c_int, "device:int F:i64 W:i32 H:i32 grid_shared:i32 origin cell occ goal r_inflate:i32 field field_status "
                                             "hip_stream"),
    "lipmpc_grid_path_batch": _sig(C.c_int, "device:int B:i64 F:i64 W:i32 H:i32 origin cell occ grid_shared:i32 field field_status goal start "
                                            "r_inflate:i32 max_seg:i32 S_max:i32 sub_goals n_sub status path_cost hip_stream"),
    "lipmpc_grid_frontier_field_batch": _sig(C.c_int, "device:int F:i64 W:i32 H:i32 evidence t_free:i32 t_occ:i32 r_inflate:i32 min_unknown:i32 "
                                                      "frontier field n_frontier hip_stream"),
    "lipmpc_grid_frontier_path_batch": _sig(C.c_int, "device:int B:i64 F:i64 W:i32 H:i32 origin cell evidence t_occ:i32 field n_frontier start "
                                                     "r_inflate:i32 max_seg:i32 S_max:i32 sub_goals n_sub status path_cost target_cell hip_stream"),
    "lipmpc_grid_frontier_assign_batch": _sig(C.c_int, f"{_ASSIGN} hip_stream"),
    "lipmpc_grid_frontier_assign_utility_batch": _sig(C.c_int, f"{_ASSIGN} gain w_gain:i32 g_cap:i32 min_gain:i32 target_gain hip_stream"),
    "lipmpc_grid_frontier_assign_keep_batch": _sig(C.c_int, f"{_ASSIGN_KEEP} hip_stream"),
    "lipmpc_grid_frontier_assign_keep_utility_batch": _sig(C.c_int, f"{_ASSIGN_KEEP} gain ufield w_gain:i32 g_cap:i32 min_gain:i32 "
                                                                    "target_gain hip_stream"),
    "lipmpc_grid_frontier_gain_batch": _sig(C.c_int, "device:int F:i64 W:i32 H:i32 evidence t_free:i32 t_occ:i32 frontier r_view:i32 gain "
                                                     "hip_stream"),
    "lipmpc_grid_frontier_utility_field_batch": _sig(C.c_int, "device:int F:i64 W:i32 H:i32 frontier field gain w_gain:i32 g_cap:i32 "
                                                              "min_gain:i32 ufield n_sources hip_stream"),
    "lipmpc_grid_frontier_utility_path_batch": _sig(C.c_int, "device:int B:i64 F:i64 W:i32 H:i32 origin cell evidence t_occ:i32 frontier gain "
                                                             "ufield n_sources w_gain:i32 g_cap:i32 min_gain:i32 start r_inflate:i32 "
                                                             "max_seg:i32 S_max:i32 sub_goals n_sub status path_cost target_cell target_gain "
                                                             "hip_stream"),
    "lipmpc_grid_tiled_info": _sig(C.c_int, "tile_w tile_h max_cells"),
    "lipmpc_grid_tiled_workspace_bytes": _sig(C.c_int64, "F:i64 W:i32 H:i32"),
    "lipmpc_grid_field_tiled_batch": _sig(C.c_int, "device:int F:i64 W:i32 H:i32 grid_shared:i32 origin cell occ goal r_inflate:i32 field "
                                                   "field_status work work_bytes:i64 max_rounds:i32 resume:i32 settled hip_stream"),
    "lipmpc_grid_frontier_field_tiled_batch": _sig(C.c_int, "device:int F:i64 W:i32 H:i32 evidence t_free:i32 t_occ:i32 r_inflate:i32 "
                                                            "min_unknown:i32 frontier field n_frontier work work_bytes:i64 max_rounds:i32 "
                                                            "resume:i32 settled hip_stream"),
    "lipmpc_grid_path_tiled_batch": _sig(C.c_int, "device:int B:i64 F:i64 W:i32 H:i32 origin cell occ grid_shared:i32 field field_status "
                                                  "settled goal start r_inflate:i32 max_seg:i32 S_max:i32 sub_goals n_sub status path_cost "
                                                  "hip_stream"),
    "lipmpc_grid_frontier_path_tiled_batch": _sig(C.c_int, "device:int B:i64 F:i64 W:i32 H:i32 origin cell evidence t_occ:i32 field "
                                                           "n_frontier settled start r_inflate:i32 max_seg:i32 S_max:i32 sub_goals n_sub "
                                                           "status path_cost target_cell hip_stream"),
    "lipmpc_grid_clearance_cost_batch": _sig(C.c_int, "device:int M:i64 W:i32 H:i32 occ evidence t_occ:i32 r_clear:i32 w_clear:i32 cost "
                                                      "hip_stream"),
    "lipmpc_grid_field_weighted_batch": _sig(C.c_int, "device:int F:i64 W:i32 H:i32 grid_shared:i32 origin cell occ cost goal r_inflate:i32 "
                                                      "field field_status work work_bytes:i64 max_rounds:i32 resume:i32 settled hip_stream"),
    "lipmpc_grid_frontier_field_weighted_batch": _sig(C.c_int, "device:int F:i64 W:i32 H:i32 evidence cost t_free:i32 t_occ:i32 "
                                                               "r_inflate:i32 min_unknown:i32 frontier field n_frontier work "
                                                               "work_bytes:i64 max_rounds:i32 resume:i32 settled hip_stream"),
    "lipmpc_grid_path_weighted_batch": _sig(C.c_int, "device:int B:i64 F:i64 W:i32 H:i32 origin cell occ grid_shared:i32 cost field "
                                                     "field_status settled goal start r_inflate:i32 max_seg:i32 S_max:i32 sub_goals n_sub "
                                                     "status path_cost hip_stream"),
    "lipmpc_grid_frontier_path_weighted_batch": _sig(C.c_int, "device:int B:i64 F:i64 W:i32 H:i32 origin cell evidence cost t_occ:i32 field "
                                                              "n_frontier settled start r_inflate:i32 max_seg:i32 S_max:i32 sub_goals "
                                                              "n_sub status path_cost target_cell hip_stream"),
    "lipmpc_grid_frontier_gain_tiled_lds_bytes": _sig(C.c_int64, "r_view:i32"),
    "lipmpc_grid_frontier_gain_tiled_batch": _sig(C.c_int, "device:int F:i64 W:i32 H:i32 evidence t_free:i32 t_occ:i32 frontier r_view:i32 "
                                                           "gain hip_stream"),
    "lipmpc_grid_frontier_utility_field_tiled_batch": _sig(C.c_int, "device:int F:i64 W:i32 H:i32 evidence t_free:i32 t_occ:i32 r_inflate:i32 "
                                                                    "frontier gain w_gain:i32 g_cap:i32 min_gain:i32 ufield n_sources work "
                                                                    "work_bytes:i64 max_rounds:i32 resume:i32 settled hip_stream"),
    "lipmpc_grid_frontier_utility_path_tiled_batch": _sig(C.c_int, "device:int B:i64 F:i64 W:i32 H:i32 origin cell evidence t_occ:i32 frontier "
                                                                   "gain ufield n_sources settled w_gain:i32 g_cap:i32 min_gain:i32 start "
                                                                   "r_inflate:i32 max_seg:i32 S_max:i32 sub_goals n_sub status path_cost "
                                                                   "target_cell target_gain hip_stream"),
    "lipmpc_grid_frontier_assign_tiled_workspace_bytes": _sig(C.c_int64, "W:i32 H:i32"),
    "lipmpc_grid_frontier_assign_tiled_batch": _sig(C.c_int, f"{_ASSIGN_TILED} hip_stream"),
    "lipmpc_grid_frontier_assign_utility_tiled_workspace_bytes": _sig(C.c_int64, "W:i32 H:i32"),
    "lipmpc_grid_frontier_assign_utility_tiled_batch": _sig(C.c_int, f"{_ASSIGN_TILED} gain w_gain:i32 g_cap:i32 min_gain:i32 target_gain "
                                                                     "hip_stream"),
    "lipmpc_grid_frontier_assign_keep_tiled_workspace_bytes": _sig(C.c_int64, "W:i32 H:i32"),
    "lipmpc_grid_frontier_assign_keep_tiled_batch": _sig(C.c_int, f"{_ASSIGN_KEEP_TILED} hip_stream"),
    "lipmpc_grid_frontier_assign_keep_utility_tiled_workspace_bytes": _sig(C.c_int64, "W:i32 H:i32"),
    "lipmpc_grid_frontier_assign_keep_utility_tiled_batch": _sig(C.c_int, f"{_ASSIGN_KEEP_TILED} gain ufield usettled w_gain:i32 g_cap:i32 "
                                                                          "min_gain:i32 target_gain hip_stream"),
    # claims from per-robot fields: the keep call's argument list with `resume` after max_rounds; prev_target, kept, n_kept nullable
    "lipmpc_grid_frontier_assign_robot_fields_workspace_bytes": _sig(C.c_int64, "B:i64 W:i32 H:i32"),
    "lipmpc_grid_frontier_assign_robot_fields_batch": _sig(C.c_int, _ASSIGN_KEEP_TILED.replace("max_rounds:i32", "max_rounds:i32 resume:i32")
                                                           + " hip_stream"),
    # the wave-per-robot path calls: the weighted / tiled-utility calls' argument lists, cost and settled nullable
    "lipmpc_grid_path_wave_batch": _sig(C.c_int, "device:int B:i64 F:i64 W:i32 H:i32 origin cell occ grid_shared:i32 cost field "
                                                 "field_status settled goal start r_inflate:i32 max_seg:i32 S_max:i32 sub_goals n_sub "
                                                 "status path_cost hip_stream"),
    "lipmpc_grid_frontier_path_wave_batch": _sig(C.c_int, "device:int B:i64 F:i64 W:i32 H:i32 origin cell evidence cost t_occ:i32 field "
                                                          "n_frontier settled start r_inflate:i32 max_seg:i32 S_max:i32 sub_goals "
                                                          "n_sub status path_cost target_cell hip_stream"),
    "lipmpc_grid_frontier_utility_path_wave_batch": _sig(C.c_int, "device:int B:i64 F:i64 W:i32 H:i32 origin cell evidence t_occ:i32 frontier "
                                                                  "gain ufield n_sources settled w_gain:i32 g_cap:i32 min_gain:i32 start "
                                                                  "r_inflate:i32 max_seg:i32 S_max:i32 sub_goals n_sub status path_cost "
                                                                  "target_cell target_gain hip_stream"),
    # frontier regions: connected frontier cells, their sizes and a table of the kept ones (rep and, with R_max == 0, table nullable)
    "lipmpc_grid_frontier_regions_workspace_bytes": _sig(C.c_int64, "F:i64 W:i32 H:i32 R_max:i32"),
    "lipmpc_grid_frontier_regions_batch": _sig(C.c_int, "device:int F:i64 W:i32 H:i32 frontier min_size:i32 R_max:i32 work work_bytes:i64 "
                                                        "label size rep table n_regions hip_stream"),
    "lipmpc_map_update_batch": _sig(C.c_int, "device:int B:i64 resolution:i32 W:i32 H:i32 grid_shared:i32 origin cell lidar_range:f64 depth:f64 "
                                             "w_hit:i32 w_miss:i32 state hits ray_table mask evidence hip_stream"),
    "lipmpc_scan_match_batch": _sig(C.c_int, "device:int B:i64 resolution:i32 W:i32 H:i32 grid_shared:i32 origin cell lidar_range:f64 depth:f64 "
                                             "n_x:i32 n_y:i32 n_yaw:i32 rot_table clamp:i32 min_score:i32 min_gain:i32 state hits mask evidence "
                                             "offset_cells yaw_index offset score n_used matched hip_stream"),
    "lipmpc_neighbour_workspace_bytes": _sig(C.c_int64, "B:i64"),
    "lipmpc_neighbour_c_eta_batch": _sig(C.c_int, "device:int B:i64 n_obs_max:i32 k_rows:i32 sense_range:f64 share:f64 state radius group "
                                                  "first_slot workspace c_eta n_rows n_near neighbours hip_stream"),
    "lipmpc_strerror": _sig(C.c_char_p, "code:int"),
    "lipmpc_version": _sig(C.c_int, ""),
}
EXPORTS = tuple(SIGNATURES)

ABI_VERSION = 5          # LIPMPC_ABI_VERSION of include/lipmpc.h this binding is written for
VARIANT_BASE = 1000      # LIPMPC_VARIANT_BASE: instrumented development builds report ABI_VERSION + this
DIAG_WORDS = 8           # LIPMPC_DIAG_WORDS
TIGHT_TOL = 1e-7         # LIPMPC_TIGHT_TOL

_lib = None
_bound = {}              # name -> (bound function, ((parameter name, is a c_void_p), ...)): what call() needs, resolved once by load()
_ADDRESSES = {type(None), int, C.c_void_p}       # what call() hands to a c_void_p parameter as it is: NULL, the stream, the handle


def load():
    """Load the shared library (once).  Raises RuntimeError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    # LIPMPC_LIB: another build of the same library (dev tools only: the instrumented / historical variants of tools/*.sh
    # are loaded from their own path instead of being copied over the shipped file)
    path = os.environ.get("LIPMPC_LIB") or LIB_PATH
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} not found: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()' or make -C <package>/csrc)")
    lib = C.CDLL(path)
    # SIGNATURES holds the argument lists of ONE ABI version: a stale or historical build (LIPMPC_LIB) would take every
    # pointer after an inserted argument shifted by one, and an instrumented variant (version >= LIPMPC_VARIANT_BASE) writes
    # other buffer shapes.  Refuse both here, before any pointer is handed over; tools that drive a variant on purpose set
    # LIPMPC_ALLOW_VARIANT=1 and hand in the buffers that variant expects.
    ver = int(lib.lipmpc_version())
    if ver != ABI_VERSION and not (ver == ABI_VERSION + VARIANT_BASE and os.environ.get("LIPMPC_ALLOW_VARIANT") == "1"):
        raise RuntimeError(f"{path}: lipmpc_version() = {ver}, this binding is written for ABI {ABI_VERSION} "
                           f"(include/lipmpc.h); rebuild the library (make -C <package>/csrc)")
    for name, (restype, params) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, [t for _, t in params]
        _bound[name] = fn, tuple((n, t is C.c_void_p) for n, t in params)
    _lib = lib
    return lib


def check(code, what):
    if code != 0:
        err = RuntimeError(f"{what} failed: {load().lipmpc_strerror(code).decode()} ({code})")
        err.code = code
        raise err


def call(name, **args):
    """Call an entry point that returns a status, every argument given by the header's parameter name (SIGNATURES), exactly
    once: a missing or an unknown name is a TypeError before anything is enqueued.  Pointer parameters take a tensor (its
    data_ptr()), None (NULL) or an address (the handle, the stream); the others go through their ctype.  A non-zero status raises
    check()'s RuntimeError, the code in its ``code`` attribute."""
    if _lib is None:
        load()
    fn, params = _bound[name]
    try:
        argv = [v.data_ptr() if is_ptr and v.__class__ not in _ADDRESSES else v for n, is_ptr in params for v in (args[n],)]
    except KeyError as e:
        raise TypeError(f"{name}: argument {e.args[0]!r} missing") from None
    if len(args) != len(argv):
        raise TypeError(f"{name}: no such argument {sorted(set(args) - {n for n, _ in params})}")
    rc = fn(*argv)
    if rc != 0:
        check(rc, name)
