"""ctypes binding of libpsfm_hip.so (include/psfm.h).

The HIP library is the product; there is NO CPU fallback.  If the library is missing, or there is
no GPU, every compute entry point raises -- loudly -- instead of silently computing elsewhere.
"""
import ctypes
import os

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("PSFM_HIP_LIB", os.path.join(_PKG, "lib", "libpsfm_hip.so"))

PSFM_OK, PSFM_ERR_ARG, PSFM_ERR_HIP, PSFM_ERR_CAPACITY, PSFM_ERR_SOLVER = 0, 1, 2, 3, 4
PROF_KINDS = {"flow_check": 0, "chain_step": 1, "respawn": 2, "solver": 3, "finalize": 4}

EXPORTS = [
    "psfm_last_error", "psfm_version", "psfm_device_count", "psfm_ctx_create", "psfm_ctx_destroy",
    "psfm_ctx_set_capacity", "psfm_flow_check", "psfm_grid_sample", "psfm_optimize_location", "psfm_track",
    "psfm_connect",
    "psfm_result_device", "psfm_result_copy", "psfm_result_solve_stats", "psfm_ctx_set_profiling",
    "psfm_profile_get", "psfm_ctx_set_chain_mode", "psfm_window_sample", "psfm_result_filter", "psfm_result_filtered_copy",
    "psfm_ctx_set_solver", "psfm_solver_counters", "psfm_traj_to_matches", "psfm_matches_copy",
    "psfm_shard_begin", "psfm_shard_step", "psfm_shard_solve_export", "psfm_shard_solve_control", "psfm_shard_solve_restore",
    "psfm_shard_solve_writeback", "psfm_shard_solve_record", "psfm_shard_finish", "psfm_result_keys",
    "psfm_shard_solve_control_async", "psfm_shard_window_state", "psfm_shard_peek_stall", "psfm_shard_frame",
    "psfm_shard_solve_control_chain_async", "psfm_shard_solve_poll", "psfm_shard_solve_local", "psfm_shard_solve_redo_local", "psfm_connect_batch", "psfm_solver_launches", "psfm_ctx_set_resident_budget", "psfm_resident_capacity", "psfm_load_flo_stack",
    "psfm_path_consistency_eval", "psfm_sort_records", "psfm_sort_records64", "psfm_ctx_get_finalize_forms", "psfm_ctx_get_finalize_placed",
    "psfm_shard_peer_area", "psfm_shard_peer_epoch", "psfm_shard_peer_open", "psfm_shard_peer_connect", "psfm_shard_solve_blocks", "psfm_shard_solve_peer",
    "psfm_labels_begin", "psfm_labels_merge_window", "psfm_labels_finish", "psfm_labels_device", "psfm_labels_copy", "psfm_labels_to_matches",
    "psfm_traj_augment", "psfm_traj_encode_weight_count", "psfm_traj_encode",
    "psfm_traj_decode_weight_count", "psfm_traj_decode_workspace_bytes", "psfm_traj_decode",
    "psfm_traj_decode_batch_workspace_bytes", "psfm_traj_decode_batch",
    "psfm_window_sample_batch", "psfm_traj_augment_batch", "psfm_traj_encode_batch",
    "psfm_traj_eval_counts", "psfm_traj_vote_labels",
    "psfm_labels_set", "psfm_matches_to_database", "psfm_database_copy", "psfm_database_chunk_rows",
    "psfm_database_compact_again",
    "psfm_sparse_depth", "psfm_sparse_depth_sort_ids", "psfm_ctx_set_sparse_depth", "psfm_ctx_get_sparse_depth_budget",
    "psfm_sparse_depth_last_ms", "psfm_colmap_points3d_count", "psfm_colmap_points3d_scan",
    "psfm_ctx_set_motion_boundary", "psfm_motion_boundary", "psfm_kill_map", "psfm_kill_map_batch",
    "psfm_depth_display", "psfm_ctx_set_depth_display", "psfm_depth_display_last_ms", "psfm_depth_display_chunk",
    "psfm_track_queries", "psfm_track_queries_optimize",
    "psfm_result_filter_batch", "psfm_traj_to_matches_batch", "psfm_labels_to_matches_batch", "psfm_matches_batch_census", "psfm_labels_sizes",
    "psfm_track_queries_batch", "psfm_query_batch_census",
    "psfm_track_queries_optimize_batch", "psfm_query_pc_batch_census",
    "psfm_ctx_set_batch_redo", "psfm_connect_batch_census", "psfm_ctx_set_frame_size",
    "psfm_ctx_get_finalize_gather",
    "psfm_result_set", "psfm_load_track_npy",
]


class SolveStats(ctypes.Structure):
    _fields_ = [("iterations", ctypes.c_int32), ("successful_steps", ctypes.c_int32),
                ("termination", ctypes.c_int32), ("dogleg_nonGN", ctypes.c_int32),
                ("initial_cost", ctypes.c_double), ("final_cost", ctypes.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class TrackInfo(ctypes.Structure):
    _fields_ = [("n_traj", ctypes.c_int64), ("n_points", ctypes.c_int64), ("n_lanes_peak", ctypes.c_int64),
                ("lane_capacity", ctypes.c_int64), ("solver_iterations", ctypes.c_int64),
                ("n_solves", ctypes.c_int32), ("chain_mode", ctypes.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class PsfmError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("libpsfm_hip status %d: %s" % (status, msg))
        self.status = status


_lib = None


def lib():
    """Load libpsfm_hip.so; raises RuntimeError (never falls back) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "libpsfm_hip.so not found at %s -- build it with `python particle-sfm_amd/build.py` "
            "(the HIP extension is mandatory, there is no CPU fallback)" % LIB_PATH)
    # torch first: its bundled HIP runtime must be the one in the process.  Loaded before torch, libpsfm_hip.so would pull
    # the system libamdhip64 in, torch would add its own copy, and the two runtimes do not see each other's devices.
    import torch  # noqa: F401
    L = ctypes.CDLL(LIB_PATH)
    vp, i32, i64, f32, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double
    L.psfm_last_error.restype = ctypes.c_char_p
    L.psfm_last_error.argtypes = []
    L.psfm_version.restype = i32
    L.psfm_device_count.restype = i32
    L.psfm_ctx_create.argtypes = [i32, ctypes.POINTER(vp)]
    L.psfm_ctx_destroy.argtypes = [vp]
    L.psfm_ctx_set_capacity.argtypes = [vp, f64, f64]
    L.psfm_load_flo_stack.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p), i32, i32, i32, vp, i32, vp]
    L.psfm_flow_check.argtypes = [vp, vp, vp, i32, i32, i32, f32, vp, vp, vp]
    L.psfm_grid_sample.argtypes = [vp, vp, i32, i32, i32, vp, i64, vp, vp]
    L.psfm_optimize_location.argtypes = [vp, vp, vp, vp, vp, vp, i64, i32, i32, vp, ctypes.POINTER(SolveStats), vp]
    L.psfm_path_consistency_eval.argtypes = [vp, vp, vp, vp, vp, vp, i64, i32, i32, vp, vp, vp]
    L.psfm_sort_records.argtypes = [vp, vp, vp, i64, i32, vp]
    L.psfm_sort_records64.argtypes = [vp, vp, vp, i64, i32, vp]
    L.psfm_ctx_get_finalize_forms.argtypes = [vp, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]
    L.psfm_ctx_get_finalize_placed.argtypes = [vp, ctypes.POINTER(ctypes.c_int32)]
    L.psfm_ctx_get_finalize_gather.argtypes = [vp, ctypes.POINTER(ctypes.c_int32)]
    L.psfm_track.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, ctypes.POINTER(TrackInfo), vp]
    L.psfm_connect.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, f32, i32, vp, vp, ctypes.POINTER(TrackInfo), vp]
    L.psfm_connect_batch.argtypes = [ctypes.POINTER(vp), i32, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp),
                                     ctypes.POINTER(i32), i32, i32, f32, i32, ctypes.POINTER(TrackInfo), vp]
    L.psfm_ctx_set_batch_redo.argtypes = [vp, i32]
    L.psfm_ctx_set_frame_size.argtypes = [vp, i32, i32]
    L.psfm_connect_batch_census.argtypes = [vp] + [ctypes.POINTER(ctypes.c_int32)] * 5
    L.psfm_track_queries.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, i64, ctypes.POINTER(TrackInfo), vp]
    L.psfm_track_queries_optimize.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, i64, ctypes.POINTER(TrackInfo), vp]
    L.psfm_track_queries_batch.argtypes = [ctypes.POINTER(vp), i32, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp),
                                           ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(vp), ctypes.POINTER(vp),
                                           ctypes.POINTER(i64), ctypes.POINTER(TrackInfo), vp]
    L.psfm_query_batch_census.argtypes = [vp, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]
    L.psfm_track_queries_optimize_batch.argtypes = [ctypes.POINTER(vp), i32] + [ctypes.POINTER(vp)] * 8 + [
        ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(i64),
        ctypes.POINTER(TrackInfo), vp]
    L.psfm_query_pc_batch_census.argtypes = [vp, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]
    L.psfm_result_device.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp)]
    L.psfm_result_copy.argtypes = [vp, vp, vp, vp, vp, vp]
    L.psfm_result_solve_stats.argtypes = [vp, ctypes.POINTER(SolveStats), i32, ctypes.POINTER(ctypes.c_int32)]
    L.psfm_ctx_set_profiling.argtypes = [vp, i32]
    L.psfm_ctx_set_chain_mode.argtypes = [vp, i32]
    L.psfm_ctx_set_solver.argtypes = [vp, i32, i32]
    L.psfm_ctx_set_motion_boundary.argtypes = [vp, i32, f32]
    L.psfm_motion_boundary.argtypes = [vp, vp, i32, i32, i32, f32, vp, vp]
    L.psfm_kill_map.argtypes = [vp, vp, vp, i32, i32, i32, f32, vp, vp]
    L.psfm_kill_map_batch.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(i32), i32, i32, i32, ctypes.POINTER(f32), i32, i32,
                                      ctypes.POINTER(vp), vp]
    L.psfm_solver_counters.argtypes = [vp, ctypes.POINTER(i64), ctypes.POINTER(i64), ctypes.POINTER(i64), ctypes.POINTER(ctypes.c_int32)]
    L.psfm_ctx_set_resident_budget.argtypes = [vp, i32]
    L.psfm_resident_capacity.argtypes = [vp, ctypes.POINTER(ctypes.c_int32)]
    L.psfm_solver_launches.argtypes = [vp, ctypes.POINTER(i64), ctypes.POINTER(i64), ctypes.POINTER(i64)]
    L.psfm_result_filter.argtypes = [vp, i32, ctypes.POINTER(i64), ctypes.POINTER(i64), vp]
    L.psfm_result_filtered_copy.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.psfm_result_set.argtypes = [vp, i64, i64, vp, vp, vp, vp, ctypes.POINTER(i64), vp]
    L.psfm_load_track_npy.argtypes = [vp, ctypes.c_char_p, vp, i32, vp, i32, ctypes.POINTER(i64), ctypes.POINTER(i64), ctypes.POINTER(i64), vp]
    L.psfm_window_sample.argtypes = [vp, i32, i32, i32, i32, i64, ctypes.c_uint64, i32, i32, i32, i32, i64, vp, vp, vp, vp,
                                     ctypes.POINTER(i64), vp]
    L.psfm_traj_augment.argtypes = [vp, vp, vp, vp, i64, i32, i32, i32, vp, vp, vp]
    L.psfm_traj_encode_weight_count.argtypes = []
    L.psfm_traj_encode.argtypes = [vp, vp, vp, vp, i64, i32, vp, vp]
    L.psfm_traj_decode_weight_count.argtypes = []
    L.psfm_traj_decode_workspace_bytes.argtypes = [i64]
    L.psfm_traj_decode.argtypes = [vp, vp, vp, i64, vp, ctypes.c_size_t, vp, vp, vp, vp]
    L.psfm_traj_decode_batch_workspace_bytes.argtypes = [ctypes.POINTER(i64), i32]
    L.psfm_traj_decode_batch.argtypes = [vp, i32, ctypes.POINTER(vp), ctypes.POINTER(i64), vp, vp, ctypes.c_size_t, ctypes.POINTER(vp),
                                         ctypes.POINTER(vp), ctypes.POINTER(vp), vp]
    L.psfm_window_sample_batch.argtypes = [vp, i32, ctypes.POINTER(i32), i32, i32, i32, i64, ctypes.POINTER(ctypes.c_uint64), i32, i32, i32, i32,
                                           i64, vp, vp, vp, vp, ctypes.POINTER(i64), vp]
    L.psfm_traj_augment_batch.argtypes = [vp, i32, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(i64), i32, i32, i32,
                                          vp, ctypes.POINTER(vp), vp]
    L.psfm_traj_encode_batch.argtypes = [vp, i32, ctypes.POINTER(vp), ctypes.POINTER(vp), vp, ctypes.POINTER(i64), i32, ctypes.POINTER(vp), vp]
    L.psfm_traj_eval_counts.argtypes = [vp, vp, vp, vp, i64, vp, vp, i32, i32, i32, vp, vp]
    L.psfm_traj_vote_labels.argtypes = [vp, vp, vp, vp, i64, i32, i32, i32, vp, vp]
    L.psfm_traj_to_matches.argtypes = [vp, i32, i32, vp, ctypes.POINTER(i64), ctypes.POINTER(i64), ctypes.POINTER(i64), vp]
    L.psfm_matches_copy.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    L.psfm_labels_begin.argtypes = [vp, vp]
    L.psfm_labels_merge_window.argtypes = [vp, i32, i32, vp, vp, i64, vp]
    L.psfm_labels_finish.argtypes = [vp, ctypes.POINTER(i64), ctypes.POINTER(i64), vp]
    L.psfm_labels_device.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp)]
    L.psfm_labels_copy.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.psfm_labels_to_matches.argtypes = [vp, i32, i32, i32, ctypes.POINTER(i64), ctypes.POINTER(i64), ctypes.POINTER(i64), vp]
    L.psfm_labels_set.argtypes = [vp, i64, i64, vp, vp, vp, vp, vp, vp]
    L.psfm_labels_sizes.argtypes = [vp, ctypes.POINTER(i64), ctypes.POINTER(i64)]
    L.psfm_result_filter_batch.argtypes = [ctypes.POINTER(vp), i32, i32, ctypes.POINTER(i64), ctypes.POINTER(i64), vp]
    L.psfm_traj_to_matches_batch.argtypes = [ctypes.POINTER(vp), i32, ctypes.POINTER(i32), i32, ctypes.POINTER(vp), ctypes.POINTER(i64),
                                             ctypes.POINTER(i64), ctypes.POINTER(i64), vp]
    L.psfm_labels_to_matches_batch.argtypes = [ctypes.POINTER(vp), i32, ctypes.POINTER(i32), i32, i32, ctypes.POINTER(i64),
                                               ctypes.POINTER(i64), ctypes.POINTER(i64), vp]
    L.psfm_matches_batch_census.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.psfm_matches_to_database.argtypes = [vp, i32, vp, vp, ctypes.POINTER(i64), ctypes.POINTER(i64), vp]
    L.psfm_database_copy.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.psfm_database_chunk_rows.argtypes = []
    L.psfm_database_compact_again.argtypes = [vp, vp]
    L.psfm_sparse_depth.argtypes = [vp, vp, vp, i64, vp, i32, vp, vp, vp, i64, vp, ctypes.POINTER(i64), vp]
    L.psfm_sparse_depth_sort_ids.argtypes = [vp, vp, i64, vp, vp, vp]
    L.psfm_ctx_set_sparse_depth.argtypes = [vp, i64, i32]
    L.psfm_ctx_get_sparse_depth_budget.argtypes = [vp, ctypes.POINTER(i64)]
    L.psfm_sparse_depth_last_ms.argtypes = [vp, ctypes.POINTER(f64)]
    L.psfm_depth_display.argtypes = [vp, vp, vp, i32, f64, vp, vp, vp, vp, vp, vp]
    L.psfm_ctx_set_depth_display.argtypes = [vp, i32]
    L.psfm_depth_display_last_ms.argtypes = [vp, ctypes.POINTER(f64)]
    L.psfm_depth_display_chunk.argtypes = []
    L.psfm_colmap_points3d_count.argtypes = [vp, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]
    L.psfm_colmap_points3d_scan.argtypes = [vp, ctypes.c_uint64, vp, vp, vp, vp]
    L.psfm_shard_begin.argtypes = [vp, i32, i32, i32, i32, i64, i64, i32, vp, i64, vp]
    L.psfm_shard_step.argtypes = [vp, vp, vp, i32, vp]
    L.psfm_shard_solve_export.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, vp, vp]
    L.psfm_shard_frame.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, vp, vp]
    L.psfm_shard_solve_control.argtypes = [vp, i32, i32, i32, vp, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                                           ctypes.POINTER(SolveStats), vp]
    L.psfm_shard_solve_control_async.argtypes = [vp, i32, i32, vp, vp]
    L.psfm_shard_solve_control_chain_async.argtypes = [vp, i32, i32, vp, vp]
    L.psfm_shard_solve_poll.argtypes = [vp, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(SolveStats), vp]
    L.psfm_shard_solve_local.argtypes = [vp, vp, vp, vp, vp, i32, i32, vp]
    L.psfm_shard_peer_area.argtypes = [vp, ctypes.POINTER(vp), vp, vp]
    L.psfm_shard_peer_open.argtypes = [vp, vp, i32, ctypes.POINTER(vp)]
    L.psfm_shard_peer_epoch.argtypes = [vp, ctypes.POINTER(ctypes.c_uint32), i32, vp]
    L.psfm_shard_peer_connect.argtypes = [vp, i32, i32, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_int32)]
    L.psfm_shard_solve_blocks.argtypes = [vp, ctypes.POINTER(ctypes.c_int32)]
    L.psfm_shard_solve_peer.argtypes = [vp, vp, vp, vp, vp, i32, ctypes.c_uint32, vp]
    L.psfm_shard_solve_redo_local.argtypes = [vp, vp, vp, vp, vp, i32, i32, ctypes.POINTER(SolveStats), vp]
    L.psfm_shard_window_state.argtypes = [vp, i32, i32, ctypes.POINTER(SolveStats), ctypes.POINTER(ctypes.c_int32), vp]
    L.psfm_shard_peek_stall.argtypes = [vp, ctypes.POINTER(ctypes.c_int32)]
    L.psfm_shard_solve_restore.argtypes = [vp, i32, vp]
    L.psfm_shard_solve_writeback.argtypes = [vp, i32, ctypes.POINTER(SolveStats), vp]
    L.psfm_shard_solve_record.argtypes = [vp, ctypes.POINTER(SolveStats)]
    L.psfm_shard_finish.argtypes = [vp, ctypes.POINTER(TrackInfo), vp]
    L.psfm_result_keys.argtypes = [vp, i32, i32, vp, vp]
    L.psfm_profile_get.argtypes = [vp, i32, ctypes.POINTER(f64), ctypes.POINTER(i64)]
    for name in EXPORTS:
        if name != "psfm_last_error":
            getattr(L, name).restype = i32
    L.psfm_traj_decode_workspace_bytes.restype = ctypes.c_size_t
    L.psfm_traj_decode_batch_workspace_bytes.restype = ctypes.c_size_t
    _lib = L
    return L


def check(status):
    if status != PSFM_OK:
        raise PsfmError(status, lib().psfm_last_error().decode("utf-8", "replace"))


class Context:
    """One psfm_ctx (device workspace).  Not thread-safe; cached per device by `context()`."""

    def __init__(self, device=0):
        self._h = ctypes.c_void_p()
        check(lib().psfm_ctx_create(int(device), ctypes.byref(self._h)))
        self.device = int(device)
        self.resident_budget = 0           # (what set_resident_budget was last given)
        self.batch_redo = 0                # (what set_batch_redo was last given)

    @property
    def handle(self):
        return self._h

    def set_capacity(self, lane_factor, traj_factor):
        check(lib().psfm_ctx_set_capacity(self._h, float(lane_factor), float(traj_factor)))

    def set_chain_mode(self, mode):
        """0 auto (persistent frame loop when the grid fits the device), 1 per-frame launches, 2 persistent loop only."""
        check(lib().psfm_ctx_set_chain_mode(self._h, int(mode)))

    def set_motion_boundary(self, enable, thres=0.02):
        """Tracks also die on motion boundaries (the reference's commented kill rule, trajectory.py:60): psfm_track / psfm_connect
        then run one launch per frame; psfm_connect_batch takes the option on all of its contexts or on none; psfm_shard_begin refuses
        the context.  Default off."""
        check(lib().psfm_ctx_set_motion_boundary(self._h, int(bool(enable)), float(thres)))

    def set_solver(self, mode, k=0):
        """track_optimize: 0 adaptive (fused solve, launch chain for windows whose solves reject steps), 1 launch chain,
        2 fused solve; k = trust-region iterations per fused launch (0: adaptive)."""
        check(lib().psfm_ctx_set_solver(self._h, int(mode), int(k)))

    BATCH_REDO = {"alone": 0, "together": 1}

    def set_batch_redo(self, mode):
        """psfm_connect_batch with this context as its first: how the sequences that leave the fused batch (their solves reject steps)
        are run again -- "alone" / 0: each through psfm_connect (default); "together" / 1: all of them through one set of launches, their
        solves as the frame-mode multi-problem launch chain (info.chain_mode 8)."""
        mode = self.BATCH_REDO.get(mode, mode)
        check(lib().psfm_ctx_set_batch_redo(self._h, int(mode)))
        self.batch_redo = int(mode)

    def set_frame_size(self, h, w):
        """The frame size of the sequence this context holds in a psfm_connect_batch call with h = w = 0 (sequences of different frame
        sizes in one batch); (0, 0) clears it.  No other entry point reads it."""
        check(lib().psfm_ctx_set_frame_size(self._h, int(h), int(w)))

    def connect_batch_census(self):
        """The last psfm_connect_batch call that had this context as its first: sequences that left the fused batch, those that were
        redone together, and of that redo the launches that do not depend on how the solves went, the trust-region iteration launches
        and the host synchronisations.  Per frame the fixed launches are three whatever the number of sequences; polls, iteration launches
        and synchronisations follow the slowest solve of the frame in the table and do not grow beyond its need."""
        v = [ctypes.c_int32() for _ in range(5)]
        check(lib().psfm_connect_batch_census(self._h, *[ctypes.byref(x) for x in v]))
        return dict(zip(("n_left", "n_together", "launches_fixed", "launches_iter", "host_syncs"), (int(x.value) for x in v)))

    def set_resident_budget(self, blocks):
        """> 0: this context's resident solves (flows whose solves reject steps) use at most `blocks` blocks and may run beside other
        contexts' -- the budgets of all contexts in flight on the device must add up to at most resident_capacity(); 0: only with the
        device to itself (default)."""
        check(lib().psfm_ctx_set_resident_budget(self._h, int(blocks)))
        self.resident_budget = int(blocks)

    def resident_capacity(self):
        n = ctypes.c_int32()
        check(lib().psfm_resident_capacity(self._h, ctypes.byref(n)))
        return int(n.value)

    def solver_counters(self):
        a, b, c_, k = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32()
        check(lib().psfm_solver_counters(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c_), ctypes.byref(k)))
        out = {"fused": a.value, "fused_redone": b.value, "chain": c_.value, "k": k.value}
        r, g, it = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        check(lib().psfm_solver_launches(self._h, ctypes.byref(r), ctypes.byref(g), ctypes.byref(it)))
        out.update({"resident_launches": r.value, "resident_giveups": g.value, "iteration_launches": it.value})
        return out

    def finalize_forms(self):
        """Which forms the last id assignment of this context ran (for a batch: the context that owns it).  sort: 0 none yet, 1 the
        library's sort on 32-bit keys, 2 on 64-bit keys, 3 rocPRIM; offsets: 0 none yet, 1 one-block group plan, 3 decode + scan
        (2: a chunked group plan, not built in)."""
        a, b = ctypes.c_int32(), ctypes.c_int32()
        check(lib().psfm_ctx_get_finalize_forms(self._h, ctypes.byref(a), ctypes.byref(b)))
        return {"sort": int(a.value), "offsets": int(b.value)}

    def finalize_placed(self):
        """1 when the last id assignment of this context placed its records by birth order and sorted them in one pass (after the
        persistent frame loop, 32-bit keys, at most 255 flows; PSFM_FIN_PLACE=0 turns it off), else 0.  Same bytes either way."""
        a = ctypes.c_int32()
        check(lib().psfm_ctx_get_finalize_placed(self._h, ctypes.byref(a)))
        return int(a.value)

    def finalize_gather(self):
        """How the last id assignment of this context summed the flow log into positions: 0 it had a position log (no sums), 1 one
        thread per trajectory in the loop's order, 2 blocked sums under the chunk rule of csrc/psfm_gather_exact.h (after the
        persistent frame loop, frames up to 3840 pixels a side; PSFM_FIN_GATHER=0 keeps 1).  Same bytes either way."""
        a = ctypes.c_int32()
        check(lib().psfm_ctx_get_finalize_gather(self._h, ctypes.byref(a)))
        return int(a.value)

    def query_batch_census(self):
        """Launches (kernels and copies, the kill maps of the motion-boundary option apart) and host synchronisations of the last
        psfm_track_queries_batch call that had this context as its first."""
        a, b = ctypes.c_int32(), ctypes.c_int32()
        check(lib().psfm_query_batch_census(self._h, ctypes.byref(a), ctypes.byref(b)))
        return {"launches": int(a.value), "host_syncs": int(b.value)}

    def query_pc_batch_census(self):
        """The last psfm_track_queries_optimize_batch call that had this context as its first: launches that do not depend on how the
        solves went (kernels and copies, the kill maps of the motion-boundary option apart), trust-region iteration launches, and
        host synchronisations."""
        a, b, c = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        check(lib().psfm_query_pc_batch_census(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return {"launches_fixed": int(a.value), "launches_iter": int(b.value), "host_syncs": int(c.value)}

    def set_result(self, ids, birth, length, xy):
        """psfm_result_set: a trajectory set from elsewhere becomes this context's result.  ids / birth / length (n,) and xy
        (n_points, 2): NumPy arrays (host) or torch tensors (host or device), converted to i32 / f64 when they are not; trajectory i
        holds frames birth[i] .. birth[i] + length[i] - 1, ids ascend strictly.  The result has ids[-1] + 1 entries -- index == id,
        ids the set does not name are entries of length 0 -- and that count is returned.  PsfmError (status PSFM_ERR_ARG, the lowest bad
        index in the message) leaves the context as it was."""
        import numpy as np
        import torch

        def arr(a, np_dt, t_dt, shape):
            if isinstance(a, torch.Tensor):
                t = a.reshape(shape).to(t_dt).contiguous()
                return t, ctypes.c_void_p(t.data_ptr() if t.numel() else 0)
            h = np.ascontiguousarray(np.asarray(a).reshape(shape), dtype=np_dt)
            return h, ctypes.c_void_p(h.ctypes.data if h.size else 0)
        keep = [arr(ids, np.int32, torch.int32, (-1,)), arr(birth, np.int32, torch.int32, (-1,)), arr(length, np.int32, torch.int32, (-1,)),
                arr(xy, np.float64, torch.float64, (-1, 2))]
        n = int(keep[0][0].shape[0])
        if int(keep[1][0].shape[0]) != n or int(keep[2][0].shape[0]) != n:
            raise ValueError("set_result: ids, birth and length must have one entry per trajectory")
        n_result = ctypes.c_int64(0)
        check(lib().psfm_result_set(self._h, n, int(keep[3][0].shape[0]), keep[0][1], keep[1][1], keep[2][1], keep[3][1],
                                    ctypes.byref(n_result), current_stream_ptr(self.device)))
        return int(n_result.value)

    def load_track_npy(self, path, threads=4):
        """psfm_load_track_npy: a track.npy that save_track_npy(layout="reference") wrote, from the file into this context's result
        (records and points through the pinned ring, decoded and validated on the device).  Returns (n_traj, n_points, n_result).
        PsfmError with status PSFM_ERR_ARG: not such a file, or one that fails a check -- the context is as it was, except behind a
        read error while the points stream (an empty result; the message says so)."""
        import numpy as np
        from . import reference_pickle
        rec, at = reference_pickle._record_template()
        tmpl = np.frombuffer(rec, np.uint8).copy()
        field_at = np.asarray([at[k] for k in ("id", "b", "bn", "s", "e", "n")], np.int32)
        n, p, r = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        check(lib().psfm_load_track_npy(self._h, os.fsencode(str(path)), tmpl.ctypes.data, len(rec), field_at.ctypes.data, int(threads),
                                        ctypes.byref(n), ctypes.byref(p), ctypes.byref(r), current_stream_ptr(self.device)))
        return int(n.value), int(p.value), int(r.value)

    def set_sparse_depth(self, budget_bytes=1 << 30, timing=False):
        """psfm_sfm.convert: bytes of depth maps + winner maps (12 per pixel) one psfm_sparse_depth call may take (0: no limit; one
        image always goes through); timing: events around the zero fill, the winner pass and the store pass (sparse_depth_ms)."""
        check(lib().psfm_ctx_set_sparse_depth(self._h, int(budget_bytes), int(bool(timing))))

    def sparse_depth_ms(self):
        ms = (ctypes.c_double * 3)()
        check(lib().psfm_sparse_depth_last_ms(self._h, ms))
        return {"fill_ms": ms[0], "winner_ms": ms[1], "store_ms": ms[2]}

    def set_depth_display(self, timing=False):
        """psfm_sfm.convert.depth_display_device: events around the count, compact, select and colour passes (depth_display_ms)."""
        check(lib().psfm_ctx_set_depth_display(self._h, int(bool(timing))))

    def depth_display_ms(self):
        ms = (ctypes.c_double * 4)()
        check(lib().psfm_depth_display_last_ms(self._h, ms))
        return {"count_ms": ms[0], "compact_ms": ms[1], "select_ms": ms[2], "colour_ms": ms[3]}

    def set_profiling(self, enable):
        check(lib().psfm_ctx_set_profiling(self._h, int(enable)))   # 0 off, 1 every launch, N>1 every N-th chain_step

    def profile(self):
        out = {}
        for name, k in PROF_KINDS.items():
            ms, n = ctypes.c_double(), ctypes.c_int64()
            check(lib().psfm_profile_get(self._h, k, ctypes.byref(ms), ctypes.byref(n)))
            out[name] = {"total_ms": ms.value, "launches": n.value}
        return out

    def close(self):
        if self._h:
            lib().psfm_ctx_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_contexts = {}
_contexts_lock = __import__("threading").Lock()   # batch.py worker threads create and release contexts concurrently


def context(device=None):
    """The psfm context of the calling THREAD on `device` (a context is not thread-safe; worker threads that process
    different sequences concurrently each get their own -- see point_trajectory.batch)."""
    import threading
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("point_trajectory (MI355X build) needs a HIP device: torch.cuda.is_available() is False "
                           "and there is no CPU fallback")
    if device is None:
        device = torch.cuda.current_device()
    device = int(device)
    key = (device, threading.get_ident())
    with _contexts_lock:
        ctx = _contexts.get(key)
    if ctx is None:
        ctx = Context(device)            # (outside the lock: creating a context allocates pinned memory)
        with _contexts_lock:
            _contexts[key] = ctx
    return ctx


def batch_contexts(n, device=None):
    """n psfm contexts of the calling thread on `device` for psfm_connect_batch (one per sequence of a batch; the first is the
    thread's ordinary context and owns the batch's shared workspace).  Cached: workspaces stay warm across batches."""
    import threading
    first = context(device)
    out = [first]
    for k in range(1, int(n)):
        key = (first.device, threading.get_ident(), "batch", k)
        with _contexts_lock:
            ctx = _contexts.get(key)
        if ctx is None:
            ctx = Context(first.device)
            with _contexts_lock:
                _contexts[key] = ctx
        out.append(ctx)
    return out


def release_thread_contexts():
    """Destroy the calling thread's contexts (worker threads call this before they exit)."""
    import threading
    tid = threading.get_ident()
    with _contexts_lock:
        mine = [_contexts.pop(k) for k in [k for k in _contexts if k[1] == tid]]
    for ctx in mine:
        ctx.close()


def current_stream_ptr(device=None):
    """torch's current stream ON `device` (default: the current device) -- pass the context's device when it may differ
    from the current one: a stream belongs to one device."""
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def ptr(t):
    """Device (or host) address of a torch tensor as c_void_p; None -> NULL."""
    if t is None:
        return ctypes.c_void_p(0)
    return ctypes.c_void_p(t.data_ptr())
