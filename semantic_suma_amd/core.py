"""Host-side mirror of the reference's hot-path classes over the C-ABI (include/suma_hip.h).

The classes keep the names, argument meaning and error behaviour of the reference interfaces they
stand for (PRBonn/semantic_suma, src/core):

    Frame            src/core/Frame.h:21-79
    Preprocessing    src/core/Preprocessing.h:47-58          process(points, frame, labels, probs, timestamp)
    Frame2Model      src/core/Frame2Model.h:28-73 / Objective.h:14-82
    LieGaussNewton   src/core/LieGaussNewton.h:25-76         minimize(objective, T0), pose(), history()
    SurfelMap        src/core/SurfelMap.h:36-78              update / render* / *MapFrame / updatePoses / size / draw
    SurfelMapping    src/core/SurfelMapping.h:47             processScan(scan); enableDeskew: raw sweeps are motion
                                                             compensated in front of the preprocessing (no counterpart)
    Localizer        (no counterpart)                        setMap / setPose / processScan / relocalize in a finished map;
                                                             enableEvidence / evidence / prunedMap: which records still hold;
                                                             enableNovelty / novel / updatedMap: what is new;
                                                             enableObjects / objects: each scan's unexplained texels as objects
                                                             enableLiveGrid / liveCells: live obstacles in the planner's grid
    PlaceIndex       (no counterpart)                        addFrame / queryFrame: place recognition over a session's scans
    Posegraph        src/core/Posegraph.h:10-78              setInitial / addEdge / optimize / poses

Everything here is plumbing: numpy arrays in, ctypes calls into ``libsuma_hip.so`` (hand-written
gfx950 kernels), numpy arrays out.  There is no CPU fallback -- if the library is missing or no
MI355X is visible the constructors raise (the reference throws ``std::runtime_error`` in the
same situations, e.g. Frame2Model.cpp:132).  Matrices are exchanged as row-major numpy 4x4 and
converted to the column-major layout of Eigen at the boundary.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .types import (ACC_WORDS, DRAW_COLORS, DRAW_LIGHTS, DRAW_MATERIAL, DRAW_MAX_LIGHTS, SURFEL_DTYPE, DrawParams,
                    IcpStats, LoopParams, LoopStatus, PosegraphParams, PosegraphStats, SemanticKnnParams,
                    SemanticParams, SumaParams, WORLD_SURFEL_DTYPE, WorldParams, WorldStats, CheckpointInfo,
                    GRID_CELL_DTYPE, GridParams, GridStats,
                    PLAN_CELL_DTYPE, PLAN_PATH_DTYPE, PATH_OK, PATH_TRUNCATED, PlanParams, PlanStats,
                    ChangeCounts, ChangeParams, ChangeRule, DeskewParams, EVIDENCE_DTYPE, NovelCounts, NovelFuseParams, NovelParams, NovelStats,
                    ObjectCounts, ObjectParams, SCAN_OBJECT_DTYPE, OBJECT_TRACK_DTYPE, ObjectTrack, TrackCounts, TrackParams, LIVE_CELL_DTYPE, LiveCounts, LiveParams, LiveStats, LocalizerParams, LocalizerResult, PLACE_MAX_MATCHES, PlaceMatch, PlaceParams, RelocalizeResult)

_HERE = os.path.dirname(os.path.abspath(__file__))
# SUMA_HIP_LIB selects another build of the same library (A/B timing of kernel variants in one GPU session)
LIB_PATH = os.environ.get("SUMA_HIP_LIB") or os.path.join(_HERE, "libsuma_hip.so")
_LIB = None


class SumaError(RuntimeError):
    """Raised for every negative return code of the C-ABI (the reference throws std::runtime_error)."""


class LoopResult(C.Structure):
    """suma_loop_result (include/suma_hip.h)"""
    _fields_ = [("gn_pose", C.c_double * 16), ("after_minimize", IcpStats), ("passed", C.c_int32),
                ("pose_old", C.c_float * 16), ("composed", IcpStats), ("JtJ", C.c_double * 36)]


class LoopTrack(C.Structure):
    """suma_loop_track (include/suma_hip.h)"""
    _fields_ = [("increment_old", C.c_double * 16), ("after_minimize", IcpStats), ("increment_difference", C.c_float),
                ("passed", C.c_int32), ("pose_old", C.c_double * 16), ("composed", IcpStats), ("JtJ", C.c_double * 36)]


class ScanRef(C.Structure):
    """suma_scan_ref (include/suma_runner.h)"""
    _fields_ = [("points", C.c_void_p), ("labels", C.c_void_p), ("probs", C.c_void_p), ("n", C.c_uint32)]


class SequenceJob(C.Structure):
    """suma_sequence_job"""
    _fields_ = [("scans", C.POINTER(ScanRef)), ("n_scans", C.c_uint32), ("on_device", C.c_int32)]


class SequenceResult(C.Structure):
    """suma_sequence_result"""
    _fields_ = [("status", C.c_int32), ("scans_done", C.c_uint32), ("map_surfels", C.c_uint32), ("track_loss", C.c_uint32),
                ("end_pose", C.c_double * 16), ("seconds", C.c_double), ("error", C.c_char * 160)]


class HypothesisJob(C.Structure):
    """suma_hypothesis_job"""
    _fields_ = [("scans", C.POINTER(ScanRef)), ("n_scans", C.c_uint32), ("on_device", C.c_int32),
                ("perturbations", C.c_void_p), ("n_hyp", C.c_uint32), ("rank", C.c_uint32), ("world", C.c_uint32)]


EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_uint32)


class IcpObjective(C.Structure):
    """suma_icp_objective (include/suma_hip.h): the parameters one Frame2Model object owns"""
    _fields_ = [("icp_max_distance", C.c_float), ("icp_max_angle", C.c_float), ("weight_function", C.c_int32),
                ("factor", C.c_float), ("bilinear_sampling", C.c_int32)]


class KernelTime(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_uint64), ("total_ms", C.c_double), ("bytes", C.c_double)]


def lib():
    """Load libsuma_hip.so (built in-tree by ``__graft_entry__.build()`` / ``make -C semantic_suma_amd/csrc``)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise SumaError(f"{LIB_PATH} not found: build it with `make -C semantic_suma_amd/csrc` "
                        "(there is no CPU fallback for the HIP path)")
    L = C.CDLL(LIB_PATH)
    vp, u32, i32, f32 = C.c_void_p, C.c_uint32, C.c_int32, C.c_float
    pp = C.POINTER(vp)
    L.suma_version.restype = C.c_char_p
    L.suma_posegraph_last_error.restype = C.c_char_p
    L.suma_posegraph_last_error.argtypes = [vp]
    L.suma_posegraph_create.argtypes = [C.c_int, u32, u32, pp]
    L.suma_posegraph_destroy.argtypes = [vp]
    L.suma_posegraph_destroy.restype = None
    L.suma_posegraph_clear.argtypes = [vp]
    L.suma_posegraph_clone.argtypes = [vp, pp]
    L.suma_posegraph_set_initial.argtypes = [vp, i32, vp]
    L.suma_posegraph_add_edge.argtypes = [vp, i32, i32, vp, vp]
    L.suma_posegraph_pose.argtypes = [vp, i32, vp]
    L.suma_posegraph_poses.argtypes = [vp, vp, u32, C.POINTER(u32)]
    L.suma_posegraph_size.argtypes = [vp]
    L.suma_posegraph_size.restype = i32
    L.suma_posegraph_edge_count.argtypes = [vp]
    L.suma_posegraph_edge_count.restype = u32
    L.suma_posegraph_error.argtypes = [vp, C.POINTER(C.c_double)]
    L.suma_posegraph_reinitialize.argtypes = [vp]
    L.suma_posegraph_optimize.argtypes = [vp, u32, C.POINTER(PosegraphParams), C.POINTER(PosegraphStats)]
    L.suma_posegraph_linearize.argtypes = [vp, vp, vp, vp, vp, vp, vp, u32, C.POINTER(u32)]
    L.suma_posegraph_reserve.argtypes = [vp, u32, u32]
    L.suma_posegraph_edge.argtypes = [vp, u32, C.POINTER(i32), C.POINTER(i32), vp, vp]
    L.suma_loop_params_default.argtypes = [C.POINTER(LoopParams)]
    L.suma_loop_params_default.restype = None
    L.suma_pipeline_enable_loop_closing.argtypes = [vp, C.POINTER(LoopParams)]
    L.suma_pipeline_check_loop_closure.argtypes = [vp]
    L.suma_pipeline_loop_status.argtypes = [vp, C.POINTER(LoopStatus)]
    L.suma_pipeline_posegraph.argtypes = [vp]
    L.suma_pipeline_posegraph.restype = vp
    L.suma_pipeline_trajectory_distances.argtypes = [vp, vp, u32, C.POINTER(u32)]
    L.suma_loop_find_candidate.argtypes = [vp, vp, u32, vp, f32, f32, i32]
    L.suma_loop_find_candidate.restype = i32
    L.suma_last_error.restype = C.c_char_p
    L.suma_last_error.argtypes = [vp]
    L.suma_ctx_create.argtypes = [C.POINTER(SumaParams), C.c_int, pp]
    L.suma_ctx_destroy.argtypes = [vp]
    L.suma_ctx_destroy.restype = None
    L.suma_set_params.argtypes = [vp, C.POINTER(SumaParams)]
    L.suma_synchronize.argtypes = [vp]
    L.suma_ctx_stream.restype = vp
    L.suma_ctx_stream.argtypes = [vp]
    L.suma_frame_create.argtypes = [vp, u32, u32, pp]
    L.suma_frame_destroy.argtypes = [vp]
    L.suma_frame_destroy.restype = None
    L.suma_frame_copy.argtypes = [vp, vp, vp]
    L.suma_frame_download.argtypes = [vp, vp, C.c_int, vp]
    L.suma_frame_upload.argtypes = [vp, vp, C.c_int, vp]
    L.suma_frame_width.restype = u32
    L.suma_frame_width.argtypes = [vp]
    L.suma_frame_height.restype = u32
    L.suma_frame_height.argtypes = [vp]
    L.suma_frame_device_ptr.restype = vp
    L.suma_frame_device_ptr.argtypes = [vp, C.c_int]
    L.suma_frame_swap.argtypes = [vp, vp, vp]
    L.suma_frame_export.argtypes = [vp, vp, C.c_int, pp, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]
    L.suma_icp_set_objective.argtypes = [vp, C.POINTER(IcpObjective)]
    L.suma_icp_information.argtypes = [vp, vp]
    L.suma_map_export_surfels.argtypes = [vp, pp, C.POINTER(u32)]
    L.suma_map_export_data_surfels.argtypes = [vp, pp, C.POINTER(u32), C.POINTER(u32)]
    L.suma_pipeline_prefetch_scan.argtypes = [vp, vp, vp, vp, u32]
    L.suma_pipeline_process_prefetched.argtypes = [vp, i32]
    L.suma_pipeline_process_scan_async.argtypes = [vp, vp, vp, vp, u32, i32]
    L.suma_device_download.argtypes = [vp, vp, vp, C.c_uint64]
    L.suma_preprocess.argtypes = [vp, vp, vp, vp, u32, u32, vp]
    L.suma_preprocess_device.argtypes = [vp, vp, vp, vp, u32, u32, vp]
    L.suma_icp_set_data.argtypes = [vp, vp, vp]
    L.suma_icp_jacobian_products.argtypes = [vp, vp, u32, vp, vp, vp, C.POINTER(IcpStats)]
    L.suma_icp_minimize.argtypes = [vp, vp, vp, vp, u32, C.POINTER(u32), C.POINTER(IcpStats)]
    L.suma_icp_history.argtypes = [vp, vp, u32, C.POINTER(u32)]
    L.suma_icp_history_sequence.argtypes = [vp]
    L.suma_icp_history_sequence.restype = C.c_uint64
    L.suma_frame_touch.argtypes = [vp, vp]
    L.suma_pipeline_minimize_stats.argtypes = [vp, C.POINTER(IcpStats)]
    L.suma_icp_minimize_batch.argtypes = [vp, vp, u32, vp, vp]
    L.suma_map_reset.argtypes = [vp]
    L.suma_map_update.argtypes = [vp, vp, vp]
    L.suma_map_render.argtypes = [vp, vp, vp, f32, vp]
    L.suma_map_render_active.argtypes = [vp, vp, f32]
    L.suma_map_render_inactive.argtypes = [vp, vp, f32]
    L.suma_map_render_composed.argtypes = [vp, vp, vp, f32]
    L.suma_map_frame.restype = vp
    L.suma_map_frame.argtypes = [vp, C.c_int]
    L.suma_map_update_poses.argtypes = [vp, vp, u32]
    L.suma_map_size.argtypes = [vp, C.POINTER(u32)]
    L.suma_map_timestamp.argtypes = [vp, C.POINTER(u32)]
    L.suma_map_download.argtypes = [vp, vp, u32, C.POINTER(u32)]
    L.suma_map_upload.argtypes = [vp, vp, u32, u32]
    L.suma_map_download_index_map.argtypes = [vp, vp]
    L.suma_map_download_radius_conf.argtypes = [vp, vp]
    L.suma_map_download_poses.argtypes = [vp, vp, u32, C.POINTER(u32)]
    L.suma_map_download_integrated.argtypes = [vp, vp]
    L.suma_map_counts.argtypes = [vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), vp]
    L.suma_map_cache_stats.argtypes = [vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]
    L.suma_map_download_cached_tile.argtypes = [vp, C.c_int32, C.c_int32, vp, u32, C.POINTER(u32)]
    L.suma_icp_set_iteration.argtypes = [vp, u32]
    L.suma_pipeline_host_entry_times.argtypes = [vp, vp, C.c_int]
    L.suma_loop_closure_verify.argtypes = [vp, vp, vp, vp, u32, vp, f32, f32, f32, C.POINTER(LoopResult)]
    L.suma_loop_closure_verify_serial.argtypes = [vp, vp, vp, vp, u32, vp, f32, f32, f32, C.POINTER(LoopResult)]
    L.suma_pipeline_create.argtypes = [C.POINTER(SumaParams), C.c_int, pp]
    L.suma_pipeline_destroy.argtypes = [vp]
    L.suma_pipeline_destroy.restype = None
    L.suma_pipeline_ctx.restype = vp
    L.suma_pipeline_ctx.argtypes = [vp]
    L.suma_pipeline_process_scan.argtypes = [vp, vp, vp, vp, u32, i32]
    L.suma_pipeline_process_scan_device.argtypes = [vp, vp, vp, vp, u32, i32]
    L.suma_pipeline_pose.argtypes = [vp, vp]
    L.suma_pipeline_begin_scan.argtypes = [vp, vp, vp, vp, u32]
    L.suma_pipeline_begin_scan_device.argtypes = [vp, vp, vp, vp, u32]
    L.suma_pipeline_begin_prefetched.argtypes = [vp]
    L.suma_pipeline_update_pose.argtypes = [vp, i32]
    L.suma_pipeline_update_map.argtypes = [vp]
    L.suma_pipeline_integrate_loop_closures.argtypes = [vp, vp, u32, vp]
    L.suma_pipeline_set_pose_old.argtypes = [vp, vp]
    L.suma_pipeline_get_pose.argtypes = [vp, C.c_int, vp]
    L.suma_pipeline_result_new.argtypes = [vp, C.POINTER(IcpStats)]
    L.suma_pipeline_verify_loop_closure.argtypes = [vp, vp, vp, u32, f32, f32, C.POINTER(LoopResult)]
    L.suma_pipeline_track_loop_closure.argtypes = [vp, C.c_double, C.c_double, C.c_double, C.POINTER(LoopTrack)]
    L.suma_loop_closure_track.argtypes = [vp, vp, vp, vp, vp, f32, C.c_double, C.c_double, C.c_double, C.POINTER(LoopTrack)]
    L.suma_se3_log.argtypes = [vp, vp]
    L.suma_se3_log.restype = None
    L.suma_pipeline_reset.argtypes = [vp]
    L.suma_pipeline_minimize_hypotheses.argtypes = [vp, vp, u32, i32, vp, vp]
    L.suma_pipeline_apply_increment.argtypes = [vp, vp]
    L.suma_run_sequences.argtypes = [C.POINTER(SumaParams), C.c_int, C.POINTER(SequenceJob), u32, u32, i32,
                                     C.POINTER(SequenceResult)]
    L.suma_run_hypotheses.argtypes = [C.POINTER(SumaParams), C.c_int, C.POINTER(HypothesisJob), i32, EXCHANGE_FN, vp, vp,
                                      vp, C.c_char_p]
    L.suma_pipeline_run_scans.argtypes = [vp, C.POINTER(SequenceJob), i32, C.POINTER(u32), vp]
    L.suma_pipeline_last_increment.argtypes = [vp, vp]
    L.suma_pipeline_last_stats.argtypes = [vp, C.POINTER(IcpStats)]
    L.suma_pipeline_timestamp.restype = u32
    L.suma_pipeline_timestamp.argtypes = [vp]
    L.suma_pipeline_track_loss.restype = u32
    L.suma_pipeline_track_loss.argtypes = [vp]
    L.suma_pipeline_frame.restype = vp
    L.suma_pipeline_frame.argtypes = [vp, C.c_int]
    sp = C.POINTER(SemanticParams)
    L.suma_semantic_project.argtypes = [vp, sp, vp, u32, vp, vp, vp]
    L.suma_semantic_unproject.argtypes = [vp, sp, vp, C.c_int, vp, u32, vp, vp]
    L.suma_pipeline_begin_scan_scores.argtypes = [vp, sp, vp, vp, C.c_int, vp, u32, vp]
    L.suma_pipeline_process_scan_scores.argtypes = [vp, sp, vp, vp, C.c_int, vp, u32, vp, i32]
    kp = C.POINTER(SemanticKnnParams)
    L.suma_semantic_unproject_knn.argtypes = [vp, sp, kp, vp, vp, C.c_int, vp, vp, u32, vp, vp]
    L.suma_pipeline_begin_scan_scores_knn.argtypes = [vp, sp, kp, vp, vp, C.c_int, vp, vp, u32, vp]
    L.suma_pipeline_process_scan_scores_knn.argtypes = [vp, sp, kp, vp, vp, C.c_int, vp, vp, u32, vp, i32]
    L.suma_map_draw.argtypes = [vp, C.POINTER(DrawParams), vp, vp]
    L.suma_world_params_default.argtypes = [C.POINTER(WorldParams)]
    L.suma_world_params_default.restype = None
    L.suma_map_cached_tiles.argtypes = [vp, vp, u32, C.POINTER(u32)]
    L.suma_map_export_world.argtypes = [vp, C.POINTER(WorldParams), vp, u32, C.POINTER(WorldStats)]
    L.suma_grid_params_default.argtypes = [C.POINTER(GridParams)]
    L.suma_grid_params_default.restype = None
    L.suma_world_grid_fit.argtypes = [vp, vp, u32, u32, C.POINTER(GridParams)]
    L.suma_world_grid.argtypes = [vp, C.POINTER(GridParams), vp, u32, vp, C.POINTER(GridStats)]
    L.suma_plan_params_default.argtypes = [C.POINTER(PlanParams)]
    L.suma_plan_params_default.restype = None
    L.suma_grid_cell_index.argtypes = [C.POINTER(GridParams), C.c_float, C.c_float]
    L.suma_grid_cell_index.restype = C.c_int64
    L.suma_grid_plan_field.argtypes = [vp, C.POINTER(GridParams), C.POINTER(PlanParams), vp, vp, u32, vp, C.POINTER(PlanStats)]
    L.suma_grid_plan_paths.argtypes = [vp, C.POINTER(GridParams), vp, vp, u32, u32, vp, vp]
    L.suma_device_alloc.argtypes = [vp, C.c_uint64, pp]
    L.suma_device_free.argtypes = [vp, vp]
    L.suma_device_upload.argtypes = [vp, vp, vp, C.c_uint64]
    L.suma_profile_enable.argtypes = [vp, C.c_int]
    L.suma_profile_reset.argtypes = [vp]
    L.suma_profile_get.argtypes = [vp, C.POINTER(KernelTime), u32]
    u64p = C.POINTER(C.c_uint64)
    L.suma_pipeline_checkpoint_size.argtypes = [vp, u64p]
    L.suma_pipeline_checkpoint_save.argtypes = [vp, vp, C.c_uint64, u64p]
    L.suma_pipeline_checkpoint_load.argtypes = [vp, vp, C.c_uint64]
    L.suma_checkpoint_info.argtypes = [vp, C.c_uint64, C.POINTER(CheckpointInfo)]
    L.suma_checkpoint_params.argtypes = [vp, C.c_uint64, C.POINTER(SumaParams)]
    L.suma_checkpoint_digest.argtypes = [vp, C.c_uint64]
    L.suma_checkpoint_digest.restype = C.c_uint64
    lpp, lrp = C.POINTER(LocalizerParams), C.POINTER(LocalizerResult)
    L.suma_localizer_params_default.argtypes = [C.POINTER(SumaParams), lpp]
    L.suma_localizer_params_default.restype = None
    L.suma_localizer_create.argtypes = [C.POINTER(SumaParams), lpp, C.c_int, pp]
    L.suma_localizer_destroy.argtypes = [vp]
    L.suma_localizer_destroy.restype = None
    L.suma_localizer_ctx.argtypes = [vp]
    L.suma_localizer_ctx.restype = vp
    L.suma_localizer_set_map.argtypes = [vp, vp, u32, C.POINTER(u32)]
    L.suma_localizer_set_map_device.argtypes = [vp, vp, u32, C.POINTER(u32)]
    L.suma_localizer_set_pose.argtypes = [vp, vp]
    L.suma_localizer_process_scan.argtypes = [vp, vp, vp, vp, u32, i32, lrp]
    L.suma_localizer_process_scan_device.argtypes = [vp, vp, vp, vp, u32, i32, lrp]
    L.suma_localizer_window.argtypes = [vp, vp, C.POINTER(u32), C.POINTER(u32)]
    L.suma_localizer_download_window.argtypes = [vp, vp, u32, C.POINTER(u32)]
    cpp, ccp, crp = C.POINTER(ChangeParams), C.POINTER(ChangeCounts), C.POINTER(ChangeRule)
    L.suma_change_params_default.argtypes = [cpp]
    L.suma_change_params_default.restype = None
    L.suma_change_rule_default.argtypes = [crp]
    L.suma_change_rule_default.restype = None
    L.suma_localizer_enable_evidence.argtypes = [vp, cpp]
    L.suma_localizer_disable_evidence.argtypes = [vp]
    L.suma_localizer_observe_frame.argtypes = [vp, vp, vp, ccp]
    L.suma_localizer_last_observation.argtypes = [vp, ccp, C.POINTER(i32)]
    L.suma_localizer_evidence.argtypes = [vp, vp, u32, C.POINTER(u32)]
    L.suma_localizer_evidence_device.argtypes = [vp, vp, u32, C.POINTER(u32)]
    L.suma_localizer_clear_evidence.argtypes = [vp]
    L.suma_change_prune_mask.argtypes = [vp, u32, crp, vp, C.POINTER(u32)]
    npp, nfp, ncp, nsp = C.POINTER(NovelParams), C.POINTER(NovelFuseParams), C.POINTER(NovelCounts), C.POINTER(NovelStats)
    L.suma_novel_params_default.argtypes = [npp]
    L.suma_novel_params_default.restype = None
    L.suma_novel_fuse_params_default.argtypes = [C.POINTER(SumaParams), nfp]
    L.suma_novel_fuse_params_default.restype = None
    L.suma_localizer_enable_novelty.argtypes = [vp, npp]
    L.suma_localizer_disable_novelty.argtypes = [vp]
    L.suma_localizer_collect_frame.argtypes = [vp, vp, vp, u32, ncp]
    L.suma_localizer_last_collection.argtypes = [vp, ncp, C.POINTER(i32)]
    L.suma_localizer_novel_candidates.argtypes = [vp, vp, u32, C.POINTER(u32)]
    L.suma_localizer_novel_candidates_device.argtypes = [vp, vp, u32, C.POINTER(u32)]
    L.suma_localizer_set_novel_candidates.argtypes = [vp, vp, u32]
    L.suma_localizer_novel.argtypes = [vp, nfp, vp, vp, u32, nsp]
    L.suma_localizer_novel_device.argtypes = [vp, nfp, vp, vp, u32, nsp]
    L.suma_localizer_novel_marks.argtypes = [vp, vp, u32, C.POINTER(u32)]
    L.suma_localizer_clear_novelty.argtypes = [vp]
    opp, ocp = C.POINTER(ObjectParams), C.POINTER(ObjectCounts)
    L.suma_object_params_default.argtypes = [opp]
    L.suma_object_params_default.restype = None
    L.suma_object_params_check.argtypes = [opp]
    L.suma_localizer_enable_objects.argtypes = [vp, opp]
    L.suma_localizer_disable_objects.argtypes = [vp]
    L.suma_localizer_objects.argtypes = [vp, vp, u32, C.POINTER(u32), ocp, C.POINTER(i32)]
    L.suma_localizer_objects_device.argtypes = [vp, vp, u32, C.POINTER(u32), ocp, C.POINTER(i32)]
    L.suma_localizer_object_ids.argtypes = [vp, vp, u32, C.POINTER(u32)]
    L.suma_localizer_segment_flags.argtypes = [vp, vp, vp, vp, u32, ocp]
    L.suma_localizer_novel_flags.argtypes = [vp, vp, u32, C.POINTER(u32)]
    L.suma_localizer_frame.argtypes = [vp]
    L.suma_localizer_frame.restype = vp
    tpp, tcp, u32p = C.POINTER(TrackParams), C.POINTER(TrackCounts), C.POINTER(u32)
    L.suma_track_params_default.argtypes = [tpp]
    L.suma_track_params_default.restype = None
    L.suma_track_params_check.argtypes = [tpp]
    L.suma_localizer_enable_tracks.argtypes = [vp, tpp]
    L.suma_localizer_disable_tracks.argtypes = [vp]
    L.suma_localizer_clear_tracks.argtypes = [vp]
    L.suma_localizer_tracks.argtypes = [vp, vp, u32, u32p, tcp, C.POINTER(i32)]
    L.suma_localizer_tracks_device.argtypes = [vp, vp, u32, u32p, tcp, C.POINTER(i32)]
    L.suma_localizer_object_tracks.argtypes = [vp, vp, u32, u32p]
    L.suma_localizer_track_objects.argtypes = [vp, vp, u32, u32, tcp]
    L.suma_localizer_track_state.argtypes = [vp, vp, u32, u32p, u32p, u32p]
    L.suma_localizer_set_track_state.argtypes = [vp, vp, u32, u32, u32]
    lvp, lcp = C.POINTER(LiveParams), C.POINTER(LiveCounts)
    L.suma_live_params_default.argtypes = [lvp]
    L.suma_live_params_default.restype = None
    L.suma_live_params_check.argtypes = [lvp]
    L.suma_localizer_enable_live_grid.argtypes = [vp, C.POINTER(GridParams), vp, lvp]
    L.suma_localizer_disable_live_grid.argtypes = [vp]
    L.suma_localizer_clear_live_grid.argtypes = [vp]
    L.suma_localizer_live_update_flags.argtypes = [vp, vp, vp, vp, u32, lcp]
    L.suma_localizer_live_counts.argtypes = [vp, lcp, C.POINTER(i32)]
    L.suma_localizer_live_cells_device.argtypes = [vp, vp, vp, C.POINTER(LiveStats)]
    L.suma_localizer_live_state.argtypes = [vp, vp, u32, C.POINTER(u32)]
    L.suma_localizer_set_live_state.argtypes = [vp, vp, u32, u32]
    dkp = C.POINTER(DeskewParams)
    L.suma_deskew_params_default.argtypes = [dkp]
    L.suma_deskew_params_default.restype = None
    L.suma_deskew_check.argtypes = [dkp, C.c_int, vp]
    L.suma_deskew_points.argtypes = [vp, dkp, vp, vp, u32, vp, vp]
    L.suma_deskew_points_device.argtypes = [vp, dkp, vp, vp, u32, vp, vp]
    for who in ("pipeline", "localizer"):
        getattr(L, f"suma_{who}_enable_deskew").argtypes = [vp, dkp]
        getattr(L, f"suma_{who}_disable_deskew").argtypes = [vp]
        getattr(L, f"suma_{who}_set_deskew_motion").argtypes = [vp, vp]
        getattr(L, f"suma_{who}_deskew_motion").argtypes = [vp, vp, C.POINTER(i32)]
    ppp, pmp = C.POINTER(PlaceParams), C.POINTER(PlaceMatch)
    L.suma_place_params_default.argtypes = [ppp]
    L.suma_place_params_default.restype = None
    L.suma_place_index_create.argtypes = [ppp, C.c_int, u32, pp]
    L.suma_place_index_destroy.argtypes = [vp]
    L.suma_place_index_destroy.restype = None
    L.suma_place_index_clear.argtypes = [vp]
    L.suma_place_index_size.argtypes = [vp]
    L.suma_place_index_size.restype = u32
    L.suma_place_index_last_error.argtypes = [vp]
    L.suma_place_index_last_error.restype = C.c_char_p
    L.suma_place_index_add_frame.argtypes = [vp, vp, vp, u32]
    L.suma_place_index_download.argtypes = [vp, u32, u32, vp, vp, vp]
    L.suma_place_index_upload.argtypes = [vp, vp, vp, u32]
    L.suma_place_index_query_frame.argtypes = [vp, vp, vp, u32, u32, u32, pmp, C.POINTER(u32)]
    L.suma_place_index_query.argtypes = [vp, vp, u32, u32, u32, pmp, C.POINTER(u32)]
    L.suma_place_index_query_all.argtypes = [vp, vp, vp, vp, vp]
    rrp = C.POINTER(RelocalizeResult)
    L.suma_localizer_relocalize.argtypes = [vp, vp, vp, u32, vp, vp, vp, u32, u32, i32, rrp]
    L.suma_localizer_relocalize_device.argtypes = [vp, vp, vp, u32, vp, vp, vp, u32, u32, i32, rrp]
    _LIB = L
    return L


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _cm(T, dtype):
    """row-major numpy 4x4 -> column-major (Eigen) buffer"""
    return np.ascontiguousarray(np.asarray(T, dtype=dtype).reshape(4, 4).T)


class Context:
    """One HIP device + stream + all device-resident state of the hot path (suma_ctx)."""

    def __init__(self, params: SumaParams, device: int = 0, handle=None, owner=None):
        self.L = lib()
        self.params = params
        self._owner = owner
        if handle is None:
            h = C.c_void_p()
            rc = self.L.suma_ctx_create(C.byref(params), device, C.byref(h))
            if rc != 0:
                raise SumaError(f"suma_ctx_create failed ({rc}): {self.L.suma_last_error(None).decode()}")
            self.h, self.owned = h, True
        else:
            self.h, self.owned = handle, False

    def check(self, rc: int, what: str = ""):
        if rc != 0:
            raise SumaError(f"{what} failed ({rc}): {self.L.suma_last_error(self.h).decode()}")

    def set_params(self, params: SumaParams):
        self.check(self.L.suma_set_params(self.h, C.byref(params)), "suma_set_params")
        self.params = params

    def synchronize(self):
        self.check(self.L.suma_synchronize(self.h), "suma_synchronize")

    @property
    def stream(self) -> int:
        return int(self.L.suma_ctx_stream(self.h) or 0)

    # device scratch for resident scans
    def device_array(self, host: np.ndarray) -> int:
        host = np.ascontiguousarray(host)
        p = C.c_void_p()
        self.check(self.L.suma_device_alloc(self.h, host.nbytes, C.byref(p)), "suma_device_alloc")
        self.check(self.L.suma_device_upload(self.h, p, _ptr(host), host.nbytes), "suma_device_upload")
        return p.value

    def device_download(self, d_ptr: int, nbytes: int) -> np.ndarray:
        """copy `nbytes` from a device address (e.g. an exported viewer buffer) to the host"""
        out = np.empty(nbytes, dtype=np.uint8)
        self.check(self.L.suma_device_download(self.h, _ptr(out), C.c_void_p(d_ptr), nbytes), "suma_device_download")
        return out

    def device_free(self, p: int):
        self.check(self.L.suma_device_free(self.h, C.c_void_p(p)), "suma_device_free")

    # profiling
    def profile(self, on):
        """0 / False: off, 1 / True: every kernel group, 2: only the Gauss-Newton chain (two events per scan)"""
        self.check(self.L.suma_profile_enable(self.h, int(on)))

    def profile_reset(self):
        self.check(self.L.suma_profile_reset(self.h))

    def profile_get(self):
        buf = (KernelTime * 64)()
        n = self.L.suma_profile_get(self.h, buf, 64)
        if n < 0:
            self.check(n, "suma_profile_get")
        return [dict(name=buf[i].name.decode(), launches=int(buf[i].launches), total_ms=float(buf[i].total_ms),
                     bytes=float(buf[i].bytes)) for i in range(min(n, 64))]

    def close(self):
        if getattr(self, "owned", False) and self.h:
            self.L.suma_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Frame:
    """Frame.h:21-79: vertex / normal / semantic maps (H x W x 4 float32, row 0 = lowest beam) in HBM."""

    def __init__(self, ctx: Context, width: int, height: int, handle=None):
        self.ctx, self.width, self.height = ctx, width, height
        if handle is None:
            h = C.c_void_p()
            ctx.check(ctx.L.suma_frame_create(ctx.h, width, height, C.byref(h)), "suma_frame_create")
            self.h, self.owned = h, True
        else:
            self.h, self.owned = C.c_void_p(handle), False

    def download(self, which: int) -> np.ndarray:
        out = np.empty((self.height, self.width, 4), dtype=np.float32)
        self.ctx.check(self.ctx.L.suma_frame_download(self.ctx.h, self.h, which, _ptr(out)), "suma_frame_download")
        return out

    def upload(self, which: int, data: np.ndarray):
        data = np.ascontiguousarray(data, dtype=np.float32).reshape(self.height, self.width, 4)
        self.ctx.check(self.ctx.L.suma_frame_upload(self.ctx.h, self.h, which, _ptr(data)), "suma_frame_upload")

    def set(self, vertex, normal, semantic):
        self.upload(0, vertex)
        self.upload(1, normal)
        self.upload(2, semantic)

    @property
    def vertex(self):
        return self.download(0)

    @property
    def normal(self):
        return self.download(1)

    @property
    def semantic(self):
        return self.download(2)

    def swap(self, other: "Frame"):
        """exchange contents with `other` (the shared_ptr swaps of SurfelMapping.cpp:323-331), O(1)"""
        self.ctx.check(self.ctx.L.suma_frame_swap(self.ctx.h, self.h, other.h), "suma_frame_swap")

    def export(self, which: int):
        """viewer feed: (device address, width, height, row_bytes) of one map"""
        p, w, h, rb = C.c_void_p(), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        self.ctx.check(self.ctx.L.suma_frame_export(self.ctx.h, self.h, which, C.byref(p), C.byref(w), C.byref(h),
                                                    C.byref(rb)), "suma_frame_export")
        return p.value, w.value, h.value, rb.value

    def touch(self):
        """the maps were written through an exported device pointer: tell the library (suma_frame_touch)"""
        self.ctx.check(self.ctx.L.suma_frame_touch(self.ctx.h, self.h), "suma_frame_touch")

    def copy(self, other: "Frame"):
        """Frame::copy (Frame.h:49-61)"""
        self.ctx.check(self.ctx.L.suma_frame_copy(self.ctx.h, self.h, other.h), "suma_frame_copy")

    def __del__(self):
        try:
            if getattr(self, "owned", False) and self.h and self.ctx.h:
                self.ctx.L.suma_frame_destroy(self.h)
                self.h = None
        except Exception:
            pass


class Preprocessing:
    """Preprocessing.h:47-58"""

    def __init__(self, ctx: Context):
        self.ctx = ctx

    def process(self, points, frame: Frame, labels, probs, timestamp: int) -> Frame:
        points = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 4)
        labels = None if labels is None else np.ascontiguousarray(labels, dtype=np.float32)
        probs = None if probs is None else np.ascontiguousarray(probs, dtype=np.float32)
        c = self.ctx
        c.check(c.L.suma_preprocess(c.h, _ptr(points), _ptr(labels), _ptr(probs), points.shape[0], timestamp, frame.h),
                "suma_preprocess")
        return frame


class Frame2Model:
    """Objective.h:14-82 as implemented by Frame2Model.h:28-73.

    Like the reference's object, an instance owns its parameters (icp-max-distance, icp-max-angle, weighting,
    factor, bilinear_sampling; Frame2Model::updateParameters, Frame2Model.cpp:65-110) and its frame pair, and sends
    both to the device before every launch -- two instances with different gates on one Context (objective_ and
    recovery_ = Frame2Model(fallback_params), SurfelMapping.cpp:87-94) do not disturb each other."""
    num_parameters = 6
    _PARAM_NAMES = {"icp-max-distance": "icp_max_distance", "icp-max-angle": "icp_max_angle", "factor": "factor",
                    "bilinear_sampling": "bilinear_sampling"}
    _WEIGHTING = {"none": 0, "huber": 1, "turkey": 2, "stability": 3}

    def __init__(self, ctx: Context, params: SumaParams = None):
        self.ctx = ctx
        p = ctx.params if params is None else params
        self.objective = IcpObjective(p.icp_max_distance, p.icp_max_angle, p.weight_function, p.factor,
                                      p.bilinear_sampling)
        self._current = self._last = None
        self._pose = np.eye(4)
        self._iteration = 0
        self.stats = IcpStats()
        self.acc = np.zeros(ACC_WORDS, dtype=np.int64)

    def setParameter(self, name: str, value):
        """Objective::setParameter(const rv::Parameter&) -> Frame2Model::setParameter (Frame2Model.cpp:112-115)"""
        if name == "weighting":
            self.objective.weight_function = self._WEIGHTING[value]
        elif name in self._PARAM_NAMES:
            setattr(self.objective, self._PARAM_NAMES[name], value)
        # other keys are stored by the reference and never read by this objective

    def setData(self, current: Frame, last: Frame):
        self._current, self._last = current, last  # keep alive
        self._iteration = 0

    def _bind(self):
        """this object's frames and parameters become the ones the next launch uses"""
        if self._current is None:
            raise SumaError("Frame2Model::setData has not been called")
        c = self.ctx
        c.check(c.L.suma_icp_set_data(c.h, self._current.h, self._last.h), "suma_icp_set_data")
        c.check(c.L.suma_icp_set_objective(c.h, C.byref(self.objective)), "suma_icp_set_objective")

    def initialize(self, pose):
        """Objective::initialize (Objective.h:58): the pose and nothing else -- iteration_ is reset by setData only"""
        self._pose = np.asarray(pose, dtype=np.float64).copy()

    def pose(self):
        return self._pose

    def jacobianProducts(self):
        """returns (F, JtJ[6,6], Jtf[6]); updates inlier()/outlier()/valid()/invalid()"""
        JtJ = np.zeros((6, 6), dtype=np.float64)
        Jtr = np.zeros(6, dtype=np.float64)
        pose = _cm(self._pose, np.float64)
        c = self.ctx
        self._bind()
        c.check(c.L.suma_icp_jacobian_products(c.h, _ptr(pose), self._iteration, _ptr(JtJ), _ptr(Jtr), _ptr(self.acc),
                                               C.byref(self.stats)), "suma_icp_jacobian_products")
        return self.stats.error, JtJ.T.copy(), Jtr

    def increment(self, delta):
        """Objective::increment (Objective.h:45-48): pose_ = SE3::exp(delta) * pose_ (host side, numpy)"""
        self._pose = se3_exp(delta) @ self._pose
        self._iteration += 1

    def inlier(self):
        return self.stats.inlier

    def outlier(self):
        return self.stats.outlier

    def valid(self):
        return self.stats.valid

    def invalid(self):
        return self.stats.invalid

    def inlier_residual(self):
        return self.stats.inlier_residual


class LieGaussNewton:
    """LieGaussNewton.h:25-76: the loop itself runs on the device (one readback per minimize)."""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self._pose = np.eye(4)
        self._history = np.zeros((0, 4, 4))
        self.stats = IcpStats()

    def minimize(self, objective: Frame2Model, T0, history_cap: int = 64) -> int:
        T0 = _cm(T0, np.float64)
        T = np.zeros((4, 4), dtype=np.float64)
        nh = C.c_uint32(0)
        c = self.ctx
        objective._bind()
        # Frame2Model::iteration_ runs on across minimisations on one setData (SurfelMapping.cpp:693-700)
        c.check(c.L.suma_icp_set_iteration(c.h, objective._iteration), "suma_icp_set_iteration")
        # the pose history stays on the device until history() asks for it (suma_icp_history)
        c.check(c.L.suma_icp_minimize(c.h, _ptr(T0), _ptr(T), None, 0, C.byref(nh), C.byref(self.stats)), "suma_icp_minimize")
        self._pose = T.T.copy()
        objective._pose = self._pose
        objective.stats = self.stats
        objective._iteration += self.stats.iterations + (1 if self.stats.converged else 0)  # one increment per step
        self._history, self._history_cap = None, history_cap
        self._history_seq = c.L.suma_icp_history_sequence(c.h)
        return 0

    def minimize_batch(self, T0s, objective: Frame2Model = None):
        """n_hyp minimisations of the same frame pair (SurfelMapping.cpp:662-779 pattern)"""
        T0s = np.ascontiguousarray(np.asarray(T0s, dtype=np.float64).reshape(-1, 4, 4).transpose(0, 2, 1))
        n = T0s.shape[0]
        out = np.zeros((n, 4, 4), dtype=np.float64)
        stats = (IcpStats * n)()
        c = self.ctx
        if objective is not None:
            objective._bind()
        c.check(c.L.suma_icp_minimize_batch(c.h, _ptr(T0s), n, _ptr(out), stats), "suma_icp_minimize_batch")
        return out.transpose(0, 2, 1).copy(), [stats[i].as_dict() for i in range(n)]

    def pose(self):
        return self._pose

    def history(self):
        if self._history is None:
            if self.ctx.L.suma_icp_history_sequence(self.ctx.h) != self._history_seq:
                raise RuntimeError("LieGaussNewton.history: a later minimisation on this context has overwritten the "
                                   "device-side history; call history() before it")
            cap = self._history_cap
            hist = np.zeros((max(cap, 1), 4, 4), dtype=np.float64)
            nh = C.c_uint32(0)
            self.ctx.check(self.ctx.L.suma_icp_history(self.ctx.h, _ptr(hist), cap, C.byref(nh)), "suma_icp_history")
            self._history = hist[:min(nh.value, cap)].transpose(0, 2, 1).copy()
        return self._history

    def iterationCount(self):
        return self.stats.iterations

    def information(self):
        """LieGaussNewton::information() (LieGaussNewton.cpp:75,103-105): J^T W J of the last step"""
        out = np.zeros((6, 6), dtype=np.float64)
        self.ctx.check(self.ctx.L.suma_icp_information(self.ctx.h, _ptr(out)), "suma_icp_information")
        return out.T.copy()

    @staticmethod
    def reason(errorno: int) -> str:
        """LieGaussNewton::reason (LieGaussNewton.cpp:110-115)"""
        return {-1: "Maximum number of iterations reached.", -2: "Diverging."}.get(errorno, "no error")


def se3_exp(x):
    """SE3::exp (lie_algebra.cpp:4-34) on the host in numpy, for Objective::increment of the mirror classes"""
    x = np.asarray(x, dtype=np.float64)
    T = np.eye(4)
    v, o = x[:3], x[3:]
    theta = float(np.sqrt(o @ o))
    if theta > 1e-10:
        K = np.array([[0, -o[2], o[1]], [o[2], 0, -o[0]], [-o[1], o[0], 0]])
        K2 = K @ K
        T[:3, :3] = np.eye(3) + np.sin(theta) / theta * K + (1 - np.cos(theta)) / theta ** 2 * K2
        V = np.eye(3) + (1 - np.cos(theta)) / theta ** 2 * K + (theta - np.sin(theta)) / theta ** 3 * K2
        T[:3, 3] = V @ v
    else:
        T[:3, 3] = v
    return T


# ---- camera helpers for SurfelMap.draw (row-major numpy 4x4, float64; mvp = projection @ view @ ROSE2GL)
# the viewport's conversion_ from the robot frame (x forward, y left, z up) to GL (x right, y up, z backwards):
# GL x = -y, GL y = z, GL z = -x
ROSE2GL = np.array([[0.0, -1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [-1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0]])


def perspective(fovy_deg: float, aspect: float, near: float, far: float) -> np.ndarray:
    """gluPerspective (the viewport's camera: 45 degrees, near 0.1, far 10000, ViewportWidget.cpp:484-487)"""
    f = 1.0 / np.tan(np.radians(fovy_deg) / 2.0)
    return np.array([[f / aspect, 0.0, 0.0, 0.0], [0.0, f, 0.0, 0.0],
                     [0.0, 0.0, (far + near) / (near - far), 2.0 * far * near / (near - far)], [0.0, 0.0, -1.0, 0.0]])


def orthographic(left: float, right: float, bottom: float, top: float, near: float, far: float) -> np.ndarray:
    """glOrtho"""
    return np.array([[2.0 / (right - left), 0.0, 0.0, -(right + left) / (right - left)],
                     [0.0, 2.0 / (top - bottom), 0.0, -(top + bottom) / (top - bottom)],
                     [0.0, 0.0, -2.0 / (far - near), -(far + near) / (far - near)], [0.0, 0.0, 0.0, 1.0]])


def look_at(eye, target, up) -> np.ndarray:
    """gluLookAt: the view matrix of a camera at `eye` looking at `target` (all in the frame the matrix maps from)"""
    eye, target, up = (np.asarray(v, dtype=np.float64).reshape(3) for v in (eye, target, up))
    f = target - eye
    f = f / np.linalg.norm(f)
    s = np.cross(f, up)
    s = s / np.linalg.norm(s)
    u = np.cross(s, f)
    V = np.eye(4)
    V[0, :3], V[1, :3], V[2, :3] = s, u, -f
    V[:3, 3] = -V[:3, :3] @ eye
    return V


def draw_params(mvp, width: int, height: int, view_pos, color_mode: int = 5, color_map=None,
                conf_threshold: float = 10.0, backface_culling: bool = False, use_stability: bool = False,
                clear_color=(1.0, 1.0, 1.0, 1.0), lights=None, material=None) -> DrawParams:
    """a suma_draw_params: ``mvp`` row-major 4x4 (projection @ view @ ROSE2GL for the viewer's camera), ``view_pos`` the
    camera position in the map frame, ``color_map`` [260, 3] uint8 RGB (default kitti.semantic_color_map()); lights and
    material default to what SurfelMap's constructor leaves (types.DRAW_LIGHTS[:1], types.DRAW_MATERIAL)"""
    from .kitti import semantic_color_map
    dp = DrawParams()
    m = _cm(mvp, np.float32).reshape(-1)
    for k in range(16):
        dp.mvp[k] = float(m[k])
    for k, v in enumerate(np.asarray(view_pos, dtype=np.float32).reshape(3)):
        dp.view_pos[k] = float(v)
    dp.width, dp.height = int(width), int(height)
    dp.color_mode, dp.conf_threshold = int(color_mode), float(conf_threshold)
    dp.backface_culling, dp.use_stability = int(bool(backface_culling)), int(bool(use_stability))
    for k, v in enumerate(clear_color):
        dp.clear_color[k] = float(v)
    lights = DRAW_LIGHTS[:1] if lights is None else list(lights)
    dp.num_lights = len(lights)
    for i, L in enumerate(lights[:DRAW_MAX_LIGHTS]):
        for name in ("position", "ambient", "diffuse", "specular"):
            arr = getattr(dp.lights[i], name)
            for k, v in enumerate(L[name]):
                arr[k] = float(v)
    mat = dict(DRAW_MATERIAL, **(material or {}))
    for name in ("ambient", "diffuse", "specular", "emission"):
        arr = getattr(dp, "mat_" + name)
        for k, v in enumerate(mat[name]):
            arr[k] = float(v)
    dp.mat_shininess, dp.mat_alpha = float(mat["shininess"]), float(mat["alpha"])
    cmap = semantic_color_map() if color_map is None else np.asarray(color_map, dtype=np.uint8)
    assert cmap.shape == (DRAW_COLORS, 3), cmap.shape
    C.memmove(C.addressof(dp.color_map), np.ascontiguousarray(cmap).ctypes.data, DRAW_COLORS * 3)
    return dp


def _dev(p):
    """a device address: an int, or anything with data_ptr() (a torch tensor on the ctx's device)"""
    if hasattr(p, "data_ptr"):
        return C.c_void_p(p.data_ptr())
    return None if p is None or int(p) == 0 else C.c_void_p(int(p))


def world_grid(ctx: "Context", records, n: int = None, params: GridParams = None, fit_margin: int = None, **kw):
    """The 2.5-D semantic traversability grid of world-frame records (suma_world_grid; csrc/k_grid.hip states the rules):
    -> (cells[height, width] of GRID_CELL_DTYPE, row = y, the GridParams used, the stats as a dict).  ``records``: a
    WORLD_SURFEL_DTYPE array (uploaded for the call), or a device address / torch tensor with ``n`` records.  ``params``:
    a GridParams, or the keywords of GridParams.defaults.  The raster is fitted to the records (suma_world_grid_fit, with
    ``fit_margin`` empty cells around them, default 1) when ``fit_margin`` is given or the parameters carry no size."""
    gp = GridParams.defaults(**kw) if params is None else GridParams.from_buffer_copy(params)
    L, h = ctx.L, ctx.h
    owned = None
    if isinstance(records, np.ndarray):
        rec = np.ascontiguousarray(records, dtype=WORLD_SURFEL_DTYPE).reshape(-1)
        n = rec.shape[0] if n is None else int(n)
        if n > rec.shape[0]:
            raise ValueError("world_grid: n exceeds the records given")
        d_rec = owned = ctx.device_array(rec[:n]) if n else None
    else:
        if n is None:
            raise ValueError("world_grid: n is needed with a device address")
        d_rec = records
    d_cells = C.c_void_p()
    try:
        if fit_margin is not None or gp.width == 0 or gp.height == 0:
            ctx.check(L.suma_world_grid_fit(h, _dev(d_rec), n, 1 if fit_margin is None else int(fit_margin), C.byref(gp)),
                      "suma_world_grid_fit")
        cells = np.zeros((gp.height, gp.width), dtype=GRID_CELL_DTYPE)
        st = GridStats()
        ctx.check(L.suma_device_alloc(h, max(cells.nbytes, 48), C.byref(d_cells)), "suma_device_alloc")
        ctx.check(L.suma_world_grid(h, C.byref(gp), _dev(d_rec), n, d_cells, C.byref(st)), "suma_world_grid")
        ctx.check(L.suma_device_download(h, _ptr(cells), d_cells, cells.nbytes), "suma_device_download")
    finally:
        if d_cells:
            L.suma_device_free(h, d_cells)
        if owned:
            L.suma_device_free(h, C.c_void_p(owned))
    return cells, gp, st.as_dict()


def grid_cell_index(gp: GridParams, x: float, y: float) -> int:
    """the cell iy * width + ix of a world position in the grid's own fp32 expression (suma_grid_cell_index); -1 outside
    the raster or for a non-finite coordinate"""
    return int(lib().suma_grid_cell_index(C.byref(gp), float(x), float(y)))


def _cell_indices(v, what: str) -> np.ndarray:
    a = np.ascontiguousarray(np.asarray(v, dtype=np.int64).reshape(-1))
    if a.size == 0:
        raise ValueError(f"{what}: no cell given")
    return a


def grid_plan(ctx: "Context", cells, gp: GridParams, goals, params: PlanParams = None, field_out=None, **kw):
    """Clearance, traversability and the cost-to-go field of a traversability grid (suma_grid_plan_field; csrc/k_plan.hip
    states the rules): -> (field[height, width] of PLAN_CELL_DTYPE, the stats as a dict).  ``cells``: the GRID_CELL_DTYPE
    array of core.world_grid (uploaded for the call), or a device address / torch tensor of gp.width * gp.height cells.
    ``goals``: cell indices (grid_cell_index makes one of a world position).  ``params``: a PlanParams, or the keywords
    of PlanParams.defaults.  ``field_out``: a device address to leave the field at; the return is then (None, stats)."""
    pp = PlanParams.defaults(**kw) if params is None else PlanParams.from_buffer_copy(params)
    g = _cell_indices(goals, "grid_plan")
    L, h = ctx.L, ctx.h
    n_cells = int(gp.width) * int(gp.height)
    owned, d_field = None, C.c_void_p()
    if isinstance(cells, np.ndarray):
        arr = np.ascontiguousarray(cells, dtype=GRID_CELL_DTYPE).reshape(-1)
        if arr.shape[0] != n_cells:
            raise ValueError(f"grid_plan: {arr.shape[0]} cells against a raster of {gp.height} x {gp.width}")
        cells = owned = ctx.device_array(arr)
    st = PlanStats()
    try:
        if field_out is None:
            ctx.check(L.suma_device_alloc(h, n_cells * PLAN_CELL_DTYPE.itemsize, C.byref(d_field)), "suma_device_alloc")
        ctx.check(L.suma_grid_plan_field(h, C.byref(gp), C.byref(pp), _dev(cells), _ptr(g), g.shape[0],
                                         d_field if field_out is None else _dev(field_out), C.byref(st)), "suma_grid_plan_field")
        field = None
        if field_out is None:
            field = np.zeros((gp.height, gp.width), dtype=PLAN_CELL_DTYPE)
            ctx.check(L.suma_device_download(h, _ptr(field), d_field, field.nbytes), "suma_device_download")
    finally:
        if d_field:
            L.suma_device_free(h, d_field)
        if owned:
            L.suma_device_free(h, C.c_void_p(owned))
    return field, st.as_dict()


def grid_paths(ctx: "Context", field, gp: GridParams, starts, capacity: int = None):
    """The paths from ``starts`` (cell indices; negative or beyond the raster: START_OUTSIDE) down a field of grid_plan
    (suma_grid_plan_paths): -> (results of PLAN_PATH_DTYPE [n], path cells uint32 [n, capacity], the start first, 0xffffffff
    behind a path's end).  ``field``: the PLAN_CELL_DTYPE array (uploaded for the call) or a device address / torch
    tensor.  ``capacity``: cells of room per path, default width + height (a path longer than that is TRUNCATED and
    reports its full length)."""
    s = _cell_indices(starts, "grid_paths")
    L, h = ctx.L, ctx.h
    capacity = int(gp.width) + int(gp.height) if capacity is None else int(capacity)
    owned = None
    if isinstance(field, np.ndarray):
        arr = np.ascontiguousarray(field, dtype=PLAN_CELL_DTYPE).reshape(-1)
        if arr.shape[0] != int(gp.width) * int(gp.height):
            raise ValueError(f"grid_paths: {arr.shape[0]} cells against a raster of {gp.height} x {gp.width}")
        field = owned = ctx.device_array(arr)
    results = np.zeros(s.shape[0], dtype=PLAN_PATH_DTYPE)
    path_cells = np.zeros((s.shape[0], max(capacity, 0)), dtype=np.uint32)
    try:
        ctx.check(L.suma_grid_plan_paths(h, C.byref(gp), _dev(field), _ptr(s), s.shape[0], max(capacity, 0), _ptr(path_cells),
                                         _ptr(results)), "suma_grid_plan_paths")
    finally:
        if owned:
            L.suma_device_free(h, C.c_void_p(owned))
    return results, path_cells


class GridPlanner:
    """A traversability grid and its cost-to-go field kept on the device: goals and starts are world (x, y), a path comes
    back as the world coordinates of its cells' centres with its cost.

        planner = GridPlanner(ctx, cells, gp, robot_radius=0.4)
        stats = planner.set_goals([(x, y)])
        xy, cost, status = planner.path((x0, y0))"""

    def __init__(self, ctx: "Context", cells: np.ndarray, gp: GridParams, params: PlanParams = None, **kw):
        self.ctx, self.gp = ctx, GridParams.from_buffer_copy(gp)
        self.params = PlanParams.defaults(**kw) if params is None else PlanParams.from_buffer_copy(params)
        arr = np.ascontiguousarray(cells, dtype=GRID_CELL_DTYPE).reshape(-1)
        if arr.shape[0] != int(gp.width) * int(gp.height):
            raise ValueError(f"GridPlanner: {arr.shape[0]} cells against a raster of {gp.height} x {gp.width}")
        self._cells = ctx.device_array(arr)
        self._field = ctx.device_array(np.zeros(arr.shape[0], dtype=PLAN_CELL_DTYPE))
        self.stats = None

    def close(self):
        for name in ("_cells", "_field"):
            if getattr(self, name, None):
                self.ctx.device_free(getattr(self, name))
                setattr(self, name, None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def cell(self, xy) -> int:
        return grid_cell_index(self.gp, xy[0], xy[1])

    def centre(self, cells) -> np.ndarray:
        """world (x, y) of the centres of cells given by index: float64 [n, 2]"""
        c = np.asarray(cells, dtype=np.int64).reshape(-1)
        ix, iy = c % self.gp.width, c // self.gp.width
        return np.stack([self.gp.origin_x + (ix + 0.5) * self.gp.cell_size, self.gp.origin_y + (iy + 0.5) * self.gp.cell_size], axis=1)

    def set_goals(self, goals_xy) -> dict:
        """the field towards these world positions; one outside the raster is an error.  -> the stats"""
        g = [self.cell(xy) for xy in np.asarray(goals_xy, dtype=np.float64).reshape(-1, 2)]
        if min(g) < 0:
            raise ValueError("GridPlanner.set_goals: a goal lies outside the raster")
        _, self.stats = grid_plan(self.ctx, self._cells, self.gp, g, self.params, field_out=self._field)
        return self.stats

    def field(self) -> np.ndarray:
        """the field [height, width] of PLAN_CELL_DTYPE, downloaded"""
        if self.stats is None:
            raise SumaError("GridPlanner.field: no goals set")
        n = int(self.gp.width) * int(self.gp.height) * PLAN_CELL_DTYPE.itemsize
        return self.ctx.device_download(self._field, n).view(PLAN_CELL_DTYPE).reshape(self.gp.height, self.gp.width)

    def paths(self, starts_xy, capacity: int = None):
        """-> a list of (xy float64 [length, 2], cost, status) per start; xy is empty unless the status is PATH_OK or
        PATH_TRUNCATED (then it holds the first ``capacity`` cells)"""
        if self.stats is None:
            raise SumaError("GridPlanner.paths: no goals set")
        s = [self.cell(xy) for xy in np.asarray(starts_xy, dtype=np.float64).reshape(-1, 2)]
        res, cells = grid_paths(self.ctx, self._field, self.gp, s, capacity)
        out = []
        for r, row in zip(res, cells):
            keep = min(int(r["length"]), row.shape[0]) if int(r["status"]) in (PATH_OK, PATH_TRUNCATED) else 0
            out.append((self.centre(row[:keep]), int(r["cost"]), int(r["status"])))
        return out

    def path(self, start_xy, capacity: int = None):
        return self.paths([start_xy], capacity)[0]


class SurfelMap:
    """SurfelMap.h:36-78"""

    def __init__(self, ctx: Context):
        self.ctx = ctx

    def reset(self):
        self.ctx.check(self.ctx.L.suma_map_reset(self.ctx.h), "suma_map_reset")

    def update(self, pose, frame: Frame):
        p = _cm(pose, np.float32)
        self.ctx.check(self.ctx.L.suma_map_update(self.ctx.h, _ptr(p), frame.h), "suma_map_update")

    def render(self, pose_old, pose_new, frame: Frame, confidence_threshold: float):
        po, pn = _cm(pose_old, np.float32), _cm(pose_new, np.float32)
        self.ctx.check(self.ctx.L.suma_map_render(self.ctx.h, _ptr(po), _ptr(pn), confidence_threshold, frame.h),
                       "suma_map_render")
        return frame

    def render_active(self, pose, confidence_threshold: float):
        p = _cm(pose, np.float32)
        self.ctx.check(self.ctx.L.suma_map_render_active(self.ctx.h, _ptr(p), confidence_threshold))

    def render_inactive(self, pose, confidence_threshold: float):
        p = _cm(pose, np.float32)
        self.ctx.check(self.ctx.L.suma_map_render_inactive(self.ctx.h, _ptr(p), confidence_threshold))

    def render_composed(self, pose_old, pose_new, confidence_threshold: float):
        po, pn = _cm(pose_old, np.float32), _cm(pose_new, np.float32)
        self.ctx.check(self.ctx.L.suma_map_render_composed(self.ctx.h, _ptr(po), _ptr(pn), confidence_threshold))

    def _frame(self, which):
        p = self.ctx.params
        return Frame(self.ctx, p.model_width, p.model_height, handle=self.ctx.L.suma_map_frame(self.ctx.h, which))

    def oldMapFrame(self):
        return self._frame(0)

    def newMapFrame(self):
        return self._frame(1)

    def composedFrame(self):
        return self._frame(2)

    def updatePoses(self, poses):
        poses = np.ascontiguousarray(np.asarray(poses, dtype=np.float32).reshape(-1, 4, 4).transpose(0, 2, 1))
        self.ctx.check(self.ctx.L.suma_map_update_poses(self.ctx.h, _ptr(poses), poses.shape[0]))

    def size(self) -> int:
        n = C.c_uint32(0)
        self.ctx.check(self.ctx.L.suma_map_size(self.ctx.h, C.byref(n)), "suma_map_size")
        return n.value

    def timestamp(self) -> int:
        t = C.c_uint32(0)
        self.ctx.check(self.ctx.L.suma_map_timestamp(self.ctx.h, C.byref(t)))
        return t.value

    def getAllSurfels(self) -> np.ndarray:
        n = self.size()
        out = np.zeros(n, dtype=SURFEL_DTYPE)
        got = C.c_uint32(0)
        self.ctx.check(self.ctx.L.suma_map_download(self.ctx.h, _ptr(out) if n else None, n, C.byref(got)))
        return out

    def getModelSurfels(self):
        """SurfelMap::getModelSurfels (SurfelMap.h:67) / the VBO SurfelMap::draw reads: (device address, count) of the
        active map, 64-byte records; valid until the next update / upload / reset"""
        p, n = C.c_void_p(), C.c_uint32(0)
        self.ctx.check(self.ctx.L.suma_map_export_surfels(self.ctx.h, C.byref(p), C.byref(n)), "suma_map_export_surfels")
        return p.value, n.value

    def draw_device(self, d_rgba8, d_ids=None, mvp=None, width: int = 0, height: int = 0, view_pos=(0.0, 0.0, 0.0),
                    params: DrawParams = None, **options):
        """SurfelMap::draw (SurfelMap.cpp:1167-1230) into caller-owned device buffers (suma_map_draw): ``d_rgba8`` width x
        height x 4 bytes, ``d_ids`` (optional) width x height int32; rows in glReadPixels order (row 0 = bottom).  Takes
        a prepared ``params`` (draw_params) or builds one from the arguments.  Enqueued on the ctx stream, not waited for."""
        dp = params if params is not None else draw_params(mvp, width, height, view_pos, **options)
        self.ctx.check(self.ctx.L.suma_map_draw(self.ctx.h, C.byref(dp), _dev(d_rgba8), _dev(d_ids)), "suma_map_draw")
        return dp

    def draw(self, mvp, width: int, height: int, view_pos, color_mode: int = 5, color_map=None, ids: bool = False,
             **options):
        """SurfelMap::draw as a picture: uint8 [height, width, 4] RGBA with row 0 at the TOP (ready to save), and with
        ``ids=True`` also the int32 [height, width] index of the surfel drawn at each pixel (-1: none).  ``options``:
        conf_threshold, backface_culling, use_stability, clear_color, lights, material (draw_params)."""
        dp = draw_params(mvp, width, height, view_pos, color_mode=color_mode, color_map=color_map, **options)
        P = int(width) * int(height)
        d_rgba = C.c_void_p()
        d_ids = C.c_void_p()
        L, h = self.ctx.L, self.ctx.h
        self.ctx.check(L.suma_device_alloc(h, 4 * P, C.byref(d_rgba)), "suma_device_alloc")
        try:
            if ids:
                self.ctx.check(L.suma_device_alloc(h, 4 * P, C.byref(d_ids)), "suma_device_alloc")
            self.ctx.check(L.suma_map_draw(h, C.byref(dp), d_rgba, d_ids if ids else None), "suma_map_draw")
            img = np.empty((int(height), int(width), 4), dtype=np.uint8)
            self.ctx.check(L.suma_device_download(h, _ptr(img), d_rgba, 4 * P), "suma_device_download")
            idm = None
            if ids:
                idm = np.empty((int(height), int(width)), dtype=np.int32)
                self.ctx.check(L.suma_device_download(h, _ptr(idm), d_ids, 4 * P), "suma_device_download")
        finally:
            L.suma_device_free(h, d_rgba)
            if d_ids.value:
                L.suma_device_free(h, d_ids)
        img = img[::-1].copy()
        return (img, idm[::-1].copy()) if ids else img

    def getDataSurfels(self):
        """SurfelMap::getDataSurfels (SurfelMap.h:64): (device address, first, count) -- the new surfels of the last
        update that survived the active-area copy, stored as the tail of the active map"""
        p, f, n = C.c_void_p(), C.c_uint32(0), C.c_uint32(0)
        self.ctx.check(self.ctx.L.suma_map_export_data_surfels(self.ctx.h, C.byref(p), C.byref(f), C.byref(n)),
                       "suma_map_export_data_surfels")
        return p.value, f.value, n.value

    def upload(self, surfels: np.ndarray, timestamp: int):
        surfels = np.ascontiguousarray(surfels, dtype=SURFEL_DTYPE)
        self.ctx.check(self.ctx.L.suma_map_upload(self.ctx.h, _ptr(surfels), surfels.shape[0], timestamp))

    # intermediates of the last update (parity tests)
    def index_map(self):
        p = self.ctx.params
        out = np.zeros((p.data_height, p.data_width), dtype=np.uint32)
        self.ctx.check(self.ctx.L.suma_map_download_index_map(self.ctx.h, _ptr(out)))
        return out

    def poses(self):
        """the pose table (SurfelMap::poses_): [timestamp, 4, 4] float32, one pose per integrated scan"""
        t = C.c_uint32(0)
        self.ctx.check(self.ctx.L.suma_map_timestamp(self.ctx.h, C.byref(t)))
        out = np.zeros((max(t.value, 1), 16), dtype=np.float32)
        n = C.c_uint32(0)
        self.ctx.check(self.ctx.L.suma_map_download_poses(self.ctx.h, _ptr(out), t.value, C.byref(n)), "suma_map_download_poses")
        return out[:min(n.value, t.value)].reshape(-1, 4, 4).transpose(0, 2, 1).copy()

    def radius_conf(self):
        p = self.ctx.params
        out = np.zeros((p.data_height, p.data_width, 4), dtype=np.float32)
        self.ctx.check(self.ctx.L.suma_map_download_radius_conf(self.ctx.h, _ptr(out)))
        return out

    def integrated(self):
        p = self.ctx.params
        out = np.zeros((p.data_height, p.data_width), dtype=np.uint8)
        self.ctx.check(self.ctx.L.suma_map_download_integrated(self.ctx.h, _ptr(out)))
        return out

    def cache_stats(self):
        """(surfels allocated from the submap cache arena, its capacity, compactions so far)"""
        a, b, cc = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        self.ctx.check(self.ctx.L.suma_map_cache_stats(self.ctx.h, C.byref(a), C.byref(b), C.byref(cc)))
        return a.value, b.value, cc.value

    def cached_tile(self, i: int, j: int) -> np.ndarray:
        """submapCache_(i, j).surfels (SurfelMap.h:186): the records parked for one tile, (n, 16) float32"""
        n = C.c_uint32(0)
        self.ctx.check(self.ctx.L.suma_map_download_cached_tile(self.ctx.h, i, j, None, 0, C.byref(n)))
        out = np.zeros((n.value, 16), dtype=np.float32)
        if n.value:
            self.ctx.check(self.ctx.L.suma_map_download_cached_tile(self.ctx.h, i, j, _ptr(out), n.value, C.byref(n)))
        return out

    def cached_tiles(self):
        """the (i, j) of every parked submap tile that holds records, ascending by (i, then j) (suma_map_cached_tiles)"""
        n = C.c_uint32(0)
        self.ctx.check(self.ctx.L.suma_map_cached_tiles(self.ctx.h, None, 0, C.byref(n)), "suma_map_cached_tiles")
        ij = np.zeros((n.value, 2), dtype=np.int32)
        if n.value:
            self.ctx.check(self.ctx.L.suma_map_cached_tiles(self.ctx.h, _ptr(ij), n.value, C.byref(n)),
                           "suma_map_cached_tiles")
        return [(int(i), int(j)) for i, j in ij[:n.value]]

    def export_world_device(self, params: WorldParams, d_out, capacity: int) -> WorldStats:
        """suma_map_export_world into a caller-owned device buffer of ``capacity`` 48-byte records (``d_out`` may be None
        with capacity 0: a size query); the stats tell how many records exist (n_out)"""
        st = WorldStats()
        self.ctx.check(self.ctx.L.suma_map_export_world(self.ctx.h, C.byref(params), _dev(d_out), capacity, C.byref(st)),
                       "suma_map_export_world")
        return st

    def export_world(self, voxel_size: float = 0.0, min_confidence=None, keep_labels=None, stats: bool = False):
        """The whole map -- active surfels and every parked tile -- in the world frame as WORLD_SURFEL_DTYPE records:
        one per surfel with ``confidence > min_confidence`` and a label in ``keep_labels`` (None: all), or with
        ``voxel_size > 0`` one per occupied voxel (the most confident member, a weighted label vote, the member count
        in ``support``).  Computed on the device (k_world.hip states the rules).  ``stats=True``: (records, dict)."""
        wp = WorldParams.defaults(voxel_size, min_confidence, keep_labels)
        L, h = self.ctx.L, self.ctx.h
        # the export runs once into a buffer of a guessed size (what the last export of this map needed, with headroom),
        # and a second time only when that was too small
        cap = max(int(getattr(self, "_world_capacity", 0)), 1 << 16)
        for attempt in range(2):
            d = C.c_void_p()
            self.ctx.check(L.suma_device_alloc(h, cap * WORLD_SURFEL_DTYPE.itemsize, C.byref(d)), "suma_device_alloc")
            try:
                st = self.export_world_device(wp, d.value, cap)
                if st.n_out <= cap:
                    out = np.zeros(st.n_out, dtype=WORLD_SURFEL_DTYPE)
                    if st.n_out:
                        self.ctx.check(L.suma_device_download(h, _ptr(out), d, out.nbytes), "suma_device_download")
                    break
            finally:
                L.suma_device_free(h, d)
            if attempt:
                raise SumaError("suma_map_export_world: the map changed between two exports")
            cap = st.n_out
        self._world_capacity = st.n_out + st.n_out // 4
        return (out, st.as_dict()) if stats else out

    def export_grid(self, cell_size: float = 0.2, params: GridParams = None, fit_margin: int = None,
                    min_confidence=None, keep_labels=None, **kw):
        """The traversability grid of the whole map (core.world_grid): the flat world export (``min_confidence``,
        ``keep_labels`` as export_world) into a device buffer, gridded there -- the records never visit the host.
        ``params`` / ``fit_margin`` / the keywords are world_grid's.  -> (cells[height, width], GridParams, stats dict)"""
        wp = WorldParams.defaults(0.0, min_confidence, keep_labels)
        L, h = self.ctx.L, self.ctx.h
        n = self.export_world_device(wp, None, 0).n_out  # the size
        d = C.c_void_p()
        self.ctx.check(L.suma_device_alloc(h, max(n, 1) * WORLD_SURFEL_DTYPE.itemsize, C.byref(d)), "suma_device_alloc")
        try:
            st = self.export_world_device(wp, d.value, n)
            if st.n_out != n:
                raise SumaError("suma_map_export_world: the map changed between two exports")
            if params is None:
                kw = dict(kw, cell_size=cell_size)
            return world_grid(self.ctx, d.value, n, params, fit_margin, **kw)
        finally:
            L.suma_device_free(h, d)

    def counts(self):
        """(S' survivors of K9, D new surfels of K10, surfels parked in submap caches, submap origin)"""
        a, b, cc = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        ij = np.zeros(2, dtype=np.int32)
        self.ctx.check(self.ctx.L.suma_map_counts(self.ctx.h, C.byref(a), C.byref(b), C.byref(cc), _ptr(ij)))
        return a.value, b.value, cc.value, (int(ij[0]), int(ij[1]))


def loop_closure_verify(ctx: Context, current: Frame, pose_prior, initializations, pose_new, conf_threshold: float,
                        min_valid_ratio: float = 0.2, max_outlier_ratio: float = 0.85, serial: bool = False):
    """device side of SurfelMapping::checkLoopClosure (SurfelMapping.cpp:662-757); returns one dict per guess.
    The guesses run as one batched Gauss-Newton chain; serial=True is the reference's one-by-one sequencing (same bits)."""
    prior = _cm(pose_prior, np.float64)
    inits = np.ascontiguousarray(np.asarray(initializations, dtype=np.float64).reshape(-1, 4, 4).transpose(0, 2, 1))
    pn = _cm(pose_new, np.float32)
    n = inits.shape[0]
    res = (LoopResult * n)()
    fn = ctx.L.suma_loop_closure_verify_serial if serial else ctx.L.suma_loop_closure_verify
    ctx.check(fn(ctx.h, current.h, _ptr(prior), _ptr(inits), n, _ptr(pn), conf_threshold, min_valid_ratio,
                 max_outlier_ratio, res), "suma_loop_closure_verify")
    return _loop_results(res, n)


def _loop_results(res, n):
    out = []
    for k in range(n):
        r = res[k]
        out.append(dict(gn_pose=np.array(r.gn_pose[:]).reshape(4, 4).T.copy(), after_minimize=r.after_minimize.as_dict(),
                        passed=bool(r.passed), pose_old=np.array(r.pose_old[:], dtype=np.float32).reshape(4, 4).T.copy(),
                        composed=r.composed.as_dict(), JtJ=np.array(r.JtJ[:]).reshape(6, 6).T.copy()))
    return out


def _loop_track(r):
    return dict(increment_old=np.array(r.increment_old[:]).reshape(4, 4).T.copy(), after_minimize=r.after_minimize.as_dict(),
                increment_difference=float(r.increment_difference), passed=bool(r.passed),
                pose_old=np.array(r.pose_old[:]).reshape(4, 4).T.copy(), composed=r.composed.as_dict(),
                JtJ=np.array(r.JtJ[:]).reshape(6, 6).T.copy())


def se3_log(T):
    """SE3::log (lie_algebra.cpp:36-71) as the library computes it on the host"""
    Tc = _cm(T, np.float64)
    x = np.zeros(6)
    lib().suma_se3_log(_ptr(Tc), _ptr(x))
    return x


def loop_closure_track(ctx, current, last_pose_old, last_increment, pose_new, conf_threshold, min_valid_ratio=0.2,
                       max_outlier_ratio=0.85, max_increment_difference=0.1):
    """device side of SurfelMapping::checkLoopClosure part 1 (SurfelMapping.cpp:546-574)"""
    r = LoopTrack()
    a, b, pn = _cm(last_pose_old, np.float64), _cm(last_increment, np.float64), _cm(pose_new, np.float32)
    ctx.check(ctx.L.suma_loop_closure_track(ctx.h, current.h, _ptr(a), _ptr(b), _ptr(pn), conf_threshold, min_valid_ratio,
                                            max_outlier_ratio, max_increment_difference, C.byref(r)),
              "suma_loop_closure_track")
    return _loop_track(r)


def _scan_refs(scans, on_device):
    """list of (points, labels, probs[, n]) -> (ScanRef array, keep-alive list).  Host scans: numpy arrays; device
    scans: (d_points, d_labels, d_probs, n) addresses from Context.device_array."""
    refs = (ScanRef * max(1, len(scans)))()
    keep = []
    for k, sc in enumerate(scans):
        if on_device:
            refs[k] = ScanRef(int(sc[0]), int(sc[1]) if sc[1] else None, int(sc[2]) if sc[2] else None, int(sc[3]))
        else:
            pts = np.ascontiguousarray(sc[0], dtype=np.float32).reshape(-1, 4)
            lab = None if sc[1] is None else np.ascontiguousarray(sc[1], dtype=np.float32)
            prob = None if sc[2] is None else np.ascontiguousarray(sc[2], dtype=np.float32)
            keep.append((pts, lab, prob))
            refs[k] = ScanRef(pts.ctypes.data, None if lab is None else lab.ctypes.data,
                              None if prob is None else prob.ctypes.data, pts.shape[0])
    return refs, keep


def run_sequences_native(params: SumaParams, sequences, device: int = 0, fixed_iterations: int = 0,
                         max_concurrent: int = 4, on_device: bool = False):
    """BASELINE configs[3] on one GPU: suma_run_sequences (include/suma_runner.h) -- the sequences (lists of scans) in
    the order given, at most max_concurrent at a time, each through a pipeline and a host thread of its own; no
    interpreter between two scans.  Returns one dict per sequence."""
    L = lib()
    n = len(sequences)
    jobs = (SequenceJob * max(1, n))()
    keep = []
    for j, scans in enumerate(sequences):
        refs, ka = _scan_refs(scans, on_device)
        keep.append((refs, ka))
        jobs[j] = SequenceJob(refs, len(scans), 1 if on_device else 0)
    res = (SequenceResult * max(1, n))()
    rc = L.suma_run_sequences(C.byref(params), device, jobs, n, max_concurrent, fixed_iterations, res)
    out = [dict(status=r.status, scans_done=r.scans_done, map_surfels=r.map_surfels, track_loss=r.track_loss,
                end_pose=np.array(r.end_pose[:]).reshape(4, 4).T.copy(), seconds=r.seconds, error=r.error.decode())
           for r in res[:n]]
    if rc != 0:
        raise SumaError(f"suma_run_sequences failed ({rc}): {[o['error'] for o in out if o['status']]}")
    return out


def run_hypotheses_native(params: SumaParams, scans, perturbations, rank: int = 0, world: int = 1, device: int = 0,
                          fixed_iterations: int = 0, exchange=None, on_device: bool = False):
    """BASELINE configs[2]: suma_run_hypotheses -- per scan len(perturbations) Gauss-Newton chains from
    lastIncrement * perturbations[k] (hypothesis k on rank k % world), one exchange per scan (exchange(local) -> the
    element-wise sum over the ranks of the [n_hyp, 18] table), the same winner on every rank, map update with it.
    Returns (poses [n, 4, 4], winners)."""
    L = lib()
    refs, keep = _scan_refs(scans, on_device)
    D = np.ascontiguousarray(np.asarray(perturbations, dtype=np.float64).reshape(-1, 4, 4).transpose(0, 2, 1))
    n_hyp, n = D.shape[0], len(scans)
    job = HypothesisJob(refs, n, 1 if on_device else 0, D.ctypes.data, n_hyp, rank, world)
    poses = np.zeros((max(1, n), 16), dtype=np.float64)
    winners = np.zeros(max(1, n), dtype=np.int32)
    err = C.create_string_buffer(160)
    failure = []

    def _cb(user, local, allp, count):
        try:
            loc = np.ctypeslib.as_array(local, shape=(count,)).reshape(n_hyp, 18).copy()
            tot = np.ascontiguousarray(exchange(loc), dtype=np.float64).reshape(-1)
            np.ctypeslib.as_array(allp, shape=(count,))[:] = tot
            return 0
        except Exception as e:  # noqa: BLE001 -- reported through the return code
            failure.append(repr(e))
            return -2

    cb = EXCHANGE_FN(_cb) if (world > 1 and exchange is not None) else C.cast(None, EXCHANGE_FN)
    rc = L.suma_run_hypotheses(C.byref(params), device, C.byref(job), fixed_iterations, cb, None, _ptr(poses), _ptr(winners),
                               err)
    if rc != 0:
        raise SumaError(f"suma_run_hypotheses failed ({rc}): {err.value.decode()} {failure}")
    return poses[:n].reshape(n, 4, 4).transpose(0, 2, 1).copy(), [int(w) for w in winners[:n]]


def loop_find_candidate(poses, trajectory_distances, timestamp: int, current_pose, radius: float,
                        min_trajectory_distance: float, delta_timestamp: int) -> int:
    """getCandidateIndexes / getClosestIndex (SurfelMapping.cpp:478-518) as the library runs it on the host
    (suma_loop_find_candidate); poses: n x 4 x 4 row-major doubles.  Returns the index or -1."""
    P = np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4).transpose(0, 2, 1))
    d = np.ascontiguousarray(trajectory_distances, dtype=np.float32)
    cur = _cm(current_pose, np.float64)
    return int(lib().suma_loop_find_candidate(_ptr(P), _ptr(d), timestamp, _ptr(cur), radius, min_trajectory_distance,
                                              delta_timestamp))


def _image_bytes(path_or_bytes) -> bytes:
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        return bytes(path_or_bytes)
    with open(path_or_bytes, "rb") as f:
        return f.read()


def checkpoint_info(path_or_bytes) -> dict:
    """suma_checkpoint_info of an image (host only, no device): version, timestamp, n_active, tiles, parked records,
    graph size, whether LOOP / OPT are present, and every section's id, bytes and digest"""
    img = _image_bytes(path_or_bytes)
    info = CheckpointInfo()
    rc = lib().suma_checkpoint_info(img, len(img), C.byref(info))
    if rc != 0:
        raise SumaError(f"suma_checkpoint_info failed ({rc}): {lib().suma_last_error(None).decode()}")
    return info.as_dict()


def checkpoint_params(path_or_bytes) -> SumaParams:
    """the suma_params an image was made with"""
    img = _image_bytes(path_or_bytes)
    p = SumaParams()
    rc = lib().suma_checkpoint_params(img, len(img), C.byref(p))
    if rc != 0:
        raise SumaError(f"suma_checkpoint_params failed ({rc}): {lib().suma_last_error(None).decode()}")
    return p


def checkpoint_digest(payload) -> int:
    payload = bytes(payload)
    return lib().suma_checkpoint_digest(payload, len(payload))


class _DeskewSwitch:
    """the motion-compensation switch SurfelMapping and Localizer share (suma_pipeline_*deskew* / suma_localizer_*deskew*,
    csrc/k_deskew.hip): while enabled, processScan* / beginScan* correct the raw sweep in front of K1 with the last
    increment as the motion over one sweep"""
    _deskew_prefix = ""

    def _dk(self, name):
        return getattr(self.L, f"suma_{self._deskew_prefix}_{name}")

    def enableDeskew(self, params: DeskewParams = None):
        """None = the defaults: azimuth time, counter-clockwise, start_azimuth 0, t_ref 0.5, scale 1"""
        self.ctx.check(self._dk("enable_deskew")(self.h, None if params is None else C.byref(params)),
                       f"suma_{self._deskew_prefix}_enable_deskew")

    def disableDeskew(self):
        self.ctx.check(self._dk("disable_deskew")(self.h), f"suma_{self._deskew_prefix}_disable_deskew")

    def setDeskewMotion(self, motion):
        """one-shot override of the motion over one sweep for the next scan (an IMU, wheel odometry, the first scans)"""
        T = _cm(motion, np.float64)
        self.ctx.check(self._dk("set_deskew_motion")(self.h, _ptr(T)), f"suma_{self._deskew_prefix}_set_deskew_motion")

    def deskewMotion(self):
        """(motion the last corrected scan used, row-major 4x4; its source: types.DESKEW_MOTION_*)"""
        T, src = np.zeros((4, 4), dtype=np.float64), C.c_int32(0)
        self.ctx.check(self._dk("deskew_motion")(self.h, _ptr(T), C.byref(src)), f"suma_{self._deskew_prefix}_deskew_motion")
        return T.T.copy(), int(src.value)


def deskew_points(ctx: "Context", points, motion, params: DeskewParams = None, times=None) -> np.ndarray:
    """suma_deskew_points: N x 4 points of one raw sweep moved into the sensor frame at ``params.t_ref``; ``motion`` is
    the sensor's motion over one sweep (row-major 4x4), ``times`` the per-point sweep fractions for the times source"""
    pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 4)
    tm = None if times is None else np.ascontiguousarray(times, dtype=np.float32).reshape(-1)
    if tm is not None and tm.shape[0] != pts.shape[0]:
        raise ValueError("one time per point is needed")
    out = np.empty_like(pts)
    T = _cm(motion, np.float64)
    ctx.check(ctx.L.suma_deskew_points(ctx.h, None if params is None else C.byref(params), _ptr(pts) if pts.shape[0] else None,
                                       _ptr(tm), pts.shape[0], _ptr(T), _ptr(out) if pts.shape[0] else None),
              "suma_deskew_points")
    return out


def deskew_points_device(ctx: "Context", d_points, motion, n: int, d_out=None, params: DeskewParams = None, d_times=None):
    """suma_deskew_points_device: the same on device addresses or torch tensors, enqueued on the ctx stream; ``d_out``
    None corrects in place"""
    T = _cm(motion, np.float64)
    ctx.check(ctx.L.suma_deskew_points_device(ctx.h, None if params is None else C.byref(params), _dev(d_points),
                                              _dev(d_times), n, _ptr(T), _dev(d_points if d_out is None else d_out)),
              "suma_deskew_points_device")


class SurfelMapping(_DeskewSwitch):
    """SurfelMapping::processScan (SurfelMapping.cpp:175-210).  processScan* run a scan in one call; beginScan /
    updatePose / updateMap are its phases.  With ``loop_params`` (types.LoopParams) the pipeline closes loops itself, as
    the reference does with close-loops = true: it keeps the pose graph (``posegraph``), every beginScan* first
    integrates a finished optimisation, processScan* run checkLoopClosure between updatePose and updateMap, and hosts
    on the phase calls place ``checkLoopClosure()`` there.  Without it, a host may still script closures by hand
    (verifyLoopClosure, trackLoopClosure, setPoseOld, integrateLoopClosures).  enableDeskew: the scans are raw sweeps;
    while it is on, the prefetch / async / scores entries and runScans refuse."""
    _deskew_prefix = "pipeline"

    def __init__(self, params: SumaParams, device: int = 0, loop_params: LoopParams = None):
        self.L = lib()
        self.params = params
        h = C.c_void_p()
        rc = self.L.suma_pipeline_create(C.byref(params), device, C.byref(h))
        if rc != 0:
            raise SumaError(f"suma_pipeline_create failed ({rc}): {self.L.suma_last_error(None).decode()}")
        self.h = h
        self.ctx = Context(params, handle=C.c_void_p(self.L.suma_pipeline_ctx(h)), owner=self)
        self.map = SurfelMap(self.ctx)
        self._staged = []
        self.device = device
        self.posegraph = None
        if loop_params is not None:
            self.enableLoopClosing(loop_params)

    # ---- loop closing inside the pipeline (suma_pipeline_enable_loop_closing ...)
    def enableLoopClosing(self, loop_params: LoopParams = None):
        """None switches it off; only between scans.  A ``posegraph`` handed out before is dead afterwards: the
        pipeline has destroyed the graph behind it."""
        old, self.posegraph = self.posegraph, None
        rc = self.L.suma_pipeline_enable_loop_closing(self.h, None if loop_params is None else C.byref(loop_params))
        h = self.L.suma_pipeline_posegraph(self.h)
        if old is not None:
            if rc != 0 and h is not None and h == old.h.value:
                self.posegraph = old  # refused: the pipeline has kept its graph
            else:
                old.h = None
        self.ctx.check(rc, "suma_pipeline_enable_loop_closing")
        if loop_params is not None:
            g = Posegraph(self.device, handle=C.c_void_p(h))
            g.borrowed = True  # the pipeline destroys it
            self.posegraph = g

    def checkLoopClosure(self):
        """SurfelMapping::checkLoopClosure, between updatePose and updateMap"""
        self.ctx.check(self.L.suma_pipeline_check_loop_closure(self.h), "suma_pipeline_check_loop_closure")

    def loopStatus(self) -> LoopStatus:
        st = LoopStatus()
        self.ctx.check(self.L.suma_pipeline_loop_status(self.h, C.byref(st)), "suma_pipeline_loop_status")
        return st

    def trajectoryDistances(self) -> np.ndarray:
        n = C.c_uint32()
        self.ctx.check(self.L.suma_pipeline_trajectory_distances(self.h, None, 0, C.byref(n)),
                       "suma_pipeline_trajectory_distances")
        out = np.zeros(max(n.value, 1), dtype=np.float32)
        self.ctx.check(self.L.suma_pipeline_trajectory_distances(self.h, _ptr(out), n.value, C.byref(n)),
                       "suma_pipeline_trajectory_distances")
        return out[:n.value]

    def getOptimizedPoses(self) -> np.ndarray:
        """SurfelMapping::getOptimizedPoses: the pose graph's poses"""
        if self.posegraph is None:
            raise SumaError("getOptimizedPoses: loop closing is not enabled")
        return self.posegraph.poses()

    def processScan(self, points, labels=None, probs=None, fixed_iterations: int = 0):
        points = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 4)
        labels = None if labels is None else np.ascontiguousarray(labels, dtype=np.float32)
        probs = None if probs is None else np.ascontiguousarray(probs, dtype=np.float32)
        self.ctx.check(self.L.suma_pipeline_process_scan(self.h, _ptr(points), _ptr(labels), _ptr(probs),
                                                         points.shape[0], fixed_iterations),
                       "suma_pipeline_process_scan")

    def runScans(self, scans, on_device: bool, fixed_iterations: int = 0, call_seconds=None) -> int:
        """the caller's loop over processScan in native code (suma_pipeline_run_scans, include/suma_runner.h): the next
        scans of this pipeline's sequence, one C call for all of them -- what the reference's visualizer thread does
        (VisualizerWindow.cpp:636-689).  scans: device tuples (d_points, d_labels, d_probs, n) or host triples.
        A prepared job (prepareScans) can be passed instead, so that no marshalling sits inside a timed region."""
        job = scans if isinstance(scans, tuple) and len(scans) == 3 and isinstance(scans[0], SequenceJob) else self.prepareScans(scans, on_device)
        done = C.c_uint32(0)
        if call_seconds is not None:  # float64 array of at least n_scans entries: host time of every call
            assert call_seconds.dtype == np.float64 and call_seconds.size >= job[0].n_scans
        self.ctx.check(self.L.suma_pipeline_run_scans(self.h, C.byref(job[0]), fixed_iterations, C.byref(done),
                                                      None if call_seconds is None else call_seconds.ctypes.data),
                       "suma_pipeline_run_scans")
        return done.value

    def prepareScans(self, scans, on_device: bool):
        refs, keep = _scan_refs(scans, on_device)
        return SequenceJob(refs, len(scans), 1 if on_device else 0), refs, keep

    def hostEntryTimes(self, reset: bool = False):
        """per-call averages (us) of where the blocking host-vector entry spends the CALLER's time
        (suma_pipeline_host_entry_times)"""
        out = np.zeros(8, dtype=np.float64)
        self.ctx.check(self.L.suma_pipeline_host_entry_times(self.h, _ptr(out), int(reset)), "suma_pipeline_host_entry_times")
        n = max(out[0], 1.0)
        keys = ("call", "slot_wait", "copy", "upload_enqueue", "kernel_enqueue", "result_wait")
        d = {k: round(1e6 * float(v) / n, 1) for k, v in zip(keys, out[1:7])}
        d["calls"] = int(out[0])
        d["copy_threads"] = int(out[7])
        return d

    def processScanDevice(self, d_points: int, d_labels: int, d_probs: int, n: int, fixed_iterations: int = 0):
        """scan already resident in HBM (device addresses from Context.device_array)"""
        self.ctx.check(self.L.suma_pipeline_process_scan_device(self.h, C.c_void_p(d_points), C.c_void_p(d_labels),
                                                                C.c_void_p(d_probs), n, fixed_iterations),
                       "suma_pipeline_process_scan_device")

    def processScanScores(self, sp: SemanticParams, d_points: int, d_scores: int, d_pixel: int, n: int,
                          logits: bool = False, producer_event: int = 0, fixed_iterations: int = 0,
                          knn: SemanticKnnParams = None, d_proj_idx: int = 0):
        """processScanDevice with the labels / probs back-projected on the device from a network's planar [C, H, W] fp32
        scores (suma_pipeline_process_scan_scores); the preprocessing waits for ``producer_event`` (a hipEvent_t, 0 =
        the buffers are complete), not for the host.  ``knn`` (segmentation.semantic_knn): RangeNet++'s KNN
        post-processing in front instead (suma_pipeline_process_scan_scores_knn), which also reads ``d_proj_idx``"""
        if knn is None:
            self.ctx.check(self.L.suma_pipeline_process_scan_scores(self.h, C.byref(sp), C.c_void_p(d_points),
                                                                    C.c_void_p(d_scores), int(bool(logits)),
                                                                    C.c_void_p(d_pixel), n,
                                                                    C.c_void_p(producer_event or None),
                                                                    fixed_iterations),
                           "suma_pipeline_process_scan_scores")
            return
        self.ctx.check(self.L.suma_pipeline_process_scan_scores_knn(self.h, C.byref(sp), C.byref(knn),
                                                                    C.c_void_p(d_points), C.c_void_p(d_scores),
                                                                    int(bool(logits)), C.c_void_p(d_pixel),
                                                                    C.c_void_p(d_proj_idx or None), n,
                                                                    C.c_void_p(producer_event or None),
                                                                    fixed_iterations),
                       "suma_pipeline_process_scan_scores_knn")

    def beginScanScores(self, sp: SemanticParams, d_points: int, d_scores: int, d_pixel: int, n: int,
                        logits: bool = False, producer_event: int = 0, knn: SemanticKnnParams = None,
                        d_proj_idx: int = 0):
        if knn is None:
            self.ctx.check(self.L.suma_pipeline_begin_scan_scores(self.h, C.byref(sp), C.c_void_p(d_points),
                                                                  C.c_void_p(d_scores), int(bool(logits)),
                                                                  C.c_void_p(d_pixel), n,
                                                                  C.c_void_p(producer_event or None)),
                           "suma_pipeline_begin_scan_scores")
            return
        self.ctx.check(self.L.suma_pipeline_begin_scan_scores_knn(self.h, C.byref(sp), C.byref(knn),
                                                                  C.c_void_p(d_points), C.c_void_p(d_scores),
                                                                  int(bool(logits)), C.c_void_p(d_pixel),
                                                                  C.c_void_p(d_proj_idx or None), n,
                                                                  C.c_void_p(producer_event or None)),
                       "suma_pipeline_begin_scan_scores_knn")

    def prefetchScan(self, points, labels=None, probs=None):
        """stage a scan (pinned copy + async upload on the ingest thread / copy stream); the arrays are kept alive
        until the matching processPrefetched() returns"""
        points = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 4)
        labels = None if labels is None else np.ascontiguousarray(labels, dtype=np.float32)
        probs = None if probs is None else np.ascontiguousarray(probs, dtype=np.float32)
        self._staged.append((points, labels, probs))
        self.ctx.check(self.L.suma_pipeline_prefetch_scan(self.h, _ptr(points), _ptr(labels), _ptr(probs),
                                                          points.shape[0]), "suma_pipeline_prefetch_scan")

    def processPrefetched(self, fixed_iterations: int = 0):
        try:
            self.ctx.check(self.L.suma_pipeline_process_prefetched(self.h, fixed_iterations),
                           "suma_pipeline_process_prefetched")
        finally:
            # the C side has consumed (and freed) the oldest slot whether or not the scan succeeded
            if self._staged:
                self._staged.pop(0)

    def processSequence(self, scans, fixed_iterations: int = 0, on_scan=None):
        """run an iterable of (points, labels, probs) with the upload of scan k+1 overlapping the kernels of scan k
        (what a reader thread feeding SurfelMapping::processScan does in the reference's visualizer loop)"""
        it = iter(scans)
        ahead = 0
        k = 0
        more = True
        while True:
            while more and ahead < 3:  # keep two scans staged beyond the one about to be processed
                nxt = next(it, None)
                if nxt is None:
                    more = False
                    break
                self.prefetchScan(*nxt[:3])
                ahead += 1
            if ahead == 0:
                return k
            self.processPrefetched(fixed_iterations)
            ahead -= 1
            if on_scan is not None:
                on_scan(k, self)
            k += 1

    # ---- the phases of processScan (SurfelMapping.cpp:175-204)
    def beginScan(self, points, labels=None, probs=None):
        points = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 4)
        labels = None if labels is None else np.ascontiguousarray(labels, dtype=np.float32)
        probs = None if probs is None else np.ascontiguousarray(probs, dtype=np.float32)
        self.ctx.check(self.L.suma_pipeline_begin_scan(self.h, _ptr(points), _ptr(labels), _ptr(probs), points.shape[0]),
                       "suma_pipeline_begin_scan")

    def beginScanDevice(self, d_points: int, d_labels: int, d_probs: int, n: int):
        self.ctx.check(self.L.suma_pipeline_begin_scan_device(self.h, C.c_void_p(d_points), C.c_void_p(d_labels),
                                                              C.c_void_p(d_probs), n), "suma_pipeline_begin_scan_device")

    def beginPrefetched(self):
        try:
            self.ctx.check(self.L.suma_pipeline_begin_prefetched(self.h), "suma_pipeline_begin_prefetched")
        finally:
            if self._staged:
                self._staged.pop(0)

    def updatePose(self, fixed_iterations: int = 0):
        self.ctx.check(self.L.suma_pipeline_update_pose(self.h, fixed_iterations), "suma_pipeline_update_pose")

    def updateMap(self):
        self.ctx.check(self.L.suma_pipeline_update_map(self.h), "suma_pipeline_update_map")

    def integrateLoopClosures(self, poses, difference):
        """poses: n x 4 x 4 (row-major numpy) optimised poses -> map_->updatePoses; difference: 4 x 4 double"""
        P = np.ascontiguousarray(np.asarray(poses, dtype=np.float32).reshape(-1, 4, 4).transpose(0, 2, 1))
        D = _cm(difference, np.float64)
        self.ctx.check(self.L.suma_pipeline_integrate_loop_closures(self.h, _ptr(P), P.shape[0], _ptr(D)),
                       "suma_pipeline_integrate_loop_closures")

    def setPoseOld(self, pose_old):
        T = _cm(pose_old, np.float64)
        self.ctx.check(self.L.suma_pipeline_set_pose_old(self.h, _ptr(T)), "suma_pipeline_set_pose_old")

    def getPose(self, which: int):
        """0 currentPose_, 1 currentPose_old_, 2 currentPose_new_, 3 lastPose_old_, 4 lastPose_"""
        T = np.zeros((4, 4), dtype=np.float64)
        self.ctx.check(self.L.suma_pipeline_get_pose(self.h, which, _ptr(T)), "suma_pipeline_get_pose")
        return T.T.copy()

    def resultNew(self) -> IcpStats:
        st = IcpStats()
        self.ctx.check(self.L.suma_pipeline_result_new(self.h, C.byref(st)), "suma_pipeline_result_new")
        return st

    def verifyLoopClosure(self, pose_prior, initializations, min_valid_ratio=0.2, max_outlier_ratio=0.85):
        n = len(initializations)
        res = (LoopResult * n)()
        prior = _cm(pose_prior, np.float64)
        inits = np.ascontiguousarray(np.stack([_cm(T, np.float64) for T in initializations]))
        self.ctx.check(self.L.suma_pipeline_verify_loop_closure(self.h, _ptr(prior), _ptr(inits), n, min_valid_ratio,
                                                                max_outlier_ratio, res),
                       "suma_pipeline_verify_loop_closure")
        return _loop_results(res, n)

    def trackLoopClosure(self, min_valid_ratio=0.2, max_outlier_ratio=0.85, max_increment_difference=0.1):
        r = LoopTrack()
        self.ctx.check(self.L.suma_pipeline_track_loop_closure(self.h, min_valid_ratio, max_outlier_ratio,
                                                               max_increment_difference, C.byref(r)),
                       "suma_pipeline_track_loop_closure")
        return _loop_track(r)

    def reset(self):
        """SurfelMapping::reset (SurfelMapping.cpp:131-169)"""
        self.ctx.check(self.L.suma_pipeline_reset(self.h), "suma_pipeline_reset")

    # ---- checkpoint / resume (suma_pipeline_checkpoint_*; the image is specified in csrc/k_checkpoint.hip)
    def save(self, path=None) -> bytes:
        """the canonical image of the pipeline's state between two scans; also written to ``path`` if given (to a
        temporary name first, then renamed).  A pipeline that loads it continues as this one would, to the bit."""
        n = C.c_uint64()
        self.ctx.check(self.L.suma_pipeline_checkpoint_size(self.h, C.byref(n)), "suma_pipeline_checkpoint_size")
        buf = np.empty(n.value, dtype=np.uint8)
        self.ctx.check(self.L.suma_pipeline_checkpoint_save(self.h, _ptr(buf), n.value, C.byref(n)),
                       "suma_pipeline_checkpoint_save")
        img = buf[:n.value].tobytes()
        if path is not None:
            tmp = f"{path}.tmp"
            with open(tmp, "wb") as f:
                f.write(img)
            os.replace(tmp, path)
        return img

    def load(self, path_or_bytes):
        """replaces this pipeline's state by an image's (a path or the bytes).  Refused -- and the pipeline left as it
        was -- unless the image is well formed, its digests hold and it was made with this pipeline's parameters.
        Loop closing is switched on with the image's parameters if it holds a LOOP section, off if not."""
        img = _image_bytes(path_or_bytes)
        old, self.posegraph = self.posegraph, None
        had = self.L.suma_pipeline_posegraph(self.h)
        rc = self.L.suma_pipeline_checkpoint_load(self.h, img, len(img))
        h = self.L.suma_pipeline_posegraph(self.h)
        if old is not None:
            if rc != 0 and h is not None and h == had:
                self.posegraph = old  # refused before anything was written: the pipeline has kept its graph
            else:
                old.h = None
        self.ctx.check(rc, "suma_pipeline_checkpoint_load")
        self._staged = []
        if h is not None:
            g = Posegraph(self.device, handle=C.c_void_p(h))
            g.borrowed = True
            self.posegraph = g

    @classmethod
    def restore(cls, path_or_bytes, device: int = 0) -> "SurfelMapping":
        """a new pipeline with the image's parameters, holding the image's state"""
        img = _image_bytes(path_or_bytes)
        pipe = cls(checkpoint_params(img), device=device)
        pipe.load(img)
        return pipe

    def minimizeHypotheses(self, starts, fixed_iterations: int = 0):
        """n Gauss-Newton chains as one batch against the rendered model, between beginScan and applyIncrement"""
        T0 = np.ascontiguousarray(np.asarray(starts, dtype=np.float64).reshape(-1, 4, 4).transpose(0, 2, 1))
        n = T0.shape[0]
        out = np.zeros((n, 4, 4), dtype=np.float64)
        st = (IcpStats * n)()
        self.ctx.check(self.L.suma_pipeline_minimize_hypotheses(self.h, _ptr(T0), n, fixed_iterations, _ptr(out), st),
                       "suma_pipeline_minimize_hypotheses")
        return out.transpose(0, 2, 1).copy(), [s.as_dict() for s in st]

    def applyIncrement(self, increment):
        T = _cm(increment, np.float64)
        self.ctx.check(self.L.suma_pipeline_apply_increment(self.h, _ptr(T)), "suma_pipeline_apply_increment")

    def getCurrentPose(self):
        T = np.zeros((4, 4), dtype=np.float64)
        self.L.suma_pipeline_pose(self.h, _ptr(T))
        return T.T.copy()

    def lastIncrement(self):
        T = np.zeros((4, 4), dtype=np.float64)
        self.L.suma_pipeline_last_increment(self.h, _ptr(T))
        return T.T.copy()

    def lastStats(self) -> IcpStats:
        st = IcpStats()
        self.L.suma_pipeline_last_stats(self.h, C.byref(st))
        return st

    def minimizeStats(self) -> IcpStats:
        """statistics of the scan's minimisation itself (iterations, converged: suma_pipeline_minimize_stats)"""
        st = IcpStats()
        self.L.suma_pipeline_minimize_stats(self.h, C.byref(st))
        return st

    def timestamp(self) -> int:
        return self.L.suma_pipeline_timestamp(self.h)

    def trackLoss(self) -> int:
        """scans on which the frame-to-frame fallback ran (trackLoss_, SurfelMapping.cpp:441)"""
        return self.L.suma_pipeline_track_loss(self.h)

    def frame(self, which: int) -> Frame:
        """0 current data frame, 1 last model frame, 2 current model frame"""
        p = self.params
        w, h = (p.data_width, p.data_height) if which == 0 else (p.model_width, p.model_height)
        return Frame(self.ctx, w, h, handle=self.L.suma_pipeline_frame(self.h, which))

    def close(self):
        if getattr(self, "h", None):
            if getattr(self, "posegraph", None) is not None:
                self.posegraph.h = None
            self.L.suma_pipeline_destroy(self.h)
            self.h = None
            self.ctx.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def prune_mask(evidence: np.ndarray, rule: ChangeRule = None) -> np.ndarray:
    """suma_change_prune_mask: bool per record, False = removed by the rule (None: the defaults).  Host only."""
    ev = np.ascontiguousarray(evidence, dtype=EVIDENCE_DTYPE).reshape(-1)
    keep = np.ones(ev.shape[0], dtype=np.uint8)
    rc = lib().suma_change_prune_mask(_ptr(ev) if ev.shape[0] else None, ev.shape[0],
                                      None if rule is None else C.byref(rule), _ptr(keep) if ev.shape[0] else None, None)
    if rc != 0:
        raise SumaError(f"suma_change_prune_mask failed ({rc}): {lib().suma_last_error(None).decode()}")
    return keep.astype(bool)


def pruned_map(records: np.ndarray, evidence: np.ndarray, rule: ChangeRule = None):
    """(records[keep], keep)"""
    records = np.asarray(records).reshape(-1)
    if records.shape[0] != np.asarray(evidence).reshape(-1).shape[0]:
        raise ValueError("one evidence entry per record is needed")
    keep = prune_mask(evidence, rule)
    return records[keep], keep


class Localizer(_DeskewSwitch):
    """Localisation of scans in a finished world map, which is left alone (suma_localizer_*, csrc/k_localize.hip): the
    map is what SurfelMap.export_world / mapio give.  ``setMap`` bins it into submap tiles on the device, ``setPose``
    gives the start pose and gathers the tiles around it (``relocalize`` finds one from a PlaceIndex instead),
    ``processScan`` renders that window from the predicted pose, minimises the scan against it and returns a dict: guess / pose / increment
    (row-major 4x4), stats, valid_ratio, outlier_ratio, tracked, window_rebuilt, origin, n_window.  Nothing is fused, so a
    run has no length limit.  enableDeskew: processScan* take raw sweeps; relocalize does not correct."""
    _deskew_prefix = "localizer"

    def __init__(self, params: SumaParams, loc_params: LocalizerParams = None, device: int = 0):
        self.L = lib()
        self.params = params
        h = C.c_void_p()
        rc = self.L.suma_localizer_create(C.byref(params), None if loc_params is None else C.byref(loc_params), device,
                                          C.byref(h))
        if rc != 0:
            raise SumaError(f"suma_localizer_create failed ({rc}): {self.L.suma_last_error(None).decode()}")
        self.h = h
        self.ctx = Context(params, handle=C.c_void_p(self.L.suma_localizer_ctx(h)), owner=self)
        self.n_dropped = 0

    @classmethod
    def from_ply(cls, path: str, params: SumaParams, loc_params: LocalizerParams = None, device: int = 0) -> "Localizer":
        """a localiser over the map a PLY written by mapio.write_ply / tools/export_map.py holds"""
        from . import mapio
        records, _ = mapio.read_ply(path)
        loc = cls(params, loc_params, device)
        loc.setMap(records)
        return loc

    def setMap(self, world_surfels: np.ndarray) -> int:
        """WORLD_SURFEL_DTYPE records; returns how many were dropped (non-finite position, outside the tile grid)"""
        ws = np.ascontiguousarray(world_surfels, dtype=WORLD_SURFEL_DTYPE).reshape(-1)
        nd = C.c_uint32(0)
        self.ctx.check(self.L.suma_localizer_set_map(self.h, _ptr(ws) if ws.shape[0] else None, ws.shape[0], C.byref(nd)),
                       "suma_localizer_set_map")
        self.n_dropped = nd.value
        return nd.value

    def setMapDevice(self, d_records, n: int) -> int:
        """the records already on the device (an address or a torch tensor); they are only read"""
        nd = C.c_uint32(0)
        self.ctx.check(self.L.suma_localizer_set_map_device(self.h, _dev(d_records), n, C.byref(nd)),
                       "suma_localizer_set_map_device")
        self.n_dropped = nd.value
        return nd.value

    def setPose(self, pose):
        T = _cm(pose, np.float64)
        self.ctx.check(self.L.suma_localizer_set_pose(self.h, _ptr(T)), "suma_localizer_set_pose")

    @staticmethod
    def _result(r: LocalizerResult) -> dict:
        m = lambda a: np.array(a[:], dtype=np.float64).reshape(4, 4).T.copy()  # noqa: E731
        return dict(guess=m(r.guess), pose=m(r.pose), increment=m(r.increment), stats=r.stats.as_dict(),
                    valid_ratio=float(r.valid_ratio), outlier_ratio=float(r.outlier_ratio), tracked=bool(r.tracked),
                    window_rebuilt=bool(r.window_rebuilt), origin=(int(r.origin_ij[0]), int(r.origin_ij[1])),
                    n_window=int(r.n_window))

    def processScan(self, points, labels=None, probs=None, fixed_iterations: int = 0) -> dict:
        points = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 4)
        labels = None if labels is None else np.ascontiguousarray(labels, dtype=np.float32)
        probs = None if probs is None else np.ascontiguousarray(probs, dtype=np.float32)
        res = LocalizerResult()
        self.ctx.check(self.L.suma_localizer_process_scan(self.h, _ptr(points), _ptr(labels), _ptr(probs), points.shape[0],
                                                          fixed_iterations, C.byref(res)), "suma_localizer_process_scan")
        return self._result(res)

    def processScanDevice(self, d_points, d_labels, d_probs, n: int, fixed_iterations: int = 0) -> dict:
        """scan already resident in HBM and complete (device addresses from Context.device_array, or torch tensors)"""
        res = LocalizerResult()
        self.ctx.check(self.L.suma_localizer_process_scan_device(self.h, _dev(d_points), _dev(d_labels), _dev(d_probs), n,
                                                                 fixed_iterations, C.byref(res)),
                       "suma_localizer_process_scan_device")
        return self._result(res)

    @staticmethod
    def _poses16(poses) -> np.ndarray:
        """row-major 4x4 poses -> n x 16 column-major doubles"""
        P = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
        return np.ascontiguousarray(P.transpose(0, 2, 1)).reshape(-1, 16)

    def _relocalized(self, res: RelocalizeResult) -> dict:
        tried = [dict(match=res.candidates[k].match.as_dict(), result=self._result(res.candidates[k].result))
                 for k in range(res.n_tried)]
        found = bool(res.found)
        return dict(found=found, n_tried=int(res.n_tried), winner=int(res.winner),
                    match=res.match.as_dict() if found else None, result=self._result(res.result) if found else None,
                    candidates=tried)

    def relocalize(self, index: "PlaceIndex", poses, points, labels=None, probs=None, max_candidates: int = 8,
                   fixed_iterations: int = 0) -> dict:
        """global relocalisation (suma_localizer_relocalize): no setPose is needed.  ``poses``: one 4x4 pose per entry of
        ``index``, by entry index.  Returns found, n_tried, winner, match, result (as processScan's) and candidates (the
        match and result of every candidate tried).  found = False leaves the localiser as it was."""
        points = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 4)
        labels = None if labels is None else np.ascontiguousarray(labels, dtype=np.float32)
        probs = None if probs is None else np.ascontiguousarray(probs, dtype=np.float32)
        P = self._poses16(poses)
        res = RelocalizeResult()
        self.ctx.check(self.L.suma_localizer_relocalize(self.h, index.h, _ptr(P) if P.shape[0] else None, P.shape[0],
                                                        _ptr(points), _ptr(labels), _ptr(probs), points.shape[0],
                                                        max_candidates, fixed_iterations, C.byref(res)),
                       "suma_localizer_relocalize")
        return self._relocalized(res)

    def relocalizeDevice(self, index: "PlaceIndex", poses, d_points, d_labels, d_probs, n: int, max_candidates: int = 8,
                         fixed_iterations: int = 0) -> dict:
        """the same with the scan already resident in HBM and complete"""
        P = self._poses16(poses)
        res = RelocalizeResult()
        self.ctx.check(self.L.suma_localizer_relocalize_device(self.h, index.h, _ptr(P) if P.shape[0] else None, P.shape[0],
                                                               _dev(d_points), _dev(d_labels), _dev(d_probs), n,
                                                               max_candidates, fixed_iterations, C.byref(res)),
                       "suma_localizer_relocalize_device")
        return self._relocalized(res)

    def window(self):
        """(origin tile (i, j), records in the window, gathers since setMap)"""
        ij = np.zeros(2, dtype=np.int32)
        n, rb = C.c_uint32(0), C.c_uint32(0)
        self.ctx.check(self.L.suma_localizer_window(self.h, _ptr(ij), C.byref(n), C.byref(rb)), "suma_localizer_window")
        return (int(ij[0]), int(ij[1])), n.value, rb.value

    def downloadWindow(self) -> np.ndarray:
        """the window's surfels as the localiser's ctx holds them (SURFEL_DTYPE)"""
        n = self.window()[1]
        out = np.zeros(n, dtype=SURFEL_DTYPE)
        got = C.c_uint32(0)
        self.ctx.check(self.L.suma_localizer_download_window(self.h, _ptr(out) if n else None, n, C.byref(got)),
                       "suma_localizer_download_window")
        return out[:min(n, got.value)]

    # -- change evidence (csrc/k_change.hip)
    def enableEvidence(self, params: ChangeParams = None):
        """from the next setMap on, every record of the map collects evidence (hits, misses, occluded, label_changes)
        from each scan processScan tracks, and from every observeFrame"""
        self.ctx.check(self.L.suma_localizer_enable_evidence(self.h, None if params is None else C.byref(params)),
                       "suma_localizer_enable_evidence")

    def disableEvidence(self):
        self.ctx.check(self.L.suma_localizer_disable_evidence(self.h), "suma_localizer_disable_evidence")

    def observeFrame(self, frame: Frame, pose) -> dict:
        """one observation of a data-sized frame of this localiser's ctx at a sensor pose (row-major 4x4, world frame)
        over the current window; returns its totals"""
        T = _cm(pose, np.float64)
        cnt = ChangeCounts()
        self.ctx.check(self.L.suma_localizer_observe_frame(self.h, frame.h, _ptr(T), C.byref(cnt)),
                       "suma_localizer_observe_frame")
        return cnt.as_dict()

    def lastObservation(self):
        """(the totals of the last processScan's observation, whether it observed)"""
        cnt, obs = ChangeCounts(), C.c_int32(0)
        self.ctx.check(self.L.suma_localizer_last_observation(self.h, C.byref(cnt), C.byref(obs)),
                       "suma_localizer_last_observation")
        return cnt.as_dict(), bool(obs.value)

    def evidence(self) -> np.ndarray:
        """EVIDENCE_DTYPE, one per record setMap was given, in that order (dropped records stay zero)"""
        n = C.c_uint32(0)
        self.ctx.check(self.L.suma_localizer_evidence(self.h, None, 0, C.byref(n)), "suma_localizer_evidence")
        out = np.zeros(n.value, dtype=EVIDENCE_DTYPE)
        if n.value:
            self.ctx.check(self.L.suma_localizer_evidence(self.h, _ptr(out), n.value, C.byref(n)), "suma_localizer_evidence")
        return out

    def evidenceDevice(self, d_out, capacity: int) -> int:
        """the same into a device buffer of ``capacity`` entries (an address or a torch tensor); returns the map's n"""
        n = C.c_uint32(0)
        self.ctx.check(self.L.suma_localizer_evidence_device(self.h, _dev(d_out), capacity, C.byref(n)),
                       "suma_localizer_evidence_device")
        return n.value

    def clearEvidence(self):
        self.ctx.check(self.L.suma_localizer_clear_evidence(self.h), "suma_localizer_clear_evidence")

    def prunedMap(self, records: np.ndarray, rule: ChangeRule = None):
        """(records[keep], keep) by suma_change_prune_mask over evidence(); ``records``: what setMap was given"""
        return pruned_map(records, self.evidence(), rule)

    # -- newly seen surfaces (csrc/k_novel.hip)
    def _novel_check(self, rc: int, what: str, allow_overflow: bool):
        """the downloads fill their outputs and then report an overflow of max_candidates (-3); ``allow_overflow``
        takes the outputs all the same"""
        if not (allow_overflow and rc == -3):
            self.ctx.check(rc, what)

    def enableNovelty(self, params: NovelParams = None):
        """from now on every scan processScan tracks ends with one collection: the texels no record of the window
        explains become world-frame candidates on the device (48 bytes each, max_candidates of them are allocated)"""
        self.ctx.check(self.L.suma_localizer_enable_novelty(self.h, None if params is None else C.byref(params)),
                       "suma_localizer_enable_novelty")

    def disableNovelty(self):
        self.ctx.check(self.L.suma_localizer_disable_novelty(self.h), "suma_localizer_disable_novelty")

    def collectFrame(self, frame: Frame, pose, scan_id: int) -> dict:
        """one collection of a data-sized frame of this localiser's ctx at a sensor pose (row-major 4x4, world frame)
        over the current window; returns its counts"""
        T = _cm(pose, np.float64)
        cnt = NovelCounts()
        self.ctx.check(self.L.suma_localizer_collect_frame(self.h, frame.h, _ptr(T), scan_id, C.byref(cnt)),
                       "suma_localizer_collect_frame")
        return cnt.as_dict()

    def lastCollection(self, allow_overflow: bool = False):
        """(the counts of the last processScan's collection, whether it collected)"""
        cnt, col = NovelCounts(), C.c_int32(0)
        self._novel_check(self.L.suma_localizer_last_collection(self.h, C.byref(cnt), C.byref(col)),
                          "suma_localizer_last_collection", allow_overflow)
        return cnt.as_dict(), bool(col.value)

    def novelCandidates(self, allow_overflow: bool = False) -> np.ndarray:
        """WORLD_SURFEL_DTYPE: the candidates in creation order (timestamp = the scan's number, support = 1)"""
        n = C.c_uint32(0)
        self._novel_check(self.L.suma_localizer_novel_candidates(self.h, None, 0, C.byref(n)),
                          "suma_localizer_novel_candidates", True)
        out = np.zeros(n.value, dtype=WORLD_SURFEL_DTYPE)
        self._novel_check(self.L.suma_localizer_novel_candidates(self.h, _ptr(out) if n.value else None, n.value, C.byref(n)),
                          "suma_localizer_novel_candidates", allow_overflow)
        return out[:n.value]

    def setNovelCandidates(self, records: np.ndarray):
        """replaces the candidates (what novelCandidates of an earlier session gave)"""
        ws = np.ascontiguousarray(records, dtype=WORLD_SURFEL_DTYPE).reshape(-1)
        self.ctx.check(self.L.suma_localizer_set_novel_candidates(self.h, _ptr(ws) if ws.shape[0] else None, ws.shape[0]),
                       "suma_localizer_set_novel_candidates")

    def novel(self, fuse_params: NovelFuseParams = None, allow_overflow: bool = False, stats: bool = False):
        """(records, views): the candidates fused per voxel, kept where at least min_views scans agree, in ascending
        voxel order; with ``stats`` the suma_novel_stats dict comes third"""
        fp = None if fuse_params is None else C.byref(fuse_params)
        st = NovelStats()
        self._novel_check(self.L.suma_localizer_novel(self.h, fp, None, None, 0, C.byref(st)), "suma_localizer_novel", True)
        n = st.n_out
        rec, views = np.zeros(n, dtype=WORLD_SURFEL_DTYPE), np.zeros(n, dtype=np.uint32)
        if n:
            self._novel_check(self.L.suma_localizer_novel(self.h, fp, _ptr(rec), _ptr(views), n, C.byref(st)),
                              "suma_localizer_novel", allow_overflow)
        elif not allow_overflow and st.n_overflow:
            self.ctx.check(self.L.suma_localizer_novel(self.h, fp, None, None, 0, C.byref(st)), "suma_localizer_novel")
        return (rec, views, st.as_dict()) if stats else (rec, views)

    def novelMarks(self) -> np.ndarray:
        """the mark image of the last collection, H x W uint8: 1 where a record of the window agrees with the texel"""
        p = self.params
        out = np.zeros((p.data_height, p.data_width), dtype=np.uint8)
        n = C.c_uint32(0)
        self.ctx.check(self.L.suma_localizer_novel_marks(self.h, _ptr(out), out.size, C.byref(n)), "suma_localizer_novel_marks")
        return out

    def clearNovelty(self):
        self.ctx.check(self.L.suma_localizer_clear_novelty(self.h), "suma_localizer_clear_novelty")

    def updatedMap(self, records: np.ndarray, rule: ChangeRule = None, fuse_params: NovelFuseParams = None) -> np.ndarray:
        """the records prunedMap keeps (all of them when evidence is off) followed by the fused novel records: what goes
        into the next setMap, mapio.write_ply or draw.  ``records``: what setMap was given"""
        records = np.ascontiguousarray(records, dtype=WORLD_SURFEL_DTYPE).reshape(-1)
        try:
            ev = self.evidence()
        except SumaError as e:
            if "no evidence" not in str(e):
                raise
            ev = None
        kept = records if ev is None else pruned_map(records, ev, rule)[0]
        return np.concatenate([kept, self.novel(fuse_params)[0]])

    # -- objects in front of the robot (csrc/k_objects.hip)
    def enableObjects(self, params: ObjectParams = None):
        """from now on every collection (novelty must be on) is followed by one segmentation of its unexplained texels
        into objects; nothing else the localiser gives changes"""
        self.ctx.check(self.L.suma_localizer_enable_objects(self.h, None if params is None else C.byref(params)),
                       "suma_localizer_enable_objects")

    def disableObjects(self):
        self.ctx.check(self.L.suma_localizer_disable_objects(self.h), "suma_localizer_disable_objects")

    def objects(self, allow_overflow: bool = False):
        """(SCAN_OBJECT_DTYPE records in ascending root order, the suma_object_counts dict) of the last segmentation, or
        None when the last scan or collectFrame segmented nothing.  More objects than max_objects raise unless
        ``allow_overflow``, which takes the first max_objects"""
        n, cnt, seg = C.c_uint32(0), ObjectCounts(), C.c_int32(0)
        self._novel_check(self.L.suma_localizer_objects(self.h, None, 0, C.byref(n), C.byref(cnt), C.byref(seg)),
                          "suma_localizer_objects", True)
        if not seg.value:
            return None
        rec = np.zeros(n.value, dtype=SCAN_OBJECT_DTYPE)
        self._novel_check(self.L.suma_localizer_objects(self.h, _ptr(rec) if n.value else None, n.value, C.byref(n),
                                                        C.byref(cnt), C.byref(seg)), "suma_localizer_objects", allow_overflow)
        return rec[:n.value], cnt.as_dict()

    def objectIds(self):
        """H x W uint32: the object number of every texel of the last segmentation, 0xffffffff for none; None when
        nothing was segmented"""
        p = self.params
        out = np.zeros((p.data_height, p.data_width), dtype=np.uint32)
        n = C.c_uint32(0)
        self.ctx.check(self.L.suma_localizer_object_ids(self.h, _ptr(out), out.size, C.byref(n)), "suma_localizer_object_ids")
        return out if n.value else None

    def scanFrame(self) -> Frame:
        """the data frame of the last processScan (vertex, normal, semantic): what its collection and segmentation read"""
        p = self.params
        return Frame(self.ctx, p.data_width, p.data_height, handle=self.L.suma_localizer_frame(self.h))

    def novelFlags(self) -> np.ndarray:
        """the flag image of the last collection, H x W uint8: 1 where the texel was novel -- what its segmentation read"""
        p = self.params
        out = np.zeros((p.data_height, p.data_width), dtype=np.uint8)
        n = C.c_uint32(0)
        self.ctx.check(self.L.suma_localizer_novel_flags(self.h, _ptr(out), out.size, C.byref(n)), "suma_localizer_novel_flags")
        return out

    def segmentFlags(self, frame: Frame, pose, flags, scan_id: int) -> dict:
        """the primitive: one segmentation of a data-sized frame of this localiser's ctx at a sensor pose (row-major 4x4,
        world frame) over the caller's flag image (H x W, non-zero = take the texel); returns its counts"""
        p = self.params
        fl = np.ascontiguousarray(flags, dtype=np.uint8)
        if fl.size != p.data_width * p.data_height:
            raise ValueError("flags must have one byte per texel of the data image")
        T = _cm(pose, np.float64)
        cnt = ObjectCounts()
        self.ctx.check(self.L.suma_localizer_segment_flags(self.h, frame.h, _ptr(T), _ptr(fl), scan_id, C.byref(cnt)),
                       "suma_localizer_segment_flags")
        return cnt.as_dict()

    # -- live obstacles for the planner (csrc/k_live.hip)
    def enableLiveGrid(self, cells, gp: GridParams, params: LiveParams = None):
        """from now on every collection (novelty must be on; after its segmentation when objects are on) is followed by
        one update of a live obstacle layer over the static grid ``cells`` / ``gp`` of core.world_grid: the
        GRID_CELL_DTYPE array (uploaded for the call), or a device address / torch tensor of gp.width * gp.height
        cells, which is only read -- the layer keeps a copy"""
        owned = None
        if isinstance(cells, np.ndarray):
            arr = np.ascontiguousarray(cells, dtype=GRID_CELL_DTYPE).reshape(-1)
            if arr.shape[0] != int(gp.width) * int(gp.height):
                raise ValueError(f"enableLiveGrid: {arr.shape[0]} cells against a raster of {gp.height} x {gp.width}")
            cells = owned = self.ctx.device_array(arr)
        try:
            self.ctx.check(self.L.suma_localizer_enable_live_grid(self.h, C.byref(gp), _dev(cells),
                                                                  None if params is None else C.byref(params)),
                           "suma_localizer_enable_live_grid")
        finally:
            if owned:
                self.L.suma_device_free(self.ctx.h, C.c_void_p(owned))
        self._live_gp = GridParams.from_buffer_copy(gp)

    def disableLiveGrid(self):
        self.ctx.check(self.L.suma_localizer_disable_live_grid(self.h), "suma_localizer_disable_live_grid")
        self._live_gp = None

    def clearLiveGrid(self):
        """no cell has a hit; setMap does this too"""
        self.ctx.check(self.L.suma_localizer_clear_live_grid(self.h), "suma_localizer_clear_live_grid")

    def liveUpdateFlags(self, frame: Frame, pose, flags, scan_id: int) -> dict:
        """the primitive: one update of the live layer with a data-sized frame of this localiser's ctx at a sensor pose
        (row-major 4x4, world frame) over the caller's flag image (H x W, non-zero = take the texel), segmented first
        when objects are on; returns the update's counts"""
        p = self.params
        fl = np.ascontiguousarray(flags, dtype=np.uint8)
        if fl.size != p.data_width * p.data_height:
            raise ValueError("flags must have one byte per texel of the data image")
        T = _cm(pose, np.float64)
        cnt = LiveCounts()
        self.ctx.check(self.L.suma_localizer_live_update_flags(self.h, frame.h, _ptr(T), _ptr(fl), scan_id, C.byref(cnt)),
                       "suma_localizer_live_update_flags")
        return cnt.as_dict()

    def liveCounts(self):
        """the suma_live_counts dict of the last update, or None when there was none since the layer was enabled or
        cleared"""
        cnt, upd = LiveCounts(), C.c_int32(0)
        self.ctx.check(self.L.suma_localizer_live_counts(self.h, C.byref(cnt), C.byref(upd)), "suma_localizer_live_counts")
        return cnt.as_dict() if upd.value else None

    def liveCells(self, out=None):
        """composes -> (cells[height, width] of GRID_CELL_DTYPE, mask[height, width] uint8: 1 live, 2 pending, the
        suma_live_stats dict): the static cells with the live obstacles written into them, what core.grid_plan and
        GridPlanner take.  ``out``: a device address / torch tensor of width * height cells (16-byte aligned) to leave
        the cells at, for core.grid_plan to read there; the return is then (None, mask, stats)"""
        gp = getattr(self, "_live_gp", None)
        if gp is None:
            raise SumaError("liveCells: the live layer is off (enableLiveGrid)")
        n = int(gp.width) * int(gp.height)
        L, h = self.L, self.ctx.h
        d_cells, d_mask, st = C.c_void_p(), C.c_void_p(), LiveStats()
        try:
            if out is None:
                self.ctx.check(L.suma_device_alloc(h, n * GRID_CELL_DTYPE.itemsize, C.byref(d_cells)), "suma_device_alloc")
            self.ctx.check(L.suma_device_alloc(h, max(n, 16), C.byref(d_mask)), "suma_device_alloc")
            self.ctx.check(L.suma_localizer_live_cells_device(self.h, d_cells if out is None else _dev(out), d_mask, C.byref(st)),
                           "suma_localizer_live_cells_device")
            cells = None
            if out is None:
                cells = np.zeros((gp.height, gp.width), dtype=GRID_CELL_DTYPE)
                self.ctx.check(L.suma_device_download(h, _ptr(cells), d_cells, cells.nbytes), "suma_device_download")
            mask = np.zeros((gp.height, gp.width), dtype=np.uint8)
            self.ctx.check(L.suma_device_download(h, _ptr(mask), d_mask, mask.nbytes), "suma_device_download")
        finally:
            if d_cells:
                L.suma_device_free(h, d_cells)
            if d_mask:
                L.suma_device_free(h, d_mask)
        return cells, mask, st.as_dict()

    def liveState(self) -> np.ndarray:
        """the raw state of the layer, LIVE_CELL_DTYPE [height, width] (for tests and for keeping a layer)"""
        gp = getattr(self, "_live_gp", None)
        if gp is None:
            raise SumaError("liveState: the live layer is off (enableLiveGrid)")
        out = np.zeros((gp.height, gp.width), dtype=LIVE_CELL_DTYPE)
        n = C.c_uint32(0)
        self.ctx.check(self.L.suma_localizer_live_state(self.h, _ptr(out), out.size, C.byref(n)), "suma_localizer_live_state")
        return out

    def setLiveState(self, state: np.ndarray, last_stamp: int):
        """puts a raw state (what liveState gave) and the stamp of its last update back"""
        st = np.ascontiguousarray(state, dtype=LIVE_CELL_DTYPE).reshape(-1)
        self.ctx.check(self.L.suma_localizer_set_live_state(self.h, _ptr(st), st.shape[0], last_stamp),
                       "suma_localizer_set_live_state")

    # -- tracks: the objects of the scans tied together (csrc/k_tracks.hip)
    def enableTracks(self, params: TrackParams = None):
        """from now on every segmentation (objects must be on) is followed by one tracker update: fragments joined into
        detections, detections associated to tracks, ids kept, velocities filtered; nothing else the localiser gives
        changes"""
        self.ctx.check(self.L.suma_localizer_enable_tracks(self.h, None if params is None else C.byref(params)),
                       "suma_localizer_enable_tracks")
        self._track_params = TrackParams.defaults() if params is None else TrackParams.from_buffer_copy(params)

    def disableTracks(self):
        self.ctx.check(self.L.suma_localizer_disable_tracks(self.h), "suma_localizer_disable_tracks")

    def clearTracks(self):
        """no tracks, the next id is 1; setMap and clearNovelty do this too"""
        self.ctx.check(self.L.suma_localizer_clear_tracks(self.h), "suma_localizer_clear_tracks")

    def tracks(self, allow_overflow: bool = False, out=None):
        """(OBJECT_TRACK_DTYPE records of the live tracks in ascending slot order, the suma_track_counts dict) of the last
        update, or None when there was none.  Detections that found no free slot raise unless ``allow_overflow``.
        ``out``: a device address / torch tensor with room for max_tracks records to leave the records at; the return
        is then (their number, counts)"""
        n, cnt, upd = C.c_uint32(0), TrackCounts(), C.c_int32(0)
        self._novel_check(self.L.suma_localizer_tracks(self.h, None, 0, C.byref(n), C.byref(cnt), C.byref(upd)),
                          "suma_localizer_tracks", True)
        if not upd.value:
            return None
        if out is not None:
            self._novel_check(self.L.suma_localizer_tracks_device(self.h, _dev(out), n.value, C.byref(n), C.byref(cnt),
                                                                  C.byref(upd)), "suma_localizer_tracks_device", allow_overflow)
            return n.value, cnt.as_dict()
        rec = np.zeros(n.value, dtype=OBJECT_TRACK_DTYPE)
        self._novel_check(self.L.suma_localizer_tracks(self.h, _ptr(rec) if n.value else None, n.value, C.byref(n),
                                                       C.byref(cnt), C.byref(upd)), "suma_localizer_tracks", allow_overflow)
        return rec[:n.value], cnt.as_dict()

    def trackList(self, confirmed_only: bool = True):
        """the live tracks of the last update as ObjectTrack objects"""
        got = self.tracks(allow_overflow=True)
        if got is None:
            return []
        return [ObjectTrack(r) for r in got[0] if not confirmed_only or r["state"] == 2]

    def objectTracks(self) -> np.ndarray:
        """per object the last update read, the id of the track its detection matched or founded, 0 for none:
        objectTracks()[objectIds()[ty, tx]] is the track of a texel"""
        n = C.c_uint32(0)
        self.ctx.check(self.L.suma_localizer_object_tracks(self.h, None, 0, C.byref(n)), "suma_localizer_object_tracks")
        out = np.zeros(n.value, dtype=np.uint32)
        if n.value:
            self.ctx.check(self.L.suma_localizer_object_tracks(self.h, _ptr(out), out.size, C.byref(n)),
                           "suma_localizer_object_tracks")
        return out

    def trackObjects(self, objects: np.ndarray, scan_id: int) -> dict:
        """the primitive: one tracker update over the caller's SCAN_OBJECT_DTYPE records in place of a segmentation's;
        returns the update's counts"""
        rec = np.ascontiguousarray(objects, dtype=SCAN_OBJECT_DTYPE).reshape(-1)
        cnt = TrackCounts()
        self.ctx.check(self.L.suma_localizer_track_objects(self.h, _ptr(rec) if rec.shape[0] else None, rec.shape[0], scan_id,
                                                           C.byref(cnt)), "suma_localizer_track_objects")
        return cnt.as_dict()

    def trackState(self):
        """(the raw table OBJECT_TRACK_DTYPE[max_tracks], last_stamp, next_id): for tests and for keeping a tracker"""
        n, last, nxt = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        self.ctx.check(self.L.suma_localizer_track_state(self.h, None, 0, C.byref(n), None, None), "suma_localizer_track_state")
        out = np.zeros(n.value, dtype=OBJECT_TRACK_DTYPE)
        self.ctx.check(self.L.suma_localizer_track_state(self.h, _ptr(out), out.size, C.byref(n), C.byref(last), C.byref(nxt)),
                       "suma_localizer_track_state")
        return out, last.value, nxt.value

    def setTrackState(self, state: np.ndarray, last_stamp: int, next_id: int):
        """puts a raw table (what trackState gave), the stamp of its last update and the next id back"""
        st = np.ascontiguousarray(state, dtype=OBJECT_TRACK_DTYPE).reshape(-1)
        self.ctx.check(self.L.suma_localizer_set_track_state(self.h, _ptr(st), st.shape[0], last_stamp, next_id),
                       "suma_localizer_set_track_state")

    def modelFrame(self) -> Frame:
        """the window as the last scan's render saw it (the ctx's oldMapFrame)"""
        p = self.params
        return Frame(self.ctx, p.model_width, p.model_height, handle=self.L.suma_map_frame(self.ctx.h, 0))

    def close(self):
        if getattr(self, "h", None):
            self.L.suma_localizer_destroy(self.h)
            self.h = None
            self.ctx.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PlaceIndex:
    """Place recognition over the scans of a mapping session (suma_place_*, csrc/k_place.hip): one descriptor per scan --
    a polar height map about the sensor -- made on the device from a frame the pipeline already holds, and a brute-force
    search that returns candidate places with a yaw.  ``addFrame(ctx, frame, id)`` after a scan
    (``SurfelMapping.frame(0)``), ``queryFrame`` / ``query`` for the k best, ``Localizer.relocalize`` to turn them into a
    pose.  places.save / places.load keep an index with its poses in one file."""

    def __init__(self, place_params: PlaceParams = None, device: int = 0, capacity: int = 0):
        self.L = lib()
        self.params = PlaceParams.defaults() if place_params is None else place_params
        h = C.c_void_p()
        rc = self.L.suma_place_index_create(C.byref(self.params), device, capacity, C.byref(h))
        if rc != 0:
            raise SumaError(f"suma_place_index_create failed ({rc}): {self.L.suma_last_error(None).decode()}")
        self.h = h

    def _check(self, rc, what):
        if rc != 0:
            raise SumaError(f"{what} failed ({rc}): {self.L.suma_place_index_last_error(self.h).decode()}")

    def size(self) -> int:
        return self.L.suma_place_index_size(self.h)

    __len__ = size

    def clear(self):
        self._check(self.L.suma_place_index_clear(self.h), "suma_place_index_clear")

    def addFrame(self, ctx: Context, frame: Frame, id: int):
        self._check(self.L.suma_place_index_add_frame(self.h, ctx.h, frame.h, id), "suma_place_index_add_frame")

    def download(self, first: int = 0, n: int = None):
        """-> (cells n x sectors x rings, norms n x sectors, ids n)"""
        n = self.size() - first if n is None else n
        S, R = self.params.sectors, self.params.rings
        cells, norms = np.zeros((n, S, R), dtype=np.float32), np.zeros((n, S), dtype=np.float32)
        ids = np.zeros(n, dtype=np.uint32)
        self._check(self.L.suma_place_index_download(self.h, first, n, _ptr(cells), _ptr(norms), _ptr(ids)),
                    "suma_place_index_download")
        return cells, norms, ids

    def upload(self, cells, ids):
        """appends entries from host cells (n x sectors x rings); their norms are made on the device"""
        S, R = self.params.sectors, self.params.rings
        cells = np.ascontiguousarray(cells, dtype=np.float32).reshape(-1, S, R)
        ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        if ids.shape[0] != cells.shape[0]:
            raise ValueError("one id per entry")
        self._check(self.L.suma_place_index_upload(self.h, _ptr(cells), _ptr(ids), cells.shape[0]),
                    "suma_place_index_upload")

    @staticmethod
    def _window(exclude):
        return (1, 0) if exclude is None else (int(exclude[0]), int(exclude[1]))

    def queryFrame(self, ctx: Context, frame: Frame, k: int = 8, exclude=None) -> list:
        """the k best entries as dicts (index, id, distance, shift, yaw); ``exclude``: an (lo, hi) window of ids"""
        m, n = (PlaceMatch * PLACE_MAX_MATCHES)(), C.c_uint32(0)
        lo, hi = self._window(exclude)
        self._check(self.L.suma_place_index_query_frame(self.h, ctx.h, frame.h, lo, hi, k, m, C.byref(n)),
                    "suma_place_index_query_frame")
        return [m[i].as_dict() for i in range(n.value)]

    def query(self, cells, k: int = 8, exclude=None) -> list:
        """the same search for a descriptor given on the host (sectors x rings)"""
        cells = np.ascontiguousarray(cells, dtype=np.float32).reshape(self.params.sectors, self.params.rings)
        m, n = (PlaceMatch * PLACE_MAX_MATCHES)(), C.c_uint32(0)
        lo, hi = self._window(exclude)
        self._check(self.L.suma_place_index_query(self.h, _ptr(cells), lo, hi, k, m, C.byref(n)),
                    "suma_place_index_query")
        return [m[i].as_dict() for i in range(n.value)]

    def queryAll(self, ctx: Context, frame: Frame):
        """unsorted: (every entry's least distance, its shift)"""
        n = self.size()
        dist, shift = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.int32)
        self._check(self.L.suma_place_index_query_all(self.h, ctx.h, frame.h, _ptr(dist), _ptr(shift)),
                    "suma_place_index_query_all")
        return dist, shift

    def close(self):
        if getattr(self, "h", None):
            self.L.suma_place_index_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def place_yaw_pose(pose, yaw: float) -> np.ndarray:
    """pose . Rz(yaw): the pose hypothesis of a match (row-major 4x4; numpy's cos / sin, for display and tools)"""
    Rz = np.eye(4)
    Rz[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
    return np.asarray(pose, dtype=np.float64) @ Rz


class Posegraph:
    """Posegraph (src/core/Posegraph.h:10-78) on the device: a prior on the first node plus BetweenFactor<Pose3> edges,
    optimised by Levenberg-Marquardt in fp64 (suma_posegraph_*, k_posegraph.hip).  Poses are row-major 4x4 numpy
    arrays; information matrices are 6x6 in gtsam's tangent order [omega, v].  Its own HIP stream: it may be optimised
    on one thread while another drives a SurfelMapping on the same device."""

    def __init__(self, device: int = 0, node_capacity: int = 1 << 17, edge_capacity: int = 1 << 18, handle=None):
        self.L = lib()
        self.device, self.node_capacity, self.edge_capacity = device, node_capacity, edge_capacity
        if handle is None:
            h = C.c_void_p()
            rc = self.L.suma_posegraph_create(device, node_capacity, edge_capacity, C.byref(h))
            if rc != 0:
                raise SumaError(f"suma_posegraph_create failed ({rc}): {self.L.suma_posegraph_last_error(None).decode()}")
            handle = h
        self.h = handle
        self.last_stats = None
        self.borrowed = False  # a pipeline's own graph (SurfelMapping.posegraph): not destroyed here

    def check(self, rc: int, what: str = ""):
        if rc != 0:
            raise SumaError(f"{what} failed ({rc}): {self.L.suma_posegraph_last_error(self.h).decode()}")

    def reserve(self, node_capacity: int, edge_capacity: int):
        self.check(self.L.suma_posegraph_reserve(self.h, node_capacity, edge_capacity), "suma_posegraph_reserve")

    def edge(self, index: int):
        """(from, to, measurement 4x4, information 6x6) of edge ``index`` in insertion order"""
        a, b = C.c_int32(), C.c_int32()
        Z = np.zeros((4, 4), dtype=np.float64)
        Om = np.zeros((6, 6), dtype=np.float64)
        self.check(self.L.suma_posegraph_edge(self.h, index, C.byref(a), C.byref(b), _ptr(Z), _ptr(Om)),
                   "suma_posegraph_edge")
        return a.value, b.value, Z.T.copy(), Om.T.copy()

    def edges(self):
        return [self.edge(k) for k in range(self.edgeCount())]

    def clone(self) -> "Posegraph":
        h = C.c_void_p()
        self.check(self.L.suma_posegraph_clone(self.h, C.byref(h)), "suma_posegraph_clone")
        return Posegraph(self.device, self.node_capacity, self.edge_capacity, handle=h)

    def clear(self):
        self.check(self.L.suma_posegraph_clear(self.h), "suma_posegraph_clear")

    def setInitial(self, id: int, initial_estimate):
        T = _cm(initial_estimate, np.float64)
        self.check(self.L.suma_posegraph_set_initial(self.h, id, _ptr(T)), "suma_posegraph_set_initial")

    def addEdge(self, from_: int, to: int, measurement, information):
        Z = _cm(measurement, np.float64)
        Om = np.ascontiguousarray(np.asarray(information, dtype=np.float64).reshape(6, 6).T)
        self.check(self.L.suma_posegraph_add_edge(self.h, from_, to, _ptr(Z), _ptr(Om)), "suma_posegraph_add_edge")

    def pose(self, id: int):
        T = np.zeros((4, 4), dtype=np.float64)
        self.check(self.L.suma_posegraph_pose(self.h, id, _ptr(T)), "suma_posegraph_pose")
        return T.T.copy()

    def poses(self):
        n = self.size()
        out = np.zeros((max(n, 1), 4, 4), dtype=np.float64)
        got = C.c_uint32()
        self.check(self.L.suma_posegraph_poses(self.h, _ptr(out), n, C.byref(got)), "suma_posegraph_poses")
        return out[:got.value].transpose(0, 2, 1).copy()

    def size(self) -> int:
        return int(self.L.suma_posegraph_size(self.h))

    def edgeCount(self) -> int:
        return int(self.L.suma_posegraph_edge_count(self.h))

    def error(self) -> float:
        e = C.c_double()
        self.check(self.L.suma_posegraph_error(self.h, C.byref(e)), "suma_posegraph_error")
        return e.value

    def reinitialize(self):
        self.check(self.L.suma_posegraph_reinitialize(self.h), "suma_posegraph_reinitialize")

    def optimize(self, num_iters: int, params: PosegraphParams = None) -> bool:
        """Posegraph::optimize (Posegraph.cpp:92-104); params None = gtsam's LevenbergMarquardtParams defaults.
        The statistics of the run are kept in ``last_stats`` (PosegraphStats)."""
        st = PosegraphStats()
        self.check(self.L.suma_posegraph_optimize(self.h, num_iters, None if params is None else C.byref(params),
                                                  C.byref(st)), "suma_posegraph_optimize")
        self.last_stats = st
        return True

    def linearize(self):
        """the optimiser's linear system at the current poses: dict of factor errors (m x 6, factor 0 = the prior),
        gradient (n x 6), diagonal blocks (n x 6 x 6), band blocks (n-1 x 6 x 6, block (i, i+1)), off-band blocks
        (k x 6 x 6) and their pairs (k x 2)"""
        n, m = self.size(), self.edgeCount() + 1
        e = np.zeros((m, 6))
        g = np.zeros((n, 6))
        D = np.zeros((n, 6, 6))
        U = np.zeros((max(n - 1, 1), 6, 6))
        no = C.c_uint32()
        self.check(self.L.suma_posegraph_linearize(self.h, _ptr(e), _ptr(g), _ptr(D), _ptr(U), None, None, 0,
                                                   C.byref(no)), "suma_posegraph_linearize")
        O = np.zeros((max(no.value, 1), 6, 6))
        P = np.zeros((max(no.value, 1), 2), dtype=np.int32)
        self.check(self.L.suma_posegraph_linearize(self.h, None, None, None, None, _ptr(O), _ptr(P), no.value,
                                                   C.byref(no)), "suma_posegraph_linearize")
        t = lambda B: B.transpose(0, 2, 1).copy()  # column-major blocks -> row-major numpy
        return dict(errors=e, gradient=g, diag=t(D), band=t(U)[:max(n - 1, 0)], off=t(O)[:no.value],
                    off_pairs=P[:no.value])

    def close(self):
        if getattr(self, "h", None):
            if not self.borrowed:
                self.L.suma_posegraph_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
