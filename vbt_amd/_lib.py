"""ctypes binding of libvbt_hip.so (include/vbt_hip.h).  There is no CPU fallback: if the
HIP library is missing this module raises, loudly."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VBT_LIB_PATH") or os.path.join(_HERE, "libvbt_hip.so")   # (VBT_LIB_PATH: developer builds with in-kernel stamps, tools/*_prof.py)
_lib = None

c_void_p, c_int, c_char_p, c_double = ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_double


class VbtError(RuntimeError):
    pass


class VbtArgError(VbtError, ValueError):
    """VBT_ERR_ARG: the library refused an argument (also a ValueError, like the host-side checks of the wrappers)."""


class TrackerParams(ctypes.Structure):
    _fields_ = [("max_age", ctypes.c_int32), ("min_hits", ctypes.c_int32), ("delta_t", ctypes.c_int32),
                ("asso", ctypes.c_int32), ("iou_threshold", c_double), ("inertia", c_double), ("det_thresh", c_double)]


class SortParams(ctypes.Structure):
    """vbt_sort_params (include/vbt_hip.h): SortTracker(max_age, min_hits, iou_threshold) + the id counter's start"""
    _fields_ = [("max_age", ctypes.c_int32), ("min_hits", ctypes.c_int32), ("id_base", ctypes.c_int32), ("iou_threshold", c_double)]


class Run(ctypes.Structure):
    """vbt_run (include/vbt_hip.h): a run of consecutive frames of one clip inside a detector batch."""
    _fields_ = [("clip", ctypes.c_int32), ("slot0", ctypes.c_int32), ("slot_stride", ctypes.c_int32), ("n_frames", ctypes.c_int32),
                ("frame0", ctypes.c_int32), ("frame_step", ctypes.c_int32), ("fps", c_double)]


class LiveClip(ctypes.Structure):
    """vbt_live_clip (include/vbt_hip.h): one clip's live rep analysis record"""
    _fields_ = [("leader_id", ctypes.c_int64), ("rows_consumed", ctypes.c_int32), ("n_phases", ctypes.c_int32),
                ("phase_state", ctypes.c_int32), ("overflow", ctypes.c_int32), ("seq", ctypes.c_uint64)]


class ClosedClip(ctypes.Structure):
    """vbt_closed_clip (include/vbt_hip.h): the result of one slot close"""
    _fields_ = [("clip", ctypes.c_int32), ("best_id", ctypes.c_int32), ("n_rows", ctypes.c_int32), ("n_phases", ctypes.c_int32),
                ("overflow", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class SetReport(ctypes.Structure):
    """vbt_set_report (include/vbt_hip.h)"""
    _fields_ = [(k, ctypes.c_int32) for k in ("n_reps", "best_rep", "stop_rep", "reserved")] + \
               [(k, c_double) for k in ("best_mv", "last_mv", "mean_mv", "mean_pv", "max_pv", "loss_last_pct", "concentric_s", "eccentric_s",
                                        "mean_x_dev")]


class PipelineParams(ctypes.Structure):
    """vbt_pipeline_params (include/vbt_hip.h)"""
    _fields_ = [("n_slots", ctypes.c_int32), ("n_clips", ctypes.c_int32), ("rows_cap", ctypes.c_int32), ("device", ctypes.c_int32),
                ("depth", ctypes.c_int32), ("tracker_stream", ctypes.c_int32), ("defer", ctypes.c_int32), ("selfcheck", ctypes.c_int32),
                ("strict_placement", ctypes.c_int32), ("model_flags", ctypes.c_int32), ("detection_threshold", ctypes.c_float),
                ("group", ctypes.c_int32), ("plate_diameter", c_double), ("diff_threshold", c_double), ("min_distance", c_double),
                ("tracker", TrackerParams)]


class PipelineInfo(ctypes.Structure):
    """vbt_pipeline_info (include/vbt_hip.h)"""
    _fields_ = [(k, ctypes.c_int32) for k in ("n_slots", "n_clips", "rows_cap", "device", "depth", "ring", "defer", "tracker_inline", "image_size",
                                               "frame_count", "steps_enqueued", "placement_ok", "queue_groups_seen", "group", "next_slot")] + \
               [("reserved", ctypes.c_int32 * 1), ("det_streams", c_void_p * 8), ("copy_stream", c_void_p), ("tracker_stream", c_void_p),
                ("h2d_bytes", ctypes.c_uint64), ("step_host_ns", ctypes.c_uint64), ("step_calls", ctypes.c_uint64)]


class EvalSummary(ctypes.Structure):
    """vbt_eval_summary (include/vbt_hip.h)"""
    _fields_ = [(k, ctypes.c_int32) for k in ("n_rows", "n_pos", "n_neg", "n_pr", "n_roc", "flags")] + [("ap", c_double), ("auc", c_double)]


class CocoSummary(ctypes.Structure):
    """vbt_coco_summary (include/vbt_hip.h)"""
    _fields_ = [("stats", c_double * 12), ("n_images", ctypes.c_int32), ("n_rows", ctypes.c_int32), ("n_gt", ctypes.c_int32 * 4)]


class OverlayParams(ctypes.Structure):
    """vbt_overlay_params (include/vbt_hip.h)"""
    _fields_ = [("trail", ctypes.c_int32), ("thickness", ctypes.c_int32), ("radius", ctypes.c_int32), ("label_scale", ctypes.c_int32),
                ("rgb", ctypes.c_uint8 * 3), ("label", ctypes.c_uint8), ("box", ctypes.c_uint8), ("reserved", ctypes.c_uint8 * 3)]


class OverlayHudParams(ctypes.Structure):
    """vbt_overlay_hud_params (include/vbt_hip.h)"""
    _fields_ = [("x", ctypes.c_int32), ("y", ctypes.c_int32), ("scale", ctypes.c_int32), ("full_scale_cm", ctypes.c_int32),
                ("bg", ctypes.c_uint8 * 3), ("reserved", ctypes.c_uint8 * 5)]


class FigureParams(ctypes.Structure):
    """vbt_figure_params (include/vbt_hip.h)"""
    _fields_ = [(k, ctypes.c_int32) for k in ("width", "height", "scale", "thickness", "max_figures", "max_rows", "max_phases", "reserved")]


class CurveFigureParams(ctypes.Structure):
    """vbt_curve_figure_params (include/vbt_hip.h)"""
    _fields_ = [(k, ctypes.c_int32) for k in ("width", "height", "scale", "thickness", "max_figures", "max_series", "max_points", "max_marks")]


class ValidationParams(ctypes.Structure):
    """vbt_validation_params (include/vbt_hip.h)"""
    _fields_ = [(k, ctypes.c_int32) for k in ("width", "height", "scale", "thickness", "max_pairs", "max_rows", "max_ref_rows", "max_grid", "reserved")]


class CurveFigureDesc(ctypes.Structure):
    """vbt_curve_figure_desc (include/vbt_hip.h)"""
    _fields_ = [(k, ctypes.c_int32) for k in ("n_series", "n_marks", "legend_corner", "minor_x", "minor_y")] + \
               [("reserved", ctypes.c_int32 * 3), ("x_title", ctypes.c_char * 32), ("y_title", ctypes.c_char * 32)]


class CurveSeries(ctypes.Structure):
    """vbt_curve_series (include/vbt_hip.h)"""
    _fields_ = [("n_points", ctypes.c_int32), ("colour", ctypes.c_int32), ("text", ctypes.c_char * 64)]


class CurveMark(ctypes.Structure):
    """vbt_curve_mark (include/vbt_hip.h)"""
    _fields_ = [("series", ctypes.c_int32), ("point", ctypes.c_int32), ("text", ctypes.c_char * 16)]


class KernelStat(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 32), ("launches", c_int), ("algorithmic_bytes", c_double), ("macs", c_double)]


class StepTime(ctypes.Structure):
    _fields_ = [("family", ctypes.c_char * 32), ("op", c_int), ("first_op", c_int), ("variant", c_int), ("ms", c_double),
                ("algorithmic_bytes", c_double), ("macs", c_double)]


class PlanStepSpace(ctypes.Structure):
    """vbt_plan_step_space (include/vbt_hip_diag.h): one step of one alternative of one plan group and what a plan file may select for it"""
    _fields_ = [("group", c_int), ("alt", c_int), ("step", c_int), ("chosen", c_int), ("variant", c_int), ("first_op", c_int),
                ("last_op", c_int), ("family", ctypes.c_char * 32),
                ("n_variants", c_int), ("variants", c_int * 48)]


class PlanStepInfo(ctypes.Structure):
    """vbt_plan_step_info (include/vbt_hip_diag.h): one step of the execution list"""
    _fields_ = [("family", ctypes.c_char * 32), ("variant", c_int), ("reads_frames", c_int), ("image0_only", c_int), ("group", c_int),
                ("step", c_int), ("first_op", c_int), ("last_op", c_int), ("n_members", c_int)]


_SIGS = {
    "vbt_last_error": (c_char_p, []),
    "vbt_device_count": (c_int, []),
    "vbt_model_create": (c_int, [c_char_p, c_int, c_int, ctypes.POINTER(c_void_p)]),
    "vbt_model_create_ex": (c_int, [c_char_p, c_int, c_int, c_int, ctypes.POINTER(c_void_p)]),
    "vbt_model_destroy": (None, [c_void_p]),
    "vbt_model_tensor_materialized": (c_int, [c_void_p, c_int]),
    "vbt_model_num_launches": (c_int, [c_void_p]),
    "vbt_model_input_shape": (c_int, [c_void_p, ctypes.POINTER(c_int)]),
    "vbt_model_num_tensors": (c_int, [c_void_p]),
    "vbt_model_num_ops": (c_int, [c_void_p]),
    "vbt_model_tensor_shape": (c_int, [c_void_p, c_int, ctypes.POINTER(c_int)]),
    "vbt_detect": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int]),
    "vbt_detect_async": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "vbt_detect_range_async": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "vbt_model_entry_steps": (c_int, [c_void_p]),
    "vbt_stream_create": (c_int, [c_int, c_void_p]),
    "vbt_stream_destroy": (c_int, [c_void_p]),
    "vbt_streams_share_queue": (c_int, [c_void_p, c_void_p, c_int, c_void_p]),
    "vbt_model_read_tensor": (c_int, [c_void_p, c_int, c_int, c_void_p]),
    "vbt_model_write_tensor": (c_int, [c_void_p, c_int, c_int, c_void_p]),
    "vbt_model_plan_space": (c_int, [c_void_p, c_void_p, c_int, ctypes.POINTER(c_int)]),
    "vbt_model_plan_steps": (c_int, [c_void_p, c_void_p, c_int, ctypes.POINTER(c_int)]),
    "vbt_model_step_proj_tail": (c_int, [c_void_p, c_int, c_int, c_int]),
    "vbt_model_step_fused_params": (c_int, [c_void_p, c_int, c_int, c_int]),
    "vbt_resize_frames": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "vbt_resize_frames_yuv": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "vbt_pix_frame_bytes": (ctypes.c_size_t, [c_int, c_int, c_int]),
    "vbt_resize_frames_pix": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "vbt_model_kernel_stats": (c_int, [c_void_p, c_int, ctypes.POINTER(KernelStat), c_int, ctypes.POINTER(c_int)]),
    "vbt_model_profile": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, ctypes.POINTER(c_double), c_int]),
    "vbt_model_profile_families": (c_int, [c_void_p, c_int, c_int, c_void_p, ctypes.POINTER(c_double), c_int]),
    "vbt_model_profile_steps": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, ctypes.POINTER(StepTime), c_int, ctypes.POINTER(c_int)]),
    "vbt_model_profile_overlap": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p]),
    "vbt_tracker_create": (c_int, [c_int, c_int, ctypes.POINTER(TrackerParams), c_int, ctypes.POINTER(c_void_p)]),
    "vbt_tracker_create_sort": (c_int, [c_int, c_int, ctypes.POINTER(SortParams), c_int, ctypes.POINTER(c_void_p)]),
    "vbt_pipeline_use_sort": (c_int, [c_void_p, ctypes.POINTER(SortParams)]),
    "vbt_tracker_destroy": (None, [c_void_p]),
    "vbt_tracker_reset":(c_int, [c_void_p]),
    "vbt_tracker_reset_clips": (c_int, [c_void_p, c_void_p, c_int, c_void_p]),
    "vbt_tracker_update": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int]),
    "vbt_tracker_update_from_detections": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_float, c_void_p]),
    "vbt_tracker_last_output": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, ctypes.POINTER(c_int)]),
    "vbt_tracker_get_trackers": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, ctypes.POINTER(c_int)]),
    "vbt_tracker_status": (c_int, [c_void_p, c_int] + [ctypes.POINTER(ctypes.c_int32)] * 5),
    "vbt_tracker_rows": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, ctypes.POINTER(c_int)]),
    "vbt_tracker_finish": (c_int, [c_void_p, c_double, c_double, c_double, c_void_p]),
    "vbt_tracker_phases": (c_int, [c_void_p, c_int, ctypes.POINTER(ctypes.c_int32), c_void_p, c_int, ctypes.POINTER(c_int)]),
    "vbt_tracker_update_from_slots": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, ctypes.c_float, c_void_p]),
    "vbt_tracker_update_from_detections_seq": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, ctypes.c_float, c_void_p]),
    "vbt_gather_frames": (c_int, [c_void_p, c_void_p, c_int, ctypes.c_size_t, c_void_p]),
    "vbt_tracker_summary": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int]),
    "vbt_tracker_rows_all": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "vbt_tracker_live_enable": (c_int, [c_void_p, c_int, c_int, c_double, c_double, c_double]),
    "vbt_tracker_live_poll": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p]),
    "vbt_tracker_live_tracks": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, ctypes.POINTER(c_int)]),
    "vbt_tracker_rep_metrics_enable": (c_int, [c_void_p]),
    "vbt_tracker_rep_metrics": (c_int, [c_void_p, c_int, c_void_p, c_int, ctypes.POINTER(c_int)]),
    "vbt_tracker_summary_ex": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int]),
    "vbt_tracker_live_poll_ex": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "vbt_pipeline_default_params": (None, [ctypes.POINTER(PipelineParams)]),
    "vbt_pipeline_create": (c_int, [c_char_p, ctypes.POINTER(PipelineParams), c_void_p, ctypes.POINTER(c_void_p)]),
    "vbt_pipeline_destroy": (None, [c_void_p]),
    "vbt_pipeline_step": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "vbt_pipeline_step_runs": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_void_p]),
    "vbt_pipeline_set_pixel_format": (c_int, [c_void_p, c_int]),
    "vbt_pipeline_set_colour": (c_int, [c_void_p, c_int, c_int]),
    "vbt_pipeline_skip_frames": (c_int, [c_void_p, c_int]),
    "vbt_pipeline_set_frame_count": (c_int, [c_void_p, c_int]),
    "vbt_pipeline_reset": (c_int, [c_void_p]),
    "vbt_pipeline_join_detectors": (c_int, [c_void_p, c_void_p]),
    "vbt_pipeline_close": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int]),
    "vbt_pipeline_finish": (c_int, [c_void_p]),
    "vbt_pipeline_close_clips_enable": (c_int, [c_void_p]),
    "vbt_pipeline_close_clips": (c_int, [c_void_p, c_void_p, c_int, c_void_p]),
    "vbt_pipeline_closed_clip": (c_int, [c_void_p, c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(ClosedClip), c_void_p, c_int, c_void_p, c_int]),
    "vbt_pipeline_drain": (c_int, [c_void_p]),
    "vbt_pipeline_rows_all": (c_int, [c_void_p, c_void_p, c_void_p, c_int]),
    "vbt_pipeline_rows": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, ctypes.POINTER(c_int)]),
    "vbt_pipeline_detections": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, ctypes.POINTER(c_int)]),
    "vbt_pipeline_tracker_only_steps": (c_int, [c_void_p, c_int, c_int]),
    "vbt_pipeline_live_enable": (c_int, [c_void_p, c_int, c_int]),
    "vbt_pipeline_live_poll": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int]),
    "vbt_pipeline_rep_metrics_enable": (c_int, [c_void_p]),
    "vbt_pipeline_close_ex": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int]),
    "vbt_pipeline_closed_clip_ex": (c_int, [c_void_p, c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(ClosedClip), c_void_p, c_void_p, c_int,
                                            c_void_p, c_int]),
    "vbt_pipeline_live_poll_ex": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int]),
    "vbt_pipeline_get_info": (c_int, [c_void_p, ctypes.POINTER(PipelineInfo)]),
    "vbt_pipeline_model": (c_void_p, [c_void_p, c_int]),
    "vbt_pipeline_tracker": (c_void_p, [c_void_p]),
    "vbt_track_clip": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, ctypes.POINTER(c_int)]),
    "vbt_host_alloc": (c_int, [ctypes.c_size_t, ctypes.POINTER(c_void_p)]),
    "vbt_host_free": (c_int, [c_void_p]),
    "vbt_device_alloc": (c_int, [c_int, ctypes.c_size_t, ctypes.POINTER(c_void_p)]),
    "vbt_device_free": (c_int, [c_void_p]),
    "vbt_memcpy": (c_int, [c_void_p, c_void_p, ctypes.c_size_t, c_int]),
    "vbt_stream_synchronize": (c_int, [c_void_p]),
    "vbt_device_synchronize": (c_int, [c_int]),
    "vbt_analyze": (c_int, [c_void_p, c_int, c_int, c_int, c_double, c_double, c_double, c_void_p, c_int, ctypes.POINTER(c_int), c_int]),
    "vbt_analyze_metrics": (c_int, [c_void_p, c_int, c_int, c_int, c_double, c_double, c_double, c_void_p, c_void_p, c_int, ctypes.POINTER(c_int),
                                    c_int]),
    "vbt_set_summary": (c_int, [c_void_p, c_void_p, c_int, c_double, ctypes.POINTER(SetReport), c_void_p, c_int]),
    "vbt_window_means": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_int]),
    "vbt_eval_create": (c_int, [c_int, c_int, c_int, ctypes.POINTER(c_void_p)]),
    "vbt_eval_destroy": (None, [c_void_p]),
    "vbt_eval_reset": (c_int, [c_void_p]),
    "vbt_eval_add_detections": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "vbt_eval_table": (c_int, [c_void_p, ctypes.POINTER(c_int), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int]),
    "vbt_eval_curves": (c_int, [c_void_p, c_double, ctypes.POINTER(EvalSummary), c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int]),
    "vbt_eval_curves_from_table": (c_int, [c_void_p, c_void_p, c_int, c_double, c_int, ctypes.POINTER(EvalSummary), c_void_p, c_void_p, c_void_p, c_int,
                                           c_void_p, c_void_p, c_void_p, c_int]),
    "vbt_coco_create": (c_int, [c_int, c_int, c_int, ctypes.POINTER(c_void_p)]),
    "vbt_coco_destroy": (None, [c_void_p]),
    "vbt_coco_reset": (c_int, [c_void_p]),
    "vbt_coco_add_detections": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "vbt_coco_table": (c_int, [c_void_p, ctypes.POINTER(c_int), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int]),
    "vbt_coco_accumulate": (c_int, [c_void_p, ctypes.POINTER(CocoSummary), c_void_p, c_void_p, c_void_p]),
    "vbt_overlay_default_params": (None, [ctypes.POINTER(OverlayParams)]),
    "vbt_overlay_create": (c_int, [c_int, c_int, c_int, c_int, ctypes.POINTER(OverlayParams), ctypes.POINTER(c_void_p)]),
    "vbt_overlay_destroy": (None, [c_void_p]),
    "vbt_overlay_set_rows": (c_int, [c_void_p, c_void_p, c_int, c_double, c_void_p]),
    "vbt_overlay_draw": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "vbt_overlay_geometry": (c_int, [c_void_p, c_void_p, c_int, ctypes.POINTER(c_int)]),
    "vbt_overlay_hud_default_params": (None, [ctypes.POINTER(OverlayHudParams)]),
    "vbt_overlay_set_hud": (c_int, [c_void_p, ctypes.POINTER(OverlayHudParams), c_void_p, c_int, c_double, c_void_p]),
    "vbt_overlay_hud_table": (c_int, [c_void_p, c_void_p, c_int, ctypes.POINTER(c_int)]),
    "vbt_overlay_hud_follow": (c_int, [c_void_p, ctypes.POINTER(OverlayHudParams), c_void_p, c_int, c_double]),
    "vbt_overlay_hud_follow_update": (c_int, [c_void_p, c_int, c_void_p]),
    "vbt_overlay_hud_follow_status": (c_int, [c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32), c_void_p]),
    "vbt_overlay_hud_follow_flush": (c_int, [c_void_p, c_int]),
    "vbt_overlay_follow": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_double]),
    "vbt_overlay_follow_update": (c_int, [c_void_p, c_void_p]),
    "vbt_overlay_follow_status": (c_int, [c_void_p, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32), c_void_p]),
    "vbt_tracker_rows_dev": (c_int, [c_void_p, c_int, ctypes.POINTER(c_void_p), ctypes.POINTER(c_void_p), ctypes.POINTER(c_int)]),
    "vbt_pipeline_overlay_draw": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "vbt_figure_default_params": (None, [ctypes.POINTER(FigureParams)]),
    "vbt_figure_create": (c_int, [c_int, ctypes.POINTER(FigureParams), ctypes.POINTER(c_void_p)]),
    "vbt_figure_destroy": (None, [c_void_p]),
    "vbt_figure_set": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "vbt_figure_render": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "vbt_figure_table": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, ctypes.POINTER(c_int), c_void_p, c_int, ctypes.POINTER(c_int)]),
    "vbt_curve_figure_default_params": (None, [ctypes.POINTER(CurveFigureParams)]),
    "vbt_curve_figure_create": (c_int, [c_int, ctypes.POINTER(CurveFigureParams), ctypes.POINTER(c_void_p)]),
    "vbt_curve_figure_destroy": (None, [c_void_p]),
    "vbt_curve_figure_set": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "vbt_curve_figure_render": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "vbt_curve_figure_table": (c_int, [c_void_p, c_int, c_void_p, c_int, ctypes.POINTER(c_int), c_void_p, c_int, ctypes.POINTER(c_int), c_void_p, c_int,
                                       ctypes.POINTER(c_int)]),
    "vbt_validation_default_params": (None, [ctypes.POINTER(ValidationParams)]),
    "vbt_validation_create": (c_int, [c_int, ctypes.POINTER(ValidationParams), ctypes.POINTER(c_void_p)]),
    "vbt_validation_destroy": (None, [c_void_p]),
    "vbt_validation_set": (c_int, [c_void_p, c_int, c_void_p, c_double, c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "vbt_validation_stats": (c_int, [c_void_p, c_void_p, c_int]),
    "vbt_validation_table": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, ctypes.POINTER(c_int), c_void_p, c_int, ctypes.POINTER(c_int), c_void_p,
                                     c_void_p, c_int, ctypes.POINTER(c_int), c_void_p, c_int, ctypes.POINTER(c_int)]),
    "vbt_validation_render": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "vbt_mjpeg_create": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_void_p)]),
    "vbt_mjpeg_destroy": (None, [c_void_p]),
    "vbt_mjpeg_encode": (c_int, [c_void_p, c_void_p, c_int, c_void_p]),
    "vbt_mjpeg_read": (c_int, [c_void_p, c_void_p, ctypes.c_uint64, c_void_p, c_void_p]),
    "vbt_display_size": (c_int, [c_int, c_int, c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "vbt_scaler_create": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_void_p)]),
    "vbt_scaler_destroy": (None, [c_void_p]),
    "vbt_scaler_run": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "vbt_scaler_tables": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, ctypes.POINTER(c_int)]),
    "vbt_mjpeg_create_scaled": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_void_p)]),
    "vbt_jpeg_probe": (c_int, [c_void_p, ctypes.c_uint64] + [ctypes.POINTER(c_int)] * 4),
    "vbt_mjpeg_decoder_create": (c_int, [c_int, c_int, c_int, c_int, ctypes.POINTER(c_void_p)]),
    "vbt_mjpeg_decoder_destroy": (None, [c_void_p]),
    "vbt_mjpeg_decode": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "vbt_mjpeg_decode_status": (c_int, [c_void_p, c_void_p, c_void_p]),
    "vbt_mjpeg_decode_stage_ms": (c_int, [c_void_p, ctypes.POINTER(ctypes.c_float)]),
    "vbt_mjpeg_decoder_set_entropy": (c_int, [c_void_p, c_int, c_int]),
    "vbt_mjpeg_decoder_get_entropy": (c_int, [c_void_p, ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "vbt_mjpeg_decode_entropy_info": (c_int, [c_void_p, c_void_p, c_void_p]),
    "vbt_jpeg_blocks": (c_int, [c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint32)]),
    "vbt_jpeg_stills_create": (c_int, [c_int, c_int, ctypes.c_uint64, ctypes.POINTER(c_void_p)]),
    "vbt_jpeg_stills_destroy": (None, [c_void_p]),
    "vbt_jpeg_stills_decode_resized": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p]),
    "vbt_jpeg_stills_decode": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "vbt_jpeg_stills_status": (c_int, [c_void_p, c_void_p, c_void_p]),
    "vbt_jpeg_stills_set_entropy": (c_int, [c_void_p, c_int, c_int]),
    "vbt_jpeg_stills_get_entropy": (c_int, [c_void_p, ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "vbt_jpeg_stills_stage_ms": (c_int, [c_void_p, ctypes.POINTER(ctypes.c_float)]),
    "vbt_jpeg_stills_entropy_info": (c_int, [c_void_p, c_void_p, c_void_p]),
    "vbt_jpeg_stills_uploaded_bytes": (c_int, [c_void_p, ctypes.POINTER(ctypes.c_uint64)]),
}


def _preload_hip_runtime():
    """One HIP runtime per process.  A torch wheel bundles its own libamdhip64 / libhsa-runtime64 (same soname as /opt/rocm's): if this
    library bound to the system copy and torch were imported afterwards, torch's runtime would find "no HIP GPUs".  So when a torch
    wheel is installed its libamdhip64 is loaded first - by path, WITHOUT importing torch - and libvbt_hip.so's DT_NEEDED entry then
    resolves to that already-loaded object by soname; `import torch`, before or after, shares it.  No import-order requirement is left.
    Without a torch wheel (or with VBT_HIP_RUNTIME=system) the system runtime under /opt/rocm is used."""
    import sys
    if "torch" in sys.modules or os.environ.get("VBT_HIP_RUNTIME") == "system":
        return
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    so = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(so):
        ctypes.CDLL(so, mode=ctypes.RTLD_GLOBAL)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise VbtError(f"{LIB_PATH} is missing: build it with `python -m vbt_amd.build` "
                           "(__graft_entry__.build()). vbt_amd has no CPU fallback.")
        _preload_hip_runtime()
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(L, name)          # AttributeError if the library does not export the symbol
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


def declared_symbols():
    return list(_SIGS)


def check(rc):
    if rc != 0:
        raise (VbtArgError if rc == -1 else VbtError)(f"libvbt_hip error {rc}: {lib().vbt_last_error().decode()}")
