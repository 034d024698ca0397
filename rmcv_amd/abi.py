"""ctypes binding of librmcv_hip.so (the C-ABI declared in include/rmcv_abi.h).

There is no fallback: if the HIP library is missing or no GPU is usable, the calls raise.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RMCV_LIB_PATH") or os.path.join(_HERE, "lib", "librmcv_hip.so")  # env: dev A/B builds

# PODs of include/rmcv_abi.h as numpy dtypes
POINT = np.dtype([("x", "<i4"), ("y", "<i4")])
RRECT = np.dtype([("cx", "<f4"), ("cy", "<f4"), ("w", "<f4"), ("h", "<f4"), ("angle", "<f4")])
LIGHTBLOB = np.dtype([("angle", "<f4"), ("target", "<i4"), ("center", "<f4", (2,)),
                      ("vertices", "<f4", (4, 2)), ("size", "<f4", (2,))])
ARMOUR = np.dtype([("icon", "<f4", (4, 2)), ("vertices", "<f4", (4, 2)), ("bbox", "<f4", (4,)),
                   ("blob_i", "<i4"), ("blob_j", "<i4")])
TRACK_IDS = 32
TRACK = np.dtype([("armour", ARMOUR), ("timestamp", "<i8"), ("lost_count", "<i4"), ("identity", "<i4"), ("position", "<f8", (3,)),
                  ("initialized", "<i4"), ("n_ids", "<i4"), ("ids", "<i4", (TRACK_IDS,)), ("counts", "<i4", (TRACK_IDS,)),
                  ("measurement", "<f8", (6,)), ("state_pre", "<f8", (6,)), ("state_post", "<f8", (6,)),
                  ("transition", "<f8", (6, 6)), ("measurement_matrix", "<f8", (6, 6)), ("process_noise_cov", "<f8", (6, 6)),
                  ("measurement_noise_cov", "<f8", (6, 6)), ("error_cov_pre", "<f8", (6, 6)), ("error_cov_post", "<f8", (6, 6)),
                  ("gain", "<f8", (6, 6))])  # rmcv_track
assert POINT.itemsize == 8 and LIGHTBLOB.itemsize == 56 and ARMOUR.itemsize == 88 and TRACK.itemsize == 2552
AIM = np.dtype([("track", "<i4"), ("identity", "<i4"), ("lost_count", "<i4"), ("status", "<i4"), ("pitch", "<f8"), ("yaw", "<f8"),
                ("flight_time", "<f8"), ("distance", "<f8"), ("point", "<f8", (3,))])  # rmcv_aim
AIM_INPUT = np.dtype([("world2camera", "<f8", (4, 4)), ("motor_angle", "<f8")])  # rmcv_aim_input
assert AIM.itemsize == 72 and AIM_INPUT.itemsize == 136
ATTITUDE = np.dtype([("roll", "<f8"), ("pitch", "<f8"), ("yaw", "<f8")])  # rmcv_attitude: radians = rm::euler<double>{x, y, z}
ATTITUDE_CONFIG = np.dtype([("gripper2camera", "<f8", (4, 4)), ("motor_angle_mode", "<i4"), ("reserved", "<i4")])  # rmcv_attitude_config
assert ATTITUDE.itemsize == 24 and ATTITUDE_CONFIG.itemsize == 136
SERIAL_PACKET_BYTES = 24
ATT_MOTOR_KEEP, ATT_MOTOR_PITCH = 0, 1

OK, ERR_BAD_ARG, ERR_CAPACITY, ERR_NOMEM, ERR_HIP, ERR_NO_DEVICE, ERR_RCCL, ERR_TIMEOUT = 0, -1, -2, -3, -4, -5, -6, -7
COMM_ID_BYTES = 128
CAMP_RED, CAMP_BLUE, CAMP_GUIDELIGHT, CAMP_NEUTRAL = 0, 1, 2, -1
MORPH_NONE, MORPH_DILATE, MORPH_CLOSE = 0, 1, 2
OPT_SPARSE_WAVES = 1
OPT_PIXEL_GROUPS = 2
OPT_FRAME_UPLOAD = 3
OPT_RUN_AHEAD = 4
OPT_CONTOUR_TIER = 5
OPT_DENSE_DEFER = 7
OPT_PIXEL_HALO_NT = 11
OPT_OVERLOADS = 13
OPT_PIXEL_SHAPE = 14
OPT_WAIT_TIMEOUT_MS = 15
OPT_TEST_DELAY_US = 16
OPT_IMAGE_EXPORT = 17
OPT_TEST_SLOW_US = 18
OPT_INPUT_FORMAT = 19
# RMCV_OPT_INPUT_FORMAT values: BGR frames, or a raw 8-bit mosaic named by its top-left 2x2 block (the Daheng SDK's DX_PIXEL_COLOR_FILTER values)
INPUT_BGR, BAYER_RG, BAYER_GB, BAYER_GR, BAYER_BG = 0, 1, 2, 3, 4
BAYER_PATTERNS = (BAYER_RG, BAYER_GB, BAYER_GR, BAYER_BG)
# the Bayer frame as the sensor delivers it: 8- or 16-bit samples, the pixel's first bit in a 16-bit sample (the Daheng SDK's DX_VALID_BIT, 0..4), mirror / flip
OPT_INPUT_SAMPLE_BITS = 20
OPT_INPUT_VALID_BIT = 21
OPT_INPUT_ORIENT = 22
ORIENT_MIRROR, ORIENT_FLIP = 1, 2
# exposure-adaptive detection: frames are read through their rm::AutoEnhance table (gains: rmcv_ctx_set_enhance_gains, defaults 100, 50)
OPT_ENHANCE = 23
ENHANCE_MAX_GAIN, ENHANCE_MIN_GAIN = 100.0, 50.0
STAGE_BINARY, STAGE_CONTOURS, STAGE_BLOBS, STAGE_ARMOURS, STAGE_ALL, STAGE_IDENTITY, STAGE_POSE, STAGE_NO_IMAGE = 1, 2, 4, 8, 15, 16, 32, 64
SVM_FEATURES = 1200
COMPENSATE_NONE, COMPENSATE_CLASSIC, COMPENSATE_NI = 0, 1, 2   # rm::CompensateMode (include/mobility.h:18-23)
AIM_NO_TARGET, AIM_NO_SOLUTION = 1, 2
AIM_HEIGHT_FIXED, AIM_HEIGHT_DELTA = 0, 1
AIM_SRC_FILTER, AIM_SRC_MEASUREMENT = 0, 1
AIM_PICK_WINDOW, AIM_PICK_NEAREST = 0, 1
VIEW_BLOBS, VIEW_NEGATIVES, VIEW_ARMOURS, VIEW_ALL = 1, 2, 4, 7  # RMCV_VIEW_*: what the debug view draws over the binary (all: the reference)
LABEL_ARMOURS, LABEL_TRACKS, LABEL_MAX_CHARS = 1, 2, 112  # RMCV_LABEL_*: what the label pass draws over finished views
LABEL_CHARSET = "0123456789-.:, naifbg"  # the characters a line can contain = the glyphs rmcv_view_glyph hands out
FRAME_OVF_CONTOURS, FRAME_OVF_POINTS, FRAME_OVF_BLOBS, FRAME_OVF_ARMOURS, FRAME_SLOW_PATH, FRAME_MID_PATH = 1, 2, 4, 8, 16, 64
# dataset harvest: a label that keeps a frame out, the flag that keeps only the model's misses, a row's 64-byte metadata
HARVEST_SKIP, HARVEST_MISSES = -2**31, 1
ICON_SAD_MAX, HARVEST_RING_MAX = 306000, 8   # novelty: the largest distance of two icon rows, the deepest ring per stream
HARVEST_META = np.dtype([("tag", "<u8"), ("frame", "<i4"), ("armour", "<i4"), ("label", "<i4"), ("identity", "<i4"), ("win_x", "<i4"), ("win_y", "<i4"),
                         ("icon", "<f4", (4, 2))])

EXPORTS = [
    "rmcv_abi_version", "rmcv_default_params", "rmcv_default_limits", "rmcv_ctx_create", "rmcv_ctx_destroy",
    "rmcv_last_error", "rmcv_ctx_set_option", "rmcv_ctx_forget_frame_buffer", "rmcv_ctx_check_guards", "rmcv_ctx_frame_timing", "rmcv_extract_color", "rmcv_filter_lightblobs", "rmcv_filter_armours", "rmcv_fit_ellipse", "rmcv_demosaic", "rmcv_demosaic_raw",
    "rmcv_batch_upload", "rmcv_batch_set_device_frames", "rmcv_batch_run", "rmcv_batch_sync", "rmcv_batch_run_timed",
    "rmcv_batch_counts", "rmcv_batch_get_binary", "rmcv_batch_get_contours", "rmcv_batch_get_blobs",
    "rmcv_batch_get_armours", "rmcv_batch_device_views", "rmcv_batch_compact_armours", "rmcv_synth_frame", "rmcv_synth_checksum",
    "rmcv_svm_load", "rmcv_classify_armours", "rmcv_batch_get_identities", "rmcv_batch_get_icons",
    "rmcv_default_pnp_config", "rmcv_pnp_load", "rmcv_locate_armours", "rmcv_batch_set_base2gripper", "rmcv_batch_get_poses",
    "rmcv_max_iou", "rmcv_identity_max", "rmcv_comm_unique_id", "rmcv_comm_create", "rmcv_comm_destroy", "rmcv_comm_info", "rmcv_comm_last_error", "rmcv_gather",
    "rmcv_default_pipeline_config", "rmcv_pipeline_create", "rmcv_pipeline_destroy", "rmcv_pipeline_last_error", "rmcv_pipeline_get_info", "rmcv_pipeline_context", "rmcv_pipeline_context_of", "rmcv_pipeline_set_hot_contexts", "rmcv_pipeline_set_wait_timeout", "rmcv_pipeline_reset_stats", "rmcv_hw_queues_hint", "rmcv_pixel_ws_launches", "rmcv_pixel_image_delta_launches", "rmcv_pixel_plane_delta_launches",
    "rmcv_pipeline_submit", "rmcv_pipeline_submit_legacy", "rmcv_pipeline_wait", "rmcv_pipeline_collect", "rmcv_pipeline_drain", "rmcv_pipeline_record",
    "rmcv_pipeline_set_hook", "rmcv_pipeline_set_gather", "rmcv_pipeline_gathered", "rmcv_device_alloc", "rmcv_device_free", "rmcv_device_upload", "rmcv_device_download",
    "rmcv_track_init", "rmcv_track_reset", "rmcv_track_update", "rmcv_track_predict", "rmcv_track_step", "rmcv_min_area_rect", "rmcv_match_lightblob", "rmcv_find_lightblobs", "rmcv_lightblob_overlap", "rmcv_batch_run_legacy",
    "rmcv_ctx_set_enhance_gains", "rmcv_ctx_get_enhance", "rmcv_gamma_lut", "rmcv_enhance_gamma", "rmcv_calc_gamma", "rmcv_auto_enhance", "rmcv_batch_get_gammas",
    "rmcv_batch_set_windows", "rmcv_batch_set_device_windows", "rmcv_batch_get_windows", "rmcv_batch_device_windows", "rmcv_pipeline_submit_windows",
    "rmcv_get_roi", "rmcv_window_origin", "rmcv_armours_to_frame",
    "rmcv_default_tracker_config", "rmcv_tracker_create", "rmcv_tracker_destroy", "rmcv_tracker_last_error", "rmcv_tracker_reset", "rmcv_tracker_set_origins",
    "rmcv_tracker_device_origins", "rmcv_batch_track", "rmcv_tracker_counts", "rmcv_tracker_get", "rmcv_tracker_step_host", "rmcv_pipeline_submit_tracked",
    "rmcv_projectile_angle", "rmcv_solve_gea", "rmcv_delta_height", "rmcv_distance", "rmcv_rigid_inverse", "rmcv_default_aim_config", "rmcv_tracker_set_aim",
    "rmcv_tracker_set_aim_inputs", "rmcv_tracker_device_aim_inputs", "rmcv_tracker_aim", "rmcv_tracker_get_aims", "rmcv_tracker_device_aims", "rmcv_tracker_put",
    "rmcv_aim_step_host",
    "rmcv_frame_key", "rmcv_batch_set_frame_camps", "rmcv_batch_set_device_frame_camps", "rmcv_batch_get_frame_keys", "rmcv_pipeline_submit_camps",
    "rmcv_tracker_set_camps", "rmcv_tracker_device_camps",
    "rmcv_euler_to_matrix", "rmcv_homogeneous", "rmcv_crc8", "rmcv_serial_decode", "rmcv_serial_encode", "rmcv_attitude_step_host", "rmcv_default_attitude_config",
    "rmcv_tracker_set_attitude", "rmcv_tracker_set_attitudes", "rmcv_tracker_get_attitudes", "rmcv_tracker_device_attitudes", "rmcv_tracker_get_aim_inputs",
    "rmcv_batch_get_base2gripper", "rmcv_batch_attitude", "rmcv_pipeline_submit_tracked_serial",
    "rmcv_frame_camera", "rmcv_pnp_load_cameras", "rmcv_batch_set_frame_cameras", "rmcv_batch_set_device_frame_cameras", "rmcv_batch_get_frame_cameras",
    "rmcv_pipeline_set_frame_cameras", "rmcv_tracker_set_stream_cameras", "rmcv_tracker_set_aim_configs",
    "rmcv_batch_debug_views", "rmcv_batch_get_debug_view", "rmcv_debug_view", "rmcv_debug_view_host", "rmcv_pipeline_set_views", "rmcv_pipeline_views",
    "rmcv_pack_bound", "rmcv_pack_host", "rmcv_unpack_host", "rmcv_pack_frames", "rmcv_unpack_frames",
    "rmcv_default_recorder_config", "rmcv_recorder_create", "rmcv_recorder_destroy", "rmcv_recorder_last_error", "rmcv_recorder_set_user", "rmcv_recorder_record",
    "rmcv_recorder_freeze", "rmcv_recorder_resume", "rmcv_recorder_count", "rmcv_recorder_entry", "rmcv_recorder_frame", "rmcv_recorder_device_frame",
    "rmcv_recorder_save", "rmcv_session_append", "rmcv_session_open", "rmcv_session_count", "rmcv_session_entry", "rmcv_session_frame", "rmcv_session_close",
    "rmcv_pipeline_set_recorder",
    "rmcv_loop_bound", "rmcv_loop_trigger_host", "rmcv_recorder_set_trigger", "rmcv_recorder_trigger", "rmcv_recorder_loop", "rmcv_session_loop", "rmcv_session_append_loop",
    "rmcv_tracker_restore", "rmcv_tracker_config_from_loop", "rmcv_tracker_aim_config_from_loop", "rmcv_tracker_attitude_config_from_loop",
    "rmcv_svm_train_defaults", "rmcv_svm_train", "rmcv_svm_train_host", "rmcv_svm_gram", "rmcv_svm_gram_host", "rmcv_svm_predict", "rmcv_svm_predict_host",
    "rmcv_dataset_create", "rmcv_dataset_destroy", "rmcv_dataset_clear", "rmcv_dataset_last_error", "rmcv_dataset_count", "rmcv_dataset_get", "rmcv_dataset_device",
    "rmcv_batch_harvest", "rmcv_batch_harvest_device", "rmcv_harvest_plan_host", "rmcv_pipeline_set_harvest", "rmcv_svm_train_dataset", "rmcv_svm_predict_dataset",
    "rmcv_icon_sad", "rmcv_dataset_set_novelty", "rmcv_dataset_novelty", "rmcv_dataset_get_rings", "rmcv_dataset_append_rows", "rmcv_harvest_novel_host",
    "rmcv_frame_model", "rmcv_svm_load_models", "rmcv_batch_set_frame_models", "rmcv_batch_set_device_frame_models", "rmcv_batch_get_frame_models",
    "rmcv_pipeline_set_frame_models", "rmcv_svm_predict_model",
    "rmcv_batch_source_views", "rmcv_batch_get_source_view", "rmcv_source_view", "rmcv_source_view_host", "rmcv_pipeline_set_source_views",
    "rmcv_format_f6", "rmcv_label_text", "rmcv_track_label_text", "rmcv_view_glyph", "rmcv_view_labels_host", "rmcv_view_labels", "rmcv_batch_view_labels",
    "rmcv_batch_view_tracks", "rmcv_pipeline_set_view_labels", "rmcv_view_text_launches",
    "rmcv_affine_correction_host", "rmcv_icon_strip", "rmcv_icon_strip_host", "rmcv_batch_icon_strips", "rmcv_batch_get_icon_strip", "rmcv_sheet_size",
    "rmcv_batch_labeler_sheets", "rmcv_batch_get_labeler_sheet", "rmcv_labeler_sheet_host", "rmcv_pipeline_set_sheets",
    "rmcv_corner_mask", "rmcv_gray_host", "rmcv_corner_subpix_host", "rmcv_corner_subpix", "rmcv_batch_refine_corners", "rmcv_batch_get_refined_corners",
    "rmcv_chess_defaults", "rmcv_find_chessboard_host", "rmcv_find_chessboard", "rmcv_batch_find_chessboards", "rmcv_batch_get_chessboard",
    "rmcv_calib_defaults", "rmcv_calibrate_camera_host", "rmcv_calibrate_cameras", "rmcv_calibrate_camera", "rmcv_calib_to_pnp_config",
    "rmcv_handeye_defaults", "rmcv_calibrate_hand_eye_host", "rmcv_calibrate_hand_eyes", "rmcv_calibrate_hand_eye", "rmcv_handeye_to_pnp_config",
    "rmcv_handeye_to_attitude_config",
]


class Params(C.Structure):
    """rmcv_params; defaults are the literals of the reference's executable/main.cpp:172-176"""
    _fields_ = [("camp", C.c_int32), ("lower_bound", C.c_int32), ("morph", C.c_int32), ("tilt_max", C.c_float),
                ("ratio_lo", C.c_float), ("ratio_hi", C.c_float), ("area_lo", C.c_double), ("area_hi", C.c_double),
                ("angle_diff_max", C.c_float), ("shear_max", C.c_float), ("length_ratio_max", C.c_float),
                ("_pad", C.c_int32)]


class LegacyParams(C.Structure):
    """rmcv_legacy_params: the float arguments of rm::MatchLightBlob / rm::FindLightBlobs (include/objdetect.h:22-37)"""
    _fields_ = [("min_ratio", C.c_float), ("max_ratio", C.c_float), ("tilt_angle", C.c_float), ("min_area", C.c_float),
                ("max_area", C.c_float), ("fit_ellipse", C.c_int32)]


class PnpConfig(C.Structure):
    """rmcv_pnp_config: cammat / discof / h_gripper2camera / exactSize of the reference's executable/main.cpp:7-19, 184"""
    _fields_ = [("camera_matrix", C.c_double * 9), ("dist", C.c_double * 5), ("gripper2camera", C.c_double * 16),
                ("square_w", C.c_float), ("square_h", C.c_float)]


class Limits(C.Structure):
    _fields_ = [("max_frames", C.c_int32), ("max_width", C.c_int32), ("max_height", C.c_int32),
                ("max_contours", C.c_int32), ("max_points", C.c_int32), ("max_blobs", C.c_int32),
                ("max_armours", C.c_int32), ("_pad", C.c_int32)]


class PipelineConfig(C.Structure):
    """rmcv_pipeline_config (0 in a field = the default)"""
    _fields_ = [("depth", C.c_int32), ("pixel_streams", C.c_int32), ("sparse_streams", C.c_int32), ("armour_cap", C.c_int32),
                ("sparse_waves", C.c_int32), ("pixel_groups", C.c_int32), ("host_results", C.c_int32), ("dense_streams", C.c_int32),
                ("hot_contexts", C.c_int32), ("_reserved", C.c_int32)]


class PipelineInfo(C.Structure):
    """rmcv_pipeline_info"""
    _fields_ = [("depth", C.c_int32), ("pixel_streams", C.c_int32), ("sparse_streams", C.c_int32), ("armour_cap", C.c_int32),
                ("sparse_waves", C.c_int32), ("pixel_groups", C.c_int32), ("host_results", C.c_int32), ("dense_streams", C.c_int32),
                ("max_frames", C.c_int32), ("hw_queues_env", C.c_int32), ("hw_queues_wanted", C.c_int32), ("_pad", C.c_int32),
                ("record_bytes", C.c_int64), ("armours_offset", C.c_int64), ("submitted", C.c_uint64), ("collected", C.c_uint64),
                ("dense_split", C.c_uint64), ("hot_batches", C.c_uint64), ("hot_contexts", C.c_int32), ("_pad2", C.c_int32), ("latency_batches", C.c_uint64),
                ("host_blocking_calls", C.c_uint64), ("wait_timeout_ms", C.c_int32), ("_pad3", C.c_int32), ("max_submit_us", C.c_double), ("heavy_batches", C.c_uint64), ("held_back", C.c_uint64)]


SVM_MAX_GRID, SVM_MAX_DF, SVM_MAX_FOLDS, SVM_MAX_SAMPLES, SVM_MAX_PAIR_SAMPLES = 16, 28, 64, 8192, 2048


class SvmTrainParams(C.Structure):
    """rmcv_svm_train_params (defaults: rmcv_svm_train_defaults = optimizer.cpp's criteria and cv::ml::SVM's default C grid)"""
    _fields_ = [("eps", C.c_double), ("max_iter", C.c_int32), ("k_fold", C.c_int32), ("n_c", C.c_int32), ("reserved", C.c_int32),
                ("c_grid", C.c_double * SVM_MAX_GRID)]


class SvmTrainReport(C.Structure):
    """rmcv_svm_train_report"""
    _fields_ = [("best_c", C.c_double), ("best_index", C.c_int32), ("n_df", C.c_int32), ("cv_errors", C.c_int32 * SVM_MAX_GRID),
                ("iterations", C.c_int32 * SVM_MAX_DF), ("converged", C.c_int32 * SVM_MAX_DF), ("objective", C.c_double * SVM_MAX_DF),
                ("phase_ms", C.c_double * 6), ("alpha_out", C.c_void_p), ("message", C.c_char * 128)]


assert C.sizeof(SvmTrainParams) == 152 and C.sizeof(SvmTrainReport) == 712

RECORDER_MAX_FRAMES = 64


class RecorderConfig(C.Structure):
    """rmcv_recorder_config (0 in a field = the default)"""
    _fields_ = [("slots", C.c_int32), ("max_frames", C.c_int32), ("max_w_bytes", C.c_int32), ("max_h", C.c_int32), ("user_bytes", C.c_int32),
                ("track_cap", C.c_int32)]


class RecordEntry(C.Structure):
    """rmcv_record_entry: what the host knew of a recorded batch at its submit, plus the packed sizes, keys and origins the device reported"""
    _fields_ = [("ticket", C.c_uint64), ("sequence", C.c_uint64), ("timestamp", C.c_int64), ("n_frames", C.c_int32), ("batch_frames", C.c_int32),
                ("w", C.c_int32), ("h", C.c_int32), ("w_bytes", C.c_int32), ("stride", C.c_int32), ("lag", C.c_int32), ("input_format", C.c_int32),
                ("sample_bits", C.c_int32), ("valid_bit", C.c_int32), ("orient", C.c_int32), ("stages", C.c_int32), ("win_w", C.c_int32), ("win_h", C.c_int32),
                ("has_keys", C.c_int32), ("has_origins", C.c_int32), ("user_bytes", C.c_int32), ("loop_bytes", C.c_int32), ("params", Params),
                ("frames", C.c_int32 * RECORDER_MAX_FRAMES), ("sizes", C.c_int64 * RECORDER_MAX_FRAMES), ("keys", (C.c_int32 * 4) * RECORDER_MAX_FRAMES),
                ("camps", C.c_int32 * RECORDER_MAX_FRAMES),
                ("origins", (C.c_int32 * 2) * RECORDER_MAX_FRAMES)]


assert C.sizeof(RecordEntry) == 2712

# ---- the recorder's loop records (include/rmcv_abi.h: rmcv_loop_state, rmcv_trigger_config)
LOOP_TRUNCATED = 1
(TRIG_NO_ARMOURS, TRIG_TRACK_DROPPED, TRIG_TRACKER_OVF, TRIG_FRAME_STATUS, TRIG_TARGET_LOST, TRIG_TARGET_SWITCH, TRIG_NO_SOLUTION, TRIG_AIM_JUMP,
 TRIG_PACKET_ERROR) = (1 << b for b in range(9))
TRIG_ALL = 511


class _Aim(C.Structure):
    """rmcv_aim"""
    _fields_ = [("track", C.c_int32), ("identity", C.c_int32), ("lost_count", C.c_int32), ("status", C.c_int32), ("pitch", C.c_double), ("yaw", C.c_double),
                ("flight_time", C.c_double), ("distance", C.c_double), ("point", C.c_double * 3)]


class _AimInput(C.Structure):
    """rmcv_aim_input"""
    _fields_ = [("world2camera", C.c_double * 16), ("motor_angle", C.c_double)]


class _Attitude(C.Structure):
    """rmcv_attitude"""
    _fields_ = [("roll", C.c_double), ("pitch", C.c_double), ("yaw", C.c_double)]


class _TrackerConfig(C.Structure):
    """rmcv_tracker_config (tracker.TrackerConfig is the same layout)"""
    _fields_ = [("n_streams", C.c_int32), ("track_cap", C.c_int32), ("process_noise", C.c_double), ("measurement_noise", C.c_double),
                ("error", C.c_double), ("tick_frequency", C.c_double), ("roi_scale_w", C.c_float), ("roi_scale_h", C.c_float),
                ("frame_w", C.c_int32), ("frame_h", C.c_int32), ("win_w", C.c_int32), ("win_h", C.c_int32)]


class _AimConfig(C.Structure):
    """rmcv_aim_config (tracker.AimConfig is the same layout)"""
    _fields_ = [("g", C.c_double), ("v0", C.c_double), ("height", C.c_double), ("offset_x", C.c_float), ("offset_y", C.c_float),
                ("angle_offset", C.c_double), ("latency_s", C.c_double), ("mode", C.c_int32), ("height_mode", C.c_int32), ("source", C.c_int32),
                ("pick", C.c_int32), ("lead_iterations", C.c_int32), ("max_lost", C.c_int32), ("overloads", C.c_int32), ("identity_mask", C.c_uint32)]


class _AttitudeConfig(C.Structure):
    """rmcv_attitude_config (tracker.AttitudeConfig is the same layout)"""
    _fields_ = [("gripper2camera", C.c_double * 16), ("motor_angle_mode", C.c_int32), ("reserved", C.c_int32)]


class LoopState(C.Structure):
    """rmcv_loop_state: the fixed part of a loop record"""
    _fields_ = [("stream", C.c_int32), ("n_tracking", C.c_int32), ("status", C.c_int32), ("n_armours", C.c_int32),
                ("origin_next", C.c_int32 * 2), ("origin_eff", C.c_int32 * 2), ("frame_status", C.c_int32), ("has_camps", C.c_int32),
                ("camp", C.c_int32), ("lower_bound", C.c_int32), ("has_key", C.c_int32), ("key", C.c_int32 * 4), ("has_cameras", C.c_int32),
                ("cam_eff", C.c_int32), ("has_aim", C.c_int32), ("has_attitude", C.c_int32), ("has_packet", C.c_int32), ("packet_errors", C.c_int32),
                ("n_tracks", C.c_int32), ("flags", C.c_int32), ("fired", C.c_uint32), ("has_prev", C.c_int32), ("trig_frame_status_mask", C.c_int32),
                ("trig_aim_jump_deg", C.c_double), ("timestamp", C.c_int64), ("sequence", C.c_uint64), ("aim", _Aim), ("aim_input", _AimInput), ("attitude", _Attitude),
                ("packet", C.c_uint8 * 24), ("tracker_config", _TrackerConfig), ("aim_config", _AimConfig), ("attitude_config", _AttitudeConfig),
                ("gripper2camera", C.c_double * 16)]


class TriggerConfig(C.Structure):
    """rmcv_trigger_config"""
    _fields_ = [("mask", C.c_uint32), ("post_batches", C.c_int32), ("frame_status_mask", C.c_int32), ("reserved", C.c_int32), ("aim_jump_deg", C.c_double)]


class TriggerInfo(C.Structure):
    """rmcv_trigger_info"""
    _fields_ = [("fired", C.c_int32), ("mask", C.c_uint32), ("sequence", C.c_uint64), ("k", C.c_int32), ("stream", C.c_int32), ("noticed", C.c_int32),
                ("batches_since", C.c_int32)]


LOOP_SIDE_BYTES = 32
assert C.sizeof(TriggerConfig) == 24 and C.sizeof(TriggerInfo) == 32 and C.sizeof(LoopState) % 8 == 0


# rmcv_pipeline_hook: int (*)(void* user, uint64_t ticket, void* d_record, int64_t record_bytes, void* hip_stream, void** done_event)
PIPELINE_HOOK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_void_p))


class RmcvError(RuntimeError):
    def __init__(self, code, msg=""):
        super().__init__("rmcv error %d: %s" % (code, msg))
        self.code = code


_lib = None


def load(path):
    """a configured handle of one build of the library (not installed as THE library: see use)"""
    if not os.path.exists(path):
        raise ImportError("%s is missing: run `make -C rmcv_amd/csrc` (or __graft_entry__.build())" % path)
    L = C.CDLL(path)
    L.rmcv_last_error.restype = C.c_char_p
    L.rmcv_last_error.argtypes = [C.c_void_p]
    L.rmcv_synth_checksum.restype = C.c_uint64
    L.rmcv_ctx_destroy.restype = None
    L.rmcv_ctx_destroy.argtypes = [C.c_void_p]
    L.rmcv_pipeline_last_error.restype = C.c_char_p
    L.rmcv_pipeline_last_error.argtypes = [C.c_void_p]
    L.rmcv_pipeline_destroy.restype = None
    L.rmcv_pipeline_destroy.argtypes = [C.c_void_p]
    L.rmcv_pipeline_context.restype = C.c_void_p
    L.rmcv_pipeline_context.argtypes = [C.c_void_p, C.c_int]
    L.rmcv_pipeline_set_hot_contexts.restype = C.c_int
    L.rmcv_pipeline_set_hot_contexts.argtypes = [C.c_void_p, C.c_int]
    L.rmcv_pipeline_set_wait_timeout.restype = C.c_int
    L.rmcv_pipeline_set_wait_timeout.argtypes = [C.c_void_p, C.c_int]
    L.rmcv_pixel_ws_launches.restype = C.c_int64
    L.rmcv_pixel_ws_launches.argtypes = []
    if hasattr(L, "rmcv_pixel_image_delta_launches"):   # (another build loaded for an A/B may predate it; build() checks THE library's exports)
        L.rmcv_pixel_image_delta_launches.restype = C.c_int64
        L.rmcv_pixel_image_delta_launches.argtypes = []
    if hasattr(L, "rmcv_pixel_plane_delta_launches"):
        L.rmcv_pixel_plane_delta_launches.restype = C.c_int64
        L.rmcv_pixel_plane_delta_launches.argtypes = []
    L.rmcv_pipeline_context_of.restype = C.c_void_p
    L.rmcv_pipeline_context_of.argtypes = [C.c_void_p, C.c_uint64]
    # the call of the timed region: fixed argument types, so that ctypes converts without looking at the Python objects' types
    L.rmcv_pipeline_submit.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_void_p]
    L.rmcv_pipeline_submit_legacy.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.rmcv_pipeline_wait.argtypes = [C.c_void_p, C.c_uint64]
    L.rmcv_pipeline_collect.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.rmcv_pipeline_record.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    L.rmcv_pipeline_gathered.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    L.rmcv_pipeline_set_gather.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    if hasattr(L, "rmcv_demosaic"):  # (builds from before raw Bayer input stay loadable for A/B runs)
        L.rmcv_demosaic.restype = C.c_int
        L.rmcv_demosaic.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    if hasattr(L, "rmcv_demosaic_raw"):
        L.rmcv_demosaic_raw.restype = C.c_int
        L.rmcv_demosaic_raw.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    if hasattr(L, "rmcv_auto_enhance"):  # (builds from before RMCV_OPT_ENHANCE stay loadable for A/B runs)
        L.rmcv_ctx_set_enhance_gains.argtypes = [C.c_void_p, C.c_float, C.c_float]
        L.rmcv_ctx_get_enhance.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rmcv_gamma_lut.argtypes = [C.c_float, C.c_void_p]
        L.rmcv_enhance_gamma.argtypes = [C.c_void_p, C.c_int64, C.c_float, C.c_float, C.c_void_p]
        L.rmcv_calc_gamma.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_int]
        L.rmcv_auto_enhance.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_int, C.c_void_p]
        L.rmcv_batch_get_gammas.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    if hasattr(L, "rmcv_get_roi"):  # (builds from before windowed detection stay loadable for A/B runs)
        L.rmcv_batch_set_windows.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.rmcv_batch_set_device_windows.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.rmcv_batch_get_windows.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.rmcv_batch_device_windows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rmcv_pipeline_submit_windows.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_int,
                                                   C.c_void_p, C.c_int, C.c_void_p]
        L.rmcv_get_roi.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.rmcv_window_origin.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.rmcv_armours_to_frame.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    if hasattr(L, "rmcv_tracker_create"):  # (builds from before the device tracker stay loadable for A/B runs)
        L.rmcv_default_tracker_config.restype = None
        L.rmcv_default_tracker_config.argtypes = [C.c_void_p]
        L.rmcv_tracker_create.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
        L.rmcv_tracker_destroy.restype = None
        L.rmcv_tracker_destroy.argtypes = [C.c_void_p]
        L.rmcv_tracker_last_error.restype = C.c_char_p
        L.rmcv_tracker_last_error.argtypes = [C.c_void_p]
        L.rmcv_tracker_reset.argtypes = [C.c_void_p]
        L.rmcv_tracker_set_origins.argtypes = [C.c_void_p, C.c_void_p]
        L.rmcv_tracker_device_origins.argtypes = [C.c_void_p, C.c_void_p]
        L.rmcv_batch_track.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        L.rmcv_tracker_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.rmcv_tracker_get.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rmcv_tracker_step_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                             C.c_int, C.c_int, C.c_int64]
        L.rmcv_pipeline_submit_tracked.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_int64, C.c_void_p]
    if hasattr(L, "rmcv_aim_step_host"):  # (builds from before device-resident aiming stay loadable for A/B runs)
        L.rmcv_projectile_angle.restype = C.c_double
        L.rmcv_projectile_angle.argtypes = [C.c_double, C.c_double, C.c_double, C.c_double]
        L.rmcv_solve_gea.restype = C.c_double
        L.rmcv_solve_gea.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_float, C.c_float, C.c_double, C.c_int, C.c_void_p]
        L.rmcv_delta_height.restype = C.c_double
        L.rmcv_delta_height.argtypes = [C.c_void_p, C.c_double, C.c_float, C.c_double]
        L.rmcv_distance.restype = C.c_double
        L.rmcv_distance.argtypes = [C.c_void_p]
        L.rmcv_rigid_inverse.argtypes = [C.c_void_p, C.c_void_p]
        L.rmcv_default_aim_config.restype = None
        L.rmcv_default_aim_config.argtypes = [C.c_void_p]
        L.rmcv_tracker_set_aim.argtypes = [C.c_void_p, C.c_void_p]
        L.rmcv_tracker_set_aim_inputs.argtypes = [C.c_void_p, C.c_void_p]
        L.rmcv_tracker_device_aim_inputs.argtypes = [C.c_void_p, C.c_void_p]
        L.rmcv_tracker_aim.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        L.rmcv_tracker_get_aims.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.rmcv_tracker_device_aims.argtypes = [C.c_void_p, C.c_void_p]
        L.rmcv_tracker_put.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.rmcv_aim_step_host.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
    if hasattr(L, "rmcv_frame_key"):  # (builds from before per-frame detection keys stay loadable for A/B runs)
        L.rmcv_frame_key.argtypes = [C.c_int32, C.c_int32, C.c_void_p]
        L.rmcv_batch_set_frame_camps.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.rmcv_batch_set_device_frame_camps.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.rmcv_batch_get_frame_keys.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.rmcv_pipeline_submit_camps.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.rmcv_tracker_set_camps.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.rmcv_tracker_device_camps.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(L, "rmcv_attitude_step_host"):  # (builds from before the per-stream gimbal attitude stay loadable for A/B runs)
        L.rmcv_euler_to_matrix.argtypes = [C.c_void_p, C.c_void_p]
        L.rmcv_homogeneous.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.rmcv_crc8.restype = C.c_uint8
        L.rmcv_crc8.argtypes = [C.c_void_p, C.c_int]
        L.rmcv_serial_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.rmcv_serial_encode.argtypes = [C.c_int32, C.c_float, C.c_float, C.c_float, C.c_void_p]
        L.rmcv_attitude_step_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rmcv_default_attitude_config.restype = None
        L.rmcv_default_attitude_config.argtypes = [C.c_void_p]
        L.rmcv_tracker_set_attitude.argtypes = [C.c_void_p, C.c_void_p]
        L.rmcv_tracker_set_attitudes.argtypes = [C.c_void_p, C.c_void_p]
        L.rmcv_tracker_get_attitudes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.rmcv_tracker_device_attitudes.argtypes = [C.c_void_p, C.c_void_p]
        L.rmcv_tracker_get_aim_inputs.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.rmcv_batch_get_base2gripper.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.rmcv_batch_attitude.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rmcv_pipeline_submit_tracked_serial.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p,
                                                          C.c_int, C.c_int64, C.c_void_p]
    if hasattr(L, "rmcv_frame_camera"):  # (builds from before the per-stream camera tables stay loadable for A/B runs)
        L.rmcv_frame_camera.argtypes = [C.c_int32, C.c_int32]
        L.rmcv_pnp_load_cameras.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.rmcv_batch_set_frame_cameras.argtypes = [C.c_void_p, C.c_void_p]
        L.rmcv_batch_set_device_frame_cameras.argtypes = [C.c_void_p, C.c_void_p]
        L.rmcv_batch_get_frame_cameras.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.rmcv_pipeline_set_frame_cameras.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.rmcv_tracker_set_stream_cameras.argtypes = [C.c_void_p, C.c_void_p]
        L.rmcv_tracker_set_aim_configs.argtypes = [C.c_void_p, C.c_void_p]
    if hasattr(L, "rmcv_debug_view_host"):  # (builds from before the debug view stay loadable for A/B runs)
        view = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                C.c_void_p, C.c_int]
        L.rmcv_debug_view_host.argtypes = view
        L.rmcv_debug_view.argtypes = [C.c_void_p] + view
        L.rmcv_batch_debug_views.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_void_p]
        L.rmcv_batch_get_debug_view.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
        L.rmcv_pipeline_set_views.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        L.rmcv_pipeline_views.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        if hasattr(L, "rmcv_source_view_host"):  # (the source view, DESIGN.md 4p: the same argument shapes)
            L.rmcv_source_view_host.argtypes = view
            L.rmcv_source_view.argtypes = [C.c_void_p] + view
            L.rmcv_batch_source_views.argtypes = L.rmcv_batch_debug_views.argtypes
            L.rmcv_batch_get_source_view.argtypes = L.rmcv_batch_get_debug_view.argtypes
            L.rmcv_pipeline_set_source_views.argtypes = L.rmcv_pipeline_set_views.argtypes
    if hasattr(L, "rmcv_view_labels_host"):  # (builds from before the view labels stay loadable for A/B runs)
        labels = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                  C.c_int, C.c_int]
        L.rmcv_format_f6.argtypes = [C.c_double, C.c_void_p, C.c_int]
        L.rmcv_label_text.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int]
        L.rmcv_track_label_text.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.rmcv_view_glyph.argtypes = [C.c_int, C.c_void_p]
        L.rmcv_view_labels_host.argtypes = labels
        L.rmcv_view_labels.argtypes = [C.c_void_p] + labels
        L.rmcv_batch_view_labels.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_void_p]
        L.rmcv_batch_view_tracks.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_void_p]
        L.rmcv_pipeline_set_view_labels.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.rmcv_view_text_launches.restype = C.c_int64
        L.rmcv_view_text_launches.argtypes = []
    if hasattr(L, "rmcv_corner_subpix_host"):  # (builds from before the corner refinement stay loadable for A/B runs)
        rule = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p]  # win_x, win_y, zero_x, zero_y, max_iters, eps, status
        L.rmcv_corner_mask.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.rmcv_gray_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
        L.rmcv_corner_subpix_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int] + rule
        L.rmcv_corner_subpix.argtypes = [C.c_void_p] + L.rmcv_corner_subpix_host.argtypes
        L.rmcv_batch_refine_corners.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p] + rule + [C.c_void_p]
        L.rmcv_batch_get_refined_corners.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int] + rule
    if hasattr(L, "rmcv_find_chessboard_host"):  # (builds from before the chessboard detector stay loadable for A/B runs)
        out = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]  # corners, status, candidates, candidate count
        L.rmcv_chess_defaults.restype = None
        L.rmcv_chess_defaults.argtypes = [C.c_void_p]
        L.rmcv_find_chessboard_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p] + out
        L.rmcv_find_chessboard.argtypes = [C.c_void_p] + L.rmcv_find_chessboard_host.argtypes
        L.rmcv_batch_find_chessboards.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rmcv_batch_get_chessboard.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p] + out
    if hasattr(L, "rmcv_calibrate_camera_host"):  # (builds from before the calibration solve stay loadable for A/B runs)
        tail = [C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]  # cols, rows, square, w, h, params, guess(es), result(s), views
        L.rmcv_calib_defaults.restype = None
        L.rmcv_calib_defaults.argtypes = [C.c_void_p]
        L.rmcv_calibrate_camera_host.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int] + tail
        L.rmcv_calibrate_camera.argtypes = [C.c_void_p] + L.rmcv_calibrate_camera_host.argtypes
        L.rmcv_calibrate_cameras.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int] + tail + [C.c_void_p]
        L.rmcv_calib_to_pnp_config.argtypes = [C.c_void_p, C.c_void_p]
    if hasattr(L, "rmcv_calibrate_hand_eye_host"):  # (builds from before the hand-eye solve stay loadable for A/B runs)
        L.rmcv_handeye_defaults.restype = None
        L.rmcv_handeye_defaults.argtypes = [C.c_void_p]
        L.rmcv_calibrate_hand_eye_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rmcv_calibrate_hand_eye.argtypes = [C.c_void_p] + L.rmcv_calibrate_hand_eye_host.argtypes
        L.rmcv_calibrate_hand_eyes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rmcv_handeye_to_pnp_config.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.rmcv_handeye_to_attitude_config.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    if hasattr(L, "rmcv_icon_strip_host"):  # (builds from before the icon strip stay loadable for A/B runs)
        strip = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
        L.rmcv_affine_correction_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.rmcv_icon_strip_host.argtypes = strip
        L.rmcv_icon_strip.argtypes = [C.c_void_p] + strip
        L.rmcv_batch_icon_strips.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p]
        L.rmcv_batch_get_icon_strip.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.rmcv_sheet_size.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.rmcv_batch_labeler_sheets.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_void_p]
        L.rmcv_batch_get_labeler_sheet.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
        L.rmcv_labeler_sheet_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                              C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
        L.rmcv_pipeline_set_sheets.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    if hasattr(L, "rmcv_pack_bound"):  # (builds from before the session recorder stay loadable for A/B runs)
        L.rmcv_pack_bound.restype = C.c_int64
        L.rmcv_pack_bound.argtypes = [C.c_int, C.c_int]
        L.rmcv_pack_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
        L.rmcv_unpack_host.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64]
        L.rmcv_pack_frames.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.rmcv_unpack_frames.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_void_p]
        L.rmcv_default_recorder_config.restype = None
        L.rmcv_default_recorder_config.argtypes = [C.c_void_p]
        L.rmcv_recorder_create.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
        L.rmcv_recorder_destroy.restype = None
        L.rmcv_recorder_destroy.argtypes = [C.c_void_p]
        L.rmcv_recorder_last_error.restype = C.c_char_p
        L.rmcv_recorder_last_error.argtypes = [C.c_void_p]
        L.rmcv_recorder_set_user.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.rmcv_recorder_record.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.rmcv_recorder_freeze.argtypes = [C.c_void_p]
        L.rmcv_recorder_resume.argtypes = [C.c_void_p]
        L.rmcv_recorder_count.argtypes = [C.c_void_p, C.c_void_p]
        L.rmcv_recorder_entry.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        L.rmcv_recorder_frame.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
        L.rmcv_recorder_device_frame.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.rmcv_recorder_save.argtypes = [C.c_void_p, C.c_char_p]
        L.rmcv_session_append.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rmcv_session_open.argtypes = [C.c_char_p, C.c_void_p]
        L.rmcv_session_count.argtypes = [C.c_void_p, C.c_void_p]
        L.rmcv_session_entry.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        L.rmcv_session_frame.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
        L.rmcv_session_close.restype = None
        L.rmcv_session_close.argtypes = [C.c_void_p]
        L.rmcv_pipeline_set_recorder.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    if hasattr(L, "rmcv_loop_bound"):  # (builds from before the recorder's loop records stay loadable for A/B runs)
        L.rmcv_loop_bound.restype = C.c_int64
        L.rmcv_loop_bound.argtypes = [C.c_int]
        L.rmcv_loop_trigger_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rmcv_recorder_set_trigger.argtypes = [C.c_void_p, C.c_void_p]
        L.rmcv_recorder_trigger.argtypes = [C.c_void_p, C.c_void_p]
        L.rmcv_recorder_loop.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
        L.rmcv_session_loop.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
        L.rmcv_session_append_loop.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rmcv_tracker_restore.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.rmcv_tracker_config_from_loop.argtypes = [C.c_void_p, C.c_void_p]
        L.rmcv_tracker_aim_config_from_loop.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.rmcv_tracker_attitude_config_from_loop.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(L, "rmcv_svm_train_host"):  # (builds from before the classifier's trainer stay loadable for A/B runs)
        train = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rmcv_svm_train_defaults.restype = None
        L.rmcv_svm_train_defaults.argtypes = [C.c_void_p]
        L.rmcv_svm_train_host.argtypes = train
        L.rmcv_svm_train.argtypes = [C.c_void_p] + train
        L.rmcv_svm_gram_host.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.rmcv_svm_gram.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.rmcv_svm_predict_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.rmcv_svm_predict.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    if hasattr(L, "rmcv_dataset_create"):  # (builds from before the dataset harvest stay loadable for A/B runs)
        L.rmcv_dataset_create.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.rmcv_dataset_destroy.restype = None
        L.rmcv_dataset_destroy.argtypes = [C.c_void_p]
        L.rmcv_dataset_clear.argtypes = [C.c_void_p]
        L.rmcv_dataset_last_error.restype = C.c_char_p
        L.rmcv_dataset_last_error.argtypes = [C.c_void_p]
        L.rmcv_dataset_count.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.rmcv_dataset_get.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.rmcv_dataset_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rmcv_batch_harvest.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p]
        L.rmcv_batch_harvest_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p]
        L.rmcv_harvest_plan_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int32, C.c_int32, C.c_int64, C.c_void_p,
                                             C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rmcv_pipeline_set_harvest.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.rmcv_svm_train_dataset.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rmcv_svm_predict_dataset.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    if hasattr(L, "rmcv_dataset_set_novelty"):  # (builds from before the harvest's novelty rings stay loadable for A/B runs)
        L.rmcv_icon_sad.restype = C.c_int32
        L.rmcv_icon_sad.argtypes = [C.c_void_p, C.c_void_p]
        L.rmcv_dataset_set_novelty.argtypes = [C.c_void_p, C.c_int, C.c_int32]
        L.rmcv_dataset_novelty.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rmcv_dataset_get_rings.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.rmcv_dataset_append_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64]
        L.rmcv_harvest_novel_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p]
    if hasattr(L, "rmcv_frame_model"):  # (builds from before the per-stream model tables stay loadable for A/B runs)
        L.rmcv_frame_model.argtypes = [C.c_int32, C.c_int32]
        L.rmcv_svm_load_models.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.rmcv_batch_set_frame_models.argtypes = [C.c_void_p, C.c_void_p]
        L.rmcv_batch_set_device_frame_models.argtypes = [C.c_void_p, C.c_void_p]
        L.rmcv_batch_get_frame_models.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.rmcv_pipeline_set_frame_models.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.rmcv_svm_predict_model.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    L.rmcv_device_free.restype = None
    L.rmcv_device_free.argtypes = [C.c_int, C.c_void_p]
    return L


def lib():
    """load librmcv_hip.so; raises (never falls back) when it has not been built"""
    global _lib
    if _lib is None:
        _lib = load(LIB_PATH)
    return _lib


def use(L):
    """dev tool (bench.py RMCV_BENCH_AB=lib:...): make another build THE library for the calls that follow; returns the previous one.
    Contexts belong to the build that made them: switch back before touching them."""
    global _lib
    prev, _lib = lib(), L
    return prev


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def gamma_lut(gamma):
    """rm::CalcGamma's 256-entry table of `gamma` (rmcv_gamma_lut: host-side, the table builder the device runs too)"""
    out = np.empty(256, np.uint8)
    rc = lib().rmcv_gamma_lut(C.c_float(gamma), ptr(out))
    if rc:
        raise RmcvError(rc, "rmcv_gamma_lut: gamma must be finite and not negative")
    return out


def enhance_gamma(sums_bgr, n_pixels, max_gain=ENHANCE_MAX_GAIN, min_gain=ENHANCE_MIN_GAIN):
    """the gamma rm::AutoEnhance derives from a frame's exact channel sums (rmcv_enhance_gamma: host-side)"""
    s = np.ascontiguousarray(sums_bgr, np.uint64)
    assert s.shape == (3,)
    g = C.c_float(0)
    rc = lib().rmcv_enhance_gamma(ptr(s), C.c_int64(int(n_pixels)), C.c_float(max_gain), C.c_float(min_gain), C.byref(g))
    if rc:
        raise RmcvError(rc, "rmcv_enhance_gamma: the gains must be finite and differ, n_pixels >= 1")
    return np.float32(g.value)


def get_roi(points, scale=1.0, frame_size=(-1, -1), previous=(0, 0, 0, 0)):
    """rm::utils::GetROI (rmcv_get_roi: host-side, verbatim -- the height grows by the WIDTH's margin, as the reference writes it):
    points (n, 2) float32, scale a float or (scale_w, scale_h), frame_size (w, h), previous (x, y, w, h) -> (x, y, w, h)"""
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 2)
    sw, sh = (scale, scale) if np.isscalar(scale) else scale
    prev = np.ascontiguousarray(previous, np.int32)
    assert prev.shape == (4,)
    out = np.zeros(4, np.int32)
    rc = lib().rmcv_get_roi(ptr(pts) if len(pts) else None, len(pts), C.c_float(sw), C.c_float(sh), int(frame_size[0]), int(frame_size[1]), ptr(prev), ptr(out))
    if rc:
        raise RmcvError(rc, "rmcv_get_roi")
    return tuple(int(v) for v in out)


def window_origin(rect, win_w, win_h):
    """the requested origin (x, y) of a win_w x win_h window centred on rect = (x, y, w, h) (rmcv_window_origin: integers; the library
    clamps it into the frame and snaps x down to a multiple of 16 when the window is used)"""
    r = np.ascontiguousarray(rect, np.int32)
    assert r.shape == (4,)
    out = np.zeros(2, np.int32)
    rc = lib().rmcv_window_origin(ptr(r), int(win_w), int(win_h), ptr(out))
    if rc:
        raise RmcvError(rc, "rmcv_window_origin: win_w, win_h >= 1")
    return int(out[0]), int(out[1])


def armours_to_frame(armours, x, y):
    """a copy of window-coordinate armours moved to frame coordinates: icon, vertices, bbox.x / .y + (float32(x), float32(y)), one f32 add each
    (rmcv_armours_to_frame; a convenience -- not what whole-frame detection would have found)"""
    a = np.ascontiguousarray(armours, ARMOUR).copy()
    rc = lib().rmcv_armours_to_frame(ptr(a) if len(a) else None, len(a), int(x), int(y))
    if rc:
        raise RmcvError(rc, "rmcv_armours_to_frame")
    return a


def frame_key(camp, lower_bound):
    """the effective detection key of raw (camp, lower_bound), any int32 (rmcv_frame_key: host-side, the function the device's prologue runs)
    -> (channel A, channel B, effective bound 1 .. 256, all-pass flag); a pixel is set where all-pass or bgr[A] - bgr[B] >= bound"""
    out = np.zeros(4, np.int32)
    rc = lib().rmcv_frame_key(C.c_int32(int(camp)), C.c_int32(int(lower_bound)), ptr(out))
    if rc:
        raise RmcvError(rc, "rmcv_frame_key")
    return tuple(int(v) for v in out)


def view_args(binary, blobs, negatives, armours, flags, size):
    """the argument list rmcv_debug_view and rmcv_debug_view_host share, and the arrays it points into (keep them until the call is through):
    binary (h, w) uint8; blobs LIGHTBLOB[]; negatives a list of (k, 2) int32 contours, or (POINT[], offs int32[n + 1]); armours ARMOUR[];
    size (vw, vh) -> (args, out (vh, vw, 3) uint8, keepalive)"""
    binary = np.ascontiguousarray(binary, np.uint8)
    h, w = binary.shape
    blobs = np.ascontiguousarray(blobs if blobs is not None else [], LIGHTBLOB).reshape(-1)
    armours = np.ascontiguousarray(armours if armours is not None else [], ARMOUR).reshape(-1)
    if isinstance(negatives, tuple):
        pts, offs = np.ascontiguousarray(negatives[0], POINT).reshape(-1), np.ascontiguousarray(negatives[1], np.int32).reshape(-1)
        assert len(offs) >= 1
    else:
        negatives = [np.ascontiguousarray(c, np.int32).reshape(-1, 2) for c in (negatives if negatives is not None else [])]
        pts = np.zeros(sum(len(c) for c in negatives), POINT)
        offs = np.zeros(len(negatives) + 1, np.int32)
        for i, c in enumerate(negatives):
            offs[i + 1] = offs[i] + len(c)
            pts["x"][offs[i]:offs[i + 1]], pts["y"][offs[i]:offs[i + 1]] = c[:, 0], c[:, 1]
    vw, vh = int(size[0]), int(size[1])
    out = np.zeros((max(vh, 0), max(vw, 0), 3), np.uint8)
    keep = (binary, blobs, armours, pts, offs)
    args = [ptr(binary), w, h, w, ptr(blobs) if len(blobs) else None, len(blobs), ptr(pts) if len(pts) else None, ptr(offs), len(offs) - 1,
            ptr(armours) if len(armours) else None, len(armours), int(flags), vw, vh, ptr(out), 3 * vw]
    return args, out, keep


def debug_view_host(binary, blobs=None, negatives=None, armours=None, size=(1024, 768), flags=VIEW_ALL):
    """the debug image of executable/main.cpp:200-207 at `size` = (vw, vh), on the CPU (rmcv_debug_view_host: the sequential restatement, no
    device): GRAY2BGR(binary), rm::debug::draw_lightblobs, rm::debug::draw_armours (no text), resized INTER_LINEAR -> (vh, vw, 3) uint8 BGR"""
    args, out, keep = view_args(binary, blobs, negatives, armours, flags, size)
    rc = lib().rmcv_debug_view_host(*args)
    if rc:
        raise RmcvError(rc, "rmcv_debug_view_host: sizes >= 1, known flags, contour offsets that do not decrease")
    return out


def source_view_args(bgr, blobs, negatives, armours, flags, size):
    """view_args for rmcv_source_view and rmcv_source_view_host: bgr (h, w, 3) uint8 in place of the binary, everything else the same"""
    bgr = np.ascontiguousarray(bgr, np.uint8)
    assert bgr.ndim == 3 and bgr.shape[2] == 3, "the source view takes an (h, w, 3) BGR image"
    args, out, keep = view_args(np.zeros(bgr.shape[:2], np.uint8), blobs, negatives, armours, flags, size)
    args[0], args[3] = ptr(bgr), 3 * bgr.shape[1]
    return args, out, keep + (bgr,)


def source_view_host(bgr, blobs=None, negatives=None, armours=None, size=(1024, 768), flags=VIEW_ALL):
    """the labeler's picture (executable/svm/labeler.cpp:108-111) at `size` = (vw, vh), on the CPU (rmcv_source_view_host: the sequential
    restatement, no device): the BGR image with rm::debug::draw_lightblobs and rm::debug::draw_armours (no text) over it, resized
    INTER_LINEAR -> (vh, vw, 3) uint8 BGR"""
    args, out, keep = source_view_args(bgr, blobs, negatives, armours, flags, size)
    rc = lib().rmcv_source_view_host(*args)
    if rc:
        raise RmcvError(rc, "rmcv_source_view_host: sizes >= 1, known flags, contour offsets that do not decrease")
    return out


# corner refinement: the status word of a corner, the limits
CORNER_ITERS_MASK, CORNER_DET_ZERO, CORNER_LEFT_IMAGE, CORNER_REVERTED, CORNER_CONVERGED, CORNER_BAD_INPUT = 0xFF, 1 << 8, 1 << 9, 1 << 10, 1 << 11, 1 << 12
CORNER_WIN_MAX, CORNER_ITERS_MAX, CORNER_PER_FRAME_MAX = 15, 100, 1024


def corner_mask(win=(8, 8), zero_zone=(-1, -1)):
    """the window's weights, (2 win_y + 1, 2 win_x + 1) float32 (rmcv_corner_mask; host)"""
    wx, wy = int(win[0]), int(win[1])
    out = np.empty((max(2 * wy + 1, 1), max(2 * wx + 1, 1)), np.float32)
    rc = lib().rmcv_corner_mask(wx, wy, int(zero_zone[0]), int(zero_zone[1]), ptr(out))
    if rc:
        raise RmcvError(rc, "rmcv_corner_mask: win 1 .. 15, a zero zone of (-1, -1) or inside the window")
    return out


def gray_host(bgr):
    """(h, w) uint8 gray of an (h, w, 3) BGR image: (1868 B + 9617 G + 4899 R + 8192) >> 14 (rmcv_gray_host)"""
    bgr = np.ascontiguousarray(bgr, np.uint8)
    assert bgr.ndim == 3 and bgr.shape[2] == 3, "gray_host takes an (h, w, 3) BGR image"
    out = np.empty(bgr.shape[:2], np.uint8)
    rc = lib().rmcv_gray_host(ptr(bgr), bgr.shape[1], bgr.shape[0], 3 * bgr.shape[1], ptr(out), bgr.shape[1])
    if rc:
        raise RmcvError(rc, "rmcv_gray_host: an image of at least 1 x 1")
    return out


def corner_args(bgr, corners):
    """(bgr, corners copy (n, 2) float32, status (n,) int32) as the corner entry points take them"""
    bgr = np.ascontiguousarray(bgr, np.uint8)
    assert bgr.ndim == 3 and bgr.shape[2] == 3, "corner refinement takes an (h, w, 3) BGR image"
    c = np.array(corners, np.float32).reshape(-1, 2)
    return bgr, c, np.zeros(len(c), np.int32)


def corner_subpix_host(bgr, corners, win=(8, 8), zero_zone=(-1, -1), max_iters=40, eps=0.001):
    """cornerSubPix(gray(bgr), corners, win, zero_zone, {EPS + COUNT, max_iters, eps}) on the CPU (rmcv_corner_subpix_host: the sequential
    statement of the pinned rule) -> (corners (n, 2) float32, status (n,) int32)"""
    bgr, c, st = corner_args(bgr, corners)
    rc = lib().rmcv_corner_subpix_host(ptr(bgr), bgr.shape[1], bgr.shape[0], 3 * bgr.shape[1], ptr(c), len(c), int(win[0]), int(win[1]), int(zero_zone[0]),
                                       int(zero_zone[1]), int(max_iters), float(eps), ptr(st))
    if rc:
        raise RmcvError(rc, "rmcv_corner_subpix_host: win 1 .. 15, a zero zone of (-1, -1) or inside the window, max_iters 1 .. 100, eps finite and >= 0")
    return c, st


# the chessboard detector: the status word of a frame, the limits
CHESS_COUNT_MASK, CHESS_FOUND, CHESS_OVERFLOW, CHESS_NO_GRID, CHESS_CAND_MAX = 0x7FF, 1 << 11, 1 << 12, 1 << 13, 1024
CHESS_PARAMS = ("threshold", "contrast", "nms", "dist_min", "dist_max")


def chess_defaults():
    """rmcv_chess_defaults as a dict: threshold, contrast, nms, dist_min, dist_max"""
    p = np.zeros(5, np.int32)
    lib().rmcv_chess_defaults(ptr(p))
    return dict(zip(CHESS_PARAMS, (int(v) for v in p)))


def chess_params(params=None, **changes):
    """struct rmcv_chess_params as 5 int32: the defaults, then `params` (a dict), then the keyword changes"""
    p = chess_defaults()
    for k, v in list((params or {}).items()) + list(changes.items()):
        assert k in p, "no chessboard parameter %r" % k
        p[k] = int(v)
    return np.array([p[k] for k in CHESS_PARAMS], np.int32)


def chess_outputs(cols, rows):
    """(corners (cols rows, 2) float32 of NaN, status (1,), candidates (1024, 3), candidate count (1,)) int32, as the entry points fill them"""
    return (np.full((max(int(cols) * int(rows), 1), 2), np.nan, np.float32), np.zeros(1, np.int32), np.zeros((CHESS_CAND_MAX, 3), np.int32),
            np.zeros(1, np.int32))


def chess_result(out):
    """(corners (cols rows, 2) float32 or None without a board, status, candidates (n, 3) int32: x, y, R)"""
    cor, st, cand, n = out
    return (cor if int(st[0]) & CHESS_FOUND else None), int(st[0]), cand[:int(n[0])].copy()


CHESS_REFUSED = "a cols x rows pattern of 2 .. 32 a side and at most 1024 corners, threshold >= 0, contrast 0 .. 255, nms 1 .. 7, 1 <= dist_min <= dist_max <= 1023"


def find_chessboard_host(bgr, cols, rows, params=None, **changes):
    """the inner corners of a cols x rows chessboard in an (h, w, 3) BGR image on the CPU (rmcv_find_chessboard_host: the sequential statement
    of the rule) -> (corners (cols rows, 2) float32 in row-major order, or None; the status word; the candidates (n, 3) int32)"""
    bgr = np.ascontiguousarray(bgr, np.uint8)
    assert bgr.ndim == 3 and bgr.shape[2] == 3, "find_chessboard_host takes an (h, w, 3) BGR image"
    out = chess_outputs(cols, rows)
    rc = lib().rmcv_find_chessboard_host(ptr(bgr), bgr.shape[1], bgr.shape[0], 3 * bgr.shape[1], int(cols), int(rows), ptr(chess_params(params, **changes)),
                                         *[ptr(a) for a in out])
    if rc:
        raise RmcvError(rc, "rmcv_find_chessboard_host: " + CHESS_REFUSED)
    return chess_result(out)


# the calibration solve: the status word of a camera, the limits, the fix mask, the records
CALIB_CONVERGED, CALIB_MAX_ITERS, CALIB_STALLED, CALIB_TOO_FEW_VIEWS, CALIB_BAD_INIT, CALIB_TOO_MANY_VIEWS = 1, 2, 4, 8, 16, 32
CALIB_SOLVED = CALIB_CONVERGED | CALIB_MAX_ITERS | CALIB_STALLED
CALIB_VIEWS_MAX, CALIB_VIEWS_PER_CAMERA_MAX, CALIB_CAMERAS_MAX = 4096, 256, 64
CALIB_FIX = dict(fx=1, fy=2, cx=4, cy=8, k1=16, k2=32, p1=64, p2=128, k3=256)
CALIB_PARAMS = np.dtype([("max_iters", "<i4"), ("fix_mask", "<i4"), ("eps", "<f8")])
CALIB_GUESS = np.dtype([("camera_matrix", "<f8", 9), ("dist", "<f8", 5)])
CALIB_RESULT = np.dtype([("camera_matrix", "<f8", 9), ("dist", "<f8", 5), ("rms", "<f8"), ("rms_init", "<f8"), ("views_used", "<i4"), ("iters", "<i4"), ("status", "<i4"),
                         ("reserved", "<i4")])
CALIB_VIEW = np.dtype([("rvec", "<f8", 3), ("tvec", "<f8", 3), ("q", "<f8", 4), ("rms", "<f8"), ("used", "<i4"), ("reserved", "<i4")])
CALIB_REFUSED = ("tables that are not null, n_views 1 .. 4096, n_cameras 1 .. 64, a cols x rows pattern of 4 .. 1024 corners, per_frame cols * rows .. 1024, a finite "
                 "square > 0, w, h >= 1, max_iters 1 .. 100, fix_mask 0 .. 511, a finite eps >= 0, finite guesses with focal lengths > 0")


def calib_defaults():
    """rmcv_calib_defaults as a dict: max_iters, fix_mask, eps"""
    p = np.zeros(1, CALIB_PARAMS)
    lib().rmcv_calib_defaults(ptr(p))
    return dict(max_iters=int(p["max_iters"][0]), fix_mask=int(p["fix_mask"][0]), eps=float(p["eps"][0]))


def calib_params(params=None, **changes):
    """struct rmcv_calib_params: the defaults, then `params` (a dict), then the keyword changes; fix_mask may be an iterable of CALIB_FIX's names"""
    p = calib_defaults()
    for k, v in list((params or {}).items()) + list(changes.items()):
        assert k in p, "no calibration parameter %r" % k
        p[k] = v
    if not isinstance(p["fix_mask"], (int, np.integer)):
        p["fix_mask"] = sum(CALIB_FIX[n] for n in p["fix_mask"])
    out = np.zeros(1, CALIB_PARAMS)
    out["max_iters"], out["fix_mask"], out["eps"] = int(p["max_iters"]), int(p["fix_mask"]), float(p["eps"])
    return out


def calib_guesses(guesses, n_cameras):
    """a table of n_cameras struct rmcv_calib_guess, or None: `guesses` is None, one (camera_matrix, dist) pair for every camera, or a list of
    pairs / None per camera (None: no guess for that camera)"""
    if guesses is None:
        return None
    if len(guesses) == 2 and np.size(guesses[0]) == 9:
        guesses = [guesses] * n_cameras
    assert len(guesses) == n_cameras, "one guess per camera"
    out = np.zeros(n_cameras, CALIB_GUESS)
    for k, g in enumerate(guesses):
        if g is not None:
            out["camera_matrix"][k] = np.asarray(g[0], np.float64).reshape(9)
            out["dist"][k] = np.asarray(g[1], np.float64).reshape(5)
    return out


class CalibResult:
    """one camera's struct rmcv_calib_result (`.rec`, a numpy record) with its fields as attributes"""

    def __init__(self, rec):
        self.rec = rec
        self.camera_matrix = np.array(rec["camera_matrix"], np.float64).reshape(3, 3)
        self.dist = np.array(rec["dist"], np.float64)
        self.rms, self.rms_init = float(rec["rms"]), float(rec["rms_init"])
        self.views_used, self.iters, self.status = int(rec["views_used"]), int(rec["iters"]), int(rec["status"])

    @property
    def solved(self):
        return bool(self.status & CALIB_SOLVED)

    def as_pnp_config(self, base=None):
        """a PnpConfig with this camera and distortion (rmcv_calib_to_pnp_config); everything else is `base`'s, or
        the defaults'"""
        cfg = default_pnp_config() if base is None else PnpConfig.from_buffer_copy(base)
        rec = np.array(self.rec, CALIB_RESULT).reshape(1)
        rc = lib().rmcv_calib_to_pnp_config(ptr(rec), C.byref(cfg))
        if rc:
            raise RmcvError(rc, "rmcv_calib_to_pnp_config: the result holds no solution (status %d)" % self.status)
        return cfg

    def __repr__(self):
        return "CalibResult(status=%d, views_used=%d, iters=%d, rms=%.6g)" % (self.status, self.views_used, self.iters, self.rms)


def calib_tables(corners, counts):
    """(corners (n_views, per_frame, 2) float32 contiguous, counts (n_views,) int32; counts None: every view has per_frame corners)"""
    corners = np.ascontiguousarray(corners, np.float32)
    assert corners.ndim == 3 and corners.shape[2] == 2, "the corner table is (n_views, per_frame, 2)"
    counts = np.full(len(corners), corners.shape[1], np.int32) if counts is None else np.ascontiguousarray(counts, np.int32).reshape(-1)
    assert len(counts) == len(corners), "one count per view"
    return corners, counts


def calib_outputs(n_cameras, n_views):
    """(results, views) as the entry points take them: zeroed, so that rows they do not touch read used = 0, status = 0"""
    return np.zeros(n_cameras, CALIB_RESULT), np.zeros(n_views, CALIB_VIEW)


def calibrate_camera_host(corners, counts, cols, rows, square, size, params=None, guess=None, **changes):
    """camera matrix and distortion from chessboard views on the CPU (rmcv_calibrate_camera_host: the sequential statement of the rule, DESIGN.md
    4u).  corners (n_views, per_frame, 2) float32 and counts (n_views,) as find / refine leave them; size = (w, h) ->
    (CalibResult, views: a CALIB_VIEW record array of n_views rows, used = 0 for a view that was skipped)"""
    corners, counts = calib_tables(corners, counts)
    res, views = calib_outputs(1, len(corners))
    g = calib_guesses(None if guess is None else [guess], 1)
    rc = lib().rmcv_calibrate_camera_host(ptr(corners), corners.shape[1], ptr(counts), len(corners), int(cols), int(rows), float(square), int(size[0]), int(size[1]),
                                          ptr(calib_params(params, **changes)), ptr(g) if g is not None else None, ptr(res), ptr(views))
    if rc:
        raise RmcvError(rc, "rmcv_calibrate_camera_host: " + CALIB_REFUSED)
    return CalibResult(res[0]), views


# the hand-eye solve: the status word of a camera and the records
HANDEYE_OK, HANDEYE_T_UNOBSERVABLE, HANDEYE_TOO_FEW_VIEWS, HANDEYE_TOO_MANY_VIEWS = 1, 2, 4, 8
HANDEYE_PARAMS = np.dtype([("min_w", "<f8"), ("reserved", "<i4", 2)])
HANDEYE_RESULT = np.dtype([("cam2gripper", "<f8", 16), ("q", "<f8", 4), ("t", "<f8", 3), ("eig", "<f8", 4), ("pivots", "<f8", 3), ("rot_rms", "<f8"), ("trans_rms", "<f8"),
                           ("world_mean", "<f8", 3), ("world_rms", "<f8"), ("views_used", "<i4"), ("pairs_used", "<i4"), ("pairs_skipped", "<i4"), ("sweeps", "<i4"),
                           ("status", "<i4"), ("reserved", "<i4", 3)])
HANDEYE_VIEW = np.dtype([("world", "<f8", 3), ("used", "<i4"), ("reserved", "<i4")])
assert HANDEYE_PARAMS.itemsize == 16 and HANDEYE_RESULT.itemsize == 320 and HANDEYE_VIEW.itemsize == 32
HANDEYE_REFUSED = "tables that are not null, n_views 1 .. 4096, n_cameras 1 .. 64, a finite min_w in [0, 1)"


def handeye_defaults():
    """rmcv_handeye_defaults as a dict: min_w"""
    p = np.zeros(1, HANDEYE_PARAMS)
    lib().rmcv_handeye_defaults(ptr(p))
    return dict(min_w=float(p["min_w"][0]))


def handeye_params(params=None, **changes):
    """struct rmcv_handeye_params: the defaults, then `params` (a dict), then the keyword changes"""
    p = handeye_defaults()
    for k, v in list((params or {}).items()) + list(changes.items()):
        assert k in p, "no hand-eye parameter %r" % k
        p[k] = v
    out = np.zeros(1, HANDEYE_PARAMS)
    out["min_w"] = float(p["min_w"])
    return out


class HandEyeResult:
    """one camera's struct rmcv_handeye_result (`.rec`, a numpy record) with its fields as attributes"""

    def __init__(self, rec):
        self.rec = rec
        self.cam2gripper = np.array(rec["cam2gripper"], np.float64).reshape(4, 4)
        self.q, self.t, self.eig, self.pivots = (np.array(rec[k], np.float64) for k in ("q", "t", "eig", "pivots"))
        self.rot_rms, self.trans_rms, self.world_rms = float(rec["rot_rms"]), float(rec["trans_rms"]), float(rec["world_rms"])
        self.world_mean = np.array(rec["world_mean"], np.float64)
        self.views_used, self.pairs_used, self.pairs_skipped = int(rec["views_used"]), int(rec["pairs_used"]), int(rec["pairs_skipped"])
        self.sweeps, self.status = int(rec["sweeps"]), int(rec["status"])

    @property
    def solved(self):
        """a rotation is there (the translation too unless the status is HANDEYE_T_UNOBSERVABLE)"""
        return bool(self.status & (HANDEYE_OK | HANDEYE_T_UNOBSERVABLE))

    def _into(self, call, name, cfg, allow_rotation_only):
        rec = np.array(self.rec, HANDEYE_RESULT).reshape(1)
        rc = call(ptr(rec), C.byref(cfg), int(bool(allow_rotation_only)))
        if rc:
            raise RmcvError(rc, "%s: the result holds no mounting (status %d)" % (name, self.status))
        return cfg

    def as_pnp_config(self, base=None, allow_rotation_only=False):
        """a PnpConfig with this gripper2camera (rmcv_handeye_to_pnp_config); everything else is `base`'s, or the defaults'"""
        cfg = default_pnp_config() if base is None else PnpConfig.from_buffer_copy(base)
        return self._into(lib().rmcv_handeye_to_pnp_config, "rmcv_handeye_to_pnp_config", cfg, allow_rotation_only)

    def as_attitude_config(self, base=None, allow_rotation_only=False):
        """an AttitudeConfig with this gripper2camera (rmcv_handeye_to_attitude_config); everything else is `base`'s, or the defaults'"""
        from .tracker import AttitudeConfig, default_attitude_config
        cfg = default_attitude_config() if base is None else AttitudeConfig.from_buffer_copy(base)
        return self._into(lib().rmcv_handeye_to_attitude_config, "rmcv_handeye_to_attitude_config", cfg, allow_rotation_only)

    def __repr__(self):
        return "HandEyeResult(status=%d, views_used=%d, pairs_used=%d, rot_rms=%.3g, trans_rms=%.3g, world_rms=%.3g)" % (
            self.status, self.views_used, self.pairs_used, self.rot_rms, self.trans_rms, self.world_rms)


def handeye_tables(views, attitudes, gripper_t=None):
    """(views CALIB_VIEW (n,), attitudes ATTITUDE (n,) -- an ATTITUDE array or (n, 3) (roll, pitch, yaw) radians --, gripper_t (n, 3) float64 or None)"""
    views = np.ascontiguousarray(views, CALIB_VIEW).reshape(-1)
    if not (isinstance(attitudes, np.ndarray) and attitudes.dtype == ATTITUDE):
        a = np.asarray(attitudes, np.float64).reshape(-1, 3)
        attitudes = np.zeros(len(a), ATTITUDE)
        attitudes["roll"], attitudes["pitch"], attitudes["yaw"] = a[:, 0], a[:, 1], a[:, 2]
    attitudes = np.ascontiguousarray(attitudes).reshape(-1)
    assert len(attitudes) == len(views), "one attitude per view"
    if gripper_t is not None:
        gripper_t = np.ascontiguousarray(gripper_t, np.float64).reshape(-1, 3)
        assert len(gripper_t) == len(views), "one gripper translation per view"
    return views, attitudes, gripper_t


def handeye_outputs(n_cameras, n_views):
    """(results, view rows) as the entry points take them: zeroed, so that rows they do not touch read used = 0, status = 0"""
    return np.zeros(n_cameras, HANDEYE_RESULT), np.zeros(n_views, HANDEYE_VIEW)


def calibrate_hand_eye_host(views, attitudes, gripper_t=None, params=None, **changes):
    """the camera's mounting on the gimbal from the calibration solve's view rows and the gimbal's attitudes, on the CPU
    (rmcv_calibrate_hand_eye_host: the sequential statement of the rule) -> (HandEyeResult, rows: a HANDEYE_VIEW record array
    of n_views rows, used = 0 for a view that was skipped)"""
    views, attitudes, gripper_t = handeye_tables(views, attitudes, gripper_t)
    res, rows = handeye_outputs(1, len(views))
    rc = lib().rmcv_calibrate_hand_eye_host(ptr(views), ptr(attitudes), ptr(gripper_t), len(views), ptr(handeye_params(params, **changes)), ptr(res), ptr(rows))
    if rc:
        raise RmcvError(rc, "rmcv_calibrate_hand_eye_host: " + HANDEYE_REFUSED)
    return HandEyeResult(res[0]), rows


ICON_SIDE_MAX, ICON_STRIP_CAP_MAX = 256, 1024   # the icon strip


def affine_correction_host(bgr, icon, size=(20, 20)):
    """rm::affine_correction(bgr, out, icon, size) on the CPU (rmcv_affine_correction_host: the sequential restatement, no device), size =
    (ow, oh) up to 256 x 256 -> (out (oh, ow, 3) uint8 BGR, zeros for a degenerate box; the icon clamped to the image, float32 [4, 2];
    whether the box was degenerate)"""
    bgr = np.ascontiguousarray(bgr, np.uint8)
    assert bgr.ndim == 3 and bgr.shape[2] == 3, "an (h, w, 3) BGR image"
    ic = np.array(icon, np.float32).reshape(4, 2).copy()
    ow, oh = int(size[0]), int(size[1])
    out = np.empty((max(oh, 0), max(ow, 0), 3), np.uint8)
    deg = C.c_int32(0)
    rc = lib().rmcv_affine_correction_host(ptr(bgr), bgr.shape[1], bgr.shape[0], 3 * bgr.shape[1], ptr(ic), ow, oh, ptr(out), 3 * ow, C.byref(deg))
    if rc:
        raise RmcvError(rc, "rmcv_affine_correction_host: an image of at least 1 x 1, an output size of 1 .. 256 x 1 .. 256")
    return out, ic, bool(deg.value)


def icon_strip_args(bgr, armours, side, cap):
    """the argument list rmcv_icon_strip and rmcv_icon_strip_host share, and the arrays it points into: bgr (h, w, 3) uint8; armours ARMOUR[];
    cap None: as many slots as armours (at least one) -> (args, out (side, cap side, 3) uint8, keepalive)"""
    bgr = np.ascontiguousarray(bgr, np.uint8)
    assert bgr.ndim == 3 and bgr.shape[2] == 3, "an (h, w, 3) BGR image"
    armours = np.ascontiguousarray(armours if armours is not None else [], ARMOUR).reshape(-1)
    side, cap = int(side), int(max(len(armours), 1) if cap is None else cap)
    out = np.empty((max(side, 0), max(cap * side, 0), 3), np.uint8)
    args = [ptr(bgr), bgr.shape[1], bgr.shape[0], 3 * bgr.shape[1], ptr(armours) if len(armours) else None, len(armours), side, cap, ptr(out), 3 * cap * side]
    return args, out, (bgr, armours)


def icon_strip_host(bgr, armours, side=80, cap=None):
    """the labeler's icon strip (executable/svm/labeler.cpp:93-106) on the CPU (rmcv_icon_strip_host): the icon of armour j < min(n, cap) at
    side x side in columns [j side, (j + 1) side), zeros elsewhere -> (side, cap side, 3) uint8 BGR"""
    args, out, keep = icon_strip_args(bgr, armours, side, cap)
    rc = lib().rmcv_icon_strip_host(*args)
    if rc:
        raise RmcvError(rc, "rmcv_icon_strip_host: an image of at least 1 x 1, side 1 .. 256, cap 1 .. 1024")
    return out


def sheet_size(size, side):
    """(sheet_w, sheet_h) = (2 vw, vh + side) of the labeler's sheet at view size `size` = (vw, vh) (rmcv_sheet_size)"""
    sw, sh = C.c_int32(0), C.c_int32(0)
    rc = lib().rmcv_sheet_size(int(size[0]), int(size[1]), int(side), C.byref(sw), C.byref(sh))
    if rc:
        raise RmcvError(rc, "rmcv_sheet_size: a view of at least 1 x 1, side 1 .. 256 and at most 2 vw")
    return sw.value, sh.value


def labeler_sheet_host(bgr, binary, blobs=None, negatives=None, armours=None, size=(640, 512), side=80, flags=VIEW_ALL):
    """the labeler's sheet (executable/svm/labeler.cpp:113-119) at view size `size` = (vw, vh) on the CPU (rmcv_labeler_sheet_host):
    source_view_host(bgr, ..., flags) | debug_view_host(binary, flags=0) over icon_strip_host -> (vh + side, 2 vw, 3) uint8 BGR"""
    args, _, keep = source_view_args(bgr, blobs, negatives, armours, flags, size)
    binary = np.ascontiguousarray(binary, np.uint8)
    assert binary.shape == keep[-1].shape[:2], "the binary image has the frame's extent"
    vw, vh, side = int(size[0]), int(size[1]), int(side)
    out = np.empty((max(vh + side, 0), max(2 * vw, 0), 3), np.uint8)
    # (view_args' tail is flags, vw, vh, out, out_stride: the sheet's is vw, vh, side, flags, out, out_stride)
    rc = lib().rmcv_labeler_sheet_host(*args[:4], ptr(binary), binary.shape[1], *args[4:11], vw, vh, side, int(flags), ptr(out), 6 * vw)
    if rc:
        raise RmcvError(rc, "rmcv_labeler_sheet_host: sizes >= 1, side 1 .. 256 and at most 2 vw, known flags")
    return out


def _text(call, what):
    buf = C.create_string_buffer(LABEL_MAX_CHARS + 1)
    rc = call(buf, len(buf))
    if rc < 0:
        raise RmcvError(rc, what)
    return buf.value.decode("ascii")


def format_f6(v):
    """std::to_string(double) as the label pass writes it (rmcv_format_f6: host-side, the function the device runs): "%f" for finite
    |v| < 1e15, correctly rounded half to even in integer arithmetic; "nan", "inf" / "-inf", and "big" / "-big" from 1e15 on"""
    return _text(lambda b, n: lib().rmcv_format_f6(C.c_double(float(v)), b, n), "rmcv_format_f6")


def label_text(identity, position=None):
    """an armour's line, 'identity: x, y, z' (rmcv_label_text; position None: zeros)"""
    pos = None if position is None else _tvec(position)
    return _text(lambda b, n: lib().rmcv_label_text(C.c_int32(int(identity)), ptr(pos), b, n), "rmcv_label_text")


def track_label_text(track):
    """a track's line, 'identity: x, y, z, lost_count' of one TRACK record (rmcv_track_label_text): the filter's posterior once the track
    is initialised, else the observation's position"""
    t = np.ascontiguousarray(track, TRACK).reshape(-1)
    assert len(t) == 1
    return _text(lambda b, n: lib().rmcv_track_label_text(ptr(t), b, n), "rmcv_track_label_text")


def view_glyph(ch):
    """the library's 5 x 7 glyph of one character of LABEL_CHARSET: 7 row bytes, top to bottom, the left column in bit 4 (rmcv_view_glyph;
    raises for any other character)"""
    rows = np.zeros(7, np.uint8)
    rc = lib().rmcv_view_glyph(ord(ch) if isinstance(ch, str) else int(ch), ptr(rows))
    if rc:
        raise RmcvError(rc, "rmcv_view_glyph: a character outside the label set")
    return rows


def view_labels_args(view, geometry, scale, armours, identities, positions, tracks, last_vertices, origin, stride=None):
    """the argument list rmcv_view_labels_host and rmcv_view_labels share, and the arrays it points into (keep them until the call is
    through).  view: (vh, vw, 3) uint8, drawn IN PLACE -- or, with `stride`, a flat uint8 buffer of rows `stride` bytes apart and
    geometry = (w, h, vw, vh); geometry otherwise (w, h), what the lists' coordinates are in"""
    if stride is None:
        assert view.dtype == np.uint8 and view.ndim == 3 and view.shape[2] == 3 and view.flags.c_contiguous
        vh, vw = view.shape[:2]
        w, h = int(geometry[0]), int(geometry[1])
        stride = 3 * vw
    else:
        assert view.dtype == np.uint8 and view.ndim == 1 and view.flags.c_contiguous
        w, h, vw, vh = (int(v) for v in geometry)
        assert len(view) >= stride * (vh - 1) + 3 * vw
    armours = np.ascontiguousarray(armours if armours is not None else [], ARMOUR).reshape(-1)
    n = len(armours)
    ids = None if identities is None else np.ascontiguousarray(identities, np.int32).reshape(-1)
    pos = None if positions is None else np.ascontiguousarray(positions, np.float64).reshape(-1, 3)
    assert ids is None or len(ids) == n
    assert pos is None or len(pos) == n
    tracks = np.ascontiguousarray(tracks if tracks is not None else [], TRACK).reshape(-1)
    nt = len(tracks)
    side = np.ascontiguousarray(last_vertices if last_vertices is not None else [], np.float32).reshape(-1, 4, 2)
    assert len(side) == nt
    keep = (view, armours, ids, pos, tracks, side)
    args = [ptr(view), vw, vh, int(stride), w, h, int(scale), ptr(armours) if n else None, ptr(ids) if n else None, ptr(pos) if n else None, n,
            ptr(tracks) if nt else None, ptr(side) if nt else None, nt, int(origin[0]), int(origin[1])]
    return args, keep


def view_labels_host(view, geometry, scale=1, armours=None, identities=None, positions=None, tracks=None, last_vertices=None, origin=(0, 0), stride=None):
    """the label pass on the CPU, in place (rmcv_view_labels_host: the sequential restatement, no device): every track's quadrilateral and
    line in (255, 0, 255), then every armour's line in (0, 255, 255), over a finished view of a frame whose lists are in `geometry` =
    (w, h).  identities None: -1; positions None: zeros; origin: the effective window origin the tracks' frame coordinates are moved by.
    Returns view."""
    args, keep = view_labels_args(view, geometry, scale, armours, identities, positions, tracks, last_vertices, origin, stride)
    rc = lib().rmcv_view_labels_host(*args)
    if rc:
        raise RmcvError(rc, "rmcv_view_labels_host: sizes >= 1, stride >= 3 vw, scale 1 .. 8")
    return view


def _tvec(tvec):
    t = np.ascontiguousarray(tvec, np.float64).reshape(-1)
    assert t.shape == (3,)
    return t


def projectile_angle(v0, g, d, h):
    """rm::ProjectileAngle (rmcv_projectile_angle: host-side): m/s, m/s^2, m, m -> rad, NaN without a real root"""
    return lib().rmcv_projectile_angle(float(v0), float(g), float(d), float(h))


def solve_gea(tvec, g, v0, h, offset=(0.0, 0.0), angle_offset=0.0, mode=COMPENSATE_NONE):
    """rm::SolveGEA (rmcv_solve_gea: host-side, the reference's statements as written) -> (flight time, [pitch, yaw] in degrees);
    COMPENSATE_NI: (NaN, None), as the reference returns before it creates the output"""
    t, gea = _tvec(tvec), np.full(2, np.nan)
    time = lib().rmcv_solve_gea(ptr(t), float(g), float(v0), float(h), C.c_float(offset[0]), C.c_float(offset[1]), float(angle_offset), int(mode), ptr(gea))
    return time, (None if mode == COMPENSATE_NI else gea)


def delta_height(tvec, motor_angle, offset=(0.0, 0.0), angle_offset=0.0):
    """rm::DeltaHeight (rmcv_delta_height: host-side) -> cm"""
    t = _tvec(tvec)
    return lib().rmcv_delta_height(ptr(t), float(motor_angle), C.c_float(offset[1]), float(angle_offset))


def distance(tvec):
    """rm::Distance (rmcv_distance: host-side)"""
    t = _tvec(tvec)
    return lib().rmcv_distance(ptr(t))


def rigid_inverse(m):
    """[R t; 0 1] -> [R^T  -R^T t; 0 1] (rmcv_rigid_inverse): what turns gripper2camera into an aim input's world2camera"""
    a, out = np.ascontiguousarray(m, np.float64).reshape(4, 4), np.zeros((4, 4))
    rc = lib().rmcv_rigid_inverse(ptr(a), ptr(out))
    if rc:
        raise RmcvError(rc, "rmcv_rigid_inverse")
    return out


def _attitude(attitude):
    """(roll, pitch, yaw) in radians, or a 1-element ATTITUDE array -> ATTITUDE[1]"""
    if isinstance(attitude, np.ndarray) and attitude.dtype == ATTITUDE:
        return np.ascontiguousarray(attitude).reshape(1).copy()
    a = np.zeros(1, ATTITUDE)
    a[0] = tuple(float(v) for v in attitude)
    return a


def euler_to_matrix(attitude):
    """rm::euler<double>::to_matrix (rmcv_euler_to_matrix: host-side): (roll, pitch, yaw) radians -> R = (Rz(yaw) Ry(pitch)) Rx(roll), (3, 3)"""
    a, out = _attitude(attitude), np.zeros((3, 3))
    rc = lib().rmcv_euler_to_matrix(ptr(a), ptr(out))
    if rc:
        raise RmcvError(rc, "rmcv_euler_to_matrix")
    return out


def homogeneous(rotation, translation=None):
    """rm::utils::homogeneous (rmcv_homogeneous: host-side): R (3, 3) and t (3,) | None: zeros, in an identity (4, 4)"""
    r, out = np.ascontiguousarray(rotation, np.float64).reshape(3, 3), np.zeros((4, 4))
    t = None if translation is None else _tvec(translation)
    rc = lib().rmcv_homogeneous(ptr(r), ptr(t), ptr(out))
    if rc:
        raise RmcvError(rc, "rmcv_homogeneous")
    return out


def crc8(data):
    """rm::lookup_CRC (rmcv_crc8: host-side): polynomial 0x31, MSB first, init 0"""
    b = np.frombuffer(bytes(data), np.uint8)
    return int(lib().rmcv_crc8(ptr(b) if len(b) else None, len(b)))


def serial_decode(packet):
    """the packet check and decode of executable/main.cpp:120-143 (rmcv_serial_decode: host-side): 24 bytes ->
    (camp, ATTITUDE record in radians), or None for a rejected packet"""
    b = np.frombuffer(bytes(packet), np.uint8)
    if len(b) != SERIAL_PACKET_BYTES:
        raise RmcvError(ERR_BAD_ARG, "a serial packet is %d bytes" % SERIAL_PACKET_BYTES)
    camp, a = C.c_int32(0), np.zeros(1, ATTITUDE)
    rc = lib().rmcv_serial_decode(ptr(b), C.byref(camp), ptr(a))
    if rc < 0:
        raise RmcvError(rc, "rmcv_serial_decode")
    return (camp.value, a[0]) if rc == 1 else None


def serial_encode(camp, yaw_deg, pitch_deg, roll_deg):
    """the packet serial_decode accepts (rmcv_serial_encode: for replay hosts and tests): camp CAMP_RED | CAMP_BLUE, degrees as f32 -> bytes"""
    out = np.zeros(SERIAL_PACKET_BYTES, np.uint8)
    rc = lib().rmcv_serial_encode(C.c_int32(int(camp)), C.c_float(yaw_deg), C.c_float(pitch_deg), C.c_float(roll_deg), ptr(out))
    if rc:
        raise RmcvError(rc, "rmcv_serial_encode: camp must be CAMP_RED or CAMP_BLUE")
    return out.tobytes()


def frame_camera(idx, n_cameras):
    """the camera-table entry a frame with raw index `idx`, any int32, uses (rmcv_frame_camera: host-side, the function k_pnp runs)"""
    idx, n_cameras = int(idx), int(n_cameras)
    assert -2**31 <= idx < 2**31 and -2**31 <= n_cameras < 2**31
    return int(lib().rmcv_frame_camera(C.c_int32(idx), C.c_int32(n_cameras)))


SVM_MAX_MODELS = 64  # RMCV_SVM_MAX_MODELS


class SvmModel(C.Structure):
    """rmcv_svm_model: one entry of rmcv_svm_load_models' table, pointers into arrays the caller keeps alive for the call"""
    _fields_ = [("weights", C.c_void_p), ("rho", C.c_void_p), ("labels", C.c_void_p), ("n_class", C.c_int32), ("reserved", C.c_int32)]


def frame_model(idx, n_models):
    """the model-table entry a frame with raw index `idx`, any int32, uses (rmcv_frame_model: host-side, the function k_classify_models runs)"""
    idx, n_models = int(idx), int(n_models)
    assert -2**31 <= idx < 2**31 and -2**31 <= n_models < 2**31
    return int(lib().rmcv_frame_model(C.c_int32(idx), C.c_int32(n_models)))


def default_pnp_config():
    c = PnpConfig()
    lib().rmcv_default_pnp_config(C.byref(c))
    return c


def default_params(**kw):
    p = Params()
    lib().rmcv_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p
