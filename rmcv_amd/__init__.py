"""rmcv_amd -- MI355X-native (gfx950, hand-written HIP) implementation of rmcv's per-frame
armour-detection hot path, behind the reference's own function names.

    from rmcv_amd import Context
    ctx = Context(device=0)
    contours, binary = ctx.extract_color(image, CAMP_BLUE, 80)
"""
from .abi import (ARMOUR, BAYER_BG, BAYER_GB, BAYER_GR, BAYER_PATTERNS, BAYER_RG, CAMP_BLUE, INPUT_BGR, OPT_ENHANCE, OPT_INPUT_FORMAT, OPT_INPUT_ORIENT, OPT_INPUT_SAMPLE_BITS, OPT_INPUT_VALID_BIT, ORIENT_FLIP, ORIENT_MIRROR, CAMP_GUIDELIGHT, CAMP_NEUTRAL, CAMP_RED, LIGHTBLOB, MORPH_CLOSE, MORPH_DILATE,
                  MORPH_NONE, FRAME_MID_PATH, FRAME_SLOW_PATH, OPT_CONTOUR_TIER, OPT_FRAME_UPLOAD, OPT_DENSE_DEFER, OPT_PIXEL_HALO_NT, OPT_OVERLOADS, OPT_PIXEL_GROUPS, OPT_PIXEL_SHAPE, OPT_WAIT_TIMEOUT_MS, OPT_TEST_DELAY_US, OPT_IMAGE_EXPORT, OPT_TEST_SLOW_US, OPT_RUN_AHEAD, OPT_SPARSE_WAVES, POINT, RRECT, STAGE_ALL, STAGE_ARMOURS, STAGE_BINARY, STAGE_BLOBS, STAGE_CONTOURS, STAGE_IDENTITY, STAGE_NO_IMAGE, STAGE_POSE,
                  SVM_FEATURES, LegacyParams, Limits,
                  Params, PnpConfig, RmcvError, armours_to_frame, default_params, default_pnp_config, frame_camera, frame_key, get_roi, window_origin,
                  AIM, AIM_INPUT, AIM_HEIGHT_DELTA, AIM_HEIGHT_FIXED, AIM_NO_SOLUTION, AIM_NO_TARGET, AIM_PICK_NEAREST, AIM_PICK_WINDOW, AIM_SRC_FILTER,
                  AIM_SRC_MEASUREMENT, COMPENSATE_CLASSIC, COMPENSATE_NI, COMPENSATE_NONE, delta_height, distance, projectile_angle, rigid_inverse, solve_gea,
                  ATTITUDE, ATTITUDE_CONFIG, ATT_MOTOR_KEEP, ATT_MOTOR_PITCH, SERIAL_PACKET_BYTES, crc8, euler_to_matrix, homogeneous, serial_decode, serial_encode,
                  VIEW_ALL, VIEW_ARMOURS, VIEW_BLOBS, VIEW_NEGATIVES, debug_view_host, source_view_host)
from .api import Context, debug_view
from .abi import LABEL_ARMOURS, LABEL_CHARSET, LABEL_MAX_CHARS, LABEL_TRACKS, format_f6, label_text, track_label_text, view_glyph, view_labels_host
from .abi import ICON_SIDE_MAX, ICON_STRIP_CAP_MAX, affine_correction_host, icon_strip_host, labeler_sheet_host, sheet_size
from .abi import (CORNER_BAD_INPUT, CORNER_CONVERGED, CORNER_DET_ZERO, CORNER_ITERS_MASK, CORNER_ITERS_MAX, CORNER_LEFT_IMAGE, CORNER_PER_FRAME_MAX, CORNER_REVERTED,
                  CORNER_WIN_MAX, corner_mask, corner_subpix_host, gray_host)
from .abi import CHESS_CAND_MAX, CHESS_COUNT_MASK, CHESS_FOUND, CHESS_NO_GRID, CHESS_OVERFLOW, chess_defaults, chess_params, find_chessboard_host
from .abi import (CALIB_BAD_INIT, CALIB_CAMERAS_MAX, CALIB_CONVERGED, CALIB_FIX, CALIB_GUESS, CALIB_MAX_ITERS, CALIB_PARAMS, CALIB_RESULT, CALIB_SOLVED, CALIB_STALLED,
                  CALIB_TOO_FEW_VIEWS, CALIB_TOO_MANY_VIEWS, CALIB_VIEW, CALIB_VIEWS_MAX, CALIB_VIEWS_PER_CAMERA_MAX, CalibResult, calib_defaults, calib_params,
                  calibrate_camera_host)
from .abi import (HANDEYE_OK, HANDEYE_PARAMS, HANDEYE_RESULT, HANDEYE_T_UNOBSERVABLE, HANDEYE_TOO_FEW_VIEWS, HANDEYE_TOO_MANY_VIEWS, HANDEYE_VIEW, HandEyeResult,
                  calibrate_hand_eye_host, handeye_defaults, handeye_params)
from .pipeline import Pipeline
from .recorder import LoopRecord, Recorder, Session, loop_bound, loop_field_at, loop_trigger, pack, pack_bound, unpack
from . import svm
from .abi import SVM_MAX_MODELS, SvmModel, frame_model
from .abi import HARVEST_META, HARVEST_MISSES, HARVEST_RING_MAX, HARVEST_SKIP, ICON_SAD_MAX
from .harvest import DeviceDataset, harvest_novel, harvest_plan, icon_sad
from .abi import (LOOP_TRUNCATED, TRIG_AIM_JUMP, TRIG_ALL, TRIG_FRAME_STATUS, TRIG_NO_ARMOURS, TRIG_NO_SOLUTION, TRIG_PACKET_ERROR, TRIG_TARGET_LOST, TRIG_TARGET_SWITCH,
                  TRIG_TRACK_DROPPED, TRIG_TRACKER_OVF, LoopState, TriggerConfig, TriggerInfo)
from .tracker import TRACKER_OVF, AimConfig, AttitudeConfig, Tracker, TrackerConfig, default_aim_config, default_attitude_config, default_tracker_config

__all__ = [n for n in dir() if not n.startswith("_")]
