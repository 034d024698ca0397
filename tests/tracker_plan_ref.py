"""What callers read of a device tracker as they read it before tracker_plan.h, expression by expression, in Python: what
tests/test_tracker_plan.py holds the header against.  File names and line numbers are those of rmcv_amd/csrc at the commit before the header
("Session recorder: loop records, tracked replay, device-side triggers"), where struct rmcv_tracker (rmcv_internal.h:495-520) was open to
every unit.  A tracker `t` here is a dict of that struct's fields: the flags as bools, the pointers as ints (0: null)."""
STAGE_ARMOURS = 8


def launch_aim_args(t):
    """k_aim.hip:40-44, launch_aim: k_aim's inputs, aims, stream_cfgs"""
    return t["aim_inputs"], t["aims"], (t["aim_cfgs"] if t["aim_cfgs_on"] else 0)


def launch_attitude_args(t):
    """k_attitude.hip:48-56, launch_attitude: k_attitude's attitudes, camps, packet_errors, inputs; the PER_STREAM build or not; stream_g2c"""
    per_stream = t["stream_g2c_on"]
    return (t["attitudes"], (t["b_camps"] if t["camps_on"] else 0), t["packet_errors"], t["aim_inputs"], per_stream,
            (t["stream_g2c"] if per_stream else 0))


def loop_args(t):
    """rmcv_host.hip:1184-1193, the LoopArgs fill of ctx_track: aims, aim_inputs, aim_cfgs, attitudes, packet_errors, stream_g2c, has_aim,
    has_att, has_camps, and whether the batch's packets are taken (1188)"""
    return (t["aims"], t["aim_inputs"], (t["aim_cfgs"] if t["aim_cfgs_on"] else 0),
            t["attitudes"], t["packet_errors"], (t["stream_g2c"] if t["stream_g2c_on"] else 0),
            int(t["aim_on"]), int(t["att_on"]), (1 if t["camps_on"] else 0) | (2 if t["camps_on"] and t["lower_bounds_on"] else 0),
            bool(t["att_on"]))


def tracked_submit(t):
    """rmcv_pipeline.hip:699-701, rmcv_pipeline_submit_tracked_serial: d_origins, win_w, win_h, d_camps, d_lower_bounds"""
    return ((t["b_origins"] if t["win_w"] > 0 else 0), t["win_w"], t["win_h"],
            (t["b_camps"] if t["camps_on"] else 0), (t["b_lower_bounds"] if t["camps_on"] and t["lower_bounds_on"] else 0))


def ctx_track_refusal(tracker_device, tc, device, n_frames, frames, frame_w, frame_h, win, w, h, stages):
    """rmcv_host.hip:1157-1171; tc = (n_streams, frame_w, frame_h, win_w, win_h)"""
    if tracker_device != device:
        return "rmcv_batch_track: the tracker lives on another device than the context"
    if n_frames <= 0 or not frames:
        return "rmcv_batch_track: no frames bound"
    if n_frames != tc[0]:
        return "rmcv_batch_track: the batch has %d frames, the tracker %d streams (frame f is the next frame of stream f)" % (n_frames, tc[0])
    if frame_w != tc[1] or frame_h != tc[2]:
        return "rmcv_batch_track: the frames are %d x %d, the tracker's config says %d x %d" % (frame_w, frame_h, tc[1], tc[2])
    if not stages & STAGE_ARMOURS:
        return "rmcv_batch_track: the last run had no RMCV_STAGE_ARMOURS: nothing to track"
    if win and (w != tc[3] or h != tc[4]):
        return "rmcv_batch_track: the batch's windows are %d x %d, the tracker's config says %d x %d" % (w, h, tc[3], tc[4])
    return None


def ctx_attitude_refusal(tracker_device, tc, attitude_on, device, n_frames, frames):
    """rmcv_host.hip:1211-1217"""
    if tracker_device != device:
        return "rmcv_batch_attitude: the tracker lives on another device than the context"
    if not attitude_on:
        return "rmcv_batch_attitude: attitude is off (rmcv_tracker_set_attitude)"
    if n_frames <= 0 or not frames:
        return "rmcv_batch_attitude: no frames bound"
    if n_frames != tc[0]:
        return "rmcv_batch_attitude: the batch has %d frames, the tracker %d streams (frame f is the next frame of stream f)" % (n_frames, tc[0])
    return None


def current_list_at(sel, n_streams, stream, track_cap):
    """k_track.hip:319 (rmcv_tracker_get), k_aim.hip:265 (rmcv_tracker_put), k_loop.hip:179 (rmcv_tracker_restore)"""
    return ((sel & 1) * n_streams + stream) * track_cap


def check_config(c, with_streams):
    """k_track.hip:154-164, check_config; c = dict of rmcv_tracker_config's fields (floats may be nan / inf)"""
    import math
    if with_streams and c["n_streams"] < 1:
        return "n_streams must be at least 1"
    if c["track_cap"] < 1 or c["track_cap"] > 64:
        return "track_cap out of range (1 .. RMCV_TRACKER_MAX_CAP)"
    if not all(math.isfinite(c[k]) for k in ("process_noise", "measurement_noise", "error")):
        return "the noises must be finite"
    if not math.isfinite(c["tick_frequency"]) or not c["tick_frequency"] > 0:
        return "tick_frequency must be finite and positive"
    if not math.isfinite(c["roi_scale_w"]) or not math.isfinite(c["roi_scale_h"]):
        return "the ROI scales must be finite"
    if c["frame_w"] < 1 or c["frame_h"] < 1 or c["frame_w"] > 65536 or c["frame_h"] > 65536:
        return "frame size out of range"
    if c["win_w"] < 0 or c["win_h"] < 0 or (c["win_w"] == 0) != (c["win_h"] == 0) or c["win_w"] > c["frame_w"] or c["win_h"] > c["frame_h"]:
        return "window size out of range (0, 0: track only; at most the frame)"
    return None
