// tracker_plan.h -- the host's state of a device-resident tracker and what everything outside rmcv_tracker.hip
// reads of it, as plain values and pure functions without HIP types, so that a host compiler alone can check them (tests/test_tracker_plan.py).
//   TrackerState  what the setters of rmcv_tracker.hip keep: the configs, the modes, the device tables
//   StreamTable   THE rule for an optional per-stream table: the pointer while its mode is on, else null
//   TrackerView   what a step, the loop record or a tracked submit reads, computed from the state by ONE function (tracker_view_of)
//   tracker_config_refusal  what rmcv_tracker_create and rmcv_tracker_step_host refuse of a config
//   step_refusal  what rmcv_batch_track and rmcv_batch_attitude refuse of the batch bound to a context
//   current_list_at  where a stream's current list starts, as the host addresses it
#pragma once

#include <cmath>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/rmcv_abi.h"

namespace rmcv {

// Device state of a tracker: two copies of every stream's list (a step reads the current one and writes the other; `sel` says which is
// current, per stream -- a stream whose step is refused or sees no observation simply does not flip).  By value into k_track, k_aim and
// k_loop_record: the layout is theirs.
struct TrackerBufs {
    rmcv_track* tracks;  // [2][n_streams][track_cap]
    float* side;         // [2][n_streams][track_cap][8]   frame-coordinate vertices of the observation that created / last matched the track
    int32_t* sel;        // [n_streams] 0 / 1
    int32_t* n_tracking; // [n_streams]
    int32_t* status;     // [n_streams] RMCV_TRACKER_OVF
    rmcv_point* origins; // [n_streams] the requested window origins (what Bufs::win_req borrows)
    int32_t* camps;      // [n_streams] every stream's enemy colour and lower bound (rmcv_tracker_set_camps; what Bufs::key_camps / key_lbs borrow)
    int32_t* lower_bounds;
};
// the start of stream `stream`'s current list in TrackerBufs::tracks (and, times 8, in ::side), `sel` as read from TrackerBufs::sel
inline size_t current_list_at(int32_t sel, int n_streams, int stream, int track_cap) { return ((size_t)(sel & 1) * n_streams + stream) * track_cap; }

// what a tracker's config is refused for (with_streams: n_streams counts -- not for the one-stream host step); null: fine
inline const char* tracker_config_refusal(const rmcv_tracker_config& c, bool with_streams)
{
    if (with_streams && c.n_streams < 1) return "n_streams must be at least 1";
    if (c.track_cap < 1 || c.track_cap > RMCV_TRACKER_MAX_CAP) return "track_cap out of range (1 .. RMCV_TRACKER_MAX_CAP)";
    if (!std::isfinite(c.process_noise) || !std::isfinite(c.measurement_noise) || !std::isfinite(c.error)) return "the noises must be finite";
    if (!std::isfinite(c.tick_frequency) || !(c.tick_frequency > 0)) return "tick_frequency must be finite and positive";
    if (!std::isfinite(c.roi_scale_w) || !std::isfinite(c.roi_scale_h)) return "the ROI scales must be finite";
    if (c.frame_w < 1 || c.frame_h < 1 || c.frame_w > 65536 || c.frame_h > 65536) return "frame size out of range";
    if (c.win_w < 0 || c.win_h < 0 || (c.win_w == 0) != (c.win_h == 0) || c.win_w > c.frame_w || c.win_h > c.frame_h) return "window size out of range (0, 0: track only; at most the frame)";
    return nullptr;
}

// An optional per-stream device table.  `p` is the memory (null: not allocated yet), `on` whether its readers take it: a table that is
// switched (camps, lower bounds, the streams' aim configs and gripper2camera) is on between its setter's table and its setter's NULL and
// keeps its memory while off; a table allocated on first use (aims, aim inputs, attitudes, packet errors) is on from its allocation on.
// Readers outside the tracker's unit see get() only.
template <typename T>
struct StreamTable {
    T* p = nullptr;
    bool on = false;
    T* get() const { return on ? p : nullptr; }
};

struct TrackerState {
    int device = 0;
    rmcv_tracker_config cfg{};
    TrackerBufs b{};
    bool aim_on = false;               // off until rmcv_tracker_set_aim
    rmcv_aim_config aim_cfg{};
    bool att_on = false;               // off until rmcv_tracker_set_attitude
    rmcv_attitude_config att_cfg{};
    StreamTable<int32_t> camps, lower_bounds;      // TrackerBufs's two tables; on: rmcv_tracker_set_camps (the bounds only with the camps)
    StreamTable<rmcv_aim_config> aim_cfgs;         // on: k_aim reads stream f's own entry instead of aim_cfg
    StreamTable<double> stream_g2c;                // [n_streams][16]  on: k_attitude takes stream f's own gripper2camera instead of att_cfg's
    StreamTable<rmcv_aim> aims;                    // first use: the first rmcv_tracker_set_aim / _set_aim_inputs / _device_aim* or attitude table
    StreamTable<rmcv_aim_input> aim_inputs;
    StreamTable<rmcv_attitude> attitudes;          // first use: the first rmcv_tracker_set_attitude / _set_attitudes / _device_attitudes
    StreamTable<int32_t> packet_errors;
};

// Everything read of a tracker outside its unit.  Every optional table is already null when off.
struct TrackerView {
    int device;
    rmcv_tracker_config cfg;
    rmcv_aim_config aim_cfg;
    rmcv_attitude_config att_cfg;
    TrackerBufs b;
    bool aim_on, att_on;
    int has_aim, has_att, has_camps;   // as LoopArgs takes them; has_camps: bit 0 the camps, bit 1 the lower bounds
    rmcv_point* origins;               // TrackerBufs::origins, null when cfg.win_w == 0 (track only): a tracked submit's windows
    int32_t *camps, *lower_bounds;     // a tracked submit's keys; the attitude step writes the camps
    const rmcv_aim_config* aim_cfgs;   // null: aim_cfg for every stream
    const double* stream_g2c;          // null: att_cfg's for every stream
    rmcv_aim* aims;                    // null: aiming was never on
    rmcv_aim_input* aim_inputs;        // null: never used (the defaults)
    rmcv_attitude* attitudes;
    int32_t* packet_errors;
};
inline TrackerView tracker_view_of(const TrackerState& s)
{
    TrackerView v{};
    v.device = s.device, v.cfg = s.cfg, v.aim_cfg = s.aim_cfg, v.att_cfg = s.att_cfg, v.b = s.b;
    v.aim_on = s.aim_on, v.att_on = s.att_on;
    v.camps = s.camps.get();
    v.lower_bounds = s.camps.on ? s.lower_bounds.get() : nullptr;
    v.has_aim = s.aim_on, v.has_att = s.att_on, v.has_camps = (s.camps.on ? 1 : 0) | (s.camps.on && s.lower_bounds.on ? 2 : 0);
    v.origins = s.cfg.win_w > 0 ? s.b.origins : nullptr;
    v.aim_cfgs = s.aim_cfgs.get(), v.stream_g2c = s.stream_g2c.get();
    v.aims = s.aims.get(), v.aim_inputs = s.aim_inputs.get(), v.attitudes = s.attitudes.get(), v.packet_errors = s.packet_errors.get();
    return v;
}

// The batch bound to a context as a step of the tracker sees it (Geom's fields; frames: Bufs::frames is set)
struct StepBatch {
    int device, n_frames;
    bool frames;
    int frame_w, frame_h, win, w, h;
};
// What `who` -- "rmcv_batch_track" (track: with the stages of the batch's last run) or "rmcv_batch_attitude" -- refuses with RMCV_ERR_BAD_ARG
// before anything is enqueued: the message, written into `buf`, or null
inline const char* step_refusal(const char* who, bool track, const TrackerView& v, const StepBatch& g, int stages, char (&buf)[200])
{
    const rmcv_tracker_config& tc = v.cfg;
    if (v.device != g.device) snprintf(buf, sizeof(buf), "%s: the tracker lives on another device than the context", who);
    else if (!track && !v.att_on) snprintf(buf, sizeof(buf), "%s: attitude is off (rmcv_tracker_set_attitude)", who);
    else if (g.n_frames <= 0 || !g.frames) snprintf(buf, sizeof(buf), "%s: no frames bound", who);
    else if (g.n_frames != tc.n_streams)
        snprintf(buf, sizeof(buf), "%s: the batch has %d frames, the tracker %d streams (frame f is the next frame of stream f)", who, g.n_frames, tc.n_streams);
    else if (!track) return nullptr;
    else if (g.frame_w != tc.frame_w || g.frame_h != tc.frame_h)
        snprintf(buf, sizeof(buf), "%s: the frames are %d x %d, the tracker's config says %d x %d", who, g.frame_w, g.frame_h, tc.frame_w, tc.frame_h);
    else if (!(stages & RMCV_STAGE_ARMOURS)) snprintf(buf, sizeof(buf), "%s: the last run had no RMCV_STAGE_ARMOURS: nothing to track", who);
    else if (g.win && (g.w != tc.win_w || g.h != tc.win_h))
        snprintf(buf, sizeof(buf), "%s: the batch's windows are %d x %d, the tracker's config says %d x %d", who, g.w, g.h, tc.win_w, tc.win_h);
    else return nullptr;
    return buf;
}

} // namespace rmcv
