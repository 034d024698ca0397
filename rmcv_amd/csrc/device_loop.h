/*
 * device_loop.h -- the session recorder's loop record, host and device from the same source: the layout of a record behind
 * its rmcv_loop_state, the checks a reader makes before it trusts one, and THE TRIGGER RULE (include/rmcv_abi.h states every comparison;
 * this is its only implementation: k_loop_record evaluates it on the device, rmcv_loop_trigger_host on the CPU).
 *
 * A loop record of an area of loop_bound(cap) bytes:
 *   [ rmcv_loop_state ][ n_tracks x { rmcv_track | float[8] side record } ][ zeros to the end of the area ]
 * Every part is a whole number of 8-byte words at an 8-byte offset; a track is NOT 16-byte aligned from one to the next (2584 bytes).
 */
#ifndef RMCV_DEVICE_LOOP_H
#define RMCV_DEVICE_LOOP_H

#include <stdint.h>
#include <string.h>

#include "../../include/rmcv_abi.h"

#if defined(__HIPCC__)
#define LOOP_FN __host__ __device__ static inline
#else
#define LOOP_FN static inline
#endif

#define LOOP_SIDE_BYTES 32
#define LOOP_TRACK_BYTES ((int64_t)sizeof(rmcv_track) + LOOP_SIDE_BYTES)
#define LOOP_TRACK_WORDS ((int)(sizeof(rmcv_track) / 8))
#define LOOP_SLOT_WORDS (LOOP_TRACK_WORDS + LOOP_SIDE_BYTES / 8)

static_assert(sizeof(rmcv_loop_state) % 8 == 0 && sizeof(rmcv_track) % 8 == 0, "a loop record is copied in 8-byte words");
static_assert(sizeof(rmcv_aim) % 8 == 0 && sizeof(rmcv_aim_input) % 8 == 0 && sizeof(rmcv_attitude) % 8 == 0, "a loop record is copied in 8-byte words");
static_assert(sizeof(rmcv_tracker_config) % 8 == 0 && sizeof(rmcv_aim_config) % 8 == 0 && sizeof(rmcv_attitude_config) % 8 == 0, "a loop record is copied in 8-byte words");

/* bytes of one loop area; -1: cap outside 0 .. RMCV_TRACKER_MAX_CAP */
LOOP_FN int64_t loop_bound(int cap)
{
    return cap < 0 || cap > RMCV_TRACKER_MAX_CAP ? -1 : (int64_t)sizeof(rmcv_loop_state) + cap * LOOP_TRACK_BYTES;
}
/* the track_cap an area of `bytes` was sized for; -1: no loop_bound of 1 .. RMCV_TRACKER_MAX_CAP */
LOOP_FN int loop_cap_of(int64_t bytes)
{
    const int64_t rest = bytes - (int64_t)sizeof(rmcv_loop_state);
    if (rest < LOOP_TRACK_BYTES || rest % LOOP_TRACK_BYTES != 0 || rest / LOOP_TRACK_BYTES > RMCV_TRACKER_MAX_CAP) return -1;
    return (int)(rest / LOOP_TRACK_BYTES);
}
/* offsets of track j and its side record inside a record */
LOOP_FN int64_t loop_track_at(int j) { return (int64_t)sizeof(rmcv_loop_state) + j * LOOP_TRACK_BYTES; }
LOOP_FN int64_t loop_side_at(int j) { return loop_track_at(j) + (int64_t)sizeof(rmcv_track); }
/* the fixed part of a record held in an area of `bytes`: its counts are what a recorder of that area can have written */
LOOP_FN int loop_counts_ok(const rmcv_loop_state* s, int64_t bytes)
{
    const int cap = loop_cap_of(bytes);
    return cap > 0 && s->n_tracks >= 0 && s->n_tracks <= cap;
}
/* ... for a reader that is handed a record without its area: n_tracks within what any recorder can have written */
LOOP_FN int loop_tracks_ok(const rmcv_loop_state* s) { return s->n_tracks >= 0 && s->n_tracks <= RMCV_TRACKER_MAX_CAP; }

/* ---- the trigger rule ---- */
LOOP_FN int loop_had_target(const rmcv_loop_state* r) { return !(r->aim.status & RMCV_AIM_NO_TARGET); }
LOOP_FN int loop_solved(const rmcv_loop_state* r) { return loop_had_target(r) && !(r->aim.status & RMCV_AIM_NO_SOLUTION); }
/* |a - b| > bound; a NaN difference (or bound) is false */
LOOP_FN int loop_jump(double a, double b, double bound)
{
    double d = a - b;
    if (d < 0) d = -d;
    return d > bound;
}
/* the bits `cur` raises against `prev`, before the mask */
LOOP_FN uint32_t loop_trigger(const rmcv_loop_state* prev, const rmcv_loop_state* cur, const rmcv_trigger_config* cfg)
{
    uint32_t f = 0;
    if (prev->n_armours > 0 && cur->n_armours == 0) f |= RMCV_TRIG_NO_ARMOURS;
    if (cur->n_tracking < prev->n_tracking) f |= RMCV_TRIG_TRACK_DROPPED;
    if ((cur->status & RMCV_TRACKER_OVF) && !(prev->status & RMCV_TRACKER_OVF)) f |= RMCV_TRIG_TRACKER_OVF;
    if (cur->frame_status & cfg->frame_status_mask & ~prev->frame_status) f |= RMCV_TRIG_FRAME_STATUS;
    if (prev->has_aim && cur->has_aim) {
        if (loop_had_target(prev) && (cur->aim.status & RMCV_AIM_NO_TARGET)) f |= RMCV_TRIG_TARGET_LOST;
        if (loop_had_target(prev) && loop_had_target(cur) && cur->aim.identity != prev->aim.identity) f |= RMCV_TRIG_TARGET_SWITCH;
        if ((cur->aim.status & RMCV_AIM_NO_SOLUTION) && !(prev->aim.status & RMCV_AIM_NO_SOLUTION)) f |= RMCV_TRIG_NO_SOLUTION;
        if (loop_solved(prev) && loop_solved(cur) &&
            (loop_jump(cur->aim.yaw, prev->aim.yaw, cfg->aim_jump_deg) || loop_jump(cur->aim.pitch, prev->aim.pitch, cfg->aim_jump_deg)))
            f |= RMCV_TRIG_AIM_JUMP;
    }
    if (prev->has_attitude && cur->has_attitude && cur->packet_errors > prev->packet_errors) f |= RMCV_TRIG_PACKET_ERROR;
    return f;
}
/* what rmcv_recorder_set_trigger refuses of a config (the recorder's track_cap apart); NULL: fine */
LOOP_FN const char* loop_trigger_refusal(const rmcv_trigger_config* c)
{
    if (c->mask & ~(uint32_t)RMCV_TRIG_ALL) return "rmcv_recorder_set_trigger: unknown bits in mask";
    if (c->post_batches < 0) return "rmcv_recorder_set_trigger: post_batches must be >= 0";
    if (!(c->aim_jump_deg >= 0)) return "rmcv_recorder_set_trigger: aim_jump_deg must be >= 0 and not NaN";
    return NULL;
}
/* the least ring that still holds the triggering batch when the recorder freezes (include/rmcv_abi.h: SIZING) */
LOOP_FN int loop_ring_bound(int depth, int post_batches) { return depth + post_batches; }

/* ---- the setup a record carries (host-side readers: the extractors behind rmcv_tracker_*_from_loop) ---- */
/* a record a replay can start from: not truncated, counts in range; RMCV_OK or RMCV_ERR_BAD_ARG */
LOOP_FN int loop_replayable(const void* rec, rmcv_loop_state* s)
{
    if (!rec) return RMCV_ERR_BAD_ARG;
    memcpy(s, rec, sizeof(*s));
    if (!loop_tracks_ok(s) || (s->flags & RMCV_LOOP_TRUNCATED) || s->n_tracks != s->n_tracking) return RMCV_ERR_BAD_ARG;
    return RMCV_OK;
}
LOOP_FN int loop_tracker_config(const void* rec, rmcv_tracker_config* out)
{
    rmcv_loop_state s;
    if (!out || loop_replayable(rec, &s)) return RMCV_ERR_BAD_ARG;
    *out = s.tracker_config;
    return RMCV_OK;
}
LOOP_FN int loop_aim_config(const void* rec, rmcv_aim_config* out, int32_t* has)
{
    rmcv_loop_state s;
    if (!out || !has || loop_replayable(rec, &s)) return RMCV_ERR_BAD_ARG;
    *has = s.has_aim != 0;
    *out = s.aim_config;
    return RMCV_OK;
}
LOOP_FN int loop_attitude_config(const void* rec, rmcv_attitude_config* out, double* g2c, int32_t* has)
{
    rmcv_loop_state s;
    if (!out || !has || loop_replayable(rec, &s)) return RMCV_ERR_BAD_ARG;
    *has = s.has_attitude != 0;
    *out = s.attitude_config;
    if (g2c) memcpy(g2c, s.gripper2camera, sizeof(s.gripper2camera));
    return RMCV_OK;
}

#endif /* RMCV_DEVICE_LOOP_H */
