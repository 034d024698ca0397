/*
 * device_aim.h -- the aim step behind the device-resident tracker for ONE camera stream, host and device from the same
 * source:
 *   rm::DeltaHeight      src/mobility.cpp:36-51
 *   rm::Distance         src/mobility.cpp:53-61
 *   rm::ProjectileAngle  src/mobility.cpp:63-82
 *   rm::SolveGEA         src/mobility.cpp:127-164
 * Every statement of the reference is one statement here, evaluated left to right as written; atan, atan2, cos and tan are
 * pinned_math.h's (the same bits on the host and on gfx950), sqrt is IEEE.  Compile with -ffp-contract=off, no fast-math.
 * Mirrored as written: COMPENSATE_CLASSIC takes cos() of the angle it has just converted to DEGREES (:147,150), and
 * divides SolveGEA's `h` by 100 (:145,147).
 *
 * Execution model.  aim_stream is written for ONE WAVEFRONT per stream: lane j takes track j (track_cap <= 64) and runs its dependent
 * fp64 chain on its own -- it loads the few fields it needs from its rmcv_track, nothing is staged -- then the pick is a reduction over
 * (key, index) pairs, smaller first, and the lane that won stores the record.  The host runs the lanes as a loop (AIM_HOST_REVERSED: in the
 * opposite order, which gives the same bytes: the pairs are totally ordered).
 */
#ifndef RMCV_DEVICE_AIM_H
#define RMCV_DEVICE_AIM_H

#include <stdint.h>

#include "../../include/rmcv_abi.h"
#include "pinned_math.h"

#define AIM_PI 3.1415926535897932384626433832795 /* CV_PI */
#define AIM_NO_INDEX 0x7fffffff

PM_FN double aim_nan(void) { return __builtin_nan(""); }
PM_FN int aim_finite(double x) { return x - x == 0.0; }
/* what leaves through the ABI: a NaN is THE quiet NaN (0x7FF8000000000000) -- the sign and payload of a computed NaN depend on the
 * machine (an invalid operation gives a negative one on x86, a positive one on gfx950) and on which operand it was inherited from */
PM_FN double aim_canon(double x) { return x != x ? __builtin_nan("") : x; }

/* the unqualified abs(double) of mobility.cpp:74,150: fabs, or -- overloads bit 0, SURVEY A.6 -- int abs(int) on the argument truncated
 * toward zero (the int result compares and divides as the double it converts to exactly).  (int)NaN is undefined in C: 0 here; an
 * argument beyond int saturates. */
PM_FN double aim_abs(double x, int overloads)
{
    if (!(overloads & 1)) return __builtin_fabs(x);
    if (x != x) return 0.0;
    if (x >= 2147483647.0) return 2147483647.0;
    if (x <= -2147483647.0) return 2147483647.0;
    {
        const int i = (int)x;
        return (double)(i < 0 ? -i : i);
    }
}

/* mobility.cpp:63-82.  pow(x, 2.0) is x * x: the correctly rounded square, which is what a correct pow returns. */
PM_FN double aim_projectile_angle(double v0, double g, double d, double h, int overloads)
{
    const double a = (g * (d * d)) / (2.0 * (v0 * v0));
    const double b = d;
    const double c = a - h;
    const double delta = (b * b) - (4 * a * c);
    if (delta > 0) {
        const double x1 = pm_atan(((-1 * b) + __builtin_sqrt(delta)) / (2 * a));
        const double x2 = pm_atan(((-1 * b) - __builtin_sqrt(delta)) / (2 * a));
        return aim_abs(x1, overloads) < aim_abs(x2, overloads) ? x1 : x2;
    } else if (delta == 0) {
        return pm_atan((-1) * (b / 2 * a)); /* the reference's precedence: (b / 2) * a, not b / (2 a) */
    }
    return aim_nan(); /* delta < 0, or NaN */
}

/* mobility.cpp:36-51 */
PM_FN double aim_delta_height(const double* tvec, double motor_angle, float offset_y, double angle_offset)
{
    const double h = tvec[1] - offset_y;
    const double d = tvec[2];
    const double dPitch = -pm_atan2(h, d) + (motor_angle - angle_offset);
    return d * pm_tan(dPitch);
}

/* mobility.cpp:53-61 */
PM_FN double aim_distance(const double* tvec)
{
    return __builtin_sqrt(tvec[0] * tvec[0] + tvec[1] * tvec[1] + tvec[2] * tvec[2]);
}

/* mobility.cpp:127-164; returns the flight time.  COMPENSATE_NI: NaN, *pitch and *yaw untouched. */
PM_FN double aim_solve_gea(const double* tvec, double g, double v0, double h, float offset_x, float offset_y, double angle_offset, int mode,
                           int overloads, double* pitch, double* yaw)
{
    double p = 0, t = 0;
    const double d = tvec[2] / 100.0, y = pm_atan2(tvec[0] - offset_x, tvec[2]) * 180.0 / AIM_PI;
    if (mode == RMCV_COMPENSATE_NONE) {
        p = -(pm_atan2(tvec[1] - offset_y, tvec[2]) * 180.0 / AIM_PI);
        t = d / v0;
    } else if (mode == RMCV_COMPENSATE_CLASSIC) {
        const double normalAngle = pm_atan2(h / 100.0, d) * 180.0 / AIM_PI;
        const double centerAngle = -pm_atan2(tvec[1] - offset_y, tvec[2]) * 180.0 / AIM_PI;
        const double targetAngle = aim_projectile_angle(v0, g, d, h / 100.0, overloads) * 180.0 / AIM_PI;
        p = (centerAngle - normalAngle + angle_offset * 180.0 / AIM_PI) + targetAngle;
        t = d / aim_abs(v0 * pm_cos(targetAngle), overloads); /* (degrees into cos, as written) */
    } else if (mode == RMCV_COMPENSATE_NI) {
        return aim_nan();
    }
    *pitch = p;
    *yaw = y;
    return t;
}

/* ---- the step ---------------------------------------------------------------------------------------------------------------------- */
/* what a lane leaves: its pair (smaller first) and, for a candidate, the record */
typedef struct {
    uint64_t key;
    int32_t  index;   /* the track, or AIM_NO_INDEX: no candidate */
    int32_t  identity, lost_count, status;
    double   pitch, yaw, flight_time, distance, px, py, pz;
} aim_lane_t;

PM_FN int aim_before(uint64_t ka, int32_t ia, uint64_t kb, int32_t ib) { return ka < kb || (ka == kb && ia < ib); }

/* cam = W . [q; 1], rows 0..2 in k_pnp's order; h; the solution */
PM_FN double aim_solve_at(const rmcv_aim_config* cfg, const rmcv_aim_input* in, double q0, double q1, double q2, double* cam, double* pitch,
                          double* yaw)
{
    const double* W = in->world2camera;
    cam[0] = ((W[0] * q0 + W[1] * q1) + W[2] * q2) + W[3] * 1.0;
    cam[1] = ((W[4] * q0 + W[5] * q1) + W[6] * q2) + W[7] * 1.0;
    cam[2] = ((W[8] * q0 + W[9] * q1) + W[10] * q2) + W[11] * 1.0;
    const double h = cfg->height_mode == RMCV_AIM_HEIGHT_DELTA ? aim_delta_height(cam, in->motor_angle, cfg->offset_y, cfg->angle_offset) : cfg->height;
    return aim_solve_gea(cam, cfg->g, cfg->v0, h, cfg->offset_x, cfg->offset_y, cfg->angle_offset, cfg->mode, cfg->overloads, pitch, yaw);
}

/* track j of the stream's current list: candidate or not, and a candidate's whole record */
PM_FN void aim_lane(const rmcv_aim_config* cfg, double tick_frequency, const rmcv_track* tr, int j, const rmcv_aim_input* in, int64_t now,
                    aim_lane_t* out)
{
    out->key = ~(uint64_t)0;
    out->index = AIM_NO_INDEX;
    const int32_t lost = tr->lost_count, id = tr->identity;
    const uint32_t bit = (id >= 0 && id <= 30) ? (uint32_t)id : 31u;
    if (lost > cfg->max_lost || !((cfg->identity_mask >> bit) & 1u)) return;
    const int64_t ts = tr->timestamp;
    double p0, p1, p2, v0 = 0.0, v1 = 0.0, v2 = 0.0;
    if (!tr->initialized) {
        p0 = tr->position[0]; p1 = tr->position[1]; p2 = tr->position[2];
    } else if (cfg->source == RMCV_AIM_SRC_MEASUREMENT) {
        p0 = tr->measurement[0]; p1 = tr->measurement[1]; p2 = tr->measurement[2];
        v0 = tr->measurement[3]; v1 = tr->measurement[4]; v2 = tr->measurement[5];
    } else {
        p0 = tr->state_post[0]; p1 = tr->state_post[1]; p2 = tr->state_post[2];
        v0 = tr->state_post[3]; v1 = tr->state_post[4]; v2 = tr->state_post[5];
    }
    const double dt = (double)(now - ts) / tick_frequency + cfg->latency_s;
    double cam[3], pitch = 0.0, yaw = 0.0;
    double t = aim_solve_at(cfg, in, p0 + v0 * dt, p1 + v1 * dt, p2 + v2 * dt, cam, &pitch, &yaw);
    for (int it = 0; it < cfg->lead_iterations; it++) {
        if (!aim_finite(t)) break;
        const double lead = dt + t;
        t = aim_solve_at(cfg, in, p0 + v0 * lead, p1 + v1 * lead, p2 + v2 * lead, cam, &pitch, &yaw);
    }
    const double dist = aim_distance(cam);
    out->index = j;
    out->identity = id;
    out->lost_count = lost;
    out->status = (aim_finite(pitch) && aim_finite(t)) ? 0 : RMCV_AIM_NO_SOLUTION;
    out->pitch = pitch;
    out->yaw = yaw;
    out->flight_time = t;
    out->distance = dist;
    out->px = cam[0];
    out->py = cam[1];
    out->pz = cam[2];
    if (cfg->pick == RMCV_AIM_PICK_NEAREST) { /* smallest distance: a distance is +0 or above, or NaN (= +infinity): its bits order as it does */
        const double dk = dist != dist ? __builtin_huge_val() : dist;
        uint64_t u;
        __builtin_memcpy(&u, &dk, 8);
        out->key = u;
    } else {                                  /* greatest timestamp: int64 -> order-preserving uint64, inverted */
        out->key = ~((uint64_t)ts ^ 0x8000000000000000ull);
    }
}

PM_FN void aim_store(rmcv_aim* out, const aim_lane_t* c)
{
    out->track = c->index;
    out->identity = c->identity;
    out->lost_count = c->lost_count;
    out->status = c->status;
    out->pitch = aim_canon(c->pitch);
    out->yaw = aim_canon(c->yaw);
    out->flight_time = aim_canon(c->flight_time);
    out->distance = aim_canon(c->distance);
    out->point[0] = aim_canon(c->px);
    out->point[1] = aim_canon(c->py);
    out->point[2] = aim_canon(c->pz);
}

PM_FN void aim_store_none(rmcv_aim* out)
{
    out->track = -1;
    out->identity = -1;
    out->lost_count = 0;
    out->status = RMCV_AIM_NO_TARGET;
    out->pitch = 0.0;
    out->yaw = 0.0;
    out->flight_time = 0.0;
    out->distance = 0.0;
    out->point[0] = 0.0;
    out->point[1] = 0.0;
    out->point[2] = 0.0;
}

/* one stream: tracks[n] is its current list (n <= 64); on the device `lane` is the caller's lane of a full wavefront */
PM_FN void aim_stream(const rmcv_aim_config* cfg, double tick_frequency, const rmcv_track* tracks, int n, const rmcv_aim_input* in, int64_t now,
                      rmcv_aim* out, int lane)
{
#if defined(__HIP_DEVICE_COMPILE__)
    aim_lane_t c;
    c.key = ~(uint64_t)0;
    c.index = AIM_NO_INDEX;
    if (lane < n) aim_lane(cfg, tick_frequency, &tracks[lane], lane, in, now, &c);
    uint64_t k = c.key;
    int32_t i = c.index;
    for (int m = 32; m >= 1; m >>= 1) { /* all-reduce: every lane ends with the pair that comes first */
        const uint64_t ok = __shfl_xor((unsigned long long)k, m, 64);
        const int32_t oi = __shfl_xor(i, m, 64);
        if (aim_before(ok, oi, k, i)) { k = ok; i = oi; }
    }
    if (i == AIM_NO_INDEX) {
        if (lane == 0) aim_store_none(out);
    } else if (lane == i) {
        aim_store(out, &c);
    }
#else
    aim_lane_t best, c;
    (void)lane;
    best.key = ~(uint64_t)0;
    best.index = AIM_NO_INDEX;
#if defined(AIM_HOST_REVERSED) /* a test build: the lanes in the opposite order (tests/test_aim_cpu.py) */
    for (int j = n - 1; j >= 0; j--) {
#else
    for (int j = 0; j < n; j++) {
#endif
        aim_lane(cfg, tick_frequency, &tracks[j], j, in, now, &c);
        if (aim_before(c.key, c.index, best.key, best.index)) best = c;
    }
    if (best.index == AIM_NO_INDEX) aim_store_none(out);
    else aim_store(out, &best);
#endif
}

/* what rmcv_tracker_set_aim refuses; NULL: fine */
PM_FN const char* aim_check_config(const rmcv_aim_config* c)
{
    if (!aim_finite(c->g) || !aim_finite(c->v0) || !aim_finite(c->height) || !aim_finite((double)c->offset_x) || !aim_finite((double)c->offset_y) ||
        !aim_finite(c->angle_offset) || !aim_finite(c->latency_s))
        return "aim config: every number must be finite";
    if (c->mode == RMCV_COMPENSATE_NI) return "aim config: RMCV_COMPENSATE_NI is not implemented (the reference returns NAN)";
    if (c->mode != RMCV_COMPENSATE_NONE && c->mode != RMCV_COMPENSATE_CLASSIC) return "aim config: mode out of range";
    if (c->height_mode != RMCV_AIM_HEIGHT_FIXED && c->height_mode != RMCV_AIM_HEIGHT_DELTA) return "aim config: height_mode out of range";
    if (c->source != RMCV_AIM_SRC_FILTER && c->source != RMCV_AIM_SRC_MEASUREMENT) return "aim config: source out of range";
    if (c->pick != RMCV_AIM_PICK_WINDOW && c->pick != RMCV_AIM_PICK_NEAREST) return "aim config: pick out of range";
    if (c->lead_iterations < 0 || c->lead_iterations > 4) return "aim config: lead_iterations out of range (0 .. 4)";
    if (c->max_lost < 0) return "aim config: max_lost must not be negative";
    return (const char*)0;
}

/* the default input of a stream: world2camera the identity, motor_angle 0 (17 doubles: the struct has no padding) */
PM_FN void aim_default_input(rmcv_aim_input* in)
{
    for (int i = 0; i < 16; i++) in->world2camera[i] = (i % 5 == 0) ? 1.0 : 0.0;
    in->motor_angle = 0.0;
}

#endif /* RMCV_DEVICE_AIM_H */
