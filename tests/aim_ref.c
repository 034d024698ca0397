/*
 * aim_ref.c -- TEST INFRASTRUCTURE: the reference of the aiming tests.  A plain-C restatement of the reference's
 *   rm::DeltaHeight / Distance / ProjectileAngle   src/mobility.cpp:36-82
 *   rm::SolveGEA                                   src/mobility.cpp:127-164
 * on arrays instead of cv::Mat, and of the aim step of include/rmcv_abi.h: a straight loop over the tracks (candidate, source, lead,
 * solution), then a pick loop.  Written on its own from the reference and the contract; it shares no code with
 * rmcv_amd/csrc/device_aim.h.  The transcendentals are pinned_math.h's (the parity contract, as in oracle/rmcv_oracle.c);
 * -DAIM_REF_LIBM takes the host libm's instead (the second opinion).
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../include/rmcv_abi.h"
#include "../rmcv_amd/csrc/pinned_math.h"

#ifdef AIM_REF_LIBM
#define R_ATAN atan
#define R_ATAN2 atan2
#define R_COS cos
#define R_TAN tan
#else
#define R_ATAN pm_atan
#define R_ATAN2 pm_atan2
#define R_COS pm_cos
#define R_TAN pm_tan
#endif

#define REF_PI 3.1415926535897932384626433832795

/* how often a comparison inside ProjectileAngle was decided by a hair since the last reset: delta next to 0, or |x1| next to |x2| --
 * two builds with different transcendentals may take different branches there */
static int fragile_count;
void aim_ref_fragile_reset(void) { fragile_count = 0; }
int aim_ref_fragile(void) { return fragile_count; }

/* a NaN that leaves is the quiet NaN 0x7FF8000000000000 (include/rmcv_abi.h): a computed NaN's sign and payload are the machine's */
static double quiet(double v)
{
    const uint64_t q = 0x7FF8000000000000ull;
    if (isnan(v)) memcpy(&v, &q, 8);
    return v;
}

static int64_t ulp_gap(double a, double b)
{
    int64_t x, y;
    memcpy(&x, &a, 8);
    memcpy(&y, &b, 8);
    return x > y ? x - y : y - x;
}

/* abs(double) as the reference's translation unit resolves it: fabs, or (bit 0 of `overloads`) int abs(int) */
static double ref_abs(double v, int overloads)
{
    if ((overloads & 1) == 0) return fabs(v);
    if (isnan(v)) return 0;                    /* the contract's choice for the undefined conversion */
    if (v >= 2147483647.0) v = 2147483647.0;   /* saturating */
    if (v <= -2147483647.0) v = -2147483647.0;
    return (double)abs((int)v);
}

double aim_ref_projectile_angle(double v0, double g, double d, double h, int overloads)
{
    double d2 = d * d, v2 = v0 * v0;            /* pow(., 2.0), correctly rounded */
    double a = (g * d2) / (2.0 * v2);
    double b = d;
    double c = a - h;
    double b2 = b * b;
    double delta = b2 - (4 * a * c);
    if (b2 > 0 && fabs(delta) <= b2 * 0x1p-44) fragile_count++;   /* (d = 0 is delta = 0 in every build) */
    if (delta > 0) {
        double root = sqrt(delta);
        double x1 = R_ATAN(((-1 * b) + root) / (2 * a));
        double x2 = R_ATAN(((-1 * b) - root) / (2 * a));
        double m1 = ref_abs(x1, overloads), m2 = ref_abs(x2, overloads);
        if (!(overloads & 1) && ulp_gap(m1, m2) <= 4) fragile_count++;
        return quiet(m1 < m2 ? x1 : x2);
    }
    if (delta == 0) return quiet(R_ATAN((-1) * (b / 2 * a)));
    return quiet(NAN);
}

double aim_ref_delta_height(const double* tvec, double motor_angle, float offset_y, double angle_offset)
{
    double h = tvec[1] - offset_y;
    double d = tvec[2];
    double dPitch = -R_ATAN2(h, d) + (motor_angle - angle_offset);
    return quiet(d * R_TAN(dPitch));
}

double aim_ref_distance(const double* tvec)
{
    double xx = tvec[0] * tvec[0], yy = tvec[1] * tvec[1], zz = tvec[2] * tvec[2];
    return quiet(sqrt(xx + yy + zz));
}

double aim_ref_solve_gea(const double* tvec, double g, double v0, double h, float offset_x, float offset_y, double angle_offset, int mode,
                         int overloads, double* gea)
{
    double p = 0, t = 0, d = tvec[2] / 100.0, y = R_ATAN2(tvec[0] - offset_x, tvec[2]) * 180.0 / REF_PI;
    switch (mode) {
    case RMCV_COMPENSATE_NONE:
        p = -(R_ATAN2(tvec[1] - offset_y, tvec[2]) * 180.0 / REF_PI);
        t = d / v0;
        break;
    case RMCV_COMPENSATE_CLASSIC: {
        double normalAngle, centerAngle, targetAngle;
        normalAngle = R_ATAN2(h / 100.0, d) * 180.0 / REF_PI;
        centerAngle = -R_ATAN2(tvec[1] - offset_y, tvec[2]) * 180.0 / REF_PI;
        targetAngle = aim_ref_projectile_angle(v0, g, d, h / 100.0, overloads) * 180.0 / REF_PI;
        p = (centerAngle - normalAngle + angle_offset * 180.0 / REF_PI) + targetAngle;
        t = d / ref_abs(v0 * R_COS(targetAngle), overloads);
        break;
    }
    case RMCV_COMPENSATE_NI:
        return quiet(NAN);
    }
    gea[0] = quiet(p);
    gea[1] = quiet(y);
    return quiet(t);
}

/* n independent solutions: out[k] = {time, pitch, yaw}, fragile[k] = 1 when a comparison of solution k was decided by a hair */
void aim_ref_solve_n(int n, const double* tvecs, const double* v0, const double* h, double g, int mode, int overloads, double* out, uint8_t* fragile)
{
    for (int k = 0; k < n; k++) {
        double gea[2] = {NAN, NAN};
        int before = fragile_count;
        out[3 * k] = aim_ref_solve_gea(tvecs + 3 * k, g, v0[k], h[k], 0.0f, 0.0f, 0.0, mode, overloads, gea);
        out[3 * k + 1] = gea[0];
        out[3 * k + 2] = gea[1];
        fragile[k] = fragile_count != before;
    }
}

/* ---- the aim step of one stream ---- */
typedef struct {
    int    candidate;
    double pitch, yaw, time, distance, cam[3];
    int    status;
} ref_solution;

static void to_camera(const double* W, const double* q, double* cam)
{
    for (int r = 0; r < 3; r++) {
        double s = W[4 * r] * q[0] + W[4 * r + 1] * q[1];
        s = s + W[4 * r + 2] * q[2];
        s = s + W[4 * r + 3] * 1.0;
        cam[r] = s;
    }
}

static int allowed(uint32_t mask, int32_t identity)
{
    int bit = (identity >= 0 && identity < 31) ? identity : 31;
    return (int)((mask >> bit) & 1u);
}

int aim_ref_step(const rmcv_aim_config* cfg, double tick_frequency, const rmcv_track* tracks, int n, const rmcv_aim_input* input, int64_t now,
                 rmcv_aim* out)
{
    static const double eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    const double* W = input ? input->world2camera : eye;
    const double motor = input ? input->motor_angle : 0.0;
    ref_solution sol[64];
    if (n < 0 || n > 64) return -1;
    for (int j = 0; j < n; j++) {
        const rmcv_track* tr = &tracks[j];
        ref_solution* s = &sol[j];
        double p[3], v[3] = {0, 0, 0}, q[3], gea[2] = {0, 0}, dt, t = 0, h;
        s->candidate = tr->lost_count <= cfg->max_lost && allowed(cfg->identity_mask, tr->identity);
        if (!s->candidate) continue;
        if (!tr->initialized) {
            for (int i = 0; i < 3; i++) p[i] = tr->position[i];
        } else if (cfg->source == RMCV_AIM_SRC_MEASUREMENT) {
            for (int i = 0; i < 3; i++) { p[i] = tr->measurement[i]; v[i] = tr->measurement[3 + i]; }
        } else {
            for (int i = 0; i < 3; i++) { p[i] = tr->state_post[i]; v[i] = tr->state_post[3 + i]; }
        }
        dt = (double)(now - tr->timestamp) / tick_frequency + cfg->latency_s;
        for (int pass = 0; pass <= cfg->lead_iterations; pass++) {
            double ahead = dt;
            if (pass > 0) {
                if (!isfinite(t)) break;
                ahead = dt + t;
            }
            for (int i = 0; i < 3; i++) q[i] = p[i] + v[i] * ahead;
            to_camera(W, q, s->cam);
            h = cfg->height_mode == RMCV_AIM_HEIGHT_DELTA ? aim_ref_delta_height(s->cam, motor, cfg->offset_y, cfg->angle_offset) : cfg->height;
            t = aim_ref_solve_gea(s->cam, cfg->g, cfg->v0, h, cfg->offset_x, cfg->offset_y, cfg->angle_offset, cfg->mode, cfg->overloads, gea);
        }
        s->pitch = gea[0];
        s->yaw = gea[1];
        s->time = t;
        s->distance = aim_ref_distance(s->cam);
        s->status = (isfinite(s->pitch) && isfinite(t)) ? 0 : RMCV_AIM_NO_SOLUTION;
    }
    int best = -1;
    for (int j = 0; j < n; j++) {
        if (!sol[j].candidate) continue;
        if (best < 0) { best = j; continue; }
        if (cfg->pick == RMCV_AIM_PICK_NEAREST) {
            double dj = isnan(sol[j].distance) ? INFINITY : sol[j].distance, db = isnan(sol[best].distance) ? INFINITY : sol[best].distance;
            if (dj < db) best = j;
        } else if (tracks[j].timestamp > tracks[best].timestamp) {
            best = j;
        }
    }
    memset(out, 0, sizeof(*out));
    if (best < 0) {
        out->track = -1;
        out->identity = -1;
        out->status = RMCV_AIM_NO_TARGET;
        return 0;
    }
    out->track = best;
    out->identity = tracks[best].identity;
    out->lost_count = tracks[best].lost_count;
    out->status = sol[best].status;
    out->pitch = sol[best].pitch;
    out->yaw = sol[best].yaw;
    out->flight_time = sol[best].time;
    out->distance = sol[best].distance;
    for (int i = 0; i < 3; i++) out->point[i] = quiet(sol[best].cam[i]);
    return 0;
}
