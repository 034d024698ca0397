// k_aim.hip -- device-resident aiming: behind a step of the device tracker, one rmcv_aim per camera stream in HBM -- the
// target chosen, led with the filter's velocity over latency and flight time, and the reference's gimbal-error-angle solution on it.
//   rm::DeltaHeight / Distance / ProjectileAngle   src/mobility.cpp:36-82
//   rm::SolveGEA                                   src/mobility.cpp:127-164
// The step itself is device_aim.h, the same source rmcv_aim_step_host and the four host functions run on the CPU.  The tracker's aim
// tables, their setters and getters and rmcv_tracker_aim: rmcv_tracker.hip; the launcher takes the view of them (tracker_plan.h).
//
// Mapping (gfx950, wave64).  A few hundred wavefronts of latency-bound scalar fp64: ONE 64-LANE WORKGROUP PER STREAM, lane = track
// (track_cap <= 64).  A lane loads the dozen fields it needs from its rmcv_track (the 2.5 KB record is not staged), runs its dependent chain
// on its own, the pick is a butterfly of __shfl_xor over a (key, index) pair and the lane that won stores the 72-byte record with ordinary
// vector stores.  No LDS, no atomics, no waits between workgroups; nothing is indexed dynamically in registers (no scratch).
#include <math.h>
#include <string.h>

#include "rmcv_internal.h"
#include "device_aim.h"
#include "device_attitude.h"

namespace rmcv {

__global__ __launch_bounds__(64) void k_aim(rmcv_aim_config cfg, double tick_frequency, TrackerBufs tb, int n_streams, int cap,
                                            const rmcv_aim_input* __restrict__ inputs, int64_t now, rmcv_aim* __restrict__ aims,
                                            const rmcv_aim_config* __restrict__ stream_cfgs /* nullable: [n_streams], the streams' own configs */)
{
    const int f = blockIdx.x, lane = threadIdx.x;
    if (f >= n_streams) return;
    if (stream_cfgs) cfg = stream_cfgs[f]; // the stream is the workgroup: a uniform (scalar) load of one entry
    const int sel = tb.sel[f] & 1;
    int nt = tb.n_tracking[f];
    nt = nt < 0 ? 0 : (nt > cap ? cap : nt);
    const rmcv_track* cur = tb.tracks + ((size_t)sel * n_streams + f) * cap;
    aim_stream(&cfg, tick_frequency, cur, nt, &inputs[f], now, &aims[f], lane);
}

// v: the tracker's (tracker_plan.h); its aim tables are there while aiming is on
hipError_t launch_aim(const TrackerView& v, int64_t now, hipStream_t s)
{
    return launch(k_aim, dim3(v.cfg.n_streams), dim3(64), 0, s, v.aim_cfg, v.cfg.tick_frequency, v.b, v.cfg.n_streams, v.cfg.track_cap,
                  (const rmcv_aim_input*)v.aim_inputs, now, v.aims, v.aim_cfgs);
}

} // namespace rmcv

using namespace rmcv;

extern "C" {

// (every NaN that leaves is the quiet NaN: aim_canon)
double rmcv_projectile_angle(double v0, double g, double d, double h) { return aim_canon(aim_projectile_angle(v0, g, d, h, 0)); }

double rmcv_solve_gea(const double tvec[3], double g, double v0, double h, float offset_x, float offset_y, double angle_offset, int mode,
                      double gea_out[2])
{
    if (!tvec || !gea_out) return aim_nan();
    const double t = aim_solve_gea(tvec, g, v0, h, offset_x, offset_y, angle_offset, mode, 0, &gea_out[0], &gea_out[1]);
    gea_out[0] = aim_canon(gea_out[0]);
    gea_out[1] = aim_canon(gea_out[1]);
    return aim_canon(t);
}

double rmcv_delta_height(const double tvec[3], double motor_angle, float offset_y, double angle_offset)
{
    if (!tvec) return aim_nan();
    return aim_canon(aim_delta_height(tvec, motor_angle, offset_y, angle_offset));
}

double rmcv_distance(const double tvec[3])
{
    if (!tvec) return aim_nan();
    return aim_canon(aim_distance(tvec));
}

int rmcv_rigid_inverse(const double m[16], double out[16])
{
    if (!m || !out) return RMCV_ERR_BAD_ARG;
    double r[16];
    att_rigid_inverse(m, r); // (the attitude step's: device_attitude.h)
    memcpy(out, r, sizeof(r));
    return RMCV_OK;
}

void rmcv_default_aim_config(rmcv_aim_config* c)
{
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->g = 9.8;
    c->v0 = 15.0;
    c->mode = RMCV_COMPENSATE_NONE; // include/mobility.h:97
    c->lead_iterations = 1;
    c->max_lost = 25;               // what the tracking thread keeps (executable/main.cpp:78)
    c->identity_mask = 0xFFFFFFFFu;
}

int rmcv_aim_step_host(const rmcv_aim_config* cfg, double tick_frequency, const rmcv_track* tracks, int n, const rmcv_aim_input* input, int64_t now,
                       rmcv_aim* out)
{
    if (!cfg || !out || n < 0 || n > RMCV_TRACKER_MAX_CAP || (n > 0 && !tracks)) return RMCV_ERR_BAD_ARG;
    if (aim_check_config(cfg) || !std::isfinite(tick_frequency) || !(tick_frequency > 0)) return RMCV_ERR_BAD_ARG;
    rmcv_aim_input def;
    if (!input) {
        aim_default_input(&def);
        input = &def;
    }
    aim_stream(cfg, tick_frequency, tracks, n, input, now, out, 0);
    return RMCV_OK;
}

} // extern "C"
