// k_aim.hip -- device-resident aiming: behind a step of the device tracker, one rmcv_aim per camera stream in HBM -- the
// target chosen, led with the filter's velocity over latency and flight time, and the reference's gimbal-error-angle solution on it.
//   rm::DeltaHeight / Distance / ProjectileAngle   src/mobility.cpp:36-82
//   rm::SolveGEA                                   src/mobility.cpp:127-164
// The step itself is device_aim.h, the same source rmcv_aim_step_host and the four host functions run on the CPU.
//
// Mapping (gfx950, wave64).  A few hundred wavefronts of latency-bound scalar fp64: ONE 64-LANE WORKGROUP PER STREAM, lane = track
// (track_cap <= 64).  A lane loads the dozen fields it needs from its rmcv_track (the 2.5 KB record is not staged), runs its dependent chain
// on its own, the pick is a butterfly of __shfl_xor over a (key, index) pair and the lane that won stores the 72-byte record with ordinary
// vector stores.  No LDS, no atomics, no waits between workgroups; nothing is indexed dynamically in registers (no scratch).
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

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

bool tracker_aim_on(const rmcv_tracker* t) { return t->aim_on; }

hipError_t launch_aim(const rmcv_tracker* t, int64_t now, hipStream_t s)
{
    return launch(k_aim, dim3(t->cfg.n_streams), dim3(64), 0, s, t->aim_cfg, t->cfg.tick_frequency, t->b, t->cfg.n_streams, t->cfg.track_cap,
                  (const rmcv_aim_input*)t->aim_inputs, now, t->aims, t->aim_cfgs_on ? t->aim_cfgs : nullptr);
}

} // namespace rmcv

using namespace rmcv;

#define ACHK(t, call, what)                                                        \
    do {                                                                           \
        hipError_t e__ = (call);                                                   \
        if (e__ != hipSuccess) return tracker_fail((t), RMCV_ERR_HIP, what, e__);  \
    } while (0)

static void default_input(rmcv_aim_input* in)
{
    memset(in, 0, sizeof(*in));
    for (int i = 0; i < 4; i++) in->world2camera[i * 5] = 1.0;
}

// the records (zero until the first aim step) and the inputs (the defaults), on first use
static int aim_alloc(rmcv_tracker* t)
{
    if (t->aims) return RMCV_OK;
    const size_t n = (size_t)t->cfg.n_streams;
    rmcv_aim* d_aims = nullptr;
    rmcv_aim_input* d_in = nullptr;
    hipError_t e = hipMalloc((void**)&d_aims, n * sizeof(rmcv_aim));
    if (e == hipSuccess) {
        t->allocs.push_back(d_aims);
        e = hipMalloc((void**)&d_in, n * sizeof(rmcv_aim_input));
    }
    if (e == hipSuccess) {
        t->allocs.push_back(d_in);
        e = hipMemset(d_aims, 0, n * sizeof(rmcv_aim));
    }
    if (e == hipSuccess) {
        std::vector<rmcv_aim_input> def(n);
        for (auto& in : def) default_input(&in);
        e = hipMemcpy(d_in, def.data(), n * sizeof(rmcv_aim_input), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) return tracker_fail(t, e == hipErrorOutOfMemory ? RMCV_ERR_NOMEM : RMCV_ERR_HIP, "allocating the aim records", e);
    t->aim_inputs = d_in;
    t->aims = d_aims;
    return RMCV_OK;
}

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

int rmcv_tracker_set_aim(rmcv_tracker* t, const rmcv_aim_config* cfg)
{
    if (!t) return RMCV_ERR_BAD_ARG;
    if (cfg) { // (the refusals need no device)
        const char* bad = aim_check_config(cfg);
        if (bad) return tracker_fail(t, RMCV_ERR_BAD_ARG, bad);
    }
    hipSetDevice(t->device);
    int rc = tracker_wait_done(t);
    if (rc) return rc;
    if (!cfg) {
        t->aim_on = false;
        return RMCV_OK;
    }
    if ((rc = aim_alloc(t))) return rc;
    t->aim_cfg = *cfg;
    t->aim_on = true;
    return RMCV_OK;
}

int rmcv_tracker_set_aim_configs(rmcv_tracker* t, const rmcv_aim_config* cfgs)
{
    if (!t) return RMCV_ERR_BAD_ARG;
    if (!t->aim_on) return tracker_fail(t, RMCV_ERR_BAD_ARG, "rmcv_tracker_set_aim_configs: aiming is off (rmcv_tracker_set_aim)");
    const size_t n = (size_t)t->cfg.n_streams;
    if (cfgs) { // (the refusals need no device)
        for (size_t f = 0; f < n; f++) {
            const char* bad = aim_check_config(&cfgs[f]);
            if (bad) {
                char msg[200];
                snprintf(msg, sizeof(msg), "rmcv_tracker_set_aim_configs: stream %d: %s", (int)f, bad);
                return tracker_fail(t, RMCV_ERR_BAD_ARG, msg);
            }
        }
    }
    hipSetDevice(t->device);
    const int rc = tracker_wait_done(t);
    if (rc) return rc;
    if (!cfgs) {
        t->aim_cfgs_on = false;
        return RMCV_OK;
    }
    if (!t->aim_cfgs) {
        rmcv_aim_config* d = nullptr;
        const hipError_t e = hipMalloc((void**)&d, n * sizeof(rmcv_aim_config));
        if (e != hipSuccess) return tracker_fail(t, e == hipErrorOutOfMemory ? RMCV_ERR_NOMEM : RMCV_ERR_HIP, "allocating the streams' aim configs", e);
        t->allocs.push_back(d);
        t->aim_cfgs = d;
    }
    ACHK(t, hipMemcpy(t->aim_cfgs, cfgs, n * sizeof(rmcv_aim_config), hipMemcpyHostToDevice), "H2D aim configs");
    t->aim_cfgs_on = true;
    return RMCV_OK;
}

int rmcv_tracker_set_aim_inputs(rmcv_tracker* t, const rmcv_aim_input* inputs)
{
    if (!t) return RMCV_ERR_BAD_ARG;
    hipSetDevice(t->device);
    int rc = tracker_wait_done(t);
    if (rc) return rc;
    if ((rc = aim_alloc(t))) return rc;
    const size_t n = (size_t)t->cfg.n_streams;
    std::vector<rmcv_aim_input> def;
    if (!inputs) {
        def.resize(n);
        for (auto& in : def) default_input(&in);
        inputs = def.data();
    }
    ACHK(t, hipMemcpy(t->aim_inputs, inputs, n * sizeof(rmcv_aim_input), hipMemcpyHostToDevice), "H2D aim inputs");
    return RMCV_OK;
}

int rmcv_tracker_device_aim_inputs(rmcv_tracker* t, void** d_inputs)
{
    if (!t || !d_inputs) return RMCV_ERR_BAD_ARG;
    hipSetDevice(t->device);
    const int rc = aim_alloc(t);
    if (rc) return rc;
    *d_inputs = t->aim_inputs;
    return RMCV_OK;
}

int rmcv_tracker_device_aims(rmcv_tracker* t, void** d_aims)
{
    if (!t || !d_aims) return RMCV_ERR_BAD_ARG;
    hipSetDevice(t->device);
    const int rc = aim_alloc(t);
    if (rc) return rc;
    *d_aims = t->aims;
    return RMCV_OK;
}

int rmcv_tracker_aim(rmcv_tracker* t, int64_t now, void* hip_stream)
{
    if (!t) return RMCV_ERR_BAD_ARG;
    if (!t->aim_on) return tracker_fail(t, RMCV_ERR_BAD_ARG, "rmcv_tracker_aim: aiming is off (rmcv_tracker_set_aim)");
    hipSetDevice(t->device);
    hipStream_t s = (hipStream_t)hip_stream;
    ACHK(t, tracker_order_begin(t, s), "aim: wait for the tracker's previous step");
    ACHK(t, launch_aim(t, now, s), "k_aim");
    ACHK(t, tracker_order_end(t, s), "aim: record the step");
    return RMCV_OK;
}

int rmcv_tracker_get_aims(rmcv_tracker* t, rmcv_aim* out, int cap)
{
    if (!t || cap < 0 || (cap > 0 && !out)) return RMCV_ERR_BAD_ARG;
    hipSetDevice(t->device);
    const int rc = tracker_wait_done(t);
    if (rc) return rc;
    const size_t n = (size_t)std::min(cap, t->cfg.n_streams);
    if (!n) return RMCV_OK;
    if (!t->aims) memset(out, 0, n * sizeof(rmcv_aim)); // (never aimed: what the records would hold)
    else ACHK(t, hipMemcpy(out, t->aims, n * sizeof(rmcv_aim), hipMemcpyDeviceToHost), "D2H aims");
    return RMCV_OK;
}

int rmcv_tracker_put(rmcv_tracker* t, int stream, const rmcv_track* tracks, int n, const float* last_vertices)
{
    if (!t) return RMCV_ERR_BAD_ARG;
    if (stream < 0 || stream >= t->cfg.n_streams) return tracker_fail(t, RMCV_ERR_BAD_ARG, "no such stream");
    if (n < 0 || (n > 0 && !tracks)) return tracker_fail(t, RMCV_ERR_BAD_ARG, "rmcv_tracker_put: bad list");
    if (n > t->cfg.track_cap) return tracker_fail(t, RMCV_ERR_CAPACITY, "rmcv_tracker_put: more tracks than track_cap");
    hipSetDevice(t->device);
    const int rc = tracker_wait_done(t);
    if (rc) return rc;
    int32_t sel = 0, count = n;
    ACHK(t, hipMemcpy(&sel, t->b.sel + stream, 4, hipMemcpyDeviceToHost), "D2H current list");
    const size_t at = ((size_t)(sel & 1) * t->cfg.n_streams + stream) * t->cfg.track_cap;
    if (n) {
        ACHK(t, hipMemcpy(t->b.tracks + at, tracks, (size_t)n * sizeof(rmcv_track), hipMemcpyHostToDevice), "H2D tracks");
        if (last_vertices) ACHK(t, hipMemcpy(t->b.side + at * 8, last_vertices, (size_t)n * 8 * sizeof(float), hipMemcpyHostToDevice), "H2D side records");
        else ACHK(t, hipMemset(t->b.side + at * 8, 0, (size_t)n * 8 * sizeof(float)), "side records");
    }
    ACHK(t, hipMemcpy(t->b.n_tracking + stream, &count, 4, hipMemcpyHostToDevice), "H2D count");
    return RMCV_OK;
}

int rmcv_aim_step_host(const rmcv_aim_config* cfg, double tick_frequency, const rmcv_track* tracks, int n, const rmcv_aim_input* input, int64_t now,
                       rmcv_aim* out)
{
    if (!cfg || !out || n < 0 || n > RMCV_TRACKER_MAX_CAP || (n > 0 && !tracks)) return RMCV_ERR_BAD_ARG;
    if (aim_check_config(cfg) || !std::isfinite(tick_frequency) || !(tick_frequency > 0)) return RMCV_ERR_BAD_ARG;
    rmcv_aim_input def;
    if (!input) {
        default_input(&def);
        input = &def;
    }
    aim_stream(cfg, tick_frequency, tracks, n, input, now, out, 0);
    return RMCV_OK;
}

} // extern "C"
