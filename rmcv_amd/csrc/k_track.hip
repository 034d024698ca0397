// k_track.hip -- the device-resident tracker: the tracking state of a batch of camera streams in HBM, stepped behind a
// batch without the host, and the next batch's window origins written from it.
//   the tracking thread        /root/reference/executable/main.cpp:57-88
//   rm::armour::reset / update /root/reference/src/core.cpp:51-122
//   rm::utils::GetROI          /root/reference/src/core.cpp:218-263
// The step itself is device_track.h, the same source rmcv_tracker_step_host runs on the CPU.
//
// Mapping (gfx950, wave64).  The work is latency-bound: per stream a tiny sequential association, then one dependent chain of 6x6 fp64
// operations per track that matched or coasts.  ONE WORKGROUP PER STREAM, 8 wavefronts: lane 0 walks the association into a plan in LDS
// (indices only: that walk is the dry run), the wavefronts then take the slots of the list the pass leaves behind, one wavefront per
// track -- the record and every matrix in LDS, one matrix element per lane (36 of 64 busy), scalars computed by every lane from LDS so
// that control flow is uniform -- and lane 0 commits: length, the current/next flip, the target rule, the next window's origin (ordinary
// vector stores).  No inter-workgroup waits; nothing is indexed dynamically in registers (no scratch).  256 streams are 256 workgroups:
// one per CU.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "rmcv_internal.h"
#include "device_track.h"

namespace rmcv {

static constexpr int TRACK_WAVES = 8;

static trk_cfg step_cfg(const rmcv_tracker_config& c)
{
    trk_cfg k;
    k.track_cap = c.track_cap;
    k.frame_w = c.frame_w;
    k.frame_h = c.frame_h;
    k.win_w = c.win_w;
    k.win_h = c.win_h;
    k.roi_scale_w = c.roi_scale_w;
    k.roi_scale_h = c.roi_scale_h;
    k.process_noise = c.process_noise;
    k.measurement_noise = c.measurement_noise;
    k.error = c.error;
    k.tick_frequency = c.tick_frequency;
    return k;
}

__global__ __launch_bounds__(TRACK_WAVES * 64) void k_track(trk_cfg cfg, TrackerBufs tb, int n_streams, const rmcv_armour* __restrict__ armours,
                                                            const int32_t* __restrict__ n_armours, const int32_t* __restrict__ identity,
                                                            const double* __restrict__ poses, int max_armours,
                                                            const rmcv_point* __restrict__ win_eff, int64_t timestamp)
{
    __shared__ trk_plan_t plan;
    __shared__ trk_ws ws[TRACK_WAVES];
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (f >= n_streams) return;
    const int cap = cfg.track_cap;
    const int sel = tb.sel[f] & 1;
    int nt = tb.n_tracking[f];
    nt = nt < 0 ? 0 : (nt > cap ? cap : nt);
    const size_t cur_at = ((size_t)sel * n_streams + f) * cap, nxt_at = ((size_t)(sel ^ 1) * n_streams + f) * cap;
    const rmcv_track* cur = tb.tracks + cur_at;
    rmcv_track* nxt = tb.tracks + nxt_at;
    const float* side_cur = tb.side + cur_at * 8;
    float* side_nxt = tb.side + nxt_at * 8;
    trk_obs ob;
    ob.armours = armours + (size_t)f * max_armours;
    ob.identity = identity ? identity + (size_t)f * max_armours : nullptr;
    ob.pos = poses ? poses + (size_t)f * max_armours * 9 + 6 : nullptr;
    ob.pos_stride = 9;
    const int na = n_armours[f];
    ob.n = na < 0 ? 0 : (na > max_armours ? max_armours : na);
    ob.fx = win_eff ? (float)win_eff[f].x : 0.0f;
    ob.fy = win_eff ? (float)win_eff[f].y : 0.0f;
    ob.timestamp = timestamp;
    if (tid == 0) trk_plan(&plan, cur, nt, &ob, &cfg);
    __syncthreads();
    const int apply = plan.apply, n_out = plan.n_src + plan.n_new;
    if (apply)
        for (int j = wave; j < n_out; j += TRACK_WAVES) trk_apply_slot(&ws[wave], &plan, j, cur, side_cur, nxt, side_nxt, &ob, &cfg, lane);
    __syncthreads();
    if (tid == 0) {
        if (plan.ovf) tb.status[f] |= RMCV_TRACKER_OVF;
        if (apply) {
            tb.n_tracking[f] = n_out;
            tb.sel[f] = sel ^ 1;
        }
        if (!plan.ovf) trk_next_window(apply ? nxt : cur, apply ? side_nxt : side_cur, apply ? n_out : nt, &cfg, &tb.origins[f]);
    }
}

hipError_t launch_track(const rmcv_tracker_config& cfg, const TrackerBufs& tb, const Bufs& b, const Limits& lim, bool identity, bool pose,
                        const rmcv_point* win_eff, int64_t timestamp, hipStream_t s)
{
    return launch(k_track, dim3(cfg.n_streams), dim3(TRACK_WAVES * 64), 0, s, step_cfg(cfg), tb, cfg.n_streams, (const rmcv_armour*)b.armours,
                  (const int32_t*)b.n_armours, (const int32_t*)(identity ? b.identity : nullptr), (const double*)(pose ? b.poses : nullptr),
                  lim.max_armours, win_eff, timestamp);
}

} // namespace rmcv

using namespace rmcv;

// (struct rmcv_tracker: rmcv_internal.h)

static int tfail(rmcv_tracker* t, int code, const char* what, hipError_t e = hipSuccess)
{
    if (t) {
        if (e != hipSuccess) snprintf(t->err, sizeof(t->err), "%s: %s", what, hipGetErrorString(e));
        else snprintf(t->err, sizeof(t->err), "%s", what);
    }
    if (e != hipSuccess) (void)hipGetLastError();
    return code;
}
#define TCHK(t, call, what)                                             \
    do {                                                                \
        hipError_t e__ = (call);                                        \
        if (e__ != hipSuccess) return tfail((t), RMCV_ERR_HIP, what, e__); \
    } while (0)

// the step in flight, with the library's usual deadline (no entry point parks its caller in the runtime without a bound)
static int tracker_wait(rmcv_tracker* t)
{
    if (!t->step_pending) return RMCV_OK;
    hipError_t e = hipSuccess;
    const int rc = wait_event_deadline(t->ev_step, 5000, &e);
    if (rc < 0) return tfail(t, RMCV_ERR_HIP, "waiting for the tracker's last step", e);
    if (rc > 0) return tfail(t, RMCV_ERR_TIMEOUT, "the tracker's last step has not finished after 5000 ms");
    t->step_pending = false;
    return RMCV_OK;
}

namespace rmcv {
int tracker_wait_done(rmcv_tracker* t) { return tracker_wait(t); }
int tracker_fail(rmcv_tracker* t, int code, const char* what, hipError_t e) { return tfail(t, code, what, e); }
const rmcv_tracker_config& tracker_config(const rmcv_tracker* t) { return t->cfg; }
const TrackerBufs& tracker_bufs(const rmcv_tracker* t) { return t->b; }
int tracker_device(const rmcv_tracker* t) { return t->device; }
hipError_t tracker_order_begin(rmcv_tracker* t, hipStream_t s)
{
    if (t->step_pending && t->last_stream != s) return hipStreamWaitEvent(s, t->ev_step, 0);
    return hipSuccess;
}
hipError_t tracker_order_end(rmcv_tracker* t, hipStream_t s)
{
    t->last_stream = s;
    t->step_pending = true;
    return hipEventRecord(t->ev_step, s);
}
hipError_t tracker_wait_on(rmcv_tracker* t, hipStream_t s)
{
    if (t->step_pending && t->last_stream != s) return hipStreamWaitEvent(s, t->ev_step, 0);
    return hipSuccess;
}
} // namespace rmcv

static const char* check_config(const rmcv_tracker_config& c, bool with_streams)
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

extern "C" {

void rmcv_default_tracker_config(rmcv_tracker_config* c)
{
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->n_streams = 256;
    c->track_cap = 64;
    c->process_noise = 5e-5; // executable/main.cpp:195
    c->measurement_noise = 0.5;
    c->error = 0.05;
    c->tick_frequency = 1e9;  // cv::getTickFrequency() on Linux
    c->roi_scale_w = c->roi_scale_h = 1.0f;
    c->frame_w = 1280;
    c->frame_h = 1024;
}

int rmcv_tracker_create(int device, const rmcv_tracker_config* cfg, rmcv_tracker** out)
{
    if (!out) return RMCV_ERR_BAD_ARG;
    *out = nullptr;
    rmcv_tracker_config c;
    if (cfg) c = *cfg;
    else rmcv_default_tracker_config(&c);
    if (check_config(c, true)) return RMCV_ERR_BAD_ARG;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) {
        (void)hipGetLastError();
        return RMCV_ERR_NO_DEVICE;
    }
    if (hipSetDevice(device) != hipSuccess) return RMCV_ERR_NO_DEVICE;
    rmcv_tracker* t = new rmcv_tracker();
    t->device = device;
    t->cfg = c;
    const size_t slots = (size_t)2 * c.n_streams * c.track_cap;
    struct { void** p; size_t bytes; } want[] = {
        {(void**)&t->b.tracks, slots * sizeof(rmcv_track)},      {(void**)&t->b.side, slots * 8 * sizeof(float)},
        {(void**)&t->b.sel, (size_t)c.n_streams * 4},            {(void**)&t->b.n_tracking, (size_t)c.n_streams * 4},
        {(void**)&t->b.status, (size_t)c.n_streams * 4},         {(void**)&t->b.origins, (size_t)c.n_streams * sizeof(rmcv_point)},
        {(void**)&t->b.camps, (size_t)c.n_streams * 4},          {(void**)&t->b.lower_bounds, (size_t)c.n_streams * 4},
    };
    hipError_t e = hipEventCreateWithFlags(&t->ev_step, hipEventDisableTiming);
    for (auto& w : want) {
        if (e != hipSuccess) break;
        e = hipMalloc(w.p, w.bytes);
        if (e == hipSuccess) {
            t->allocs.push_back(*w.p);
            e = hipMemset(*w.p, 0, w.bytes);
        }
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        rmcv_tracker_destroy(t);
        return e == hipErrorOutOfMemory ? RMCV_ERR_NOMEM : RMCV_ERR_HIP;
    }
    *out = t;
    return RMCV_OK;
}

void rmcv_tracker_destroy(rmcv_tracker* t)
{
    if (!t) return;
    hipSetDevice(t->device);
    const bool done = tracker_wait(t) == RMCV_OK;
    if (done) // (a step that has still not finished keeps its memory: leaked rather than freed under a kernel, as rmcv_ctx_destroy does)
        for (void* p : t->allocs) (void)hipFree(p);
    if (t->ev_step && done) (void)hipEventDestroy(t->ev_step);
    delete t;
}

const char* rmcv_tracker_last_error(const rmcv_tracker* t) { return t ? t->err : "null tracker"; }

int rmcv_tracker_reset(rmcv_tracker* t)
{
    if (!t) return RMCV_ERR_BAD_ARG;
    hipSetDevice(t->device);
    const int rc = tracker_wait(t);
    if (rc) return rc;
    const size_t n = (size_t)t->cfg.n_streams * 4;
    TCHK(t, hipMemset(t->b.n_tracking, 0, n), "reset");
    TCHK(t, hipMemset(t->b.status, 0, n), "reset");
    TCHK(t, hipMemset(t->b.sel, 0, n), "reset");
    return RMCV_OK;
}

int rmcv_tracker_set_origins(rmcv_tracker* t, const rmcv_point* origins)
{
    if (!t) return RMCV_ERR_BAD_ARG;
    if (!origins) return tfail(t, RMCV_ERR_BAD_ARG, "null origins");
    hipSetDevice(t->device);
    const int rc = tracker_wait(t);
    if (rc) return rc;
    TCHK(t, hipMemcpy(t->b.origins, origins, (size_t)t->cfg.n_streams * sizeof(rmcv_point), hipMemcpyHostToDevice), "H2D origins");
    return RMCV_OK;
}

int rmcv_tracker_device_origins(rmcv_tracker* t, void** d_origins)
{
    if (!t || !d_origins) return RMCV_ERR_BAD_ARG;
    *d_origins = t->b.origins;
    return RMCV_OK;
}

int rmcv_tracker_set_camps(rmcv_tracker* t, const int32_t* camps, const int32_t* lower_bounds)
{
    if (!t) return RMCV_ERR_BAD_ARG;
    hipSetDevice(t->device);
    const int rc = tracker_wait(t); // (the step in flight belongs to a batch whose pixel pass may still read the tables)
    if (rc) return rc;
    if (!camps) { // off: tracked submits take rmcv_params::camp and ::lower_bound again
        t->camps_on = t->lower_bounds_on = false;
        return RMCV_OK;
    }
    TCHK(t, hipMemcpy(t->b.camps, camps, (size_t)t->cfg.n_streams * 4, hipMemcpyHostToDevice), "H2D camps");
    if (lower_bounds) TCHK(t, hipMemcpy(t->b.lower_bounds, lower_bounds, (size_t)t->cfg.n_streams * 4, hipMemcpyHostToDevice), "H2D lower bounds");
    t->camps_on = true;
    t->lower_bounds_on = lower_bounds != nullptr;
    return RMCV_OK;
}

int rmcv_tracker_device_camps(rmcv_tracker* t, void** d_camps, void** d_lower_bounds)
{
    if (!t) return RMCV_ERR_BAD_ARG;
    if (d_camps) *d_camps = t->b.camps;
    if (d_lower_bounds) *d_lower_bounds = t->b.lower_bounds;
    return RMCV_OK;
}

int rmcv_tracker_counts(rmcv_tracker* t, int32_t* n_tracking, int32_t* status, int cap)
{
    if (!t || cap < 0) return RMCV_ERR_BAD_ARG;
    hipSetDevice(t->device);
    const int rc = tracker_wait(t);
    if (rc) return rc;
    const size_t n = (size_t)std::min(cap, t->cfg.n_streams) * 4;
    if (n_tracking && n) TCHK(t, hipMemcpy(n_tracking, t->b.n_tracking, n, hipMemcpyDeviceToHost), "D2H counts");
    if (status && n) TCHK(t, hipMemcpy(status, t->b.status, n, hipMemcpyDeviceToHost), "D2H status");
    return RMCV_OK;
}

int rmcv_tracker_get(rmcv_tracker* t, int stream, rmcv_track* tracks_out, int cap, int32_t* n_out, float* last_vertices_out, rmcv_point* origin_out)
{
    if (!t || cap < 0) return RMCV_ERR_BAD_ARG;
    if (stream < 0 || stream >= t->cfg.n_streams) return tfail(t, RMCV_ERR_BAD_ARG, "no such stream");
    hipSetDevice(t->device);
    const int rc = tracker_wait(t);
    if (rc) return rc;
    int32_t n = 0, sel = 0;
    TCHK(t, hipMemcpy(&n, t->b.n_tracking + stream, 4, hipMemcpyDeviceToHost), "D2H count");
    TCHK(t, hipMemcpy(&sel, t->b.sel + stream, 4, hipMemcpyDeviceToHost), "D2H current list");
    if (n_out) *n_out = n;
    if (origin_out) TCHK(t, hipMemcpy(origin_out, t->b.origins + stream, sizeof(rmcv_point), hipMemcpyDeviceToHost), "D2H origin");
    if (n > cap && (tracks_out || last_vertices_out)) return tfail(t, RMCV_ERR_CAPACITY, "output capacity exceeded");
    const size_t at = ((size_t)(sel & 1) * t->cfg.n_streams + stream) * t->cfg.track_cap;
    if (tracks_out && n) TCHK(t, hipMemcpy(tracks_out, t->b.tracks + at, (size_t)n * sizeof(rmcv_track), hipMemcpyDeviceToHost), "D2H tracks");
    if (last_vertices_out && n) TCHK(t, hipMemcpy(last_vertices_out, t->b.side + at * 8, (size_t)n * 8 * sizeof(float), hipMemcpyDeviceToHost), "D2H side records");
    return RMCV_OK;
}

int rmcv_tracker_step_host(const rmcv_tracker_config* cfg, rmcv_track* tracks, float* last_vertices, int32_t* n_tracking, int32_t* status,
                           rmcv_point* origin, const rmcv_armour* armours, int n_obs, const int32_t* identities, const double* positions,
                           int x_eff, int y_eff, int64_t timestamp)
{
    if (!cfg || !tracks || !last_vertices || !n_tracking || !status || !origin || n_obs < 0 || (n_obs > 0 && !armours)) return RMCV_ERR_BAD_ARG;
    if (check_config(*cfg, false) || *n_tracking < 0 || *n_tracking > cfg->track_cap) return RMCV_ERR_BAD_ARG;
    const trk_cfg k = step_cfg(*cfg);
    trk_obs ob;
    ob.armours = armours;
    ob.identity = identities;
    ob.pos = positions;
    ob.pos_stride = 3;
    ob.n = n_obs;
    ob.fx = (float)x_eff;
    ob.fy = (float)y_eff;
    ob.timestamp = timestamp;
    std::vector<trk_plan_t> plan(1);
    trk_plan(&plan[0], tracks, *n_tracking, &ob, &k);
    const trk_plan_t& pl = plan[0];
    if (pl.ovf) {
        *status |= RMCV_TRACKER_OVF;
        return RMCV_OK;
    }
    if (pl.apply) {
        const int n_out = pl.n_src + pl.n_new;
        std::vector<rmcv_track> nxt((size_t)n_out);
        std::vector<float> side_nxt((size_t)n_out * 8);
        std::vector<trk_ws> ws(1);
        for (int j = 0; j < n_out; j++) trk_apply_slot(&ws[0], &pl, j, tracks, last_vertices, nxt.data(), side_nxt.data(), &ob, &k, 0);
        memcpy(tracks, nxt.data(), (size_t)n_out * sizeof(rmcv_track));
        memcpy(last_vertices, side_nxt.data(), (size_t)n_out * 8 * sizeof(float));
        *n_tracking = n_out;
    }
    trk_next_window(tracks, last_vertices, *n_tracking, &k, origin);
    return RMCV_OK;
}

} // extern "C"
