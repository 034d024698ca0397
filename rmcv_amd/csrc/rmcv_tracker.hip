// rmcv_tracker.hip -- the device-resident tracker as an object: the ONE unit that knows struct rmcv_tracker.
// Its lifetime, the order of its steps (one event), the host's wait with its deadline, and every rmcv_tracker_* entry point: the setters
// and getters of the tracker's, the aim step's and the attitude step's tables, put / get / restore of a stream's list, rmcv_tracker_aim.
// The state is tracker_plan.h's TrackerState; everything outside this unit -- the steps' launchers (k_track.hip, k_aim.hip,
// k_attitude.hip), ctx_track / ctx_attitude (rmcv_host.hip), the tracked submits (rmcv_pipeline.hip) -- reads a TrackerView of it and
// orders its work with tracker_order_begin / _end.  No kernel lives here.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "rmcv_internal.h"
#include "device_aim.h"
#include "device_attitude.h"
#include "device_loop.h"

using namespace rmcv;

struct rmcv_tracker {
    TrackerState s;
    TrackerView view{};           // tracker_view_of(s), kept: every change of `s` ends in refresh() -- a step or submit reads it without building it
    hipEvent_t ev_step = nullptr; // recorded behind the step enqueued last
    bool step_pending = false;
    hipStream_t last_stream = nullptr;
    char err[256] = {0};
    std::vector<void*> allocs;    // everything hipMalloc'ed, freed by rmcv_tracker_destroy
};

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
// what every synchronous entry point starts with: the tracker's device, no step in flight
static int ready(rmcv_tracker* t)
{
    hipSetDevice(t->s.device);
    return tracker_wait(t);
}

static void refresh(rmcv_tracker* t) { t->view = tracker_view_of(t->s); }

namespace rmcv {
const TrackerView& tracker_view(const rmcv_tracker* t) { return t->view; }
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
} // namespace rmcv

// ---- one helper per shape of a per-stream table's life ----
// a new table of n_streams x per_stream entries into *d, every entry `*fill`, or zero bytes (zero), or left as allocated; what: the error's
// text.  The CALLER publishes *d in its StreamTable, so that tables which belong together (aims and aim inputs; attitudes and packet errors)
// appear together or not at all: a failure leaves the memory to `allocs` and the tables as they were
template <typename T>
static int table_new(rmcv_tracker* t, T** d, size_t per_stream, const T* fill, bool zero, const char* what)
{
    const size_t n = (size_t)t->s.cfg.n_streams * per_stream;
    hipError_t e = hipMalloc((void**)d, n * sizeof(T));
    if (e == hipSuccess) {
        t->allocs.push_back(*d);
        if (fill) e = hipMemcpy(*d, std::vector<T>(n, *fill).data(), n * sizeof(T), hipMemcpyHostToDevice);
        else if (zero) e = hipMemset(*d, 0, n * sizeof(T));
    }
    if (e != hipSuccess) return tfail(t, e == hipErrorOutOfMemory ? RMCV_ERR_NOMEM : RMCV_ERR_HIP, what, e);
    return RMCV_OK;
}
// copy n entries of a host table in (the caller has waited for the step in flight)
template <typename T>
static int copy_in(rmcv_tracker* t, T* dst, const T* src, size_t n, const char* what)
{
    TCHK(t, hipMemcpy(dst, src, n * sizeof(T), hipMemcpyHostToDevice), what);
    return RMCV_OK;
}
// copy the first n entries out (out nullable: nothing); never allocated: what the table would hold -- `*never` n times (null: zero bytes)
template <typename T>
static int copy_out(rmcv_tracker* t, T* out, const StreamTable<T>& tb, size_t n, const T* never, const char* what)
{
    if (!out || !n) return RMCV_OK;
    if (tb.p) TCHK(t, hipMemcpy(out, tb.p, n * sizeof(T), hipMemcpyDeviceToHost), what);
    else if (never) std::fill(out, out + n, *never);
    else memset(out, 0, n * sizeof(T));
    return RMCV_OK;
}
// a switched table's setter behind its refusals: NULL switches it off (the memory stays); a host table is copied in and switched on
template <typename T>
static int table_set(rmcv_tracker* t, StreamTable<T>& tb, const T* host, size_t per_stream, const char* what_alloc, const char* what_copy)
{
    int rc = ready(t);
    if (rc) return rc;
    if (host) {
        if (!tb.p && (rc = table_new(t, &tb.p, per_stream, (const T*)nullptr, false, what_alloc))) return rc;
        if ((rc = copy_in(t, tb.p, host, (size_t)t->s.cfg.n_streams * per_stream, what_copy))) return rc;
    }
    tb.on = host != nullptr;
    refresh(t);
    return RMCV_OK;
}

static rmcv_aim_input default_input()
{
    rmcv_aim_input in;
    aim_default_input(&in);
    return in;
}
// the records (zero until the first aim step) and the inputs (the defaults), on first use: both or neither
static int aim_alloc(rmcv_tracker* t)
{
    TrackerState& s = t->s;
    if (s.aims.p) return RMCV_OK;
    const rmcv_aim_input def = default_input();
    rmcv_aim* d_aims = nullptr;
    rmcv_aim_input* d_in = nullptr;
    int rc = table_new(t, &d_aims, 1, (const rmcv_aim*)nullptr, true, "allocating the aim records");
    if (!rc) rc = table_new(t, &d_in, 1, &def, false, "allocating the aim records");
    if (rc) return rc;
    s.aims = {d_aims, true}, s.aim_inputs = {d_in, true};
    refresh(t);
    return RMCV_OK;
}
// the attitudes and the packet counters (zero), on first use: both or neither; the aim tables with them (the step writes the inputs)
static int att_alloc(rmcv_tracker* t)
{
    TrackerState& s = t->s;
    int rc = aim_alloc(t);
    if (rc || s.attitudes.p) return rc;
    rmcv_attitude* d_att = nullptr;
    int32_t* d_err = nullptr;
    if (!(rc = table_new(t, &d_att, 1, (const rmcv_attitude*)nullptr, true, "allocating the attitude tables")))
        rc = table_new(t, &d_err, 1, (const int32_t*)nullptr, true, "allocating the attitude tables");
    if (rc) return rc;
    s.attitudes = {d_att, true}, s.packet_errors = {d_err, true};
    refresh(t);
    return RMCV_OK;
}
// the entries a getter with `cap` hands out
static size_t streams_out(const rmcv_tracker* t, int cap) { return (size_t)std::min(cap, t->s.cfg.n_streams); }

extern "C" {

/* ---- lifetime ---- */

int rmcv_tracker_create(int device, const rmcv_tracker_config* cfg, rmcv_tracker** out)
{
    if (!out) return RMCV_ERR_BAD_ARG;
    *out = nullptr;
    rmcv_tracker_config c;
    if (cfg) c = *cfg;
    else rmcv_default_tracker_config(&c);
    if (tracker_config_refusal(c, true)) return RMCV_ERR_BAD_ARG;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) {
        (void)hipGetLastError();
        return RMCV_ERR_NO_DEVICE;
    }
    if (hipSetDevice(device) != hipSuccess) return RMCV_ERR_NO_DEVICE;
    rmcv_tracker* t = new rmcv_tracker();
    t->s.device = device;
    t->s.cfg = c;
    TrackerBufs& b = t->s.b;
    const size_t slots = (size_t)2 * c.n_streams * c.track_cap;
    struct { void** p; size_t bytes; } want[] = {
        {(void**)&b.tracks, slots * sizeof(rmcv_track)},      {(void**)&b.side, slots * 8 * sizeof(float)},
        {(void**)&b.sel, (size_t)c.n_streams * 4},            {(void**)&b.n_tracking, (size_t)c.n_streams * 4},
        {(void**)&b.status, (size_t)c.n_streams * 4},         {(void**)&b.origins, (size_t)c.n_streams * sizeof(rmcv_point)},
        {(void**)&b.camps, (size_t)c.n_streams * 4},          {(void**)&b.lower_bounds, (size_t)c.n_streams * 4},
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
    t->s.camps.p = b.camps, t->s.lower_bounds.p = b.lower_bounds; // (there from the start, off until rmcv_tracker_set_camps)
    refresh(t);
    *out = t;
    return RMCV_OK;
}

void rmcv_tracker_destroy(rmcv_tracker* t)
{
    if (!t) return;
    const bool done = ready(t) == RMCV_OK;
    if (done) // (a step that has still not finished keeps its memory: leaked rather than freed under a kernel, as rmcv_ctx_destroy does)
        for (void* p : t->allocs) (void)hipFree(p);
    if (t->ev_step && done) (void)hipEventDestroy(t->ev_step);
    delete t;
}

const char* rmcv_tracker_last_error(const rmcv_tracker* t) { return t ? t->err : "null tracker"; }

int rmcv_tracker_reset(rmcv_tracker* t)
{
    if (!t) return RMCV_ERR_BAD_ARG;
    const int rc = ready(t);
    if (rc) return rc;
    const size_t n = (size_t)t->s.cfg.n_streams * 4;
    TCHK(t, hipMemset(t->s.b.n_tracking, 0, n), "reset");
    TCHK(t, hipMemset(t->s.b.status, 0, n), "reset");
    TCHK(t, hipMemset(t->s.b.sel, 0, n), "reset");
    return RMCV_OK;
}

/* ---- the tracker's own tables ---- */

int rmcv_tracker_set_origins(rmcv_tracker* t, const rmcv_point* origins)
{
    if (!t) return RMCV_ERR_BAD_ARG;
    if (!origins) return tfail(t, RMCV_ERR_BAD_ARG, "null origins");
    const int rc = ready(t);
    return rc ? rc : copy_in(t, t->s.b.origins, origins, (size_t)t->s.cfg.n_streams, "H2D origins");
}

int rmcv_tracker_device_origins(rmcv_tracker* t, void** d_origins)
{
    if (!t || !d_origins) return RMCV_ERR_BAD_ARG;
    *d_origins = t->s.b.origins;
    return RMCV_OK;
}

int rmcv_tracker_set_camps(rmcv_tracker* t, const int32_t* camps, const int32_t* lower_bounds)
{
    if (!t) return RMCV_ERR_BAD_ARG;
    int rc = ready(t); // (the step in flight belongs to a batch whose pixel pass may still read the tables)
    if (rc) return rc;
    TrackerState& s = t->s;
    if (!camps) { // off: tracked submits take rmcv_params::camp and ::lower_bound again
        s.camps.on = s.lower_bounds.on = false;
        refresh(t);
        return RMCV_OK;
    }
    const size_t n = (size_t)s.cfg.n_streams;
    if ((rc = copy_in(t, s.camps.p, camps, n, "H2D camps"))) return rc;
    if (lower_bounds && (rc = copy_in(t, s.lower_bounds.p, lower_bounds, n, "H2D lower bounds"))) return rc;
    s.camps.on = true;
    s.lower_bounds.on = lower_bounds != nullptr;
    refresh(t);
    return RMCV_OK;
}

int rmcv_tracker_device_camps(rmcv_tracker* t, void** d_camps, void** d_lower_bounds)
{
    if (!t) return RMCV_ERR_BAD_ARG;
    if (d_camps) *d_camps = t->s.b.camps;
    if (d_lower_bounds) *d_lower_bounds = t->s.b.lower_bounds;
    return RMCV_OK;
}

int rmcv_tracker_counts(rmcv_tracker* t, int32_t* n_tracking, int32_t* status, int cap)
{
    if (!t || cap < 0) return RMCV_ERR_BAD_ARG;
    const int rc = ready(t);
    if (rc) return rc;
    const size_t n = streams_out(t, cap) * 4;
    if (n_tracking && n) TCHK(t, hipMemcpy(n_tracking, t->s.b.n_tracking, n, hipMemcpyDeviceToHost), "D2H counts");
    if (status && n) TCHK(t, hipMemcpy(status, t->s.b.status, n, hipMemcpyDeviceToHost), "D2H status");
    return RMCV_OK;
}

/* ---- one stream's current list ---- */

int rmcv_tracker_get(rmcv_tracker* t, int stream, rmcv_track* tracks_out, int cap, int32_t* n_out, float* last_vertices_out, rmcv_point* origin_out)
{
    if (!t || cap < 0) return RMCV_ERR_BAD_ARG;
    const rmcv_tracker_config& c = t->s.cfg;
    const TrackerBufs& b = t->s.b;
    if (stream < 0 || stream >= c.n_streams) return tfail(t, RMCV_ERR_BAD_ARG, "no such stream");
    const int rc = ready(t);
    if (rc) return rc;
    int32_t n = 0, sel = 0;
    TCHK(t, hipMemcpy(&n, b.n_tracking + stream, 4, hipMemcpyDeviceToHost), "D2H count");
    TCHK(t, hipMemcpy(&sel, b.sel + stream, 4, hipMemcpyDeviceToHost), "D2H current list");
    if (n_out) *n_out = n;
    if (origin_out) TCHK(t, hipMemcpy(origin_out, b.origins + stream, sizeof(rmcv_point), hipMemcpyDeviceToHost), "D2H origin");
    if (n > cap && (tracks_out || last_vertices_out)) return tfail(t, RMCV_ERR_CAPACITY, "output capacity exceeded");
    const size_t at = current_list_at(sel, c.n_streams, stream, c.track_cap);
    if (tracks_out && n) TCHK(t, hipMemcpy(tracks_out, b.tracks + at, (size_t)n * sizeof(rmcv_track), hipMemcpyDeviceToHost), "D2H tracks");
    if (last_vertices_out && n) TCHK(t, hipMemcpy(last_vertices_out, b.side + at * 8, (size_t)n * 8 * sizeof(float), hipMemcpyDeviceToHost), "D2H side records");
    return RMCV_OK;
}

int rmcv_tracker_put(rmcv_tracker* t, int stream, const rmcv_track* tracks, int n, const float* last_vertices)
{
    if (!t) return RMCV_ERR_BAD_ARG;
    const rmcv_tracker_config& c = t->s.cfg;
    const TrackerBufs& b = t->s.b;
    if (stream < 0 || stream >= c.n_streams) return tfail(t, RMCV_ERR_BAD_ARG, "no such stream");
    if (n < 0 || (n > 0 && !tracks)) return tfail(t, RMCV_ERR_BAD_ARG, "rmcv_tracker_put: bad list");
    if (n > c.track_cap) return tfail(t, RMCV_ERR_CAPACITY, "rmcv_tracker_put: more tracks than track_cap");
    int rc = ready(t);
    if (rc) return rc;
    int32_t sel = 0, count = n;
    TCHK(t, hipMemcpy(&sel, b.sel + stream, 4, hipMemcpyDeviceToHost), "D2H current list");
    const size_t at = current_list_at(sel, c.n_streams, stream, c.track_cap);
    if (n) {
        if ((rc = copy_in(t, b.tracks + at, tracks, (size_t)n, "H2D tracks"))) return rc;
        if (last_vertices) rc = copy_in(t, b.side + at * 8, last_vertices, (size_t)n * 8, "H2D side records");
        else TCHK(t, hipMemset(b.side + at * 8, 0, (size_t)n * 8 * sizeof(float)), "side records");
        if (rc) return rc;
    }
    return copy_in(t, b.n_tracking + stream, &count, 1, "H2D count");
}

// a replay's way back from a loop record (device_loop.h)
int rmcv_tracker_restore(rmcv_tracker* t, int stream, const void* rec)
{
    if (!t) return RMCV_ERR_BAD_ARG;
    TrackerState& st = t->s;
    const TrackerBufs& b = st.b;
    if (!rec) return tfail(t, RMCV_ERR_BAD_ARG, "rmcv_tracker_restore: null record");
    if (stream < 0 || stream >= st.cfg.n_streams) return tfail(t, RMCV_ERR_BAD_ARG, "no such stream");
    rmcv_loop_state s;
    memcpy(&s, rec, sizeof(s));
    if (s.flags & RMCV_LOOP_TRUNCATED) return tfail(t, RMCV_ERR_BAD_ARG, "rmcv_tracker_restore: the record is truncated (RMCV_LOOP_TRUNCATED): it does not hold the stream's whole list");
    if (!loop_tracks_ok(&s) || s.n_tracks != s.n_tracking) return tfail(t, RMCV_ERR_BAD_ARG, "rmcv_tracker_restore: the record's counts are not a recorder's");
    if (s.n_tracks > st.cfg.track_cap) return tfail(t, RMCV_ERR_BAD_ARG, "rmcv_tracker_restore: more tracks than the tracker's track_cap");
    if (s.has_aim && !st.aim_on) return tfail(t, RMCV_ERR_BAD_ARG, "rmcv_tracker_restore: the record has an aim step and the tracker's aiming is off (rmcv_tracker_set_aim)");
    if (s.has_attitude && !st.att_on) return tfail(t, RMCV_ERR_BAD_ARG, "rmcv_tracker_restore: the record has an attitude and the tracker's attitude is off (rmcv_tracker_set_attitude)");
    const int rc = ready(t);
    if (rc) return rc;
    const uint8_t* base = static_cast<const uint8_t*>(rec);
    int32_t sel = 0;
    hipError_t e = hipMemcpy(&sel, b.sel + stream, 4, hipMemcpyDeviceToHost);
    const size_t at = current_list_at(sel, st.cfg.n_streams, stream, st.cfg.track_cap);
    for (int j = 0; j < s.n_tracks && e == hipSuccess; j++) {
        e = hipMemcpy(b.tracks + at + j, base + loop_track_at(j), sizeof(rmcv_track), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(b.side + (at + j) * 8, base + loop_side_at(j), LOOP_SIDE_BYTES, hipMemcpyHostToDevice);
    }
    const auto put = [&e](void* dst, const void* src, size_t n) { if (e == hipSuccess) e = hipMemcpy(dst, src, n, hipMemcpyHostToDevice); };
    put(b.n_tracking + stream, &s.n_tracking, 4);
    put(b.status + stream, &s.status, 4);
    put(b.origins + stream, &s.origin_next, sizeof(rmcv_point));
    if (s.has_camps & 1) {
        put(b.camps + stream, &s.camp, 4);
        put(b.lower_bounds + stream, &s.lower_bound, 4);
        st.camps.on = true;
        st.lower_bounds.on = (s.has_camps & 2) != 0;
        refresh(t);
    }
    // (aim_on / att_on are set only behind aim_alloc / att_alloc, which publish their tables together: a mode that is on has them, the aim inputs with either)
    if (s.has_aim) put(st.aims.get() + stream, &s.aim, sizeof(rmcv_aim));
    if (s.has_aim || s.has_attitude) put(st.aim_inputs.get() + stream, &s.aim_input, sizeof(rmcv_aim_input));
    if (s.has_attitude) {
        put(st.attitudes.get() + stream, &s.attitude, sizeof(rmcv_attitude));
        put(st.packet_errors.get() + stream, &s.packet_errors, 4);
    }
    if (e != hipSuccess) return tfail(t, RMCV_ERR_HIP, "rmcv_tracker_restore: H2D", e);
    return RMCV_OK;
}

/* ---- aiming ---- */

int rmcv_tracker_set_aim(rmcv_tracker* t, const rmcv_aim_config* cfg)
{
    if (!t) return RMCV_ERR_BAD_ARG;
    if (cfg) { // (the refusals need no device)
        const char* bad = aim_check_config(cfg);
        if (bad) return tfail(t, RMCV_ERR_BAD_ARG, bad);
    }
    int rc = ready(t);
    if (rc) return rc;
    if (!cfg) {
        t->s.aim_on = false;
        refresh(t);
        return RMCV_OK;
    }
    if ((rc = aim_alloc(t))) return rc;
    t->s.aim_cfg = *cfg;
    t->s.aim_on = true;
    refresh(t);
    return RMCV_OK;
}

int rmcv_tracker_set_aim_configs(rmcv_tracker* t, const rmcv_aim_config* cfgs)
{
    if (!t) return RMCV_ERR_BAD_ARG;
    if (!t->s.aim_on) return tfail(t, RMCV_ERR_BAD_ARG, "rmcv_tracker_set_aim_configs: aiming is off (rmcv_tracker_set_aim)");
    if (cfgs) { // (the refusals need no device)
        for (int f = 0; f < t->s.cfg.n_streams; f++) {
            const char* bad = aim_check_config(&cfgs[f]);
            if (bad) {
                char msg[200];
                snprintf(msg, sizeof(msg), "rmcv_tracker_set_aim_configs: stream %d: %s", f, bad);
                return tfail(t, RMCV_ERR_BAD_ARG, msg);
            }
        }
    }
    return table_set(t, t->s.aim_cfgs, cfgs, 1, "allocating the streams' aim configs", "H2D aim configs");
}

int rmcv_tracker_set_aim_inputs(rmcv_tracker* t, const rmcv_aim_input* inputs)
{
    if (!t) return RMCV_ERR_BAD_ARG;
    int rc = ready(t);
    if (rc) return rc;
    if ((rc = aim_alloc(t))) return rc;
    const size_t n = (size_t)t->s.cfg.n_streams;
    std::vector<rmcv_aim_input> def;
    if (!inputs) {
        def.assign(n, default_input());
        inputs = def.data();
    }
    return copy_in(t, t->s.aim_inputs.p, inputs, n, "H2D aim inputs");
}

int rmcv_tracker_device_aim_inputs(rmcv_tracker* t, void** d_inputs)
{
    if (!t || !d_inputs) return RMCV_ERR_BAD_ARG;
    hipSetDevice(t->s.device);
    const int rc = aim_alloc(t);
    if (rc) return rc;
    *d_inputs = t->s.aim_inputs.p;
    return RMCV_OK;
}

int rmcv_tracker_device_aims(rmcv_tracker* t, void** d_aims)
{
    if (!t || !d_aims) return RMCV_ERR_BAD_ARG;
    hipSetDevice(t->s.device);
    const int rc = aim_alloc(t);
    if (rc) return rc;
    *d_aims = t->s.aims.p;
    return RMCV_OK;
}

int rmcv_tracker_aim(rmcv_tracker* t, int64_t now, void* hip_stream)
{
    if (!t) return RMCV_ERR_BAD_ARG;
    if (!t->s.aim_on) return tfail(t, RMCV_ERR_BAD_ARG, "rmcv_tracker_aim: aiming is off (rmcv_tracker_set_aim)");
    hipSetDevice(t->s.device);
    hipStream_t s = (hipStream_t)hip_stream;
    TCHK(t, tracker_order_begin(t, s), "aim: wait for the tracker's previous step");
    TCHK(t, launch_aim(tracker_view(t), now, s), "k_aim");
    TCHK(t, tracker_order_end(t, s), "aim: record the step");
    return RMCV_OK;
}

int rmcv_tracker_get_aims(rmcv_tracker* t, rmcv_aim* out, int cap)
{
    if (!t || cap < 0 || (cap > 0 && !out)) return RMCV_ERR_BAD_ARG;
    const int rc = ready(t);
    return rc ? rc : copy_out(t, out, t->s.aims, streams_out(t, cap), (const rmcv_aim*)nullptr, "D2H aims");
}

int rmcv_tracker_get_aim_inputs(rmcv_tracker* t, rmcv_aim_input* out, int cap)
{
    if (!t || cap < 0 || (cap > 0 && !out)) return RMCV_ERR_BAD_ARG;
    const int rc = ready(t);
    const rmcv_aim_input def = default_input();
    return rc ? rc : copy_out(t, out, t->s.aim_inputs, streams_out(t, cap), &def, "D2H aim inputs");
}

/* ---- gimbal attitude ---- */

int rmcv_tracker_set_attitude(rmcv_tracker* t, const rmcv_attitude_config* cfg)
{
    if (!t) return RMCV_ERR_BAD_ARG;
    if (cfg) { // (the refusals need no device)
        const char* bad = att_check_config(cfg);
        if (bad) return tfail(t, RMCV_ERR_BAD_ARG, bad);
    }
    int rc = ready(t);
    if (rc) return rc;
    if (!cfg) {
        t->s.att_on = false;
        refresh(t);
        return RMCV_OK;
    }
    if ((rc = att_alloc(t))) return rc;
    t->s.att_cfg = *cfg;
    t->s.att_on = true;
    refresh(t);
    return RMCV_OK;
}

int rmcv_tracker_set_stream_cameras(rmcv_tracker* t, const double* gripper2camera)
{
    if (!t) return RMCV_ERR_BAD_ARG;
    if (gripper2camera) { // (the refusals need no device)
        for (int f = 0; f < t->s.cfg.n_streams; f++)
            for (int i = 0; i < 16; i++)
                if (!att_finite(gripper2camera[(size_t)f * 16 + i])) {
                    char msg[160];
                    snprintf(msg, sizeof(msg), "rmcv_tracker_set_stream_cameras: stream %d: every entry of gripper2camera must be finite", f);
                    return tfail(t, RMCV_ERR_BAD_ARG, msg);
                }
    }
    return table_set(t, t->s.stream_g2c, gripper2camera, 16, "allocating the streams' gripper2camera table", "H2D stream cameras");
}

int rmcv_tracker_set_attitudes(rmcv_tracker* t, const rmcv_attitude* attitudes)
{
    if (!t) return RMCV_ERR_BAD_ARG;
    int rc = ready(t);
    if (rc) return rc;
    if ((rc = att_alloc(t))) return rc;
    const size_t n = (size_t)t->s.cfg.n_streams;
    if (attitudes) return copy_in(t, t->s.attitudes.p, attitudes, n, "H2D attitudes");
    TCHK(t, hipMemset(t->s.attitudes.p, 0, n * sizeof(rmcv_attitude)), "attitudes");
    return RMCV_OK;
}

int rmcv_tracker_get_attitudes(rmcv_tracker* t, rmcv_attitude* out, int32_t* packet_errors, int cap)
{
    if (!t || cap < 0) return RMCV_ERR_BAD_ARG;
    int rc = ready(t);
    if (rc) return rc;
    const size_t n = streams_out(t, cap);
    if ((rc = copy_out(t, out, t->s.attitudes, n, (const rmcv_attitude*)nullptr, "D2H attitudes"))) return rc;
    return copy_out(t, packet_errors, t->s.packet_errors, n, (const int32_t*)nullptr, "D2H packet errors");
}

int rmcv_tracker_device_attitudes(rmcv_tracker* t, void** d_attitudes)
{
    if (!t || !d_attitudes) return RMCV_ERR_BAD_ARG;
    hipSetDevice(t->s.device);
    const int rc = att_alloc(t);
    if (rc) return rc;
    *d_attitudes = t->s.attitudes.p;
    return RMCV_OK;
}

} // extern "C"
