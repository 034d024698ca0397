// rmcv_pipeline.hip -- rmcv_pipeline_*: the pipelined batch schedule behind the C-ABI (include/rmcv_abi.h).
//
// The reference's process_function (/root/reference/executable/main.cpp:163-209) is a loop: newest frame in, three detection calls,
// armours out.  On one MI355X the loop's batch form keeps `depth` batches in flight: the HBM-bound pixel kernel of batch i + 1 streams
// while the latency-bound per-frame kernel of batch i (contours, fits, pairing: a few waves per CU) runs beside it.  Rounds 1-3 had
// this schedule in bench.py (Python + torch streams and events); it lives here now, in the host language of the reference, and
// bench.py, tools/pipeline_bench.c and a C++ host all drive the same three calls.  What the schedule DECIDES is batch_plan.h, pure
// functions of plain values; this file asks the runtime what they need to know and enqueues what they answer.
//
// One slot of the ring = one context (own work buffers) + one record in HBM (frame_offs | status | armours: the payload of the
// multi-GPU gather) + its pinned host mirror.  A ticket's slot and streams are ticket_place's: a slot always meets the same sparse
// stream, so a record's rewrite is ordered behind its last reader on that stream by stream order alone.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <new>
#include <vector>

#include "batch_plan.h"
#include "pixel_sets_plan.h"
#include "rmcv_internal.h"

using namespace rmcv;

// one slot of the ring: the record, its events and the batch that lives in it
struct Slot {
    hipEvent_t ev_bin = nullptr;  // behind the pixel kernel                                               -> waited for by the slot's sparse kernel
    hipEvent_t ev_done = nullptr; // behind the compaction: the slot's context buffers are free            -> waited for by the slot's next pixel kernel
    hipEvent_t ev_host = nullptr; // behind the record's gather (rmcv_pipeline_set_gather)                  -> waited for by collect / wait (host)
    hipEvent_t ev_sp = nullptr;   // behind the slot's first sparse launch
    hipEvent_t ev_free = nullptr; // behind the LAST READER of its batch's pixel outputs (the sparse stage; before the compaction)
    hipEvent_t ev_chg = nullptr;  // the tail of the stream the slot's record was finished on, when that stream changes
    void* ev_hook = nullptr;      // (the hook's own, not owned, or null) the record has been read on another stream -> waited for by the slot's next compaction
    // the record in HBM, its pinned host mirror, the mirror's device address; root of the built-in gather: n_ranks x record_bytes
    uint8_t *d_rec = nullptr, *h_rec = nullptr, *hd_rec = nullptr, *d_recv = nullptr;
    uint64_t ticket = 0;          // ticket + 1 of the batch that lives in the slot (0: none yet)
    hipStream_t stream = nullptr; // the stream the slot's record was finished on
    int frames = 0, ctx = 0;      // of its batch: frames, and the context it ran in
    int set = 0;                  // ... and the pixel-output set of that context it used (pixel_sets_plan.h)
    bool lean = false;            // its batch's sparse stage ran the lean build (every frame of its record reports the mid tier)
    // debug views (rmcv_pipeline_set_views): the slot's buffer, and what its batch rendered into it (view_n == 0: nothing)
    uint8_t* d_views = nullptr;
    int view_n = 0, view_w = 0, view_h = 0;
};

// what a submit asks for: each rmcv_pipeline_submit* fills one -- what every submit has by position (down to `stages`), the rest by name
struct BatchRequest {
    const void* d_frames;
    int n_frames, w, h, stride;
    int64_t frame_pitch;
    const rmcv_params* p;                  // (null: refused.  Pending points p and lp at its own copies)
    int stages;
    const rmcv_legacy_params* lp = nullptr;
    const void* d_origins = nullptr;       // non-null: a windowed batch (rmcv_pipeline_submit_windows) -- every frame read through a win_w x win_h window
    int win_w = 0, win_h = 0;
    const void *d_camps = nullptr, *d_lower_bounds = nullptr; // d_camps non-null: per-frame detection keys (rmcv_pipeline_submit_camps) -- taken per batch, as windows are
    rmcv_tracker* trk = nullptr;           // rmcv_pipeline_submit_tracked: the tracker's step goes behind the batch's compaction, in front of ev_done
    int64_t timestamp = 0;
    const void* d_packets = nullptr;       // a tracked batch's serial packets (rmcv_pipeline_submit_tracked_serial); the attitude step runs whenever the tracker's attitude is on
};

struct rmcv_pipeline {
    int device = 0;
    rmcv_pipeline_config cfg{};
    Limits lim{};
    RecordLayout rec{};
    std::vector<rmcv_ctx*> ring;
    std::vector<int> ctx_last;          // per CONTEXT: the slot of its last batch (-1: none)
    // per context and pixel-output set (2 j + s): recorded beside ev_done of every batch that used the set.  An event of the set's own: the
    // slot of the set's last batch may have a later batch in it by the time the set comes round again (2 hot > depth)
    std::vector<hipEvent_t> ev_set;
    std::vector<Slot> slots;
    std::vector<hipStream_t> pix, sp, dn; // pixel streams, sparse streams, streams of the dense frames' second launch
    uint64_t next_ticket = 0, collected = 0;
    // Contexts in rotation (rmcv_pipeline_config::hot_contexts; profiles/r04f_*): while the batches are CALM they use the first `hot` contexts
    // in turn -- the slot (record, events, streams, ticket window) is still one of `depth` -- and the wave-specialised pixel kernel; a batch of
    // dense frames would stall the pixel stream there: those run as before, every slot its own context, k_binary, the ring's full depth as slack.
    int hot = 0;                        // contexts in rotation while calm (0: a slot always uses its own)
    int hot_cfg = 0;                    // BatchConfig::hot_cfg
    Mood mood{};                        // of the stream: calm, heavy (batch_plan.h: stream_mood)
    bool split_now = false;             // the batches of the moment have a FEW dense frames: give those a launch and a stream of their own
    bool was_cold = false;              // the batch before the newest one found the pixel stream idle (a burst's first launch)
    uint64_t hot_seq = 0, hot_batches = 0, heavy_batches = 0, split_batches = 0, latency_batches = 0;
    // The back half of the NEWEST batch (sparse stage, compaction, events, hook) is enqueued by the next call, not by its own submit: the next
    // submit enqueues it as before (its first kernel waits for the pixel kernel anyway), but a call that WAITS for the newest batch (wait /
    // collect of it, drain) finds that no pixel launch will be beside it and runs it with the latency kernel (0.09 against 0.18 ms alone).
    struct Pending {
        bool valid = false;
        uint64_t t = 0;
        BatchRequest req{};
        rmcv_params p{};        // (what req.p and req.lp point at)
        rmcv_legacy_params lp{};
        size_t k = 0;           // the decisions made for it: slot, context, whether the slot had a batch before
        rmcv_ctx* c = nullptr;
        bool used = false;
        RunPlan plan{};         // the context's options, the pixel shape submit chose, SPARSE_LEAN in dense mode
        int sparse = 0;         // its stages behind the pixel stage
        hipStream_t B = nullptr;
        bool views = false;     // debug views are rendered behind its sparse stage
        LoopTicket loop{};      // a recorded tracked batch: the recorder slot its loop records go into (chosen at the submit; the step runs a call later)
        bool harvest = false;   // its armours' icon rows are appended to the dataset behind its sparse stage
        int labels = 0;         // RMCV_LABEL_* drawn over its views (0: none)
    } pend;
    rmcv_pipeline_hook hook = nullptr; // ... or the built-in gather hook
    void* hook_user = nullptr;
    rmcv_comm* comm = nullptr;
    int root = 0, n_ranks = 0, rank = 0;
    hipEvent_t ev_gather = nullptr;    // behind the last gather: one communicator's operations run in ONE order on every rank
    bool gather_pending = false;
    // Nothing in submit blocks the host (rmcv_abi.h).  The counter proves it: allocations, host-side synchronisations and blocking copies made
    // inside submit (by the pipeline or by the contexts' binding of a geometry) since the pipeline was created.
    uint64_t own_blocking = 0, held_back = 0;
    int wait_timeout_ms = 5000;        // rmcv_pipeline_set_wait_timeout
    const char* last_what = "nothing"; // the enqueue made last (PCHK's label): named when a wait runs out
    const void* cam_idx = nullptr;     // rmcv_pipeline_set_frame_cameras: the frames' camera indices (device, borrowed), for every pose submit
    int cam_frames = 0;
    const void* model_idx = nullptr;   // rmcv_pipeline_set_frame_models: the frames' model indices (device, borrowed), for every submit with the classifier
    int model_frames = 0;
    double max_submit_us = 0;          // the longest single submit call (host time) since rmcv_pipeline_reset_stats
    // rmcv_pipeline_set_views: every following batch renders these frames behind its sparse stage (n == 0: off)
    struct Views {
        int n = 0, vw = 0, vh = 0, flags = 0, max_index = 0, need = 0; // need: the stages the flags read the results of
        bool source = false;           // rmcv_pipeline_set_source_views set them: the source view, not the binary's
        int side = 0;                  // > 0: rmcv_pipeline_set_sheets set them: the labeler's sheet, 2 vw x (vh + side) pixels each
        int stride() const { return side ? 6 * vw : 3 * vw; }
        int64_t pitch() const { return (int64_t)stride() * (vh + side); }
        int32_t* d_frames = nullptr;   // [n] the frame list, on the device
        int label_what = 0, label_scale = 0; // rmcv_pipeline_set_view_labels: RMCV_LABEL_* drawn over them (0: nothing)
    } views;
    // rmcv_pipeline_set_recorder: every following batch packs these frames into the recorder behind its pixel kernel (n == 0: off)
    struct Recording {
        rmcv_recorder* rec = nullptr;
        int n = 0, max_index = 0;
        int32_t frames[RMCV_RECORDER_MAX_FRAMES] = {};
    } recd;
    // rmcv_pipeline_set_harvest: every following batch appends its armours' icon rows to the dataset behind its sparse stage (ds null: off)
    struct Harvest {
        rmcv_dataset* ds = nullptr;
        int32_t* d_labels = nullptr; // [n_labels] the label table, on the device (the pipeline's own copy)
        int n_labels = 0, flags = 0;
    } harv;
    char err[256] = {0};
};

static int finish_back(rmcv_pipeline* pl, bool latency);

static int pfail(rmcv_pipeline* pl, int code, const char* what, hipError_t e = hipSuccess)
{
    if (pl) {
        if (e != hipSuccess) snprintf(pl->err, sizeof(pl->err), "%s: %s", what, hipGetErrorString(e));
        else snprintf(pl->err, sizeof(pl->err), "%s", what);
    }
    if (e != hipSuccess) (void)hipGetLastError();
    return code;
}
#define PCHK(pl, call, what)                                               \
    do {                                                                   \
        (pl)->last_what = what;                                            \
        hipError_t e__ = (call);                                           \
        if (e__ != hipSuccess) return pfail((pl), RMCV_ERR_HIP, what, e__); \
    } while (0)
// a context call failed: its message is the pipeline's
static int cfail(rmcv_pipeline* pl, rmcv_ctx* c, int rc)
{
    snprintf(pl->err, sizeof(pl->err), "%s", rmcv_last_error(c));
    return rc;
}

// the second pixel-output set (pixel_sets_plan.h) for the first n contexts of the ring, where the rotation can run at all: allocated and
// zeroed NOW -- rmcv_pipeline_submit never allocates; a context without one takes every batch in set 0 and keeps the old wait
static int prepare_pixel_sets(rmcv_pipeline* pl, int n)
{
    if (pl->cfg.host_results != 1 || pl->cfg.sparse_waves != 4) return RMCV_OK;
    for (int j = 0; j < n && j < (int)pl->ring.size(); j++)
        if (const int rc = ctx_prepare_pixel_sets(pl->ring[(size_t)j])) return cfail(pl, pl->ring[(size_t)j], rc);
    return RMCV_OK;
}

// a wait with the pipeline's deadline (wait: wait_event_deadline / wait_stream_deadline): RMCV_ERR_TIMEOUT names the enqueue made last
template <class Wait, class What> static int pwait(rmcv_pipeline* pl, Wait wait, What on, const char* what)
{
    hipError_t e = hipSuccess;
    const int rcw = wait(on, pl->wait_timeout_ms, &e);
    if (rcw < 0) return pfail(pl, RMCV_ERR_HIP, what, e);
    if (rcw == 0) return RMCV_OK;
    snprintf(pl->err, sizeof(pl->err), "%s: not finished after %d ms (rmcv_pipeline_set_wait_timeout); enqueued last: %s", what, pl->wait_timeout_ms, pl->last_what);
    return RMCV_ERR_TIMEOUT;
}
static int pwait_event(rmcv_pipeline* pl, hipEvent_t ev, const char* what) { return pwait(pl, wait_event_deadline, ev, what); }
static int pwait_stream(rmcv_pipeline* pl, hipStream_t st, const char* what) { return pwait(pl, wait_stream_deadline, st, what); }
static uint64_t ring_blocking(const rmcv_pipeline* pl)
{
    uint64_t n = 0;
    for (auto c : pl->ring) n += ctx_blocking_calls(c);
    return n;
}

// Events: HIP's default (a system-scope release when the event fires).  hipEventDisableSystemFence / hipEventReleaseToDevice for the
// device-only events ev_bin / ev_done measured the same as the default (round 4, alternating pipelines of one process against a
// calibration pair: 1.049-1.063 against 1.051-1.061 for two identical pipelines), so nothing non-default is asked for.
// (the host reads the record's mirror behind ev_done: it must stay a system-scope event)
static hipError_t slot_create(Slot& s, size_t record_bytes, bool host_mirror)
{
    hipError_t e = hipSuccess;
    for (hipEvent_t* ev : {&s.ev_sp, &s.ev_free, &s.ev_chg, &s.ev_bin, &s.ev_done, &s.ev_host})
        if (e == hipSuccess) e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipMalloc((void**)&s.d_rec, record_bytes);
    if (e == hipSuccess) e = hipMemset(s.d_rec, 0, record_bytes);
    if (e == hipSuccess && host_mirror) {
        e = hipHostMalloc((void**)&s.h_rec, record_bytes, hipHostMallocMapped);
        if (e == hipSuccess) memset(s.h_rec, 0, record_bytes);
        if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&s.hd_rec, s.h_rec, 0);
    }
    return e;
}
static void slot_destroy(Slot& s) // (a slot of a pipeline whose creation failed has null members)
{
    for (hipEvent_t ev : {s.ev_bin, s.ev_done, s.ev_host, s.ev_sp, s.ev_free, s.ev_chg}) if (ev) hipEventDestroy(ev);
    if (s.d_rec) hipFree(s.d_rec);
    if (s.d_recv) hipFree(s.d_recv);
    if (s.h_rec) hipHostFree(s.h_rec);
    if (s.d_views) hipFree(s.d_views);
}
// what the slot's record, in its host mirror, says of its batch
static RecordReport slot_report(const rmcv_pipeline* pl, const Slot& s) { return record_report(reinterpret_cast<const uint32_t*>(s.h_rec)[pl->rec.report_word]); }
// the slot of a live ticket; or null, and the pipeline's message says so
static Slot* live_slot(rmcv_pipeline* pl, uint64_t ticket)
{
    Slot* s = ticket < pl->next_ticket ? &pl->slots[ticket_place(ticket, pl->cfg).slot] : nullptr;
    if (s && s->ticket == ticket + 1) return s;
    pfail(pl, RMCV_ERR_BAD_ARG, "no such ticket in flight (never issued, or its slot has been reused)");
    return nullptr;
}
// the back half of the batch in hand, if there is one: with the latency kernel if it is the one `ticket` names
static constexpr uint64_t NO_TICKET = ~0ull;
static int finish_newest(rmcv_pipeline* pl, uint64_t ticket)
{
    if (!pl->pend.valid) return RMCV_OK;
    hipSetDevice(pl->device);
    return finish_back(pl, pl->pend.t == ticket);
}

extern "C" {

void rmcv_default_pipeline_config(rmcv_pipeline_config* c) { if (c) *c = default_batch_config(); }

void rmcv_pipeline_destroy(rmcv_pipeline* pl)
{
    if (!pl) return;
    hipSetDevice(pl->device);
    if (!pl->ring.empty()) (void)finish_back(pl, true);
    {   // with the deadline: batches that do not finish are not waited for without one -- the pipeline is leaked instead
        bool stuck = false;
        for (auto streams : {&pl->pix, &pl->sp, &pl->dn})
            for (auto s : *streams) if (s) stuck |= pwait_stream(pl, s, "destroy") == RMCV_ERR_TIMEOUT;
        if (stuck) {
            fprintf(stderr, "rmcv_pipeline_destroy: %s; the pipeline's buffers are leaked\n", pl->err);
            return;
        }
    }
    for (auto c : pl->ring) rmcv_ctx_destroy(c);
    for (auto& s : pl->slots) slot_destroy(s);
    if (pl->views.d_frames) hipFree(pl->views.d_frames);
    if (pl->harv.d_labels) hipFree(pl->harv.d_labels);
    if (pl->ev_gather) hipEventDestroy(pl->ev_gather);
    for (hipEvent_t ev : pl->ev_set) if (ev) hipEventDestroy(ev);
    for (auto streams : {&pl->pix, &pl->sp, &pl->dn})
        for (auto s : *streams) if (s) hipStreamDestroy(s);
    delete pl;
}

int rmcv_pipeline_create(int device, const rmcv_limits* limits, const rmcv_pipeline_config* cfg, rmcv_pipeline** out)
{
    if (!out) return RMCV_ERR_BAD_ARG;
    *out = nullptr;
    const BatchConfig bc = resolve_config(cfg);
    if (bc.rc != RMCV_OK) return bc.rc;
    const rmcv_pipeline_config& d = bc.cfg;
    rmcv_pipeline* pl = new (std::nothrow) rmcv_pipeline();
    if (!pl) return RMCV_ERR_NOMEM;
    pl->device = device;
    pl->cfg = d, pl->hot_cfg = bc.hot_cfg;
    int rc = RMCV_OK;
    for (int k = 0; k < d.depth && rc == RMCV_OK; k++) {
        rmcv_ctx* c = nullptr;
        rc = rmcv_ctx_create(device, limits, &c);
        if (rc == RMCV_OK) {
            pl->ring.push_back(c);
            rc = rmcv_ctx_set_option(c, RMCV_OPT_SPARSE_WAVES, d.sparse_waves);
            if (rc == RMCV_OK) rc = rmcv_ctx_set_option(c, RMCV_OPT_PIXEL_GROUPS, d.pixel_groups);
            // everything a batch will need is allocated NOW, for every context of the ring: rmcv_pipeline_submit never allocates
            if (rc == RMCV_OK) rc = ctx_prepare_ring(c);
        }
    }
    if (rc != RMCV_OK) {
        rmcv_pipeline_destroy(pl);
        return rc;
    }
    pl->lim = ctx_limits(pl->ring[0]);
    pl->rec = record_layout(pl->lim.max_frames, pl->cfg.armour_cap);
    pl->cfg.armour_cap = pl->rec.armour_cap;
    hipError_t e = hipSetDevice(device);
    int lo = 0, hi = 0;
    if (e == hipSuccess) e = hipDeviceGetStreamPriorityRange(&lo, &hi); // hi = the numerically lowest = the highest priority
    // pixel streams at normal priority, sparse streams above them: the per-frame kernels are latency chains whose workgroups must be
    // placed as soon as their batch's planes are there, ahead of the next batches' streaming workgroups; the dense frames' streams at
    // normal priority: a dense frame is long work, not a latency chain
    const auto streams = [&e](std::vector<hipStream_t>& v, int n, int priority) {
        for (int i = 0; i < n && e == hipSuccess; i++) {
            v.push_back(nullptr);
            e = hipStreamCreateWithPriority(&v.back(), hipStreamNonBlocking, priority);
        }
    };
    streams(pl->pix, d.pixel_streams, 0);
    streams(pl->sp, d.sparse_streams, hi);
    streams(pl->dn, d.dense_streams, 0);
    for (int k = 0; k < d.depth && e == hipSuccess; k++) {
        pl->slots.emplace_back();
        e = slot_create(pl->slots.back(), (size_t)pl->rec.record_bytes, d.host_results == 1);
        if (e == hipSuccess) ctx_external_order(pl->ring[(size_t)k], pl->slots.back().ev_done);
    }
    if (e == hipSuccess) e = hipEventCreateWithFlags(&pl->ev_gather, hipEventDisableTiming);
    pl->ctx_last.assign((size_t)d.depth, -1);
    pl->ev_set.assign(2 * (size_t)d.depth, nullptr);
    for (hipEvent_t& ev : pl->ev_set) if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    pl->hot = hot_for(pl->hot_cfg, d.depth, pl->lim.max_frames, pl->lim.max_width, pl->lim.max_height); // (derived again for the geometry of every submit)
    // (the contexts the rotation reaches at the limits' geometry; a smaller one may reach further: those contexts keep one set)
    if (e == hipSuccess && prepare_pixel_sets(pl, pl->hot) != RMCV_OK) e = hipErrorOutOfMemory;
    pl->wait_timeout_ms = ctx_wait_timeout_ms(pl->ring[0]);
    if (e != hipSuccess) {
        fprintf(stderr, "rmcv_pipeline_create: %s\n", hipGetErrorString(e));
        (void)hipGetLastError();
        rmcv_pipeline_destroy(pl);
        return e == hipErrorOutOfMemory ? RMCV_ERR_NOMEM : RMCV_ERR_HIP;
    }
    *out = pl;
    return RMCV_OK;
}

int rmcv_hw_queues_hint(void)
{
    setenv("GPU_MAX_HW_QUEUES", "12", 0);
    const char* q = getenv("GPU_MAX_HW_QUEUES");
    return q ? atoi(q) : 0;
}

const char* rmcv_pipeline_last_error(const rmcv_pipeline* pl) { return pl ? pl->err : "null pipeline"; }

int rmcv_pipeline_get_info(const rmcv_pipeline* pl, rmcv_pipeline_info* o)
{
    if (!pl || !o) return RMCV_ERR_BAD_ARG;
    memset(o, 0, sizeof(*o));
    const rmcv_pipeline_config& c = pl->cfg;
    o->depth = c.depth, o->pixel_streams = c.pixel_streams, o->sparse_streams = c.sparse_streams, o->armour_cap = c.armour_cap;
    o->sparse_waves = c.sparse_waves, o->pixel_groups = c.pixel_groups, o->host_results = c.host_results, o->dense_streams = c.dense_streams;
    const char* q = getenv("GPU_MAX_HW_QUEUES");
    o->hw_queues_env = q ? atoi(q) : 0;
    o->hw_queues_wanted = 1 + pl->cfg.pixel_streams + pl->cfg.sparse_streams + pl->cfg.dense_streams + (pl->comm ? 1 : 0);
    o->record_bytes = pl->rec.record_bytes, o->armours_offset = pl->rec.head_bytes;
    o->submitted = pl->next_ticket, o->collected = pl->collected;
    o->dense_split = pl->split_batches, o->hot_batches = pl->hot_batches, o->latency_batches = pl->latency_batches;
    o->hot_contexts = pl->hot, o->max_frames = pl->lim.max_frames;
    o->host_blocking_calls = pl->own_blocking, o->max_submit_us = pl->max_submit_us, o->wait_timeout_ms = pl->wait_timeout_ms;
    o->held_back = pl->held_back, o->heavy_batches = pl->heavy_batches;
    return RMCV_OK;
}

rmcv_ctx* rmcv_pipeline_context(rmcv_pipeline* pl, int slot)
{
    if (!pl || slot < 0 || slot >= pl->cfg.depth) return nullptr;
    return pl->ring[(size_t)slot];
}

int rmcv_pipeline_set_hot_contexts(rmcv_pipeline* pl, int n)
{
    if (!pl) return RMCV_ERR_BAD_ARG;
    if (n <= 0) { pl->hot = 0; pl->hot_cfg = -1; return RMCV_OK; }
    if (const char* no = hot_contexts_refusal(n, pl->cfg)) return pfail(pl, RMCV_ERR_BAD_ARG, no);
    hipSetDevice(pl->device);
    if (const int rc = prepare_pixel_sets(pl, n)) return rc;
    pl->hot = pl->hot_cfg = n;
    return RMCV_OK;
}

int rmcv_pipeline_set_wait_timeout(rmcv_pipeline* pl, int ms)
{
    if (!pl || ms < 0) return RMCV_ERR_BAD_ARG;
    pl->wait_timeout_ms = ms;
    for (auto c : pl->ring) rmcv_ctx_set_option(c, RMCV_OPT_WAIT_TIMEOUT_MS, ms);
    return RMCV_OK;
}

rmcv_ctx* rmcv_pipeline_context_of(rmcv_pipeline* pl, uint64_t ticket)
{
    if (!pl || finish_newest(pl, ticket)) return nullptr;
    const Slot* s = live_slot(pl, ticket);
    if (!s) return nullptr;
    // (with the hot contexts a context is reused as early as ticket + hot_contexts, while the ticket's RECORD lives until ticket + depth)
    if (pl->ctx_last[(size_t)s->ctx] != (int)(s - pl->slots.data())) { pfail(pl, RMCV_ERR_BAD_ARG, "the ticket's context has been reused by a later batch (its record is still there: rmcv_pipeline_collect)"); return nullptr; }
    return pl->ring[(size_t)s->ctx];
}

int rmcv_pipeline_set_hook(rmcv_pipeline* pl, rmcv_pipeline_hook fn, void* user)
{
    if (!pl) return RMCV_ERR_BAD_ARG;
    if (const int rcb = finish_newest(pl, NO_TICKET)) return rcb; // (the batch in hand keeps the hook it was submitted under)
    if (pl->comm && fn) return pfail(pl, RMCV_ERR_BAD_ARG, "the pipeline already gathers with rmcv_gather (rmcv_pipeline_set_gather): one hook at a time");
    pl->hook = fn, pl->hook_user = user;
    return RMCV_OK;
}

int rmcv_pipeline_set_gather(rmcv_pipeline* pl, rmcv_comm* comm, int root)
{
    if (!pl) return RMCV_ERR_BAD_ARG;
    if (const int rcb = finish_newest(pl, NO_TICKET)) return rcb;
    if (pl->hook && comm) return pfail(pl, RMCV_ERR_BAD_ARG, "the pipeline already has a hook (rmcv_pipeline_set_hook): one at a time");
    int rc = rmcv_pipeline_drain(pl);
    if (rc) return rc;
    hipSetDevice(pl->device);
    for (auto& s : pl->slots) if (s.d_recv) { hipFree(s.d_recv); s.d_recv = nullptr; }
    pl->comm = nullptr, pl->gather_pending = false;
    if (!comm) return RMCV_OK;
    int32_t n = 0, r = 0;
    if ((rc = rmcv_comm_info(comm, &n, &r))) return pfail(pl, rc, "rmcv_comm_info");
    if (root < 0 || root >= n) return pfail(pl, RMCV_ERR_BAD_ARG, "root out of range");
    if (r == root)
        for (auto& s : pl->slots) PCHK(pl, hipMalloc((void**)&s.d_recv, (size_t)pl->rec.record_bytes * (size_t)n), "hipMalloc (gather receive buffer)");
    pl->comm = comm;
    pl->root = root, pl->n_ranks = n, pl->rank = r;
    return RMCV_OK;
}

// the back half of the newest batch (see rmcv_pipeline::Pending); latency: nothing will be launched beside it
static int finish_back(rmcv_pipeline* pl, bool latency)
{
    if (!pl->pend.valid) return RMCV_OK;
    pl->pend.valid = false;
    const rmcv_pipeline::Pending& P = pl->pend; // (as it is until the next submit)
    const BatchRequest& q = P.req;
    Slot& S = pl->slots[P.k];
    hipStream_t B = P.B;
    int rc = RMCV_OK;
    // whether a FEW frames of the batch that last left this slot were dense (batch_plan.h: split_rule)
    if (P.used && !pl->dn.empty() && hipEventQuery(S.ev_done) == hipSuccess) pl->split_now = split_rule(slot_report(pl, S), S.frames);
    (void)hipGetLastError(); // (hipErrorNotReady is not an error)
    const BackPlan bp = back_plan(latency, pl->cfg, q.lp != nullptr, P.plan, pl->split_now, (int)pl->dn.size(), P.sparse, P.k);
    RunPlan plan = {P.plan.pixel_ws, P.plan.pixel_groups, bp.sparse_waves, bp.first};
    if (bp.w8) pl->latency_batches++;
    if (bp.split) pl->split_batches++;
    hipStream_t T = bp.dense_stream >= 0 ? pl->dn[(size_t)bp.dense_stream] : B; // the stream the batch's list is finished on
    // (a record's rewrite is ordered behind its readers by stream order: the slot meets the same stream every time -- unless the
    // caller mixes stage masks that finish on different streams, or a stream's dense frames come and go)
    // ... the new stream waits, on the GPU, for the tail of the old one
    if (P.used && S.stream && S.stream != T) {
        PCHK(pl, hipEventRecord(S.ev_chg, S.stream), "pipeline: change of the slot's stream (mark)");
        PCHK(pl, hipStreamWaitEvent(T, S.ev_chg, 0), "pipeline: change of the slot's stream (wait)");
    }
    bool lean = false; // (the launcher takes the lean build where it applies: fused stages, no classifier, the mid tier's scratch there)
    if (P.sparse) {
        if (bp.split) {
            rc = ctx_run(P.c, q.p, nullptr, P.sparse & ~RMCV_STAGE_POSE, B, plan);
            if (rc == RMCV_OK) {
                PCHK(pl, hipEventRecord(S.ev_sp, B), "pipeline: mark the first sparse launch");
                PCHK(pl, hipStreamWaitEvent(T, S.ev_sp, 0), "pipeline: chain the dense frames");
                plan.form = bp.second;
                rc = ctx_run(P.c, q.p, nullptr, P.sparse, T, plan);
            }
        } else {
            rc = ctx_run(P.c, q.p, q.lp, P.sparse, B, plan, &lean);
        }
        if (rc) return cfail(pl, P.c, rc);
    }
    // the debug views: behind the sparse stage (they read its tables), in front of ev_free (they read the pixel stage's bit planes)
    S.view_n = 0;
    if (P.views) {
        const rmcv_pipeline::Views& V = pl->views; // (as at the submit: rmcv_pipeline_set_views drains first)
        // (the source view also reads the frames, through the effective origins / gamma tables: in front of ev_free for that too, as the harvest is)
        if (V.side) rc = ctx_sheet_enqueue(P.c, V.d_frames, V.n, V.vw, V.vh, V.side, V.flags, S.d_views, V.stride(), V.pitch(), T);
        else rc = (V.source ? ctx_source_view_enqueue : ctx_view_enqueue)(P.c, V.d_frames, V.n, V.vw, V.vh, V.flags, S.d_views, V.stride(), V.pitch(), T);
        if (rc) return cfail(pl, P.c, rc);
        pl->last_what = V.side ? "k_icon_strip" : (V.source ? "k_view_source" : "k_view_resize");
        S.view_n = V.n, S.view_w = V.side ? 2 * V.vw : V.vw, S.view_h = V.vh + V.side;
    }
    // the dataset harvest: behind the sparse stage (it reads the armours, and the identities behind the classifier), in front of ev_free (it reads
    // the frames through the effective origins / gamma tables the next pixel pass of this context rewrites); an append waits, on the GPU, for
    // the dataset's previous one, so the rows land in ticket order whichever streams the slots finish on
    if (P.harvest) {
        const rmcv_pipeline::Harvest& Hv = pl->harv; // (as at the submit: rmcv_pipeline_set_harvest drains first)
        rc = ctx_harvest(P.c, Hv.ds, nullptr, Hv.d_labels, Hv.n_labels, Hv.flags, P.t, q.stages, T);
        if (rc) return cfail(pl, P.c, rc);
        pl->last_what = "k_harvest_rows";
    }
    PCHK(pl, hipEventRecord(S.ev_free, T), "pipeline: mark the pixel outputs' last reader");
    // the record is rewritten: a reader on another stream (the hook's) must be through; readers on B are by stream order
    if (S.ev_hook) {
        PCHK(pl, hipStreamWaitEvent(T, (hipEvent_t)S.ev_hook, 0), "pipeline: wait for the record's reader");
        S.ev_hook = nullptr;
    }
    int32_t* offs = reinterpret_cast<int32_t*>(S.d_rec);
    // host_results: the compaction kernel stores the record a second time, straight into the slot's pinned host mirror (posted
    // writes over PCIe, only the armours there are); the slot's event -- a default event: system-scope release -- makes them visible
    rc = ctx_compact(P.c, S.d_rec + pl->rec.head_bytes, pl->cfg.armour_cap, offs, offs + pl->rec.status_word, T, S.hd_rec, (int)pl->rec.head_bytes);
    if (rc) return cfail(pl, P.c, rc);
    // a tracked batch: the tracker's step right behind the compaction, on the stream the list was finished on -- it reads the context's
    // armours, identities, poses and effective origins, so it comes BEFORE ev_done frees them; ctx_track records the tracker's event
    // behind it (the next tracked submit's k_window_origins waits for that), and wait / collect / drain of the ticket cover the step
    if (q.trk) {
        rc = ctx_track(P.c, q.trk, q.timestamp, q.stages, T, &P.loop);
        if (rc) return cfail(pl, P.c, rc);
        pl->last_what = P.loop.rec ? "k_loop_record" : "k_track";
    }
    // the view labels: over the views rendered above, behind the tracker's step (they read its lists; ctx_label_enqueue makes the tracker's
    // next step wait for them) and in front of ev_done (they read the context's armours, identities, poses and effective origins)
    if (P.labels) {
        const rmcv_pipeline::Views& V = pl->views; // (as at the submit: rmcv_pipeline_set_view_labels drains first)
        // (a sheet's left pane starts at the sheet's first byte: the labels get its pointer, the sheet's stride and pitch)
        rc = ctx_label_enqueue(P.c, q.trk, P.labels, q.stages, V.d_frames, V.n, V.vw, V.vh, V.label_scale, S.d_views, V.stride(), V.pitch(), T);
        if (rc) return cfail(pl, P.c, rc);
        pl->last_what = "k_view_text";
    }
    // the context's buffers are free from here on: the next pixel kernel of this slot does not wait for the hook
    PCHK(pl, hipEventRecord(S.ev_done, T), "pipeline: mark the slot");
    PCHK(pl, hipEventRecord(pl->ev_set[2 * (size_t)S.ctx + (size_t)S.set], T), "pipeline: mark the pixel-output set");
    S.ticket = P.t + 1;
    S.frames = q.n_frames;
    S.lean = lean;
    S.stream = T;
    if (pl->comm) {
        // one communicator: its operations must execute in one order on every rank; they are issued in ticket order on alternating
        // streams, so each gather first waits (an event, on the GPU) for the one before
        if (pl->gather_pending) PCHK(pl, hipStreamWaitEvent(T, pl->ev_gather, 0), "pipeline: order the gathers");
        rc = rmcv_gather(pl->comm, S.d_rec, pl->rec.record_bytes, pl->rank == pl->root ? S.d_recv : nullptr, pl->root, T);
        if (rc) return pfail(pl, rc, rmcv_comm_last_error(pl->comm));
        PCHK(pl, hipEventRecord(pl->ev_gather, T), "pipeline: mark the gather");
        pl->gather_pending = true;
        PCHK(pl, hipEventRecord(S.ev_host, T), "pipeline: mark the gather"); // wait / collect cover the gather too
    } else if (pl->hook) {
        void* done = nullptr;
        rc = pl->hook(pl->hook_user, P.t, S.d_rec, pl->rec.record_bytes, T, &done);
        if (rc) return pfail(pl, rc, "the pipeline hook failed");
        S.ev_hook = done;
    }
    return RMCV_OK;
}

static int submit(rmcv_pipeline* pl, const BatchRequest& q, uint64_t* ticket)
{
    if (!pl || !q.d_frames || !q.p) return RMCV_ERR_BAD_ARG;
    const rmcv_legacy_params* lp = q.lp;
    const int stages = q.stages;
    if (!(stages & RMCV_STAGE_BINARY)) return pfail(pl, RMCV_ERR_BAD_ARG, "a pipelined batch starts at RMCV_STAGE_BINARY");
    bool attitude = false;
    if (q.trk) {
        const TrackerView& v = tracker_view(q.trk);
        attitude = v.att_on;
        if (const char* no = tracked_refusal(v.device, pl->device, v.cfg, q.n_frames, q.w, q.h, stages, q.d_packets != nullptr, attitude))
            return pfail(pl, RMCV_ERR_BAD_ARG, no);
    }
    if (pl->views.n) { // (with no views set: nothing here, and nothing further down)
        if (q.n_frames <= pl->views.max_index)
            return pfail(pl, RMCV_ERR_BAD_ARG, pl->views.side ? SHEET_FEWER_FRAMES : pl->views.source ? SOURCE_VIEW_FEWER_FRAMES : "the batch has fewer frames than the debug views name (rmcv_pipeline_set_views)");
        if ((stages & pl->views.need) != pl->views.need)
            return pfail(pl, RMCV_ERR_BAD_ARG, pl->views.side ? SHEET_FEWER_STAGES : pl->views.source ? SOURCE_VIEW_FEWER_STAGES : "the batch's stages lack what the debug views' flags need (rmcv_pipeline_set_views)");
        if (pl->views.label_what) { // (with no labels set: nothing here, and nothing further down)
            if (!(stages & RMCV_STAGE_ARMOURS)) return pfail(pl, RMCV_ERR_BAD_ARG, "the batch's stages lack RMCV_STAGE_ARMOURS, which the view labels need (rmcv_pipeline_set_view_labels)");
            if ((pl->views.label_what & RMCV_LABEL_TRACKS) && !q.trk)
                return pfail(pl, RMCV_ERR_BAD_ARG, "RMCV_LABEL_TRACKS is set (rmcv_pipeline_set_view_labels): the submit needs a tracker (rmcv_pipeline_submit_tracked)");
        }
    }
    if (pl->recd.n) { // (with no recorder set: nothing here, and nothing further down)
        if (q.n_frames <= pl->recd.max_index) return pfail(pl, RMCV_ERR_BAD_ARG, "the batch has fewer frames than the recorder's frame list names (rmcv_pipeline_set_recorder)");
        if (const char* no = recorder_refusal(pl->recd.rec, pl->device, pl->recd.n, q.w * ctx_frame_pixel_bytes(pl->ring[0]), q.h)) return pfail(pl, RMCV_ERR_BAD_ARG, no);
        if (const char* no = recorder_trigger_refusal(pl->recd.rec, pl->cfg.depth)) return pfail(pl, RMCV_ERR_BAD_ARG, no); // (armed since rmcv_pipeline_set_recorder)
    }
    if (pl->harv.ds) // (with no dataset set: nothing here, and nothing further down)
        if (const char* no = ctx_harvest_refusal(pl->device, q.n_frames, true, pl->harv.ds, pl->harv.n_labels, pl->harv.flags, stages, pl->lim.max_armours)) return pfail(pl, RMCV_ERR_BAD_ARG, no);
    hipSetDevice(pl->device);
    int rc = finish_back(pl, false); // the batch before this one: a pixel launch follows it
    if (rc) return rc;
    const uint64_t t = pl->next_ticket;
    const TicketPlace at = ticket_place(t, pl->cfg);
    const size_t k = at.slot;
    Slot& S = pl->slots[k];
    const bool used = S.ticket != 0;
    pl->hot = hot_for(pl->hot_cfg, pl->cfg.depth, q.n_frames, q.d_origins ? q.win_w : q.w, q.d_origins ? q.win_h : q.h);
    if (pl->cfg.host_results == 1) { // the newest record that has come back: did any of its frames go beyond the LDS tables?  how heavy was it?
        for (uint64_t d = 1; d <= (uint64_t)pl->cfg.depth && d <= t; d++) {
            const Slot& s = pl->slots[ticket_place(t - d, pl->cfg).slot];
            if (s.ticket != t - d + 1 || !s.h_rec) break;
            if (hipEventQuery(s.ev_done) != hipSuccess) continue;
            pl->mood = stream_mood(slot_report(pl, s), s.lean, s.frames);
            break;
        }
        (void)hipGetLastError(); // (hipErrorNotReady is not an error)
    }
    // the front half of the batch's plan: the hot rotation or the slot's own context, dense mode
    const bool ws_variant = PIXEL_VARIANTS[pixel_variant(RMCV_INPUT_BGR, ctx_enhance(pl->ring[k]), q.d_origins != nullptr, q.d_camps != nullptr)].ws;
    const FrontPlan fp = front_plan(pl->hot, pl->mood.calm, pl->mood.heavy, pl->cfg, stages, lp != nullptr, ws_variant, q.trk != nullptr, pl->hot_seq, k);
    rmcv_ctx* c = pl->ring[fp.j];
    // the rotation is decided from the slot's own context and the batch may run in another (ring[fp.j]): a ring whose contexts disagree
    // about the option would mix the two paths batch by batch -- refused, loudly, whichever slot this batch would take
    for (size_t i = 1; i < pl->ring.size(); i++)
        if (ctx_enhance(pl->ring[i]) != ctx_enhance(pl->ring[0]))
            return pfail(pl, RMCV_ERR_BAD_ARG, "RMCV_OPT_ENHANCE differs between the pipeline's contexts: set it on EVERY slot (rmcv_pipeline_context)");
    // the sticky camera table (rmcv_pipeline_set_frame_cameras) is this batch's when it has a pose stage
    const bool cameras = pl->cam_idx && (stages & RMCV_STAGE_POSE);
    if (cameras) {
        bool agree = true;
        char msg[200];
        for (size_t i = 1; i < pl->ring.size(); i++) agree &= ctx_n_cameras(pl->ring[i]) == ctx_n_cameras(pl->ring[0]);
        if (const char* no = cameras_refusal(q.n_frames, pl->cam_frames, agree, msg)) return pfail(pl, RMCV_ERR_BAD_ARG, no);
    }
    // ... and the sticky model index table (rmcv_pipeline_set_frame_models) when it has the classifier
    const bool models = pl->model_idx && (stages & RMCV_STAGE_IDENTITY);
    if (models) {
        bool agree = true;
        char msg[200];
        for (size_t i = 1; i < pl->ring.size(); i++) agree &= ctx_n_models(pl->ring[i]) == ctx_n_models(pl->ring[0]);
        if (const char* no = pipeline_models_refusal(q.n_frames, pl->model_frames, agree, msg)) return pfail(pl, RMCV_ERR_BAD_ARG, no);
    }
    // what the legacy matcher and per-frame keys refuse of the context's options (a Bayer input format, RMCV_OPT_ENHANCE); what windows and
    // the options refuse of each other: the binding below, as for every batch
    if ((lp || q.d_camps) && (rc = ctx_check_modes(c, q.d_camps != nullptr, lp != nullptr))) return cfail(pl, c, rc);
    // a batch is several runs on several streams: everything that could refuse it is checked before the first enqueue (the binding's, on A)
    if ((rc = ctx_check_stages(c, q.p, stages))) return cfail(pl, c, rc);
    const RunPlan plan = fp.plan(ctx_plan(c));
    hipStream_t A = pl->pix[at.pixel], B = pl->sp[at.sparse];
    // the context's pixel-output set the batch takes, and what its streams wait for (pixel_sets_plan.h)
    const int set = pixel_set_for(fp.fast, pl->hot_seq, pl->hot, ctx_pixel_sets(c));
    const SetWaits sw = pixel_set_waits(fp.fast, ctx_pixel_sets(c), ctx_bind_enqueues(c, q.n_frames, q.d_origins ? q.win_w : q.w, q.d_origins ? q.win_h : q.h));
    // ---- waits first: stream A is behind everything that still uses the slot and the context when the binding below enqueues on it.
    // (Nothing of the pipeline's own state moves before the batch has been accepted: an error return leaves tickets, rotation and
    // context ownership as they were; the waits already enqueued on A are harmless.)
    // the slot's context buffers are free once its previous list is compacted
    if (used) PCHK(pl, hipStreamWaitEvent(A, S.ev_done, 0), "pipeline: wait for the slot");
    // the context's last batch (another slot's, when the hot contexts take turns): its sparse stage or its compaction (batch_plan.h: waits_for_free)
    // -- or, with two pixel-output sets, the last batch in the SAME set, and the pixel kernel alone of the context's last batch
    if (pl->ctx_last[fp.j] >= 0 && pl->ctx_last[fp.j] != (int)k) {
        const Slot& last = pl->slots[(size_t)pl->ctx_last[fp.j]];
        if (sw.pixel_ctx_last) PCHK(pl, hipStreamWaitEvent(A, waits_for_free(last.stream, B) ? last.ev_free : last.ev_done, 0), "pipeline: wait for the context");
        if (sw.pixel_ctx_bin) PCHK(pl, hipStreamWaitEvent(A, last.ev_bin, 0), "pipeline: wait for the context's pixel kernel");
    }
    // (an event that has never been recorded is not waited for)
    if (sw.pixel_set_last) PCHK(pl, hipStreamWaitEvent(A, pl->ev_set[2 * fp.j + (size_t)set], 0), "pipeline: wait for the context's pixel-output set");
    // the sparse stage shares the context's one set of tables with the context's last batch: its stream waits, the pixel stream does not
    // (enqueued here, in front of the chain to the pixel kernel: the batch's sparse stage is enqueued by the next call)
    if (sw.sparse_ctx_last && pl->ctx_last[fp.j] >= 0 && pl->ctx_last[fp.j] != (int)k)
        PCHK(pl, hipStreamWaitEvent(B, pl->slots[(size_t)pl->ctx_last[fp.j]].ev_done, 0), "pipeline: the sparse stream waits for the context");
    // ---- bind: a new geometry's work (planes zeroed, frame order) is ENQUEUED on A, nothing blocks
    rc = ctx_bind_frames(c, q.d_frames, q.n_frames, q.w, q.h, q.stride, q.frame_pitch, A, q.d_origins, q.win_w, q.win_h, q.d_camps, q.d_lower_bounds);
    if (rc) return cfail(pl, c, rc);
    if (cameras) ctx_set_frame_cameras(c, pl->cam_idx); // (read by the batch's k_pnp, on its stream)
    if (models) ctx_set_frame_models(c, pl->model_idx); // (read by the batch's k_classify_models, on its stream)
    const int pixel = stages & (RMCV_STAGE_BINARY | RMCV_STAGE_NO_IMAGE), sparse = stages & ~(RMCV_STAGE_BINARY | RMCV_STAGE_NO_IMAGE);
    ctx_external_order(c, S.ev_done);
    // a burst's second pixel launch is held back (batch_plan.h: hold_back, which says when each of these is asked)
    bool prev_live = false, prev_done = false;
    if (fp.fast && t > 0) {
        const Slot& prev = pl->slots[ticket_place(t - 1, pl->cfg).slot];
        prev_live = prev.ticket == t;
        prev_done = prev_live && hipEventQuery(prev.ev_done) == hipSuccess;
        (void)hipGetLastError();
    }
    const bool ws_full = prev_live && !prev_done && pl->was_cold && pixel_ws_full(c, q.p->lower_bound, plan);
    const HoldBack hb = hold_back(fp.fast, t, pl->was_cold, prev_live, prev_done, ws_full, q.n_frames, q.w, q.h);
    if (hb.hold_us > 0) {
        PCHK(pl, launch_delay((unsigned long long)hb.hold_us * 1000ull, A), "pipeline: k_delay");
        pl->held_back++;
    }
    // strict closed loop: the origins k_window_origins is about to read are those the tracker's last step wrote -- an event wait on the GPU
    // (that step was enqueued by the finish_back above, or earlier)
    if (q.trk && q.d_origins && !attitude) PCHK(pl, tracker_order_begin(q.trk, A), "pipeline: wait for the tracker's last step");
    // attitude on: the attitude step first -- it makes that wait itself, for whole-frame trackers too (the step in flight reads the aim inputs
    // this one writes), and the camps it may write are read by the k_frame_keys of the run below.  Everything it could refuse has been checked.
    if (attitude) {
        rc = ctx_attitude(c, q.trk, q.d_packets, A);
        if (rc) return cfail(pl, c, rc);
    }
    // (the binding is the same for both sets; a refused run leaves the context with the set of its last batch, which the getters read)
    const int set_before = ctx_pixel_set(c);
    ctx_use_pixel_set(c, set);
    rc = ctx_run(c, q.p, nullptr, pixel, A, plan);
    if (rc) {
        ctx_use_pixel_set(c, set_before);
        return cfail(pl, c, rc);
    }
    pl->last_what = PIXEL_VARIANTS[ctx_pixel_variant(c)].step;
    // ---- accepted: the pipeline's state moves
    pl->was_cold = hb.cold;
    if (fp.fast) { pl->hot_seq++; pl->hot_batches++; }
    if (fp.heavy) pl->heavy_batches++;
    pl->ctx_last[fp.j] = (int)k;
    S.ctx = (int)fp.j, S.set = set;
    PCHK(pl, hipEventRecord(S.ev_bin, A), "pipeline: mark the pixel kernel");
    PCHK(pl, hipStreamWaitEvent(B, S.ev_bin, 0), "pipeline: chain the sparse stages");
    // the recorder: the chosen frames as delivered, and the effective keys and origins the pixel stage's prologue has just written, packed on
    // the batch's sparse stream in front of its sparse stage -- off the pixel stream, and in front of ev_done: a wait for the ticket covers it
    LoopTicket loop{};
    if (pl->recd.n) {
        RecordBatch rb{};
        rb.d_frames = q.d_frames, rb.w = q.w, rb.h = q.h, rb.stride = q.stride, rb.pitch = q.frame_pitch, rb.batch_frames = q.n_frames;
        rb.stages = stages, rb.win_w = q.d_origins ? q.win_w : 0, rb.win_h = q.d_origins ? q.win_h : 0;
        rb.params = *q.p, rb.timestamp = q.timestamp, rb.ticket = t;
        ctx_record_batch(c, &rb);
        rb.trk = q.trk;
        if ((rc = recorder_enqueue(pl->recd.rec, rb, pl->recd.frames, pl->recd.n, B, &loop))) return pfail(pl, rc, rmcv_recorder_last_error(pl->recd.rec));
        loop.d_packets = q.d_packets;
        pl->last_what = "k_pack_emit";
    }
    pl->next_ticket = t + 1;
    if (ticket) *ticket = t;
    pl->pend = {true, t, q, *q.p, lp ? *lp : rmcv_legacy_params{}, k, c, used, plan, sparse, B, pl->views.n > 0, loop, pl->harv.ds != nullptr};
    pl->pend.labels = pl->views.n > 0 ? pl->views.label_what : 0;
    pl->pend.req.p = &pl->pend.p; // (the caller's params live as long as its call)
    pl->pend.req.lp = lp ? &pl->pend.lp : nullptr;
    // (a hook or the gather hands the record to a consumer the pipeline does not see waiting: its batches are finished here and now)
    if (pl->hook || pl->comm) return finish_back(pl, false);
    return RMCV_OK;
}

// submit + its own bookkeeping: the host time of the call, and the blocking calls the ring's contexts counted during it
static int submit_counted(rmcv_pipeline* pl, const BatchRequest& q, uint64_t* ticket)
{
    if (!pl) return RMCV_ERR_BAD_ARG;
    timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    const uint64_t b0 = ring_blocking(pl);
    const int rc = submit(pl, q, ticket);
    pl->own_blocking += ring_blocking(pl) - b0;
    clock_gettime(CLOCK_MONOTONIC, &t1);
    const double us = (t1.tv_sec - t0.tv_sec) * 1e6 + (t1.tv_nsec - t0.tv_nsec) * 1e-3;
    if (us > pl->max_submit_us) pl->max_submit_us = us;
    return rc;
}

int rmcv_pipeline_set_frame_cameras(rmcv_pipeline* pl, const void* d_idx, int n_frames)
{
    if (!pl) return RMCV_ERR_BAD_ARG;
    if (d_idx && (n_frames < 1 || n_frames > pl->lim.max_frames)) return pfail(pl, RMCV_ERR_BAD_ARG, "rmcv_pipeline_set_frame_cameras: n_frames out of range");
    pl->cam_idx = d_idx;
    pl->cam_frames = d_idx ? n_frames : 0;
    return RMCV_OK;
}

int rmcv_pipeline_set_frame_models(rmcv_pipeline* pl, const void* d_idx, int n_frames)
{
    if (!pl) return RMCV_ERR_BAD_ARG;
    if (d_idx && (n_frames < 1 || n_frames > pl->lim.max_frames)) return pfail(pl, RMCV_ERR_BAD_ARG, "rmcv_pipeline_set_frame_models: n_frames out of range");
    pl->model_idx = d_idx;
    pl->model_frames = d_idx ? n_frames : 0;
    return RMCV_OK;
}

int rmcv_pipeline_reset_stats(rmcv_pipeline* pl)
{
    if (!pl) return RMCV_ERR_BAD_ARG;
    pl->max_submit_us = 0;
    return RMCV_OK;
}

int rmcv_pipeline_submit(rmcv_pipeline* pl, const void* d_frames, int n_frames, int w, int h, int stride, int64_t frame_pitch,
                         const rmcv_params* p, int stages, uint64_t* ticket)
{
    return submit_counted(pl, {d_frames, n_frames, w, h, stride, frame_pitch, p, stages}, ticket);
}

int rmcv_pipeline_submit_legacy(rmcv_pipeline* pl, const void* d_frames, int n_frames, int w, int h, int stride, int64_t frame_pitch,
                                const rmcv_params* p, const rmcv_legacy_params* lp, int stages, uint64_t* ticket)
{
    if (!lp) return RMCV_ERR_BAD_ARG;
    BatchRequest q{d_frames, n_frames, w, h, stride, frame_pitch, p, stages};
    q.lp = lp;
    return submit_counted(pl, q, ticket);
}

int rmcv_pipeline_submit_windows(rmcv_pipeline* pl, const void* d_frames, int n_frames, int frame_w, int frame_h, int stride, int64_t frame_pitch,
                                 const void* d_origins, int win_w, int win_h, const rmcv_params* p, int stages, uint64_t* ticket)
{
    if (!pl) return RMCV_ERR_BAD_ARG;
    if (!d_origins) return pfail(pl, RMCV_ERR_BAD_ARG, "rmcv_pipeline_submit_windows: null origins (device memory: one rmcv_point per frame)");
    if (win_w < 1 || win_h < 1) return pfail(pl, RMCV_ERR_BAD_ARG, "rmcv_pipeline_submit_windows: window size out of range");
    BatchRequest q{d_frames, n_frames, frame_w, frame_h, stride, frame_pitch, p, stages};
    q.d_origins = d_origins, q.win_w = win_w, q.win_h = win_h;
    return submit_counted(pl, q, ticket);
}

int rmcv_pipeline_submit_tracked(rmcv_pipeline* pl, rmcv_tracker* trk, const void* d_frames, int n_frames, int frame_w, int frame_h, int stride,
                                 int64_t frame_pitch, const rmcv_params* p, int stages, int64_t timestamp, uint64_t* ticket)
{
    return rmcv_pipeline_submit_tracked_serial(pl, trk, d_frames, n_frames, frame_w, frame_h, stride, frame_pitch, nullptr, p, stages, timestamp, ticket);
}

int rmcv_pipeline_submit_tracked_serial(rmcv_pipeline* pl, rmcv_tracker* trk, const void* d_frames, int n_frames, int frame_w, int frame_h, int stride,
                                        int64_t frame_pitch, const void* d_packets, const rmcv_params* p, int stages, int64_t timestamp,
                                        uint64_t* ticket)
{
    if (!pl) return RMCV_ERR_BAD_ARG;
    if (!trk) return pfail(pl, RMCV_ERR_BAD_ARG, "rmcv_pipeline_submit_tracked: null tracker");
    const TrackerView& v = tracker_view(trk);
    BatchRequest q{d_frames, n_frames, frame_w, frame_h, stride, frame_pitch, p, stages};
    q.trk = trk, q.timestamp = timestamp, q.d_packets = d_packets;
    // win_w > 0: a windowed submit whose origins are the tracker's; win_w == 0: whole frames (track only)
    q.d_origins = v.origins, q.win_w = v.cfg.win_w, q.win_h = v.cfg.win_h;
    // a tracker with per-stream camps (rmcv_tracker_set_camps): a stream's colour is the stream's -- the submit takes the tracker's tables
    q.d_camps = v.camps, q.d_lower_bounds = v.lower_bounds;
    return submit_counted(pl, q, ticket);
}

int rmcv_pipeline_submit_camps(rmcv_pipeline* pl, const void* d_frames, int n_frames, int frame_w, int frame_h, int stride, int64_t frame_pitch,
                               const void* d_camps, const void* d_lower_bounds, const void* d_origins, int win_w, int win_h, const rmcv_params* p,
                               int stages, uint64_t* ticket)
{
    if (!pl) return RMCV_ERR_BAD_ARG;
    if (!d_camps) return pfail(pl, RMCV_ERR_BAD_ARG, "rmcv_pipeline_submit_camps: null camps (device memory: one int32 per frame)");
    if (win_w != 0 && !d_origins) return pfail(pl, RMCV_ERR_BAD_ARG, "rmcv_pipeline_submit_camps: null origins (device memory: one rmcv_point per frame; win_w == 0: whole frames)");
    if (win_w < 0 || (win_w > 0 && win_h < 1)) return pfail(pl, RMCV_ERR_BAD_ARG, "rmcv_pipeline_submit_camps: window size out of range");
    BatchRequest q{d_frames, n_frames, frame_w, frame_h, stride, frame_pitch, p, stages};
    q.d_origins = win_w > 0 ? d_origins : nullptr, q.win_w = win_w, q.win_h = win_h;
    q.d_camps = d_camps, q.d_lower_bounds = d_lower_bounds;
    return submit_counted(pl, q, ticket);
}

int rmcv_pipeline_wait(rmcv_pipeline* pl, uint64_t ticket)
{
    if (!pl) return RMCV_ERR_BAD_ARG;
    if (const int rcb = finish_newest(pl, ticket)) return rcb; // (the newest batch's back half: with the latency kernel if it is the one waited for)
    const Slot* s = live_slot(pl, ticket);
    if (!s) return RMCV_ERR_BAD_ARG;
    hipSetDevice(pl->device);
    const int rcw = pwait_event(pl, s->ev_done, "rmcv_pipeline_wait");
    return rcw || !pl->comm ? rcw : pwait_event(pl, s->ev_host, "rmcv_pipeline_wait (gather)");
}

int rmcv_pipeline_collect(rmcv_pipeline* pl, uint64_t ticket, rmcv_armour* armours_out, int cap, int32_t* frame_offs, int32_t* n_total)
{
    if (!pl || cap < 0) return RMCV_ERR_BAD_ARG;
    int rc = rmcv_pipeline_wait(pl, ticket);
    if (rc) return rc;
    const Slot& S = *live_slot(pl, ticket);
    const int64_t head = pl->rec.head_bytes;
    std::vector<uint8_t> tmp;
    const uint8_t* rec = S.h_rec;
    if (pl->cfg.host_results != 1) { // lists stay on the device until asked for: the head first, then exactly the armours there are
        tmp.resize((size_t)head);
        PCHK(pl, hipMemcpy(tmp.data(), S.d_rec, (size_t)head, hipMemcpyDeviceToHost), "pipeline: D2H head");
        rec = tmp.data();
    }
    const int32_t* offs = reinterpret_cast<const int32_t*>(rec);
    const int32_t total = offs[S.frames], st = offs[pl->rec.status_word];
    if (n_total) *n_total = total;
    if (frame_offs) memcpy(frame_offs, offs, (size_t)(S.frames + 1) * 4);
    pl->collected++;
    if (st & (RMCV_FRAME_OVF_CONTOURS | RMCV_FRAME_OVF_POINTS | RMCV_FRAME_OVF_BLOBS | RMCV_FRAME_OVF_ARMOURS))
        return pfail(pl, RMCV_ERR_CAPACITY, "context limits exceeded on at least one frame of the batch (rmcv_batch_counts on the slot's context names it)");
    if (total > pl->cfg.armour_cap) return pfail(pl, RMCV_ERR_CAPACITY, "the batch has more armours than the pipeline's armour_cap");
    if (total > cap) return pfail(pl, RMCV_ERR_CAPACITY, "output capacity exceeded");
    if (armours_out && total) {
        if (pl->cfg.host_results == 1) memcpy(armours_out, rec + head, (size_t)total * sizeof(rmcv_armour));
        else PCHK(pl, hipMemcpy(armours_out, S.d_rec + head, (size_t)total * sizeof(rmcv_armour), hipMemcpyDeviceToHost), "pipeline: D2H armours");
    }
    return RMCV_OK;
}

int rmcv_pipeline_drain(rmcv_pipeline* pl)
{
    if (!pl) return RMCV_ERR_BAD_ARG;
    hipSetDevice(pl->device);
    int rcw = finish_back(pl, true);
    if (rcw) return rcw;
    for (auto s : pl->pix) if ((rcw = pwait_stream(pl, s, "rmcv_pipeline_drain (pixel stream)"))) return rcw;
    for (auto s : pl->sp) if ((rcw = pwait_stream(pl, s, "rmcv_pipeline_drain (sparse stream)"))) return rcw;
    for (auto s : pl->dn) if ((rcw = pwait_stream(pl, s, "rmcv_pipeline_drain (dense stream)"))) return rcw;
    for (auto& s : pl->slots)
        if (s.ev_hook) {
            if ((rcw = pwait_event(pl, (hipEvent_t)s.ev_hook, "rmcv_pipeline_drain (hook)"))) return rcw;
            s.ev_hook = nullptr;
        }
    return RMCV_OK;
}

int rmcv_pipeline_record(rmcv_pipeline* pl, uint64_t ticket, void** d_record, void** hip_stream)
{
    if (!pl) return RMCV_ERR_BAD_ARG;
    if (const int rcb = finish_newest(pl, ticket)) return rcb;
    const Slot* s = live_slot(pl, ticket);
    if (!s) return RMCV_ERR_BAD_ARG;
    if (d_record) *d_record = s->d_rec;
    if (hip_stream) *hip_stream = s->stream;
    return RMCV_OK;
}

// rmcv_pipeline_set_views, rmcv_pipeline_set_source_views and rmcv_pipeline_set_sheets (side > 0): one set of views per pipeline, of the kind set last
static int set_views(rmcv_pipeline* pl, const int32_t* frames, int n, int vw, int vh, int flags, bool source, int side = 0, bool sheets = false)
{
    if (!pl || n < 0) return RMCV_ERR_BAD_ARG;
    hipSetDevice(pl->device);
    // the slots' buffers may be replaced: everything submitted so far is through first (this call may block; no submit does)
    int rc = rmcv_pipeline_drain(pl);
    if (rc) return rc;
    if (n == 0) {
        pl->views.n = 0;
        pl->views.label_what = 0; // (labels are drawn over views: off with them)
        return RMCV_OK;
    }
    rmcv_ctx* c0 = pl->ring[0];
    if (sheets) rc = ctx_sheet_check(c0, frames, n, pl->lim.max_frames, ~0, vw, vh, side, flags, 6 * vw, (int64_t)6 * vw * ((int64_t)vh + side));
    else rc = (source ? ctx_source_view_check : ctx_view_check)(c0, frames, n, pl->lim.max_frames, ~0, vw, vh, flags, 3 * vw, (int64_t)3 * vw * vh);
    if (rc) return cfail(pl, c0, rc);
    pl->views.n = 0; // (off, should anything below fail)
    for (auto c : pl->ring)
        if ((rc = ctx_view_prepare(c, n))) return cfail(pl, c, rc);
    const size_t bytes = sheets ? (size_t)n * 6 * vw * ((size_t)vh + side) : (size_t)n * 3 * vw * vh;
    hipError_t e = hipSuccess;
    for (auto& S : pl->slots) {
        if (S.d_views) (void)hipFree(S.d_views);
        S.d_views = nullptr;
        S.view_n = 0;
        if (e == hipSuccess) e = hipMalloc((void**)&S.d_views, bytes);
    }
    if (pl->views.d_frames) (void)hipFree(pl->views.d_frames);
    pl->views.d_frames = nullptr;
    if (e == hipSuccess) e = hipMalloc((void**)&pl->views.d_frames, (size_t)n * 4);
    if (e == hipSuccess) e = hipMemcpy(pl->views.d_frames, frames, (size_t)n * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) return pfail(pl, e == hipErrorOutOfMemory ? RMCV_ERR_NOMEM : RMCV_ERR_HIP, sheets ? "rmcv_pipeline_set_sheets" : source ? "rmcv_pipeline_set_source_views" : "rmcv_pipeline_set_views", e);
    int top = 0;
    for (int k = 0; k < n; k++) top = frames[k] > top ? frames[k] : top;
    pl->views.vw = vw, pl->views.vh = vh, pl->views.flags = flags, pl->views.max_index = top;
    pl->views.need = view_stages_needed(flags) | (sheets ? RMCV_STAGE_ARMOURS : 0);
    pl->views.source = source;
    pl->views.side = sheets ? side : 0;
    pl->views.n = n;
    return RMCV_OK;
}

int rmcv_pipeline_set_views(rmcv_pipeline* pl, const int32_t* frames, int n, int vw, int vh, int flags) { return set_views(pl, frames, n, vw, vh, flags, false); }

int rmcv_pipeline_set_source_views(rmcv_pipeline* pl, const int32_t* frames, int n, int vw, int vh, int flags) { return set_views(pl, frames, n, vw, vh, flags, true); }

int rmcv_pipeline_set_sheets(rmcv_pipeline* pl, const int32_t* frames, int n, int vw, int vh, int side, int flags) { return set_views(pl, frames, n, vw, vh, flags, true, side, true); }

int rmcv_pipeline_set_view_labels(rmcv_pipeline* pl, int what, int scale)
{
    if (!pl) return RMCV_ERR_BAD_ARG;
    hipSetDevice(pl->device);
    // the batch in hand keeps the labels it was submitted under: everything submitted so far is through first (this call may block; no submit does)
    const int rc = rmcv_pipeline_drain(pl);
    if (rc) return rc;
    if (what == 0) {
        pl->views.label_what = 0;
        return RMCV_OK;
    }
    if (what < 0 || what > (RMCV_LABEL_ARMOURS | RMCV_LABEL_TRACKS)) return pfail(pl, RMCV_ERR_BAD_ARG, "rmcv_pipeline_set_view_labels: unknown RMCV_LABEL_* bits");
    if (scale < 1 || scale > 8) return pfail(pl, RMCV_ERR_BAD_ARG, "rmcv_pipeline_set_view_labels: scale outside 1 .. 8");
    if (!pl->views.n) return pfail(pl, RMCV_ERR_BAD_ARG, "rmcv_pipeline_set_view_labels: no views are set (rmcv_pipeline_set_views, rmcv_pipeline_set_source_views)");
    pl->views.label_what = what, pl->views.label_scale = scale;
    return RMCV_OK;
}

int rmcv_pipeline_set_recorder(rmcv_pipeline* pl, rmcv_recorder* rec, const int32_t* frames, int n)
{
    if (!pl || n < 0) return RMCV_ERR_BAD_ARG;
    hipSetDevice(pl->device);
    // batches in flight keep the recorder they were submitted under: everything submitted so far is through first (this call may block)
    int rc = rmcv_pipeline_drain(pl);
    if (rc) return rc;
    if (n == 0 || !rec) {
        pl->recd.n = 0, pl->recd.rec = nullptr;
        return RMCV_OK;
    }
    if (!frames) return pfail(pl, RMCV_ERR_BAD_ARG, "rmcv_pipeline_set_recorder: null frame list");
    // (the rows and the height are the batch's: checked at every submit)
    if (const char* no = recorder_refusal(rec, pl->device, n, 1, 1)) return pfail(pl, RMCV_ERR_BAD_ARG, no);
    if (const char* no = recorder_trigger_refusal(rec, pl->cfg.depth)) return pfail(pl, RMCV_ERR_BAD_ARG, no);
    int top = 0;
    for (int k = 0; k < n; k++) {
        if (frames[k] < 0 || frames[k] >= pl->lim.max_frames) return pfail(pl, RMCV_ERR_BAD_ARG, "rmcv_pipeline_set_recorder: a frame index out of range");
        for (int q = 0; q < k; q++) if (frames[q] == frames[k]) return pfail(pl, RMCV_ERR_BAD_ARG, "rmcv_pipeline_set_recorder: a frame index is repeated");
        top = frames[k] > top ? frames[k] : top;
    }
    pl->recd.rec = rec, pl->recd.max_index = top;
    for (int k = 0; k < n; k++) pl->recd.frames[k] = frames[k];
    pl->recd.n = n;
    return RMCV_OK;
}

int rmcv_pipeline_set_harvest(rmcv_pipeline* pl, rmcv_dataset* ds, const int32_t* labels, int n_labels, int flags)
{
    if (!pl) return RMCV_ERR_BAD_ARG;
    hipSetDevice(pl->device);
    // batches in flight keep the dataset and the labels they were submitted under: everything submitted so far is through first (this call may block)
    int rc = rmcv_pipeline_drain(pl);
    if (rc) return rc;
    pl->harv.ds = nullptr; // (off, should anything below fail)
    if (pl->harv.d_labels) (void)hipFree(pl->harv.d_labels);
    pl->harv.d_labels = nullptr;
    if (!ds) return RMCV_OK;
    if (!labels) return pfail(pl, RMCV_ERR_BAD_ARG, "rmcv_pipeline_set_harvest: null labels");
    if (n_labels < 1 || n_labels > pl->lim.max_frames) return pfail(pl, RMCV_ERR_BAD_ARG, "rmcv_pipeline_set_harvest: n_labels outside 1 .. max_frames");
    // (the frames and the stages are the batch's: checked at every submit)
    if (const char* no = ctx_harvest_refusal(pl->device, 1, true, ds, n_labels, flags, ~0, pl->lim.max_armours)) return pfail(pl, RMCV_ERR_BAD_ARG, no);
    hipError_t e = hipMalloc((void**)&pl->harv.d_labels, (size_t)n_labels * 4);
    if (e == hipSuccess) e = hipMemcpy(pl->harv.d_labels, labels, (size_t)n_labels * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) return pfail(pl, e == hipErrorOutOfMemory ? RMCV_ERR_NOMEM : RMCV_ERR_HIP, "rmcv_pipeline_set_harvest", e);
    pl->harv.ds = ds, pl->harv.n_labels = n_labels, pl->harv.flags = flags;
    return RMCV_OK;
}

int rmcv_pipeline_views(rmcv_pipeline* pl, uint64_t ticket, void** d_views, int32_t* stride, int64_t* pitch, int32_t* n)
{
    if (!pl) return RMCV_ERR_BAD_ARG;
    if (const int rcb = finish_newest(pl, ticket)) return rcb;
    const Slot* s = live_slot(pl, ticket);
    if (!s) return RMCV_ERR_BAD_ARG;
    if (!s->view_n) return pfail(pl, RMCV_ERR_BAD_ARG, "rmcv_pipeline_views: the ticket's batch was submitted without views");
    if (d_views) *d_views = s->d_views;
    if (stride) *stride = 3 * s->view_w; // (a sheet's view_w is its own: 2 vw, and view_h its vh + side)
    if (pitch) *pitch = (int64_t)3 * s->view_w * s->view_h;
    if (n) *n = s->view_n;
    return RMCV_OK;
}

int rmcv_pipeline_gathered(rmcv_pipeline* pl, uint64_t ticket, void** d_recv, int64_t* bytes)
{
    if (!pl) return RMCV_ERR_BAD_ARG;
    if (const int rcb = finish_newest(pl, ticket)) return rcb; // (before the other argument checks, as ever)
    if (!pl->comm) return RMCV_ERR_BAD_ARG;
    const Slot* s = live_slot(pl, ticket);
    if (!s) return RMCV_ERR_BAD_ARG;
    if (d_recv) *d_recv = pl->rank == pl->root ? s->d_recv : nullptr;
    if (bytes) *bytes = pl->rec.record_bytes * pl->n_ranks;
    return RMCV_OK;
}

// ---- device memory for hosts without HIP headers ----
int rmcv_device_alloc(int device, int64_t bytes, void** d_ptr)
{
    if (!d_ptr || bytes <= 0) return RMCV_ERR_BAD_ARG;
    *d_ptr = nullptr;
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return RMCV_ERR_NO_DEVICE; }
    const hipError_t e = hipMalloc(d_ptr, (size_t)bytes);
    if (e != hipSuccess) { (void)hipGetLastError(); return e == hipErrorOutOfMemory ? RMCV_ERR_NOMEM : RMCV_ERR_HIP; }
    return RMCV_OK;
}

void rmcv_device_free(int device, void* d_ptr)
{
    if (!d_ptr) return;
    if (hipSetDevice(device) == hipSuccess) (void)hipFree(d_ptr);
    (void)hipGetLastError();
}

int rmcv_device_upload(int device, void* d_dst, const void* h_src, int64_t bytes)
{
    if (!d_dst || !h_src || bytes < 0) return RMCV_ERR_BAD_ARG;
    if (hipSetDevice(device) != hipSuccess || hipMemcpy(d_dst, h_src, (size_t)bytes, hipMemcpyHostToDevice) != hipSuccess) { (void)hipGetLastError(); return RMCV_ERR_HIP; }
    return RMCV_OK;
}

int rmcv_device_download(int device, void* h_dst, const void* d_src, int64_t bytes)
{
    if (!h_dst || !d_src || bytes < 0) return RMCV_ERR_BAD_ARG;
    if (hipSetDevice(device) != hipSuccess || hipMemcpy(h_dst, d_src, (size_t)bytes, hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return RMCV_ERR_HIP; }
    return RMCV_OK;
}

} // extern "C"
