// rmcv_record.hip -- rmcv_recorder_* and rmcv_session_*: the session recorder behind the C-ABI (include/rmcv_abi.h).
//
// The reference's rm::debug::logger (include/debug.h:13-29, src/debug.cpp:9-41) writes every frame the detector saw to a lossless video and
// a `data` record beside it.  Here the frames are in HBM and a batch is one non-blocking submit, so the recorder is a ring in HBM too:
// slot = sequence mod slots, every chosen frame a fixed area of rmcv_pack_bound bytes (no allocator on the device), a small device table
// of the packed sizes (and the batch's effective keys and window origins), and on the host the entry with everything known at the submit.
// Recording is three launches and two event calls on the caller's stream; the readers wait for the slot's event with the 5 s deadline.
// With track_cap > 0 a tracked batch of a pipeline also gets loop records (k_loop.hip): a second fixed area per chosen frame, written by
// one launch behind the batch's tracker step -- on another stream and a pipeline call later than the packing, so the slot has a second
// event and the readers wait for both -- and the trigger latch, whose mapped host copy recorder_enqueue reads with a plain load.
#include <stdio.h>
#include <string.h>

#include <new>
#include <vector>

#include "rmcv_internal.h"
#include "session_file.h"

using namespace rmcv;

struct RecSlot {
    uint8_t* d_area = nullptr;       // [max_frames] areas of `area` bytes
    int64_t* d_sizes = nullptr;      // [max_frames]
    int32_t* d_keys = nullptr;       // [max_frames][4]
    int32_t* d_camps = nullptr;      // [max_frames]
    rmcv_point* d_origins = nullptr; // [max_frames]
    hipEvent_t ev = nullptr;         // behind the slot's last packing
    uint8_t* d_loop = nullptr;       // [max_frames] loop areas of `loop_bytes` bytes (track_cap > 0)
    hipEvent_t ev_loop = nullptr;    // behind the slot's last k_loop_record
    bool used = false;
    bool loop_on = false;            // the slot's batch has loop records ...
    bool loop_pending = false;       // ... whose launch has not been enqueued yet (the pipeline's next call does)
    bool loop_ever = false;          // ev_loop has been recorded
    bool chained = false;            // the batch may be compared with the previous slot's (no resume in between)
    const rmcv_tracker* trk = nullptr; // the tracker of the slot's batch (compared, never dereferenced)
    rmcv_record_entry e{};           // (sizes, keys, origins: filled by the readers)
    std::vector<uint8_t> user;
};

struct rmcv_recorder {
    int device = 0;
    rmcv_recorder_config cfg{};
    int64_t area = 0;                // rmcv_pack_bound(max_w_bytes, max_h)
    std::vector<RecSlot> slots;
    uint64_t seq = 0;                // batches recorded
    bool frozen = false;
    int64_t loop_bytes = 0;          // loop_bound(track_cap); 0: no loop records
    // the trigger latch (track_cap > 0): a device word taken by compare-and-swap, the latch record in device memory and in mapped host memory
    uint32_t* d_latch_word = nullptr;
    LoopLatch *d_latch = nullptr, *h_latch = nullptr, *hd_latch = nullptr;
    rmcv_trigger_config trig{};      // mask 0: off
    bool noticed = false;            // a recorder_enqueue has seen the latch ...
    int remaining = 0;               // ... and this many batches are still recorded
    int since = 0;                   // batches recorded since it was noticed
    bool rechain = true;             // the next batch has no predecessor (the first one; the first after a resume)
    std::vector<uint8_t> user;       // the blob of the next batch
    int wait_timeout_ms = 5000;
    char err[256] = {0};
};

struct rmcv_session {
    std::vector<uint8_t> data;
    std::vector<SessionRec> recs;
};

static int rfail(rmcv_recorder* r, int code, const char* what, hipError_t e = hipSuccess)
{
    if (r) {
        if (e != hipSuccess) snprintf(r->err, sizeof(r->err), "%s: %s", what, hipGetErrorString(e));
        else snprintf(r->err, sizeof(r->err), "%s", what);
    }
    if (e != hipSuccess) (void)hipGetLastError();
    return code;
}

static int held(const rmcv_recorder* r) { return (int)(r->seq < (uint64_t)r->cfg.slots ? r->seq : (uint64_t)r->cfg.slots); }
// the slot of held batch i (0: the oldest), once its packing is through; null with the error set
static RecSlot* held_slot(rmcv_recorder* r, int i, int* rc)
{
    const int n = held(r);
    if (i < 0 || i >= n) { *rc = rfail(r, RMCV_ERR_BAD_ARG, "no such batch in the recorder"); return nullptr; }
    RecSlot& S = r->slots[(size_t)((r->seq - (uint64_t)n + (uint64_t)i) % (uint64_t)r->cfg.slots)];
    hipSetDevice(r->device);
    hipError_t e = hipSuccess;
    const int rcw = wait_event_deadline(S.ev, r->wait_timeout_ms, &e);
    if (rcw < 0) { *rc = rfail(r, RMCV_ERR_HIP, "recorder: wait for the packing", e); return nullptr; }
    if (rcw > 0) { *rc = rfail(r, RMCV_ERR_TIMEOUT, "recorder: the packing has not finished after 5000 ms"); return nullptr; }
    if (S.loop_on) { // the loop records: a launch of the pipeline call AFTER the batch's submit, on the stream of its tracker step
        if (S.loop_pending) { *rc = rfail(r, RMCV_ERR_BAD_ARG, "recorder: the newest batch's tracker step has not been enqueued yet (rmcv_pipeline_wait its ticket, or drain, first)"); return nullptr; }
        const int rcl = wait_event_deadline(S.ev_loop, r->wait_timeout_ms, &e);
        if (rcl < 0) { *rc = rfail(r, RMCV_ERR_HIP, "recorder: wait for the loop records", e); return nullptr; }
        if (rcl > 0) { *rc = rfail(r, RMCV_ERR_TIMEOUT, "recorder: the loop records have not finished after 5000 ms"); return nullptr; }
    }
    return &S;
}
// the device's part of a slot's entry
static int slot_tables(rmcv_recorder* r, RecSlot& S)
{
    rmcv_record_entry& e = S.e;
    const size_t n = (size_t)e.n_frames;
    hipError_t h = n ? hipMemcpy(e.sizes, S.d_sizes, n * 8, hipMemcpyDeviceToHost) : hipSuccess;
    if (h == hipSuccess && e.has_keys && n) h = hipMemcpy(e.keys, S.d_keys, n * 16, hipMemcpyDeviceToHost);
    if (h == hipSuccess && e.has_keys && n) h = hipMemcpy(e.camps, S.d_camps, n * 4, hipMemcpyDeviceToHost);
    if (h == hipSuccess && e.has_origins && n) h = hipMemcpy(e.origins, S.d_origins, n * sizeof(rmcv_point), hipMemcpyDeviceToHost);
    if (h != hipSuccess) return rfail(r, RMCV_ERR_HIP, "recorder: D2H tables", h);
    for (size_t k = 0; k < n; k++)
        if (e.sizes[k] < 0 || e.sizes[k] > r->area) return rfail(r, RMCV_ERR_HIP, "recorder: a packed size beyond its area");
    return RMCV_OK;
}

namespace rmcv {

const char* recorder_refusal(const rmcv_recorder* r, int device, int n, int w_bytes, int h)
{
    if (!r) return "null recorder";
    if (device != r->device) return "the recorder lives on another device";
    if (n < 1 || n > r->cfg.max_frames) return "more frames chosen than the recorder's max_frames (or none)";
    if (w_bytes < 1 || w_bytes > r->cfg.max_w_bytes || h < 1 || h > r->cfg.max_h) return "the frames' rows or height are beyond the recorder's max_w_bytes / max_h";
    return nullptr;
}

const char* recorder_trigger_refusal(const rmcv_recorder* r, int depth)
{
    if (!r || !r->trig.mask) return nullptr;
    return r->cfg.slots < loop_ring_bound(depth, r->trig.post_batches)
               ? "the recorder's triggers are armed and its ring is smaller than the pipeline's depth + post_batches: the triggering batch could be overwritten before the recorder freezes (rmcv_recorder_set_trigger)"
               : nullptr;
}

int recorder_enqueue(rmcv_recorder* r, const RecordBatch& b, const int32_t* frames, int n, hipStream_t s, LoopTicket* loop)
{
    if (loop) *loop = LoopTicket{};
    // the trigger latch: a plain load of the mapped host copy.  Once seen, post_batches more batches are recorded, this one the first
    if (r->trig.mask && !r->frozen && !r->noticed && r->h_latch && *(volatile int32_t*)&r->h_latch->set) {
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        r->noticed = true, r->remaining = r->trig.post_batches, r->since = 0;
    }
    if (r->noticed && !r->frozen) {
        if (r->remaining == 0) r->frozen = true;
        else r->remaining--, r->since++;
    }
    if (r->frozen) return RMCV_OK;
    const int w_bytes = b.w_bytes, lag = b.lag;
    RecSlot& S = r->slots[(size_t)(r->seq % (uint64_t)r->cfg.slots)];
    // the slot's last packing may have run on another stream: this one goes behind it, on the GPU
    if (S.used) {
        const hipError_t e = hipStreamWaitEvent(s, S.ev, 0);
        if (e != hipSuccess) return rfail(r, RMCV_ERR_HIP, "recorder: wait for the slot", e);
    }
    PackJob j{};
    j.frames = (const uint8_t*)b.d_frames, j.pitch = b.pitch, j.stride = b.stride, j.w_bytes = w_bytes, j.h = b.h, j.lag = lag, j.n = n;
    j.out = S.d_area, j.out_pitch = r->area, j.sizes = S.d_sizes;
    j.use_idx = 1;
    for (int k = 0; k < n; k++) j.idx.f[k] = frames[k];
    if (b.key_eff) j.key_eff = b.key_eff, j.keys_out = S.d_keys, j.key_enemy = b.key_enemy, j.camps_out = S.d_camps;
    if (b.win_eff) j.win_eff = b.win_eff, j.origins_out = S.d_origins;
    hipError_t e = launch_pack(j, s);
    if (e == hipSuccess) e = hipEventRecord(S.ev, s);
    if (e != hipSuccess) return rfail(r, RMCV_ERR_HIP, "recorder: k_pack", e);
    rmcv_record_entry& E = S.e;
    memset(&E, 0, sizeof(E));
    E.ticket = b.ticket, E.sequence = r->seq, E.timestamp = b.timestamp;
    E.n_frames = n, E.batch_frames = b.batch_frames, E.w = b.w, E.h = b.h, E.w_bytes = w_bytes, E.stride = b.stride, E.lag = lag;
    E.input_format = b.input_format, E.sample_bits = b.sample_bits, E.valid_bit = b.valid_bit, E.orient = b.orient, E.stages = b.stages;
    E.win_w = b.win_w, E.win_h = b.win_h, E.has_keys = b.key_eff != nullptr, E.has_origins = b.win_eff != nullptr;
    E.user_bytes = (int32_t)r->user.size();
    E.params = b.params;
    for (int k = 0; k < n; k++) E.frames[k] = frames[k];
    S.user = r->user;
    S.used = true;
    S.loop_on = S.loop_pending = b.trk && r->loop_bytes;
    S.trk = b.trk;
    S.chained = !r->rechain;
    r->rechain = false;
    if (S.loop_on) {
        E.loop_bytes = (int32_t)r->loop_bytes;
        if (loop) loop->rec = r, loop->slot = (int)(r->seq % (uint64_t)r->cfg.slots), loop->sequence = r->seq;
    }
    r->seq++;
    return RMCV_OK;
}

int recorder_loop_begin(const LoopTicket& t, const rmcv_tracker* trk, LoopArgs* a, hipStream_t s)
{
    rmcv_recorder* r = t.rec;
    const int slots = r->cfg.slots;
    RecSlot& S = r->slots[(size_t)t.slot];
    if (!S.used || S.e.sequence != t.sequence || !S.loop_on) return rfail(r, RMCV_ERR_BAD_ARG, "recorder: the batch's slot has been reused before its tracker step was enqueued");
    const rmcv_record_entry& E = S.e;
    a->n = E.n_frames, a->rec_cap = r->cfg.track_cap;
    for (int k = 0; k < E.n_frames; k++) a->idx.f[k] = E.frames[k];
    a->out = S.d_loop, a->pitch = r->loop_bytes, a->prev = nullptr, a->sequence = t.sequence;
    // the predecessor: the previous slot, when it holds the immediately preceding sequence of the same tracker with the same chosen frames,
    // recorded with loop records, and no resume lies between
    const RecSlot& P = r->slots[(size_t)((t.slot + slots - 1) % slots)];
    if (slots >= 2 && S.chained && t.sequence > 0 && P.used && P.e.sequence + 1 == t.sequence && P.loop_on && !P.loop_pending && P.trk == trk &&
        P.e.n_frames == E.n_frames && memcmp(P.e.frames, E.frames, (size_t)E.n_frames * 4) == 0)
        a->prev = P.d_loop;
    a->trig = r->trig;
    a->latch_word = r->d_latch_word, a->d_latch = r->d_latch, a->hd_latch = r->hd_latch;
    // the areas are rewritten: the launch that wrote them last, and the one that read them as ITS predecessor (the next slot's), may have run
    // on other streams
    const RecSlot& N = r->slots[(size_t)((t.slot + 1) % slots)];
    hipError_t e = S.loop_ever ? hipStreamWaitEvent(s, S.ev_loop, 0) : hipSuccess;
    if (e == hipSuccess && &N != &S && N.loop_ever) e = hipStreamWaitEvent(s, N.ev_loop, 0);
    if (e != hipSuccess) return rfail(r, RMCV_ERR_HIP, "recorder: wait for the slot's loop records", e);
    return RMCV_OK;
}

int recorder_loop_end(const LoopTicket& t, hipStream_t s)
{
    rmcv_recorder* r = t.rec;
    RecSlot& S = r->slots[(size_t)t.slot];
    const hipError_t e = hipEventRecord(S.ev_loop, s);
    if (e != hipSuccess) return rfail(r, RMCV_ERR_HIP, "recorder: k_loop_record", e);
    S.loop_ever = true;
    S.loop_pending = false;
    return RMCV_OK;
}

} // namespace rmcv

extern "C" {

void rmcv_default_recorder_config(rmcv_recorder_config* c)
{
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->slots = 8, c->max_frames = 8, c->max_w_bytes = 3 * 1280, c->max_h = 1024, c->user_bytes = 256;
}

void rmcv_recorder_destroy(rmcv_recorder* r)
{
    if (!r) return;
    hipSetDevice(r->device);
    for (auto& S : r->slots) { // with the deadline: a packing that does not finish is not waited for without one
        hipError_t e = hipSuccess;
        if ((S.used && wait_event_deadline(S.ev, r->wait_timeout_ms, &e) > 0) || (S.loop_ever && wait_event_deadline(S.ev_loop, r->wait_timeout_ms, &e) > 0)) {
            fprintf(stderr, "rmcv_recorder_destroy: a packing has not finished; the recorder's buffers are leaked\n");
            return;
        }
    }
    for (auto& S : r->slots) {
        for (void* p : {(void*)S.d_area, (void*)S.d_sizes, (void*)S.d_keys, (void*)S.d_camps, (void*)S.d_origins, (void*)S.d_loop}) if (p) (void)hipFree(p);
        if (S.ev) (void)hipEventDestroy(S.ev);
        if (S.ev_loop) (void)hipEventDestroy(S.ev_loop);
    }
    for (void* p : {(void*)r->d_latch_word, (void*)r->d_latch}) if (p) (void)hipFree(p);
    if (r->h_latch) (void)hipHostFree(r->h_latch);
    (void)hipGetLastError();
    delete r;
}

int rmcv_recorder_create(int device, const rmcv_recorder_config* cfg, rmcv_recorder** out)
{
    if (!out) return RMCV_ERR_BAD_ARG;
    *out = nullptr;
    rmcv_recorder_config c;
    rmcv_default_recorder_config(&c);
    if (cfg) {
        if (cfg->slots) c.slots = cfg->slots;
        if (cfg->max_frames) c.max_frames = cfg->max_frames;
        if (cfg->max_w_bytes) c.max_w_bytes = cfg->max_w_bytes;
        if (cfg->max_h) c.max_h = cfg->max_h;
        if (cfg->user_bytes) c.user_bytes = cfg->user_bytes;
        c.track_cap = cfg->track_cap; // (0: no loop records -- nothing below is allocated, nothing further is ever launched)
    }
    if (c.slots < 1 || c.slots > 4096 || c.max_frames < 1 || c.max_frames > RMCV_RECORDER_MAX_FRAMES || c.user_bytes < 0 || c.user_bytes > (1 << 20) ||
        !pack_geometry_ok(c.max_w_bytes, c.max_h, 1) || c.track_cap < 0 || c.track_cap > RMCV_TRACKER_MAX_CAP)
        return RMCV_ERR_BAD_ARG;
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return RMCV_ERR_NO_DEVICE; }
    rmcv_recorder* r = new (std::nothrow) rmcv_recorder();
    if (!r) return RMCV_ERR_NOMEM;
    r->device = device, r->cfg = c, r->area = pack_bound(c.max_w_bytes, c.max_h);
    r->loop_bytes = c.track_cap ? loop_bound(c.track_cap) : 0;
    r->trig.aim_jump_deg = __builtin_inf(); // (triggers off: the records' fired is the rule with no jump bound and no status bits)
    r->slots.resize((size_t)c.slots);
    hipError_t e = hipSuccess;
    const size_t n = (size_t)c.max_frames;
    for (auto& S : r->slots) {
        if (e == hipSuccess) e = hipMalloc((void**)&S.d_area, n * (size_t)r->area);
        if (e == hipSuccess) e = hipMalloc((void**)&S.d_sizes, n * 8);
        if (e == hipSuccess) e = hipMalloc((void**)&S.d_keys, n * 16);
        if (e == hipSuccess) e = hipMalloc((void**)&S.d_camps, n * 4);
        if (e == hipSuccess) e = hipMalloc((void**)&S.d_origins, n * sizeof(rmcv_point));
        if (e == hipSuccess) e = hipEventCreateWithFlags(&S.ev, hipEventDisableTiming);
        if (e == hipSuccess && r->loop_bytes) e = hipMalloc((void**)&S.d_loop, n * (size_t)r->loop_bytes);
        if (e == hipSuccess && r->loop_bytes) e = hipEventCreateWithFlags(&S.ev_loop, hipEventDisableTiming);
    }
    if (r->loop_bytes) { // the latch: free
        if (e == hipSuccess) e = hipMalloc((void**)&r->d_latch_word, sizeof(uint32_t));
        if (e == hipSuccess) e = hipMalloc((void**)&r->d_latch, sizeof(LoopLatch));
        if (e == hipSuccess) e = hipHostMalloc((void**)&r->h_latch, sizeof(LoopLatch), hipHostMallocMapped);
        if (e == hipSuccess) memset(r->h_latch, 0, sizeof(LoopLatch));
        if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&r->hd_latch, r->h_latch, 0);
        if (e == hipSuccess) e = hipMemset(r->d_latch_word, 0, sizeof(uint32_t));
        if (e == hipSuccess) e = hipMemset(r->d_latch, 0, sizeof(LoopLatch));
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        rmcv_recorder_destroy(r);
        return e == hipErrorOutOfMemory ? RMCV_ERR_NOMEM : (e == hipErrorNoDevice || e == hipErrorInvalidDevice ? RMCV_ERR_NO_DEVICE : RMCV_ERR_HIP);
    }
    *out = r;
    return RMCV_OK;
}

const char* rmcv_recorder_last_error(const rmcv_recorder* r) { return r ? r->err : "null recorder"; }

int rmcv_recorder_set_user(rmcv_recorder* r, const void* data, int bytes)
{
    if (!r || bytes < 0 || (bytes > 0 && !data)) return RMCV_ERR_BAD_ARG;
    if (bytes > r->cfg.user_bytes) return rfail(r, RMCV_ERR_BAD_ARG, "the user blob is larger than the recorder's user_bytes");
    r->user.assign((const uint8_t*)data, (const uint8_t*)data + bytes);
    return RMCV_OK;
}

int rmcv_recorder_record(rmcv_recorder* r, const void* d_frames, int w_bytes, int h, int stride, int64_t pitch, int lag, const int32_t* frames, int n,
                         void* hip_stream)
{
    if (!r) return RMCV_ERR_BAD_ARG;
    if (const char* no = recorder_refusal(r, r->device, n, w_bytes, h)) return rfail(r, RMCV_ERR_BAD_ARG, no);
    if (const char* no = pack_job_refusal(d_frames, n, w_bytes, h, stride, pitch, lag, r->slots[0].d_area, r->area)) return rfail(r, RMCV_ERR_BAD_ARG, no);
    int32_t idx[RMCV_RECORDER_MAX_FRAMES];
    int top = 0;
    for (int k = 0; k < n; k++) {
        idx[k] = frames ? frames[k] : k;
        if (idx[k] < 0) return rfail(r, RMCV_ERR_BAD_ARG, "a negative frame index");
        for (int q = 0; q < k; q++) if (idx[q] == idx[k]) return rfail(r, RMCV_ERR_BAD_ARG, "a frame index is repeated");
        top = idx[k] > top ? idx[k] : top;
    }
    if (top > 0 && pitch < (int64_t)stride * (h - 1) + w_bytes) return rfail(r, RMCV_ERR_BAD_ARG, "frame pitch smaller than a frame");
    hipSetDevice(r->device);
    // (a stand-alone record describes a plane of bytes: the format fields say "one byte a sample" and the lag is the caller's)
    RecordBatch b{};
    b.d_frames = d_frames, b.w = w_bytes, b.h = h, b.stride = stride, b.pitch = pitch, b.batch_frames = top + 1;
    b.w_bytes = w_bytes, b.lag = lag, b.input_format = -1, b.sample_bits = 8, b.ticket = r->seq;
    return recorder_enqueue(r, b, idx, n, (hipStream_t)hip_stream);
}

int rmcv_recorder_freeze(rmcv_recorder* r) { if (!r) return RMCV_ERR_BAD_ARG; r->frozen = true; return RMCV_OK; }
int rmcv_recorder_resume(rmcv_recorder* r)
{
    if (!r) return RMCV_ERR_BAD_ARG;
    if (r->loop_bytes) { // clear the latch and re-arm it: behind every launch of the recorder's that is in flight (this call may block; no submit does)
        hipSetDevice(r->device);
        for (auto& S : r->slots) {
            hipError_t e = hipSuccess;
            const int rcw = S.loop_ever ? wait_event_deadline(S.ev_loop, r->wait_timeout_ms, &e) : 0;
            if (rcw < 0) return rfail(r, RMCV_ERR_HIP, "rmcv_recorder_resume: wait for the loop records", e);
            if (rcw > 0) return rfail(r, RMCV_ERR_TIMEOUT, "rmcv_recorder_resume: the loop records have not finished after 5000 ms");
        }
        hipError_t e = hipMemset(r->d_latch_word, 0, sizeof(uint32_t));
        if (e == hipSuccess) e = hipMemset(r->d_latch, 0, sizeof(LoopLatch));
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        if (e != hipSuccess) return rfail(r, RMCV_ERR_HIP, "rmcv_recorder_resume: clearing the latch", e);
        memset(r->h_latch, 0, sizeof(LoopLatch));
        r->noticed = false, r->remaining = 0, r->since = 0;
    }
    r->rechain = true; // (the first batch behind a resume has no predecessor)
    r->frozen = false;
    return RMCV_OK;
}

int rmcv_recorder_set_trigger(rmcv_recorder* r, const rmcv_trigger_config* cfg)
{
    if (!r) return RMCV_ERR_BAD_ARG;
    if (!cfg) { r->trig = rmcv_trigger_config{}; r->trig.aim_jump_deg = __builtin_inf(); return RMCV_OK; }
    if (const char* no = loop_trigger_refusal(cfg)) return rfail(r, RMCV_ERR_BAD_ARG, no);
    if (cfg->mask && !r->loop_bytes) return rfail(r, RMCV_ERR_BAD_ARG, "rmcv_recorder_set_trigger: a mask on a recorder without loop records (track_cap == 0)");
    r->trig = *cfg;
    r->trig.reserved = 0;
    return RMCV_OK;
}

int rmcv_recorder_trigger(rmcv_recorder* r, rmcv_trigger_info* info)
{
    if (!r || !info) return RMCV_ERR_BAD_ARG;
    memset(info, 0, sizeof(*info));
    if (r->h_latch && *(volatile int32_t*)&r->h_latch->set) {
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        info->fired = 1, info->mask = r->h_latch->fired, info->sequence = r->h_latch->sequence, info->k = r->h_latch->k, info->stream = r->h_latch->stream;
    }
    info->noticed = r->noticed, info->batches_since = r->since;
    return RMCV_OK;
}

int rmcv_recorder_loop(rmcv_recorder* r, int i, int k, void* out, int64_t cap, int64_t* size)
{
    if (!r || cap < 0 || (cap > 0 && !out)) return RMCV_ERR_BAD_ARG;
    int rc = RMCV_OK;
    RecSlot* S = held_slot(r, i, &rc);
    if (!S) return rc;
    if (k < 0 || k >= S->e.n_frames) return rfail(r, RMCV_ERR_BAD_ARG, "no such frame in the recorded batch");
    if (!S->loop_on) return rfail(r, RMCV_ERR_BAD_ARG, "the recorded batch has no loop records (an untracked submit, or track_cap == 0)");
    if (size) *size = r->loop_bytes;
    if (r->loop_bytes > cap) return rfail(r, RMCV_ERR_CAPACITY, "output capacity exceeded");
    // the fixed part first: it says how many tracks the area holds; the tail behind them is zero for every reader
    uint8_t* o = static_cast<uint8_t*>(out);
    const uint8_t* d = S->d_loop + (int64_t)k * r->loop_bytes;
    hipError_t e = hipMemcpy(o, d, sizeof(rmcv_loop_state), hipMemcpyDeviceToHost);
    rmcv_loop_state st;
    if (e == hipSuccess) {
        memcpy(&st, o, sizeof(st));
        if (!loop_counts_ok(&st, r->loop_bytes)) return rfail(r, RMCV_ERR_HIP, "recorder: a loop record's counts beyond its area");
        const int64_t live = loop_bound(st.n_tracks);
        if (live > (int64_t)sizeof(st)) e = hipMemcpy(o + sizeof(st), d + sizeof(st), (size_t)(live - (int64_t)sizeof(st)), hipMemcpyDeviceToHost);
        memset(o + live, 0, (size_t)(r->loop_bytes - live));
    }
    if (e != hipSuccess) return rfail(r, RMCV_ERR_HIP, "recorder: D2H loop record", e);
    return RMCV_OK;
}

int rmcv_recorder_count(rmcv_recorder* r, int32_t* n)
{
    if (!r || !n) return RMCV_ERR_BAD_ARG;
    *n = held(r);
    int rc = RMCV_OK;
    for (int i = 0; i < *n; i++) if (!held_slot(r, i, &rc)) return rc; // what is counted is complete
    return RMCV_OK;
}

int rmcv_recorder_entry(rmcv_recorder* r, int i, rmcv_record_entry* entry, void* user_out, int user_cap)
{
    if (!r || !entry || user_cap < 0 || (user_cap > 0 && !user_out)) return RMCV_ERR_BAD_ARG;
    int rc = RMCV_OK;
    RecSlot* S = held_slot(r, i, &rc);
    if (!S) return rc;
    if ((rc = slot_tables(r, *S))) return rc;
    *entry = S->e;
    const size_t n = S->user.size() < (size_t)user_cap ? S->user.size() : (size_t)user_cap;
    if (n) memcpy(user_out, S->user.data(), n);
    return RMCV_OK;
}

int rmcv_recorder_device_frame(rmcv_recorder* r, int i, int k, void** d_packed, int64_t* size)
{
    if (!r) return RMCV_ERR_BAD_ARG;
    int rc = RMCV_OK;
    RecSlot* S = held_slot(r, i, &rc);
    if (!S) return rc;
    if (k < 0 || k >= S->e.n_frames) return rfail(r, RMCV_ERR_BAD_ARG, "no such frame in the recorded batch");
    if ((rc = slot_tables(r, *S))) return rc;
    if (d_packed) *d_packed = S->d_area + (int64_t)k * r->area;
    if (size) *size = S->e.sizes[k];
    return RMCV_OK;
}

int rmcv_recorder_frame(rmcv_recorder* r, int i, int k, void* out, int64_t cap, int64_t* size)
{
    if (!r || cap < 0 || (cap > 0 && !out)) return RMCV_ERR_BAD_ARG;
    void* d = nullptr;
    int64_t n = 0;
    const int rc = rmcv_recorder_device_frame(r, i, k, &d, &n);
    if (rc) return rc;
    if (size) *size = n;
    if (n > cap) return rfail(r, RMCV_ERR_CAPACITY, "output capacity exceeded");
    const hipError_t e = hipMemcpy(out, d, (size_t)n, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return rfail(r, RMCV_ERR_HIP, "recorder: D2H packed frame", e);
    return RMCV_OK;
}

int rmcv_recorder_save(rmcv_recorder* r, const char* path)
{
    if (!r || !path) return RMCV_ERR_BAD_ARG;
    int32_t n = 0;
    int rc = rmcv_recorder_count(r, &n);
    if (rc) return rc;
    FILE* f = fopen(path, "wb");
    if (!f) return rfail(r, RMCV_ERR_BAD_ARG, "rmcv_recorder_save: the file cannot be created");
    rc = session_write_header(f);
    std::vector<std::vector<uint8_t>> bufs;
    for (int i = 0; i < n && rc == RMCV_OK; i++) {
        rmcv_record_entry e;
        if ((rc = rmcv_recorder_entry(r, i, &e, nullptr, 0))) break;
        const RecSlot& S = r->slots[(size_t)(e.sequence % (uint64_t)r->cfg.slots)];
        bufs.assign((size_t)e.n_frames, {});
        const uint8_t* ptrs[RMCV_RECORDER_MAX_FRAMES] = {nullptr};
        for (int k = 0; k < e.n_frames && rc == RMCV_OK; k++) {
            bufs[(size_t)k].resize((size_t)e.sizes[k]);
            rc = rmcv_recorder_frame(r, i, k, bufs[(size_t)k].data(), e.sizes[k], nullptr);
            ptrs[k] = bufs[(size_t)k].data();
        }
        std::vector<uint8_t> loops((size_t)e.n_frames * (size_t)e.loop_bytes);
        const uint8_t* lptrs[RMCV_RECORDER_MAX_FRAMES] = {nullptr};
        for (int k = 0; k < e.n_frames && e.loop_bytes && rc == RMCV_OK; k++) {
            lptrs[k] = loops.data() + (size_t)k * (size_t)e.loop_bytes;
            rc = rmcv_recorder_loop(r, i, k, loops.data() + (size_t)k * (size_t)e.loop_bytes, e.loop_bytes, nullptr);
        }
        if (rc == RMCV_OK && (rc = session_write_record(f, e, S.user.data(), ptrs, e.loop_bytes ? lptrs : nullptr))) rfail(r, rc, "rmcv_recorder_save: write failed");
    }
    if (fclose(f) != 0 && rc == RMCV_OK) rc = rfail(r, RMCV_ERR_BAD_ARG, "rmcv_recorder_save: write failed");
    return rc;
}

int rmcv_session_append(const char* path, const rmcv_record_entry* entry, const void* user, const uint8_t* const* packed)
{
    return rmcv_session_append_loop(path, entry, user, packed, nullptr);
}

int rmcv_session_append_loop(const char* path, const rmcv_record_entry* entry, const void* user, const uint8_t* const* packed,
                             const uint8_t* const* loops)
{
    if (!path || !entry) return RMCV_ERR_BAD_ARG;
    if ((entry->loop_bytes != 0) != (loops != nullptr)) return RMCV_ERR_BAD_ARG; // (before a file is created)
    FILE* f = fopen(path, "r+b");
    int rc = RMCV_OK;
    if (f) { // an existing file must be a session of this version
        uint8_t h[16];
        if (fread(h, 1, sizeof(h), f) != sizeof(h) || memcmp(h, SESSION_MAGIC, 8) != 0 || pack_get32(h + 8) != SESSION_VERSION ||
            pack_get32(h + 12) != sizeof(rmcv_record_entry) || fseek(f, 0, SEEK_END) != 0)
            rc = RMCV_ERR_BAD_ARG;
    } else {
        f = fopen(path, "wb");
        if (!f) return RMCV_ERR_BAD_ARG;
        rc = session_write_header(f);
    }
    if (rc == RMCV_OK) rc = session_write_record(f, *entry, user, packed, loops);
    if (fclose(f) != 0 && rc == RMCV_OK) rc = RMCV_ERR_BAD_ARG;
    return rc;
}

int rmcv_session_open(const char* path, rmcv_session** out)
{
    if (!path || !out) return RMCV_ERR_BAD_ARG;
    *out = nullptr;
    FILE* f = fopen(path, "rb");
    if (!f) return RMCV_ERR_BAD_ARG;
    rmcv_session* s = new (std::nothrow) rmcv_session();
    if (!s) { fclose(f); return RMCV_ERR_NOMEM; }
    uint8_t chunk[1 << 16];
    size_t got;
    while ((got = fread(chunk, 1, sizeof(chunk), f)) > 0) s->data.insert(s->data.end(), chunk, chunk + got);
    const bool bad = ferror(f) != 0;
    fclose(f);
    if (bad || session_parse(s->data.data(), (int64_t)s->data.size(), &s->recs) != RMCV_OK) {
        delete s;
        return RMCV_ERR_BAD_ARG;
    }
    *out = s;
    return RMCV_OK;
}

int rmcv_session_count(const rmcv_session* s, int32_t* n)
{
    if (!s || !n) return RMCV_ERR_BAD_ARG;
    *n = (int32_t)s->recs.size();
    return RMCV_OK;
}

int rmcv_session_entry(const rmcv_session* s, int i, rmcv_record_entry* entry, void* user_out, int user_cap)
{
    if (!s || !entry || i < 0 || (size_t)i >= s->recs.size() || user_cap < 0 || (user_cap > 0 && !user_out)) return RMCV_ERR_BAD_ARG;
    memcpy(entry, s->data.data() + s->recs[(size_t)i].entry, sizeof(*entry));
    const int n = entry->user_bytes < user_cap ? entry->user_bytes : user_cap;
    if (n > 0) memcpy(user_out, s->data.data() + s->recs[(size_t)i].user, (size_t)n);
    return RMCV_OK;
}

int rmcv_session_frame(const rmcv_session* s, int i, int k, void* out, int64_t cap, int64_t* size)
{
    if (!s || i < 0 || (size_t)i >= s->recs.size() || cap < 0 || (cap > 0 && !out)) return RMCV_ERR_BAD_ARG;
    rmcv_record_entry e;
    memcpy(&e, s->data.data() + s->recs[(size_t)i].entry, sizeof(e));
    if (k < 0 || k >= e.n_frames) return RMCV_ERR_BAD_ARG;
    if (size) *size = e.sizes[k];
    if (e.sizes[k] > cap) return RMCV_ERR_CAPACITY;
    memcpy(out, s->data.data() + s->recs[(size_t)i].frame[k], (size_t)e.sizes[k]);
    return RMCV_OK;
}

int rmcv_session_loop(const rmcv_session* s, int i, int k, void* out, int64_t cap, int64_t* size)
{
    if (!s || i < 0 || (size_t)i >= s->recs.size() || cap < 0 || (cap > 0 && !out)) return RMCV_ERR_BAD_ARG;
    rmcv_record_entry e;
    memcpy(&e, s->data.data() + s->recs[(size_t)i].entry, sizeof(e));
    if (k < 0 || k >= e.n_frames || !e.loop_bytes) return RMCV_ERR_BAD_ARG;
    if (size) *size = e.loop_bytes;
    if (e.loop_bytes > cap) return RMCV_ERR_CAPACITY;
    memcpy(out, s->data.data() + s->recs[(size_t)i].loop + (int64_t)k * e.loop_bytes, (size_t)e.loop_bytes);
    return RMCV_OK;
}

void rmcv_session_close(rmcv_session* s) { delete s; }

} // extern "C"
