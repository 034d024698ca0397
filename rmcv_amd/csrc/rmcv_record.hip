// rmcv_record.hip -- rmcv_recorder_* and rmcv_session_*: the session recorder behind the C-ABI (include/rmcv_abi.h).
//
// The reference's rm::debug::logger (include/debug.h:13-29, src/debug.cpp:9-41) writes every frame the detector saw to a lossless video and
// a `data` record beside it.  Here the frames are in HBM and a batch is one non-blocking submit, so the recorder is a ring in HBM too:
// slot = sequence mod slots, every chosen frame a fixed area of rmcv_pack_bound bytes (no allocator on the device), a small device table
// of the packed sizes (and the batch's effective keys and window origins), and on the host the entry with everything known at the submit.
// Recording is three launches and two event calls on the caller's stream; the readers wait for the slot's event with the 5 s deadline.
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
    bool used = false;
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

int recorder_enqueue(rmcv_recorder* r, const RecordBatch& b, const int32_t* frames, int n, hipStream_t s)
{
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
    r->seq++;
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
        if (S.used && wait_event_deadline(S.ev, r->wait_timeout_ms, &e) > 0) {
            fprintf(stderr, "rmcv_recorder_destroy: a packing has not finished; the recorder's buffers are leaked\n");
            return;
        }
    }
    for (auto& S : r->slots) {
        for (void* p : {(void*)S.d_area, (void*)S.d_sizes, (void*)S.d_keys, (void*)S.d_camps, (void*)S.d_origins}) if (p) (void)hipFree(p);
        if (S.ev) (void)hipEventDestroy(S.ev);
    }
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
    }
    if (c.slots < 1 || c.slots > 4096 || c.max_frames < 1 || c.max_frames > RMCV_RECORDER_MAX_FRAMES || c.user_bytes < 0 || c.user_bytes > (1 << 20) ||
        !pack_geometry_ok(c.max_w_bytes, c.max_h, 1))
        return RMCV_ERR_BAD_ARG;
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return RMCV_ERR_NO_DEVICE; }
    rmcv_recorder* r = new (std::nothrow) rmcv_recorder();
    if (!r) return RMCV_ERR_NOMEM;
    r->device = device, r->cfg = c, r->area = pack_bound(c.max_w_bytes, c.max_h);
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
int rmcv_recorder_resume(rmcv_recorder* r) { if (!r) return RMCV_ERR_BAD_ARG; r->frozen = false; return RMCV_OK; }

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
        if (rc == RMCV_OK && (rc = session_write_record(f, e, S.user.data(), ptrs))) rfail(r, rc, "rmcv_recorder_save: write failed");
    }
    if (fclose(f) != 0 && rc == RMCV_OK) rc = rfail(r, RMCV_ERR_BAD_ARG, "rmcv_recorder_save: write failed");
    return rc;
}

int rmcv_session_append(const char* path, const rmcv_record_entry* entry, const void* user, const uint8_t* const* packed)
{
    if (!path || !entry) return RMCV_ERR_BAD_ARG;
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
    if (rc == RMCV_OK) rc = session_write_record(f, *entry, user, packed);
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

void rmcv_session_close(rmcv_session* s) { delete s; }

} // extern "C"
