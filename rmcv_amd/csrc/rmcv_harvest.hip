// rmcv_harvest.hip -- the device-resident dataset as an object: the ONE unit that knows struct rmcv_dataset.  Its lifetime,
// the order of its appends (one event), the host's wait with the creating context's deadline, and the entry points around it:
// rmcv_dataset_*, rmcv_batch_harvest / _device, rmcv_harvest_plan_host (device_harvest.h compiled for the host), and the trainer's and the
// predictor's forms that read the dataset in place (rmcv_svm_train_dataset, rmcv_svm_predict_dataset: the gather on the device, then
// rmcv_svm.hip's own path with the upload skipped).  The append itself is ctx_harvest (rmcv_host.hip); the kernels are k_harvest.hip's.
#include <string.h>

#include "rmcv_ctx.h"

using namespace rmcv;

struct rmcv_dataset {
    DatasetView v{};
    rmcv_ctx* owner = nullptr;      // the creating context: its deadline is the dataset's
    int deadline_ms = 5000;         // ... as it was read last (rmcv_dataset_destroy does not touch the context: it may be gone already)
    hipEvent_t ev_append = nullptr; // recorded behind the append enqueued last
    bool append_pending = false;
    hipStream_t last_stream = nullptr;
    char err[256] = {0};
    std::vector<void*> allocs;
    // what rmcv_dataset_append_rows stages its host tables in (free once the last append has finished: it waits for that first)
    int32_t* src_tables = nullptr; // [4][label_cap]: n_rows, row_off, zeros, (spare)
    uint8_t* src_rows = nullptr;
    size_t src_rows_bytes = 0;
};

static int dfail(rmcv_dataset* d, int code, const char* what, hipError_t e = hipSuccess)
{
    if (d) {
        if (e != hipSuccess) snprintf(d->err, sizeof(d->err), "%s: %s", what, hipGetErrorString(e));
        else snprintf(d->err, sizeof(d->err), "%s", what);
    }
    if (e != hipSuccess) (void)hipGetLastError();
    return code;
}
#define DCHK(d, call, what)                                              \
    do {                                                                 \
        hipError_t e__ = (call);                                         \
        if (e__ != hipSuccess) return dfail((d), RMCV_ERR_HIP, what, e__); \
    } while (0)

// the dataset's device, its last append finished (with the creating context's deadline; ask_owner: read it again)
static int ready(rmcv_dataset* d, bool ask_owner = true)
{
    hipSetDevice(d->v.device);
    if (ask_owner) d->deadline_ms = ctx_wait_timeout_ms(d->owner);
    if (!d->append_pending) return RMCV_OK;
    hipError_t e = hipSuccess;
    const int ms = d->deadline_ms;
    const int rc = wait_event_deadline(d->ev_append, ms, &e);
    if (rc < 0) return dfail(d, RMCV_ERR_HIP, "waiting for the dataset's last append", e);
    if (rc > 0) {
        snprintf(d->err, sizeof(d->err), "the dataset's last append has not finished after %d ms (RMCV_OPT_WAIT_TIMEOUT_MS)", ms);
        return RMCV_ERR_TIMEOUT;
    }
    d->append_pending = false;
    return RMCV_OK;
}
static int counters(rmcv_dataset* d, HarvestCounters* out)
{
    if (const int rc = ready(d)) return rc;
    DCHK(d, hipMemcpy(out, d->v.ctr, sizeof(*out), hipMemcpyDeviceToHost), "D2H dataset counters");
    return RMCV_OK;
}

namespace rmcv {
const DatasetView& dataset_view(const rmcv_dataset* ds) { return ds->v; }
hipError_t dataset_order_begin(rmcv_dataset* ds, hipStream_t s)
{
    if (ds->append_pending && ds->last_stream != s) return hipStreamWaitEvent(s, ds->ev_append, 0);
    return hipSuccess;
}
hipError_t dataset_order_end(rmcv_dataset* ds, hipStream_t s)
{
    ds->last_stream = s;
    ds->append_pending = true;
    return hipEventRecord(ds->ev_append, s);
}
} // namespace rmcv

// the slots a training or prediction call names, on the device: checked against count on the host first.  *d_idx stays null for rows == NULL.
static int stage_rows(rmcv_ctx* c, rmcv_dataset* ds, const int32_t* rows, int n, int32_t** d_idx, std::vector<void*>& blocks, const char* who)
{
    char msg[160];
    if (ds->v.device != c->device) {
        snprintf(msg, sizeof(msg), "%s: the dataset belongs to another device", who);
        return fail(c, RMCV_ERR_BAD_ARG, msg);
    }
    if (const int rc = ctx_ready(c)) return rc;
    HarvestCounters k{};
    if (const int rc = counters(ds, &k)) return fail(c, rc, ds->err);
    bool ok = n <= k.count;
    for (int i = 0; rows && ok && i < n; i++) ok = rows[i] >= 0 && rows[i] < k.count;
    if (!ok) {
        snprintf(msg, sizeof(msg), "%s: a row index outside 0 .. count - 1 (the dataset holds %d rows)", who, k.count);
        return fail(c, RMCV_ERR_BAD_ARG, msg);
    }
    *d_idx = nullptr;
    if (rows) {
        hipError_t e = hipMalloc((void**)d_idx, (size_t)n * 4);
        if (e != hipSuccess) return fail(c, RMCV_ERR_NOMEM, "dataset row indices", e);
        blocks.push_back(*d_idx);
        HIPCHK(c, hipMemcpy(*d_idx, rows, (size_t)n * 4, hipMemcpyHostToDevice), "H2D dataset row indices");
    }
    return RMCV_OK;
}
struct Blocks { // device memory of one call
    std::vector<void*> p;
    ~Blocks() { for (void* q : p) hipFree(q); }
};

extern "C" {

int rmcv_dataset_create(rmcv_ctx* c, int capacity_rows, rmcv_dataset** out)
{
    if (!c || !out) return RMCV_ERR_BAD_ARG;
    *out = nullptr;
    if (capacity_rows < 1) return fail(c, RMCV_ERR_BAD_ARG, "rmcv_dataset_create: capacity_rows < 1");
    hipSetDevice(c->device);
    rmcv_dataset* d = new (std::nothrow) rmcv_dataset();
    if (!d) return RMCV_ERR_NOMEM;
    d->owner = c;
    d->deadline_ms = c->wait_timeout_ms;
    d->v.device = c->device, d->v.capacity = capacity_rows, d->v.label_cap = c->lim.max_frames;
    const size_t cap = (size_t)capacity_rows;
    hipError_t e = hipSuccess;
    const auto get = [&](auto** p, size_t bytes) {
        if (e != hipSuccess) return;
        e = hipMalloc((void**)p, bytes);
        if (e == hipSuccess) d->allocs.push_back(*p);
    };
    get(&d->v.rows, cap * RMCV_SVM_FEATURES);
    get(&d->v.meta, cap * sizeof(rmcv_harvest_meta));
    get(&d->v.ctr, sizeof(HarvestCounters));
    get(&d->v.list, cap * sizeof(HarvestItem));
    get(&d->v.labels, (size_t)d->v.label_cap * 4);
    if (e == hipSuccess) e = hipMemset(d->v.ctr, 0, sizeof(HarvestCounters));
    if (e == hipSuccess) e = hipEventCreateWithFlags(&d->ev_append, hipEventDisableTiming);
    if (e != hipSuccess) {
        const int rc = fail(c, e == hipErrorOutOfMemory ? RMCV_ERR_NOMEM : RMCV_ERR_HIP, "rmcv_dataset_create", e);
        rmcv_dataset_destroy(d);
        return rc;
    }
    *out = d;
    return RMCV_OK;
}

void rmcv_dataset_destroy(rmcv_dataset* d)
{
    if (!d) return;
    if (ready(d, false) == RMCV_ERR_TIMEOUT) { // an append that does not finish is not waited for without a deadline: the memory is leaked instead
        fprintf(stderr, "rmcv_dataset_destroy: %s; the dataset's buffers are leaked\n", d->err);
        return;
    }
    for (void* p : d->allocs) hipFree(p);
    if (d->ev_append) hipEventDestroy(d->ev_append);
    delete d;
}

const char* rmcv_dataset_last_error(const rmcv_dataset* d) { return d ? d->err : "null dataset"; }

// the novelty state emptied: every pushed, every ring position (and near, on a clear)
static int novelty_reset(rmcv_dataset* d, bool near_too)
{
    if (!d->v.rings) return RMCV_OK;
    DCHK(d, hipMemset(d->v.rings, 0, (size_t)d->v.label_cap * RMCV_HARVEST_RING_MAX * RMCV_SVM_FEATURES), "emptying the dataset's rings");
    DCHK(d, hipMemset(d->v.pushed, 0, (size_t)d->v.label_cap * 8), "emptying the dataset's rings");
    if (near_too) DCHK(d, hipMemset(d->v.near, 0, 8), "clearing the dataset's near counter");
    return RMCV_OK;
}

int rmcv_dataset_clear(rmcv_dataset* d)
{
    if (!d) return RMCV_ERR_BAD_ARG;
    if (const int rc = ready(d)) return rc;
    DCHK(d, hipMemset(d->v.ctr, 0, sizeof(HarvestCounters)), "clearing the dataset's counters");
    return novelty_reset(d, true);
}

int32_t rmcv_icon_sad(const uint8_t* a, const uint8_t* b) { return a && b ? icon_sad(a, b) : -1; }

int rmcv_dataset_set_novelty(rmcv_dataset* d, int ring_rows, int32_t max_sad)
{
    if (!d) return RMCV_ERR_BAD_ARG;
    if (const char* no = novelty_refusal(ring_rows, max_sad)) return dfail(d, RMCV_ERR_BAD_ARG, no);
    if (const int rc = ready(d)) return rc;
    if (ring_rows > 0 && !d->v.rings) { // first use: rings of the largest depth, so that a later depth needs no memory
        const size_t n = (size_t)d->v.label_cap;
        d->v.keep_armours = d->owner->lim.max_armours;
        uint8_t *rings = nullptr, *keep = nullptr;
        int64_t* state = nullptr; // near, then pushed[label_cap]
        hipError_t e = hipMalloc((void**)&rings, n * RMCV_HARVEST_RING_MAX * RMCV_SVM_FEATURES);
        if (e == hipSuccess) e = hipMalloc((void**)&keep, n * (size_t)d->v.keep_armours);
        if (e == hipSuccess) e = hipMalloc((void**)&state, (n + 1) * 8);
        if (e == hipSuccess) e = hipMemset(state, 0, (n + 1) * 8);
        if (e != hipSuccess) {
            hipFree(rings), hipFree(keep), hipFree(state);
            return dfail(d, e == hipErrorOutOfMemory ? RMCV_ERR_NOMEM : RMCV_ERR_HIP, "rmcv_dataset_set_novelty", e);
        }
        d->allocs.push_back(rings), d->allocs.push_back(keep), d->allocs.push_back(state);
        d->v.rings = rings, d->v.keep = keep, d->v.near = reinterpret_cast<unsigned long long*>(state), d->v.pushed = state + 1;
    }
    if (const int rc = novelty_reset(d, false)) return rc;
    d->v.ring_rows = ring_rows, d->v.max_sad = max_sad;
    return RMCV_OK;
}

int rmcv_dataset_novelty(rmcv_dataset* d, int* ring_rows, int32_t* max_sad, int64_t* near)
{
    if (!d) return RMCV_ERR_BAD_ARG;
    if (const int rc = ready(d)) return rc;
    if (ring_rows) *ring_rows = d->v.ring_rows;
    if (max_sad) *max_sad = d->v.max_sad;
    if (near) {
        *near = 0;
        if (d->v.near) DCHK(d, hipMemcpy(near, d->v.near, 8, hipMemcpyDeviceToHost), "D2H dataset near counter");
    }
    return RMCV_OK;
}

int rmcv_dataset_get_rings(rmcv_dataset* d, int first_stream, int n_streams, uint8_t* rows_out, int64_t* pushed_out)
{
    if (!d) return RMCV_ERR_BAD_ARG;
    if (const int rc = ready(d)) return rc;
    if (first_stream < 0 || n_streams < 0 || (int64_t)first_stream + n_streams > d->v.label_cap)
        return dfail(d, RMCV_ERR_BAD_ARG, "rmcv_dataset_get_rings: streams outside 0 .. max_frames - 1");
    if (n_streams == 0) return RMCV_OK;
    const size_t per = (size_t)d->v.ring_rows * RMCV_SVM_FEATURES;
    if (pushed_out) {
        if (d->v.pushed) DCHK(d, hipMemcpy(pushed_out, d->v.pushed + first_stream, (size_t)n_streams * 8, hipMemcpyDeviceToHost), "D2H dataset pushed");
        else memset(pushed_out, 0, (size_t)n_streams * 8);
    }
    if (rows_out && per) DCHK(d, hipMemcpy(rows_out, d->v.rings + first_stream * per, n_streams * per, hipMemcpyDeviceToHost), "D2H dataset rings");
    return RMCV_OK;
}

int rmcv_dataset_append_rows(rmcv_dataset* d, const uint8_t* rows, const int32_t* n_rows, const int32_t* labels, int n_streams, uint64_t tag)
{
    if (!d) return RMCV_ERR_BAD_ARG;
    rmcv_ctx* c = d->owner;
    const int cap = d->v.label_cap;
    if (const char* no = novelty_rows_refusal(rows, n_rows, labels, n_streams, cap, c->lim.max_armours)) return dfail(d, RMCV_ERR_BAD_ARG, no);
    if (const int rc = ready(d)) return rc; // the staged tables of the previous call are free from here on
    std::vector<int32_t> tables((size_t)3 * cap, 0); // n_rows, row_off, zeros
    int64_t total = 0;
    for (int s = 0; s < n_streams; s++) {
        tables[s] = n_rows[s];
        tables[(size_t)cap + s] = (int32_t)total;
        total += n_rows[s];
    }
    const size_t bytes = (size_t)total * RMCV_SVM_FEATURES;
    if (!d->src_tables) {
        hipError_t e = hipMalloc((void**)&d->src_tables, (size_t)3 * cap * 4);
        if (e != hipSuccess) return dfail(d, RMCV_ERR_NOMEM, "rmcv_dataset_append_rows: tables", e);
        d->allocs.push_back(d->src_tables);
    }
    if (bytes > d->src_rows_bytes) {
        uint8_t* p = nullptr;
        hipError_t e = hipMalloc((void**)&p, bytes);
        if (e != hipSuccess) return dfail(d, RMCV_ERR_NOMEM, "rmcv_dataset_append_rows: rows", e);
        for (void*& q : d->allocs)
            if (q == d->src_rows && q) { hipFree(q); q = nullptr; } // (hipFree(nullptr) at the end is harmless)
        d->allocs.push_back(p);
        d->src_rows = p, d->src_rows_bytes = bytes;
    }
    DCHK(d, hipMemcpy(d->src_tables, tables.data(), tables.size() * 4, hipMemcpyHostToDevice), "H2D append_rows tables");
    DCHK(d, hipMemcpy(d->v.labels, labels, (size_t)n_streams * 4, hipMemcpyHostToDevice), "H2D append_rows labels");
    if (bytes) DCHK(d, hipMemcpy(d->src_rows, rows, bytes, hipMemcpyHostToDevice), "H2D append_rows rows");
    DatasetRowsSource src;
    src.rows = d->src_rows, src.n_rows = d->src_tables, src.row_off = d->src_tables + cap, src.zeros = d->src_tables + 2 * (size_t)cap, src.labels = d->v.labels;
    src.n_streams = n_streams, src.max_armours = c->lim.max_armours;
    hipStream_t s = c->stream;
    DCHK(d, dataset_order_begin(d, s), "append_rows: wait for the dataset's previous append");
    DCHK(d, launch_harvest_rows_source(src, d->v, c->geom.n_cu, tag, s), "k_harvest_novel + k_harvest_plan + k_harvest_copy_rows");
    DCHK(d, dataset_order_end(d, s), "append_rows: record the append");
    return RMCV_OK;
}

int rmcv_harvest_novel_host(const uint8_t* rows, const int32_t* n_rows, const int32_t* labels, int n_streams, int ring_rows, int32_t max_sad, uint8_t* rings,
                            int64_t* pushed, uint8_t* keep_out, int32_t* min_sad_out, int64_t* near_out)
{
    if (n_streams < 0 || novelty_refusal(ring_rows, max_sad)) return RMCV_ERR_BAD_ARG;
    if (n_streams && (!n_rows || !labels)) return RMCV_ERR_BAD_ARG;
    if (n_streams && ring_rows && (!rings || !pushed)) return RMCV_ERR_BAD_ARG;
    int64_t total = 0;
    for (int s = 0; s < n_streams; s++) {
        if (n_rows[s] < 0) return RMCV_ERR_BAD_ARG;
        total += n_rows[s];
    }
    if (total && (!rows || !keep_out)) return RMCV_ERR_BAD_ARG;
    const int64_t near = novelty_seq(rows, n_rows, labels, n_streams, ring_rows, max_sad, rings, pushed, keep_out, min_sad_out);
    if (near_out) *near_out = near;
    return RMCV_OK;
}

int rmcv_dataset_count(rmcv_dataset* d, int32_t* rows, int64_t* dropped)
{
    if (!d) return RMCV_ERR_BAD_ARG;
    HarvestCounters k{};
    if (const int rc = counters(d, &k)) return rc;
    if (rows) *rows = k.count;
    if (dropped) *dropped = k.dropped;
    return RMCV_OK;
}

int rmcv_dataset_get(rmcv_dataset* d, int first, int n, uint8_t* rows_out, rmcv_harvest_meta* meta_out)
{
    if (!d) return RMCV_ERR_BAD_ARG;
    HarvestCounters k{};
    if (const int rc = counters(d, &k)) return rc;
    if (first < 0 || n < 0 || (int64_t)first + n > k.count) return dfail(d, RMCV_ERR_BAD_ARG, "rmcv_dataset_get: rows outside 0 .. count - 1");
    if (n == 0) return RMCV_OK;
    if (rows_out) DCHK(d, hipMemcpy(rows_out, d->v.rows + (size_t)first * RMCV_SVM_FEATURES, (size_t)n * RMCV_SVM_FEATURES, hipMemcpyDeviceToHost), "D2H dataset rows");
    if (meta_out) DCHK(d, hipMemcpy(meta_out, d->v.meta + first, (size_t)n * sizeof(rmcv_harvest_meta), hipMemcpyDeviceToHost), "D2H dataset metadata");
    return RMCV_OK;
}

int rmcv_dataset_device(rmcv_dataset* d, void** d_rows, void** d_meta, void** d_count)
{
    if (!d) return RMCV_ERR_BAD_ARG;
    if (d_rows) *d_rows = d->v.rows;
    if (d_meta) *d_meta = d->v.meta;
    if (d_count) *d_count = &d->v.ctr->count;
    return RMCV_OK;
}

int rmcv_batch_harvest(rmcv_ctx* c, rmcv_dataset* ds, const int32_t* labels, int flags, uint64_t tag, void* hip_stream)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    if (!labels) return fail(c, RMCV_ERR_BAD_ARG, "harvest: null labels");
    hipSetDevice(c->device);
    return ctx_harvest(c, ds, labels, nullptr, 0, flags, tag, c->last_stages, hip_stream ? (hipStream_t)hip_stream : c->stream);
}

int rmcv_batch_harvest_device(rmcv_ctx* c, rmcv_dataset* ds, const void* d_labels, int flags, uint64_t tag, void* hip_stream)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    hipSetDevice(c->device);
    return ctx_harvest(c, ds, nullptr, d_labels, c->geom.n_frames, flags, tag, c->last_stages, hip_stream ? (hipStream_t)hip_stream : c->stream);
}

int rmcv_harvest_plan_host(const int32_t* n_armours, const int32_t* status, const int32_t* labels, const int32_t* identity, int n_frames, int max_armours,
                           int flags, int32_t count, int32_t capacity, int64_t dropped_in, rmcv_harvest_item* items_out, int cap, int32_t* n_items,
                           int32_t* count_out, int64_t* dropped_out)
{
    if (n_frames < 0 || max_armours < 1 || capacity < 1 || count < 0 || count > capacity || cap < 0 || (flags & ~RMCV_HARVEST_MISSES)) return RMCV_ERR_BAD_ARG;
    if (n_frames && (!n_armours || !status || !labels)) return RMCV_ERR_BAD_ARG;
    if ((flags & RMCV_HARVEST_MISSES) && n_frames && !identity) return RMCV_ERR_BAD_ARG;
    std::vector<HarvestItem> list((size_t)(capacity - count) + 1);
    int32_t now = 0;
    int64_t drop = 0;
    const int32_t n = harvest_plan_seq(n_armours, status, labels, identity, n_frames, max_armours, flags, count, capacity, list.data(), &now, &drop);
    if (n_items) *n_items = n;
    if (count_out) *count_out = now;
    if (dropped_out) *dropped_out = dropped_in + drop;
    if (n > cap) return RMCV_ERR_CAPACITY;
    if (n && !items_out) return RMCV_ERR_BAD_ARG;
    static_assert(sizeof(HarvestItem) == sizeof(rmcv_harvest_item), "the work list's entry is the ABI's item");
    if (n) memcpy(items_out, list.data(), (size_t)n * sizeof(HarvestItem));
    return RMCV_OK;
}

int rmcv_svm_train_dataset(rmcv_ctx* c, rmcv_dataset* ds, const int32_t* rows, int n, const int32_t* perm, const rmcv_svm_train_params* params,
                           float* weights_out, double* rho_out, int32_t* labels_out, int32_t* n_class_out, rmcv_svm_train_report* report)
{
    svm_report_reset(report, nullptr);
    if (!c) return RMCV_ERR_BAD_ARG;
    const auto refuse_train = [&](const char* why) {
        svm_report_reset(report, why);
        return fail(c, RMCV_ERR_BAD_ARG, why);
    };
    if (!ds || !weights_out || !rho_out || !labels_out || !n_class_out) return refuse_train("svm train: a null pointer");
    if (n < 1 || n > RMCV_SVM_MAX_SAMPLES) return refuse_train("svm train: n outside 1 .. RMCV_SVM_MAX_SAMPLES");
    Blocks ws;
    int32_t *d_idx = nullptr, *d_resp = nullptr;
    uint8_t* d_rows = nullptr;
    int rc = stage_rows(c, ds, rows, n, &d_idx, ws.p, "rmcv_svm_train_dataset");
    if (rc) {
        svm_report_reset(report, c->err);
        return rc;
    }
    hipError_t e = hipMalloc((void**)&d_resp, (size_t)n * 4);
    if (e == hipSuccess) ws.p.push_back(d_resp);
    if (e == hipSuccess && rows) { // a subset: contiguous rows; the whole prefix is read where it lies
        e = hipMalloc((void**)&d_rows, (size_t)n * RMCV_SVM_FEATURES);
        if (e == hipSuccess) ws.p.push_back(d_rows);
    }
    if (e != hipSuccess) return fail(c, RMCV_ERR_NOMEM, "svm train workspace (dataset)", e);
    HIPCHK(c, launch_harvest_gather(ds->v, d_idx, n, d_rows, d_resp, c->stream), "k_harvest_gather");
    WAITCHK(c, wait_stream(c, c->stream, "rmcv_svm_train_dataset (gather)"));
    std::vector<int32_t> responses((size_t)n);
    HIPCHK(c, hipMemcpy(responses.data(), d_resp, (size_t)n * 4, hipMemcpyDeviceToHost), "D2H dataset responses");
    return svm_train_rows(c, rows ? d_rows : ds->v.rows, nullptr, responses.data(), n, perm, params, weights_out, rho_out, labels_out, n_class_out, report);
}

int rmcv_svm_predict_dataset(rmcv_ctx* c, rmcv_dataset* ds, const int32_t* rows, int n, int32_t* identity_out)
{
    if (!c || !ds || n < 0 || (n && !identity_out)) return RMCV_ERR_BAD_ARG;
    if (n == 0) return RMCV_OK;
    if (n > RMCV_SVM_MAX_SAMPLES && rows) return fail(c, RMCV_ERR_BAD_ARG, "rmcv_svm_predict_dataset: more than RMCV_SVM_MAX_SAMPLES row indices");
    if (!c->bufs.svm_w) return fail(c, RMCV_ERR_BAD_ARG, "rmcv_svm_predict needs a model: rmcv_svm_load first");
    Blocks ws;
    int32_t* d_idx = nullptr;
    uint8_t* d_rows = nullptr;
    if (const int rc = stage_rows(c, ds, rows, n, &d_idx, ws.p, "rmcv_svm_predict_dataset")) return rc;
    if (rows) {
        const hipError_t e = hipMalloc((void**)&d_rows, (size_t)n * RMCV_SVM_FEATURES);
        if (e != hipSuccess) return fail(c, RMCV_ERR_NOMEM, "svm predict workspace (dataset)", e);
        ws.p.push_back(d_rows);
        HIPCHK(c, launch_harvest_gather(ds->v, d_idx, n, d_rows, nullptr, c->stream), "k_harvest_gather"); // (the predictor follows on the same stream)
    }
    return svm_predict_rows(c, rows ? d_rows : ds->v.rows, nullptr, n, identity_out);
}

} // extern "C"
