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

int rmcv_dataset_clear(rmcv_dataset* d)
{
    if (!d) return RMCV_ERR_BAD_ARG;
    if (const int rc = ready(d)) return rc;
    DCHK(d, hipMemset(d->v.ctr, 0, sizeof(HarvestCounters)), "clearing the dataset's counters");
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
