// rmcv_ctx.h -- the context behind the ABI's handle and what the units that implement its entry points share: rmcv_host.hip (context,
// binding, run, batch setters and getters), rmcv_views.hip and rmcv_capture.hip (the views and the calibration capture: chosen frames of the
// batch bound, and their stage-wise twins), rmcv_stagewise.hip (the other helpers that run on the caller's own data), rmcv_calib.hip and
// rmcv_handeye.hip (the two solves) and rmcv_frame.hip (the per-frame chain); rmcv_svm.hip (the classifier's trainer) and rmcv_harvest.hip (the dataset's entry points) take
// the error and wait helpers.  Private to those: every other unit goes through the ctx_* functions of rmcv_internal.h.
#pragma once
#include <stdio.h>
#include <string.h>
#include <time.h>

#include <vector>

#include "rmcv_internal.h"
#include "frame_plan.h"

// What the per-frame drop-in path (rmcv_extract_color -> rmcv_filter_lightblobs -> rmcv_filter_armours, executable/main.cpp:172-176)
// keeps between its calls; rmcv_frame.hip.  A context that only runs batches pays for two handles of it.
struct FrameChain {
    int frame_upload = 3;          // RMCV_OPT_FRAME_UPLOAD (3: the runtime's pageable copy, the pinned staging buffer while that is slow)
    int run_ahead = 1;             // RMCV_OPT_RUN_AHEAD
    struct Reg { const void* p; size_t bytes; };
    std::vector<Reg> registered;   // caller buffers pinned by hipHostRegister (RMCV_OPT_FRAME_UPLOAD = 2)
    uint8_t* h_frame = nullptr;    // pinned staging (lazy): the BGR frame on its way up (RMCV_OPT_FRAME_UPLOAD = 1); small results on their way down:
    size_t h_frame_bytes = 0;
    int32_t* h_hdr = nullptr;      // [16]: contours at 0, blobs at 4, armours at 8
    // the same pinned buffers as the device addresses them (k_export stores into them); null: not mappable, copies are used
    int32_t *hd_hdr = nullptr, *hd_offs = nullptr, *hd_blob_src = nullptr, *hd_neg = nullptr;
    rmcv_point* hd_pts = nullptr;
    rmcv_lightblob* hd_blobs = nullptr;
    rmcv_armour* hd_armours = nullptr;
    rmcv_point* h_pts = nullptr;   // [max_points]      the CSR the last rmcv_extract_color returned
    int32_t* h_offs = nullptr;     // [max_contours + 1]
    rmcv_lightblob* h_blobs = nullptr; // [max_blobs]   the positive list the last rmcv_filter_lightblobs returned
    int32_t* h_blob_src = nullptr; // [max_blobs]
    int32_t* h_neg = nullptr;      // [max_contours]
    rmcv_armour* h_armours = nullptr; // [max_armours]
    int32_t* d_hdr = nullptr;      // device [16]
    // Device-resident hand-over: what frame slot 0 of the device buffers holds right now.  When the next call of the chain is
    // handed exactly these bytes back (the usual case: the reference passes the results straight on), nothing is re-uploaded.
    int res_nc = -1, res_total = 0; // contours (+ the fit stage's work list) = h_pts / h_offs; -1: not resident
    int res_nb = -1;                // light blobs = h_blobs; -1: not resident
    // Run-ahead: a caller that filters every frame with the same parameters (executable/main.cpp:172-176 does) gets the blob and
    // armour stages enqueued by rmcv_extract_color already, with the parameters its previous frame used -- one stream sequence and
    // one synchronisation for the whole chain; rmcv_filter_lightblobs / rmcv_filter_armours then only hand the results over.
    rmcv::LbParams last_lb{};
    rmcv::ArParams last_ar{};
    bool last_lb_valid = false, last_ar_valid = false; // what the previous frame's calls asked for
    bool ahead_lb = false, ahead_ar = false;           // this frame's extract_color has run them: headers + windows are in pinned memory
    hipStream_t side = nullptr;   // the library's own second stream: the byte image's download runs on it beside the sparse kernels
    hipEvent_t ev_fork = nullptr;
    uint8_t *h_image = nullptr, *hd_image = nullptr; // the byte image on its way home: pinned + mapped, written by k_image_export chunk by chunk
    size_t h_image_bytes = 0;
    uint32_t *h_iflags = nullptr, *hd_iflags = nullptr; // [IMG_CHUNKS] a chunk's flag = the sequence number of the frame whose bytes it holds
    uint32_t img_seq = 0;
    int image_export = 2;         // RMCV_OPT_IMAGE_EXPORT (2: the runtime's pageable copy, the library's export while that is slow)
    // The library measures both large copies on every frame and leaves the runtime's while they are slow: the rule, its constants and
    // why are in frame_plan.h (copy_path, copy_path_step).
    int upload_now = 0, image_now = 0;   // the paths the last frame took (upload: 0 pageable / 1 pinned staging / 2 registered; image: 0 runtime / 1 export)
    rmcv::CopyPathState copy_up{}, copy_img{}; // the rule's state per direction (setting the direction's option zeroes it)
    int test_slow_us = 0;                // RMCV_OPT_TEST_SLOW_US: added to what the library measures of the runtime's copies (tests of the switch)
    uint32_t* d_iarrived = nullptr; // [IMG_CHUNKS] device: workgroups of k_image_export that have stored their slice of a chunk
    double marks[9] = {};         // rmcv_ctx_frame_timing: host clock at the steps of the last rmcv_extract_color (microseconds)

    hipError_t init();            // the side stream and its event; RMCV_FRAME_UPLOAD / RMCV_IMAGE_EXPORT as the options' defaults
    void release();               // everything above that is not in rmcv_ctx::allocs (the context's work has finished)
};

struct rmcv_ctx {
    int device = 0;
    rmcv::Limits lim{};
    rmcv::Geom geom{};
    rmcv::Bufs bufs{};
    hipStream_t stream = nullptr;
    hipEvent_t ev[6] = {};
    uint8_t* own_frames = nullptr; // upload buffer (lazy)
    size_t own_frames_bytes = 0;
    rmcv_point* pack_pts = nullptr; // CSR download staging
    int32_t* pack_offs = nullptr;
    hipStream_t last_stream = nullptr;
    int geom_w = -1, geom_h = -1; // geometry the planes were zeroed for
    rmcv::ImageState image = rmcv::IMAGE_STATE_UNKNOWN; // what Bufs::imgmask is known to say about Bufs::binary (image_plan.h); every launch_binary keeps it
    int plane_sync = 0;           // frames whose bit plane and row masks are in step with the image and its mask (image_plan.h: plane_step); kept beside `image`
    // A second set of what the pixel kernel writes ("two pixel-output sets"): a pipeline's hot context takes its batches in the
    // two sets in turn, so that a pixel launch need not wait for the sparse stage of the context's batch before.  Bufs, `image` and
    // `plane_sync` are the CURRENT set's; `parked` holds the other one's (ctx_use_pixel_set swaps them).  n_sets 1: there is no second set.
    struct PixelSet {
        uint8_t* binary = nullptr;
        uint64_t* bits = nullptr;
        uint32_t *rowmask = nullptr, *imgmask = nullptr;
        rmcv::ImageState image = rmcv::IMAGE_STATE_UNKNOWN;
        int plane_sync = 0;
    } parked;
    int n_sets = 1, cur_set = 0;
    int order_n = -1, order_h = -1; // (n_frames, h) the frame order on the device was computed for
    hipEvent_t ev_order = nullptr; // recorded behind the work enqueued last: a call on ANOTHER stream first waits for it
    bool order_pending = false;
    bool external_order = false;  // a pipeline owns the ordering of this context's launches (rmcv_internal.h: ctx_external_order)
    hipEvent_t ext_done = nullptr; // ... and records this event behind the last of them
    FrameChain chain;             // the per-frame drop-in path
    int mid_frames = 0;           // frame slots Bufs::mid holds (ensure_mid)
    bool mid_failed = false;      // ... could not be allocated: the mid tier is absent for this context
    int sparse_waves = 8;         // RMCV_OPT_SPARSE_WAVES
    int pixel_groups = 3;         // RMCV_OPT_PIXEL_GROUPS
    int pixel_shape = 1;          // RMCV_OPT_PIXEL_SHAPE
    int dense_defer = 0;          // RMCV_OPT_DENSE_DEFER
    rmcv::InputOptions input;     // RMCV_OPT_INPUT_*, RMCV_OPT_ENHANCE and its gains: what the next binding records in Geom (bind_plan.h)
    // Waits with a deadline (round 5): no entry point parks its caller in the runtime without a bound.  `last_what` names the kernel or
    // copy enqueued last (every HIPCHK of an enqueue leaves its label here): a wait that runs out returns RMCV_ERR_TIMEOUT with it.
    int wait_timeout_ms = 5000;   // RMCV_OPT_WAIT_TIMEOUT_MS (0: no deadline)
    const char* last_what = "nothing";
    bool timed_out = false;       // a wait ran out: work of this context may still be in flight (cleared by the next wait that completes)
    int test_delay_us = 0;        // RMCV_OPT_TEST_DELAY_US: the next rmcv_extract_color holds its stream back this long first (tests of the deadline)
    uint64_t blocking_calls = 0;  // allocations, host-side synchronisations and blocking copies made while binding a geometry (ctx_blocking_calls)
    int32_t* order_scratch = nullptr; // [2 * max_frames] k_frame_order's work lists for batches beyond its LDS tables
    int last_stages = 0;              // the stages the batch bound has been through since its last pixel pass (rmcv_batch_track asks for RMCV_STAGE_ARMOURS)
    rmcv_point* win_own = nullptr;    // [max_frames] the context's copy of host origins (rmcv_batch_set_windows); Bufs::win_req points here or at the caller's
    int32_t* key_own = nullptr;       // [2][max_frames] the context's copy of host camps | lower bounds (rmcv_batch_set_frame_camps); Bufs::key_camps / key_lbs point here or at the caller's
    int32_t* cam_own = nullptr;       // [max_frames] the context's copy of host camera indices (rmcv_batch_set_frame_cameras); Bufs::cam_req points here or at the caller's
    int32_t* model_own = nullptr;     // [max_frames] the context's copy of host model indices (rmcv_batch_set_frame_models); Bufs::model_idx points here or at the caller's
    int model_classes[RMCV_SVM_MAX_MODELS] = {0}; // n_class of every entry of Bufs::svm_table (rmcv_svm_predict_model launches with it)
    int last_camp = RMCV_CAMP_BLUE, last_lower_bound = 80; // rmcv_params::camp, ::lower_bound of the last run with the pixel pass (rmcv_batch_get_frame_keys without per-frame keys)
    // the debug view: allocated on first use (ctx_view_prepare), never by a run
    uint64_t* view_overlay = nullptr; // [view_cap][2] colour planes, each as large as a plane of the largest frame
    int view_cap = 0;                 // views the overlay holds
    uint8_t* view_out = nullptr;      // [3 * max_width * max_height] one view on its way to the host (rmcv_batch_get_debug_view)
    // [max_frames] the chosen frames of the view, label, strip, sheet, corner or chessboard call enqueued last (below:
    // frame_list_begin; allocated on first use).  One table serves them all: it is written behind order_begin, and order_begin /
    // order_end put all work of a context in one order whatever stream it comes on, so no call's copy lands before the kernels of the
    // call before have read theirs.  Under external_order nothing orders these calls, which a table per family did not mend either.
    int32_t* frame_list = nullptr;
    // corner refinement: allocated on first use, never by a run
    float* corner_mask = nullptr;     // [CORNER_MASK_MAX] the mask of the call enqueued last, behind its host copy
    float corner_mask_host[rmcv::CORNER_MASK_MAX] = {0};
    int32_t* corner_tab = nullptr;    // [3 * RMCV_CORNER_PER_FRAME_MAX] one frame's corners and status words on their way (rmcv_batch_get_refined_corners)
    // the chessboard detector: allocated on first use, never by a run
    uint32_t* chess_lists = nullptr;  // [max_frames][1 + CHESS_LIST_WORDS] the candidates between its two kernels
    int32_t* chess_tab = nullptr;     // one frame's corners, count, status and candidates on their way (rmcv_batch_get_chessboard)
    // the calibration solve: allocated on first use, never by a run
    double* calib_ws = nullptr;       // [RMCV_CALIB_VIEWS_MAX][CALIB_VIEW_WS] a view's homography, poses and eliminated blocks
    int32_t* calib_vcam = nullptr;    // [RMCV_CALIB_VIEWS_MAX] a view's effective camera, -1 for one not used
    rmcv_calib_guess* calib_guesses = nullptr; // [RMCV_CALIB_CAMERAS_MAX] the guesses of the call enqueued last
    char err[256] = {0};
    std::vector<void*> allocs;
    struct Guarded { uint8_t* base; size_t bytes; const char* name; size_t rear = 0; };
    std::vector<Guarded> guarded; // every dalloc'd buffer with its guard zones (rmcv_ctx_check_guards)
};

static int fail(rmcv_ctx* c, int code, const char* what, hipError_t e = hipSuccess)
{
    if (c) {
        if (e != hipSuccess) snprintf(c->err, sizeof(c->err), "%s: %s", what, hipGetErrorString(e));
        else snprintf(c->err, sizeof(c->err), "%s", what);
    }
    if (e != hipSuccess) (void)hipGetLastError(); // reported through the return code: do not leave it in the thread's sticky slot for others
    return code;
}

// a refusal of the plan headers (a message, or a code with it; none: RMCV_OK) as an entry point returns it
static int refuse(rmcv_ctx* c, const char* why) { return why ? fail(c, RMCV_ERR_BAD_ARG, why) : RMCV_OK; }
static int refuse(rmcv_ctx* c, const rmcv::Refusal& r) { return r ? fail(c, r.code, r.why) : RMCV_OK; }
// ... behind the name of an entry point whose plan header words its refusals without one
static int refuse_as(rmcv_ctx* c, const char* entry, const char* why)
{
    if (!why) return RMCV_OK;
    char msg[160];
    snprintf(msg, sizeof(msg), "%s: %s", entry, why);
    return fail(c, RMCV_ERR_BAD_ARG, msg);
}

#define HIPCHK(c, call, what)                                        \
    do {                                                                \
        (c)->last_what = what;                                          \
        hipError_t e__ = (call);                                        \
        if (e__ != hipSuccess) return fail((c), RMCV_ERR_HIP, what, e__); \
    } while (0)

namespace rmcv {
static inline double now_us()
{
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e6 + ts.tv_nsec * 1e-3;
}
} // namespace rmcv

// waits with a deadline (rmcv_host.hip: poll_deadline)
static int wait_failed(rmcv_ctx* c, int rcw, const char* what, hipError_t e)
{
    if (rcw < 0) return fail(c, RMCV_ERR_HIP, what, e);
    c->timed_out = true;
    snprintf(c->err, sizeof(c->err), "%s: not finished after %d ms (RMCV_OPT_WAIT_TIMEOUT_MS); enqueued last: %s", what, c->wait_timeout_ms, c->last_what);
    return RMCV_ERR_TIMEOUT;
}
static int wait_stream(rmcv_ctx* c, hipStream_t s, const char* what)
{
    hipError_t e = hipSuccess;
    const int rcw = rmcv::wait_stream_deadline(s, c->wait_timeout_ms, &e);
    if (rcw) return wait_failed(c, rcw, what, e);
    return RMCV_OK;
}
static int wait_event(rmcv_ctx* c, hipEvent_t ev, const char* what)
{
    hipError_t e = hipSuccess;
    const int rcw = rmcv::wait_event_deadline(ev, c->wait_timeout_ms, &e);
    if (rcw) return wait_failed(c, rcw, what, e);
    return RMCV_OK;
}
#define WAITCHK(c, call)            \
    do {                            \
        const int rcw__ = (call);   \
        if (rcw__) return rcw__;    \
    } while (0)
// how an entry point that reads results, or rewrites what a batch in flight may read, begins: on the context's device, with all its work finished
static int ctx_ready(rmcv_ctx* c) { hipSetDevice(c->device); return rmcv_batch_sync(c); }

// Work of one context is ordered, whatever streams the caller hands in: every launch shares the context's buffers (and
// k_binary's strip queue).  An event is recorded behind the work enqueued last; a call on ANOTHER stream first waits for it,
// so two streams on one context interleave correctly instead of racing (a context still has ONE owner thread).
static int order_begin(rmcv_ctx* c, hipStream_t s)
{
    if (c->external_order) return RMCV_OK;
    if (c->order_pending && c->last_stream != s) HIPCHK(c, hipStreamWaitEvent(s, c->ev_order, 0), "order: wait for the previous stream");
    return RMCV_OK;
}
static int order_end(rmcv_ctx* c, hipStream_t s)
{
    c->last_stream = s;
    if (c->external_order) return RMCV_OK;
    HIPCHK(c, hipEventRecord(c->ev_order, s), "order: record");
    c->order_pending = true;
    return RMCV_OK;
}

// The device block of ONE call that keeps nothing of its own in the context (a stage-wise helper's image, lists and result; a getter's
// staging).  It is freed when the call returns -- unless a wait of the call ran out: the kernels enqueued may still be using it, and it is
// leaked, as rmcv_ctx_destroy leaks a context whose work does not finish.  Every wait behind a launch on the block goes through waited().
// (In an unnamed namespace, as the functions here are static: the library exports nothing of it.)
namespace {
struct Scratch {
    uint8_t* d = nullptr;
    bool in_flight = false;
    Scratch() = default;
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
    ~Scratch()
    {
        if (d && !in_flight) hipFree(d);
    }
    hipError_t alloc(size_t bytes) { return hipMalloc((void**)&d, bytes); }
    int waited(int rc)
    {
        in_flight = rc == RMCV_ERR_TIMEOUT;
        return rc;
    }
};
} // namespace

// Every device buffer of a context lies between two GUARD-byte zones filled with a fixed pattern when the context is created;
// rmcv_ctx_check_guards reads them back.  A kernel that stores one row, word or record past either end of its buffer -- the
// partial last strip of a 1200-row frame, the ragged last block of a 1920-pixel row -- shows up there instead of in a neighbour.
#ifndef RMCV_GUARD
#define RMCV_GUARD 4096
#endif
static constexpr size_t GUARD = RMCV_GUARD;
static constexpr int GUARD_BYTE = 0xA5;
template <typename T>
static hipError_t dalloc_named(rmcv_ctx* c, T** p, size_t count, const char* name)
{
    void* q = nullptr;
    const size_t bytes = (count * sizeof(T) + 255) & ~(size_t)255;
    hipError_t e = hipMalloc(&q, bytes + 2 * GUARD);
    if (e == hipSuccess) {
        c->allocs.push_back(q);
        c->guarded.push_back({(uint8_t*)q, bytes, name});
        *p = (T*)((uint8_t*)q + GUARD);
        e = hipMemset(q, GUARD_BYTE, GUARD);
        // the rounding slack behind the payload belongs to the rear zone
        if (e == hipSuccess) e = hipMemset((uint8_t*)q + GUARD + count * sizeof(T), GUARD_BYTE, bytes - count * sizeof(T) + GUARD);
        c->guarded.back().bytes = count * sizeof(T);
        c->guarded.back().rear = bytes - count * sizeof(T) + GUARD;
    }
    return e;
}
#define dalloc(c, p, count) dalloc_named((c), (p), (count), #p)

// ---- what the entry points on chosen frames of a batch and their stage-wise twins share (rmcv_views.hip, rmcv_capture.hip) ----
static int hip_failed(rmcv_ctx* c, const char* what, hipError_t e) { return fail(c, e == hipErrorOutOfMemory ? RMCV_ERR_NOMEM : RMCV_ERR_HIP, what, e); }
static hipStream_t stream_of(rmcv_ctx* c, void* hip_stream) { return hip_stream ? (hipStream_t)hip_stream : c->stream; }
// a table of the context's, allocated when the first call needs it; `what` words the failure
template <typename T>
static int lazy_table(rmcv_ctx* c, T** p, size_t count, const char* name, const char* what)
{
    if (*p) return RMCV_OK;
    const hipError_t e = dalloc_named(c, p, count, name);
    return e == hipSuccess ? RMCV_OK : hip_failed(c, what, e);
}
#define LAZY_TABLE(c, p, count, what) lazy_table((c), (p), (count), #p, (what))
// How every batch form begins to enqueue: the call takes its place in the context's order and its chosen frames (host values, checked) go
// to rmcv_ctx::frame_list behind the work enqueued before.  The caller launches on `s` and ends with order_end.
static int frame_list_begin(rmcv_ctx* c, const int32_t* frames, int n, hipStream_t s, const char* what)
{
    int rc = LAZY_TABLE(c, &c->frame_list, (size_t)c->lim.max_frames, "allocating the chosen frames' list");
    if (rc || (rc = order_begin(c, s))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->frame_list, frames, (size_t)n * 4, hipMemcpyHostToDevice, s), what);
    return RMCV_OK;
}
// The host block of a stage-wise helper: the caller's BGR image first, as rows of 3 w bytes rounded up to 16, the parts behind it 16-byte aligned
static size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }
static int bgr_row_bytes(int w) { return (3 * w + 15) & ~15; }
static void pack_bgr(uint8_t* dst, const uint8_t* bgr, int w, int h, int stride)
{
    for (int y = 0; y < h; y++) memcpy(dst + (size_t)y * bgr_row_bytes(w), bgr + (size_t)y * stride, (size_t)3 * w);
}
// How such a helper runs, behind its checks and ctx_ready: a Scratch block of `total` bytes, its first `in_bytes` uploaded from `host`,
// launch(d) on the context's stream (`what` names it for a later timeout), the wait under `kernel`, then download(d); `who` words a failure
template <typename Launch, typename Download>
static int scratch_call(rmcv_ctx* c, size_t total, const void* host, size_t in_bytes, Launch launch, const char* what, const char* kernel, const char* who,
                        Download download)
{
    Scratch d;
    hipError_t e = d.alloc(total);
    if (e == hipSuccess) e = hipMemcpyAsync(d.d, host, in_bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = launch(d.d);
    c->last_what = what;
    int rcw = 0;
    if (e == hipSuccess) rcw = d.waited(wait_stream(c, c->stream, kernel));
    if (e == hipSuccess && rcw == 0) e = download(d.d);
    return e != hipSuccess ? hip_failed(c, who, e) : rcw;
}

// ---- what the chain needs of the batch side (rmcv_host.hip) and the batch side of the chain (rmcv_frame.hip) ----
namespace rmcv {
inline PixelVariant geom_variant(const Geom& g) { return pixel_variant(g.input_format, g.enhance, g.win, g.keys); }
// bytes of one sample of what the context's options describe: 3 per BGR pixel, 1 or 2 per Bayer sample
inline int ctx_pixel_bytes(const rmcv_ctx* c) { return c->input.pixel_bytes(); }
// every per-frame mode of a binding off: per-run keys (Geom::keys is bind_geom's), camera 0 and model 0 for every frame, no window requests
inline void reset_modes(rmcv_ctx* c)
{
    c->bufs.key_camps = c->bufs.key_lbs = nullptr;
    c->bufs.cam_req = nullptr;
    c->bufs.model_idx = nullptr;
    c->geom.models = 0;
    c->bufs.win_req = nullptr;
}
// one armour's row of Bufs::poses, rvec | tvec | world position, into the callers' three arrays (each may be null)
struct PoseRow { double v[9]; };
inline void scatter_pose(const PoseRow& row, double* rvecs, double* tvecs, double* positions, size_t dst)
{
    for (int k = 0; k < 3; k++) {
        if (rvecs) rvecs[3 * dst + k] = row.v[k];
        if (tvecs) tvecs[3 * dst + k] = row.v[3 + k];
        if (positions) positions[3 * dst + k] = row.v[6 + k];
    }
}
// frame slot 0 of what is bound, for a stage-wise call on the caller's own data (the caller's enemy, whatever keys the batch bound to
// the context has)
inline Geom one_frame_geom(const rmcv_ctx* c)
{
    Geom g1 = c->geom;
    g1.n_frames = 1;
    g1.keys = 0;
    return g1;
}
// the batch bound to `c` as step_refusal (tracker_plan.h) reads it
inline StepBatch step_batch(const rmcv_ctx* c)
{
    const Geom& g = c->geom;
    return {c->device, g.n_frames, c->bufs.frames != nullptr, g.frame_w, g.frame_h, g.win, g.w, g.h};
}
// checks and records a binding (bind_plan.h) and enqueues what a change of extent costs; win_w > 0: the frames are read through
// win_w x win_h windows.  The per-frame modes of the binding before are the caller's to reset (reset_modes).
int set_geom(rmcv_ctx* c, int n_frames, int w, int h, int stride, int64_t frame_pitch, hipStream_t as = nullptr, int win_w = 0, int win_h = 0);
int ensure_own_frames(rmcv_ctx* c, size_t need);
int check_layout(rmcv_ctx* c);
int check_sample_ptr(rmcv_ctx* c, const void* p);
// frame slot 0 of the device buffers no longer holds what the per-frame chain returned last (see FrameChain::res_nc)
void resident_none(rmcv_ctx* c);
// load host CSR contours (findContours order) into frame slot 0 (stored in discovery order = reversed)
int load_contours(rmcv_ctx* c, const rmcv_point* pts, const int32_t* offs, int n);
} // namespace rmcv
