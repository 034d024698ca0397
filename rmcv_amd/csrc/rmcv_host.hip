// rmcv_host.hip -- the C-ABI of include/rmcv_abi.h: the context and its HBM buffers, binding a batch, the run, sync, and the batch
// setters and getters; the tracker, attitude and harvest steps of a batch.  What a binding and a run decide is bind_plan.h's (pure, checked
// by a host compiler); the views and the calibration capture of a batch are rmcv_views.hip and rmcv_capture.hip, the stage-wise helpers
// rmcv_stagewise.hip, the context-free entry points rmcv_rules.hip.
//
// Host side of the drop-in boundary.  The reference's boundary is the C++ linkage of `librmcv`
// (/root/reference/CMakeLists.txt:13-16); the calls a maintainer re-hosts on this ABI are exactly
// rm::extract_color / rm::filter_lightblobs / rm::filter_armours (executable/main.cpp:172-176).
// No CPU path exists here: every entry point enqueues hand-written HIP kernels.
#include <sched.h>
#include <time.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "rmcv_ctx.h"
#include "device_pack.h"

using namespace rmcv;

// ---- waits with a deadline ------------------------------------------------------------------------------------------------------
// hipStreamSynchronize / hipEventSynchronize spin for ~0.1 ms and then park the thread on an interrupt; the wake-up costs another
// 0.1 ms or more (the per-frame chain from a C host, 0.16 ms of GPU work: 0.18 / 0.28 / 0.40 ms depending on how many of its two waits
// went to sleep -- VERDICT r4 weak #4), and a kernel that never finishes parks the caller for good (weak #3).  These poll instead:
// spinning for the first 2 ms, yielding up to 20 ms, sleeping 0.2 ms at a time after that, up to the context's deadline.
namespace rmcv {
template <typename Q>
static int poll_deadline(Q query, int timeout_ms, hipError_t* err)
{
    const double t0 = now_us();
    int rc = 0;
    for (;;) {
        const hipError_t e = query();
        if (e == hipSuccess) break;
        if (e != hipErrorNotReady) { *err = e; rc = -1; break; }
        const double dt = now_us() - t0;
        if (timeout_ms > 0 && dt > timeout_ms * 1000.0) { rc = 1; break; }
        if (dt < 2000.0) __builtin_ia32_pause();
        else if (dt < 20000.0) sched_yield();
        else { timespec nap = {0, 200000}; nanosleep(&nap, nullptr); }
    }
    (void)hipGetLastError(); // (hipErrorNotReady is not an error)
    return rc;
}
int wait_stream_deadline(hipStream_t s, int timeout_ms, hipError_t* err) { return poll_deadline([s] { return hipStreamQuery(s); }, timeout_ms, err); }
int wait_event_deadline(hipEvent_t ev, int timeout_ms, hipError_t* err) { return poll_deadline([ev] { return hipEventQuery(ev); }, timeout_ms, err); }
} // namespace rmcv

extern "C" {

int rmcv_abi_version(void) { return RMCV_ABI_VERSION; }
int64_t rmcv_pixel_ws_launches(void) { return pixel_ws_launches(); }
int64_t rmcv_pixel_image_delta_launches(void) { return pixel_image_delta_launches(); }
int64_t rmcv_pixel_plane_delta_launches(void) { return pixel_plane_delta_launches(); }

const char* rmcv_last_error(const rmcv_ctx* ctx) { return ctx ? ctx->err : "null context"; }

void rmcv_ctx_destroy(rmcv_ctx* c)
{
    if (!c) return;
    hipSetDevice(c->device);
    {   // Work that does not finish within the deadline is not waited for a second time without one: the context's device memory,
        // streams and pinned buffers are LEAKED (a kernel may still be writing them) instead of the caller being parked for good.
        hipError_t e = hipSuccess;
        const int t = c->wait_timeout_ms;
        bool stuck = false;
        if (c->external_order && c->ext_done && c->timed_out) stuck |= wait_event_deadline(c->ext_done, t, &e) != 0;
        if (c->order_pending) stuck |= wait_event_deadline(c->ev_order, t, &e) == 1;
        if (c->stream) stuck |= wait_stream_deadline(c->stream, t, &e) == 1;
        if (c->chain.side) stuck |= wait_stream_deadline(c->chain.side, t, &e) == 1;
        if (stuck) {
            fprintf(stderr, "rmcv_ctx_destroy: work of this context has not finished after %d ms (enqueued last: %s); its buffers are leaked\n", t, c->last_what);
            delete c;
            return;
        }
    }
    c->chain.release();
    for (void* p : c->allocs) hipFree(p);
    if (c->own_frames) hipFree(c->own_frames);
    for (auto& e : c->ev)
        if (e) hipEventDestroy(e);
    if (c->ev_order) hipEventDestroy(c->ev_order);
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;
}

int rmcv_ctx_create(int device, const rmcv_limits* limits, rmcv_ctx** out)
{
    if (!out) return RMCV_ERR_BAD_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return RMCV_ERR_NO_DEVICE;
    rmcv_limits d;
    rmcv_default_limits(&d);
    if (limits) {
        if (limits->max_frames > 0) d.max_frames = limits->max_frames;
        if (limits->max_width > 0) d.max_width = limits->max_width;
        if (limits->max_height > 0) d.max_height = limits->max_height;
        if (limits->max_contours > 0) d.max_contours = limits->max_contours;
        if (limits->max_points > 0) d.max_points = limits->max_points;
        if (limits->max_blobs > 0) d.max_blobs = limits->max_blobs;
        if (limits->max_armours > 0) d.max_armours = limits->max_armours;
    }
    rmcv_ctx* c = new (std::nothrow) rmcv_ctx();
    if (!c) return RMCV_ERR_NOMEM;
    c->device = device;
    c->lim = Limits{d.max_frames, d.max_width, d.max_height, d.max_contours, d.max_points, d.max_blobs, d.max_armours};
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    for (int i = 0; i < 6 && e == hipSuccess; i++) e = hipEventCreate(&c->ev[i]);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_order, hipEventDisableTiming);
    if (e == hipSuccess) e = c->chain.init();
    if (e == hipSuccess) {
        hipDeviceProp_t prop;
        c->geom.device = device;
        c->geom.n_cu = (device < MAX_DEVICES && hipGetDeviceProperties(&prop, device) == hipSuccess) ? prop.multiProcessorCount : 0;
        if (device >= MAX_DEVICES) e = hipErrorInvalidDevice;
    }
    const size_t F = (size_t)d.max_frames;
    const size_t plane = (size_t)(d.max_height + 2) * ((d.max_width + 63) / 64 + 2);
    Bufs& b = c->bufs;
    if (e == hipSuccess) e = dalloc(c, &b.binary, F * d.max_width * d.max_height);
    if (e == hipSuccess) e = dalloc(c, &b.bits, F * plane);
    if (e == hipSuccess) e = dalloc(c, &b.rowmask, F * d.max_height);
    if (e == hipSuccess) e = dalloc(c, &b.strip_ctr, 9 * CTR_STRIDE);
    if (e == hipSuccess) e = dalloc(c, &b.lab, F * plane);
    if (e == hipSuccess) e = dalloc(c, &b.neg, F * plane);
    if (e == hipSuccess) e = dalloc(c, &b.points, F * d.max_points);
    if (e == hipSuccess) e = dalloc(c, &c->pack_pts, F * d.max_points);
    if (e == hipSuccess) e = dalloc(c, &c->pack_offs, F * (d.max_contours + 1));
    if (e == hipSuccess) e = dalloc(c, &b.cont_start, F * d.max_contours);
    if (e == hipSuccess) e = dalloc(c, &b.cont_len, F * d.max_contours);
    if (e == hipSuccess) e = dalloc(c, &b.n_contours, F);
    if (e == hipSuccess) e = dalloc(c, &b.n_points, F);
    if (e == hipSuccess) e = dalloc(c, &b.visit_xy, F * VISIT_CAP);
    { // the mid tier's tables (one 4.5-5.7 MB block per frame slot) are allocated when a geometry is bound, for the frames bound: ensure_mid
        const int64_t words = (int64_t)((d.max_width + 63) / 64) * d.max_height;
        b.mid_slot_cap = (int)std::min<int64_t>(words, 65535);
        b.mid_stride = (int64_t)((mid_bytes(b.mid_slot_cap) + 255) & ~(size_t)255);
        b.mid = nullptr;
    }
    if (e == hipSuccess) e = dalloc(c, &b.blobs, F * d.max_blobs);
    if (e == hipSuccess) e = dalloc(c, &b.blob_src, F * d.max_blobs);
    if (e == hipSuccess) e = dalloc(c, &b.ellipses, F * d.max_blobs);
    if (e == hipSuccess) e = dalloc(c, &b.neg_idx, F * d.max_contours);
    if (e == hipSuccess) e = dalloc(c, &b.elig, F * d.max_contours);
    if (e == hipSuccess) e = dalloc(c, &b.n_elig, F);
    if (e == hipSuccess) e = dalloc(c, &b.slot_kind, F * d.max_contours);
    if (e == hipSuccess) e = dalloc(c, &b.slot_ell, F * d.max_contours);
    if (e == hipSuccess) e = dalloc(c, &b.n_blobs, F);
    if (e == hipSuccess) e = dalloc(c, &b.n_neg, F);
    if (e == hipSuccess) e = dalloc(c, &b.armours, F * d.max_armours);
    if (e == hipSuccess) e = dalloc(c, &b.n_armours, F);
    if (e == hipSuccess) e = dalloc(c, &b.status, F);
    if (e == hipSuccess) e = dalloc(c, &b.frame_order, F);
    if (e == hipSuccess) e = dalloc(c, &c->order_scratch, 2 * F);
    if (e == hipSuccess) e = dalloc(c, &b.enh_sums, 3 * F);
    if (e == hipSuccess) e = dalloc(c, &b.enh_gamma, F);
    if (e == hipSuccess) e = dalloc(c, &b.enh_lut, 256 * F);
    if (e == hipSuccess) e = dalloc(c, &b.enh_m, 256 * F);
    if (e == hipSuccess) e = dalloc(c, &b.win_eff, F);
    if (e == hipSuccess) e = dalloc(c, &c->win_own, F);
    if (e == hipSuccess) e = dalloc(c, &b.imgmask, F * d.max_height); // (last: every other buffer stays where it was before there was a mask)
    if (e == hipSuccess) e = dalloc(c, &b.key_eff, F); // (per-frame detection keys: behind the mask, for the same reason)
    if (e == hipSuccess) e = dalloc(c, &b.key_enemy, F);
    if (e == hipSuccess) e = dalloc(c, &c->key_own, 2 * F);
    if (e == hipSuccess) {
        hipMemset(b.strip_ctr, 0, 9 * CTR_STRIDE * sizeof(int));
        hipMemset(b.n_contours, 0, F * 4);
        hipMemset(b.n_points, 0, F * 4);
        hipMemset(b.n_blobs, 0, F * 4);
        hipMemset(b.n_neg, 0, F * 4);
        hipMemset(b.n_armours, 0, F * 4);
        e = hipMemset(b.status, 0, F * 4);
        if (e == hipSuccess) e = hipMemset(b.win_eff, 0, F * sizeof(rmcv_point));
        if (e == hipSuccess) e = hipMemset(c->win_own, 0, F * sizeof(rmcv_point));
        if (e == hipSuccess) e = hipMemset(b.key_eff, 0, F * sizeof(FrameKey));
        if (e == hipSuccess) e = hipMemset(b.key_enemy, 0, F * 4);
    }
    if (e == hipSuccess) { // rmcv_batch_get_gammas before the first run with the option: every frame reads 1 (the identity table)
        const std::vector<float> ones(F, 1.0f);
        e = hipMemcpy(b.enh_gamma, ones.data(), F * sizeof(float), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        fprintf(stderr, "rmcv_ctx_create: %s\n", hipGetErrorString(e));
        rmcv_ctx_destroy(c);
        return e == hipErrorOutOfMemory ? RMCV_ERR_NOMEM : RMCV_ERR_HIP;
    }
    *out = c;
    return RMCV_OK;
}

} // extern "C"

namespace rmcv {
void ctx_external_order(rmcv_ctx* c, hipEvent_t done)
{
    c->external_order = true;
    c->ext_done = done;
}
const Limits& ctx_limits(const rmcv_ctx* c) { return c->lim; }
uint64_t ctx_blocking_calls(const rmcv_ctx* c) { return c->blocking_calls; }
int ctx_wait_timeout_ms(const rmcv_ctx* c) { return c->wait_timeout_ms; }
bool pixel_ws_full(const rmcv_ctx* c, int lower_bound, const RunPlan& plan)
{
    return pixel_shape(pixel_batch(c->geom, c->bufs, geom_variant(c->geom), lower_bound, plan)).ws_full;
}
int ctx_pixel_sets(const rmcv_ctx* c) { return c->n_sets; }
int ctx_pixel_set(const rmcv_ctx* c) { return c->cur_set; }
void ctx_use_pixel_set(rmcv_ctx* c, int s)
{
    if (s == c->cur_set || s < 0 || s >= c->n_sets) return;
    Bufs& b = c->bufs;
    const rmcv_ctx::PixelSet mine = {b.binary, b.bits, b.rowmask, b.imgmask, c->image, c->plane_sync};
    b.binary = c->parked.binary, b.bits = c->parked.bits, b.rowmask = c->parked.rowmask, b.imgmask = c->parked.imgmask;
    c->image = c->parked.image, c->plane_sync = c->parked.plane_sync;
    c->parked = mine;
    c->cur_set = s;
}
bool ctx_bind_enqueues(const rmcv_ctx* c, int n_frames, int w, int h)
{
    const ExtentChange change = extent_change(c->geom_w, c->geom_h, c->order_n, c->order_h, w, h, n_frames);
    return change.planes || change.order;
}
RunPlan ctx_plan(const rmcv_ctx* c) { return {c->pixel_shape, c->pixel_groups, c->sparse_waves, c->dense_defer ? SPARSE_SPLIT_BOTH : SPARSE_STANDARD}; }
int ctx_enhance(const rmcv_ctx* c) { return c->input.enhance; }
int ctx_n_cameras(const rmcv_ctx* c) { return c->bufs.pnp_cams ? c->bufs.n_cameras : 0; }
void ctx_set_frame_cameras(rmcv_ctx* c, const void* d_idx) { c->bufs.cam_req = (const int32_t*)d_idx; }
int ctx_n_models(const rmcv_ctx* c) { return c->bufs.svm_table ? c->bufs.svm_models : 0; }
void ctx_set_frame_models(rmcv_ctx* c, const void* d_idx)
{
    c->bufs.model_idx = (const int32_t*)d_idx;
    c->geom.models = d_idx != nullptr;
}
PixelVariant ctx_pixel_variant(const rmcv_ctx* c) { return geom_variant(c->geom); }
int ctx_frame_pixel_bytes(const rmcv_ctx* c) { return ctx_pixel_bytes(c); }
void ctx_record_batch(const rmcv_ctx* c, RecordBatch* b)
{
    const Geom& g = c->geom;
    b->input_format = g.input_format, b->sample_bits = 8 * g.sample_bytes, b->valid_bit = g.valid_bit, b->orient = g.orient;
    b->w_bytes = g.frame_w * geom_pixel_bytes(g);
    b->lag = pack_lag(g.input_format, b->sample_bits);
    b->key_eff = g.keys ? c->bufs.key_eff : nullptr;
    b->key_enemy = g.keys ? c->bufs.key_enemy : nullptr;
    b->win_eff = g.win ? c->bufs.win_eff : nullptr;
}
int ctx_compact(rmcv_ctx* c, void* d_armours_out, int cap, void* d_frame_offs, void* d_status_or, hipStream_t s, void* hd_record, int host_head)
{
    HIPCHK(c, launch_compact_armours(c->geom, c->bufs, c->lim, (rmcv_armour*)d_armours_out, cap, (int32_t*)d_frame_offs, s, (int32_t*)d_status_or, (uint8_t*)hd_record, host_head), "k_compact_armours");
    return RMCV_OK;
}
} // namespace rmcv

int rmcv::ensure_own_frames(rmcv_ctx* c, size_t need)
{
    if (need <= c->own_frames_bytes) return RMCV_OK;
    if (c->own_frames) hipFree(c->own_frames);
    c->own_frames = nullptr;
    c->own_frames_bytes = 0;
    size_t cap = (size_t)((3 * c->lim.max_width + 15) & ~15) * c->lim.max_height * c->lim.max_frames;
    if (cap < need) cap = need;
    HIPCHK(c, hipMalloc((void**)&c->own_frames, cap), "hipMalloc frames");
    c->own_frames_bytes = cap;
    return RMCV_OK;
}

// The mid tier's scratch (Bufs::mid) for the first `n_frames` frame slots, grow-only.  A context that only ever binds one frame (the
// per-frame drop-in chain) holds 5.7 MB of it, a 256-frame batch context 1.2-1.5 GB -- allocated for every slot at creation it more
// than doubled a default context's footprint for users who never see a dense frame.  If the memory is not to be had the tier is
// simply absent (mid == nullptr): the kernels hand such frames to the sequential scanner instead of failing the call.
// A pipeline allocates it for every context of its ring when it is created (ctx_prepare_ring): rmcv_pipeline_submit never allocates.
static int ensure_mid(rmcv_ctx* c, int n_frames)
{
    if (n_frames <= c->mid_frames || c->mid_failed) return RMCV_OK;
    const bool no_mid = getenv("RMCV_NO_MID") && atoi(getenv("RMCV_NO_MID")); // test knob: behave as if the allocation had failed (read at every binding)
    c->blocking_calls++;
    if (c->bufs.mid) { // grow: nothing of this context may still be running on the old block
        const int rcs = rmcv_batch_sync(c);
        if (rcs) return rcs;
        uint8_t* raw = c->bufs.mid - GUARD;
        for (size_t i = 0; i < c->allocs.size(); i++)
            if (c->allocs[i] == raw) { c->allocs.erase(c->allocs.begin() + i); break; }
        for (size_t i = 0; i < c->guarded.size(); i++)
            if (c->guarded[i].base == raw) { c->guarded.erase(c->guarded.begin() + i); break; }
        (void)hipFree(raw);
        c->bufs.mid = nullptr;
        c->mid_frames = 0;
    }
    // (a batch context binds its full batch sooner or later: go there at once rather than in steps)
    const int want = n_frames > 1 ? c->lim.max_frames : 1;
    uint8_t* m = nullptr;
    const hipError_t e = no_mid ? hipErrorOutOfMemory : dalloc_named(c, &m, (size_t)want * (size_t)c->bufs.mid_stride, "b.mid");
    if (e != hipSuccess) {
        (void)hipGetLastError();
        c->mid_failed = true; // degrade, once: frames beyond the LDS tables take the sequential scanner (RMCV_FRAME_SLOW_PATH)
        return RMCV_OK;
    }
    c->bufs.mid = m;
    c->mid_frames = want;
    return RMCV_OK;
}

// The order in which the sparse kernel's workgroups take frames (Bufs::frame_order), computed ON the device, on the stream of the batch
// that needs it (round 5: it used to be a host computation + a blocking copy inside rmcv_pipeline_submit).  k_binary hands XCD q the
// strips [q * per_xcd, (q + 1) * per_xcd) in order, so XCD q completes the frames whose LAST strip lies in that range, one after the
// other; workgroups are dealt to the XCDs round-robin (workgroup b runs on XCD b & 7).  Round t therefore offers the t-th frame of
// every XCD's list; XCDs whose list is shorter leave holes that the remaining frames fill.  Any bijection is correct -- this one makes
// a frame's plane reads hits in the L2 its planes were written through.  Sequential by nature and a few hundred entries long: one lane
// on LDS tables (global scratch beyond 2048 frames), once per change of (n_frames, h).
namespace rmcv {
static constexpr int ORDER_LDS = 2048;
__global__ __launch_bounds__(256) void k_frame_order(int32_t* __restrict__ order, int32_t* __restrict__ scratch, int n, int strips)
{
    __shared__ int32_t s_o[ORDER_LDS], s_rest[ORDER_LDS], s_used[ORDER_LDS];
    __shared__ int s_lo[9];
    const bool in_lds = n <= ORDER_LDS;
    int32_t* o = in_lds ? s_o : order;
    int32_t* rest = in_lds ? s_rest : scratch;
    int32_t* used = in_lds ? s_used : scratch + n;
    const int tid = threadIdx.x;
    for (int i = tid; i < n; i += 256) { o[i] = -1; used[i] = 0; }
    __threadfence_block();
    __syncthreads();
    if (tid == 0) {
        const int per_xcd = (n * strips + 7) >> 3;
        int q = 0;
        s_lo[0] = 0; // list q = the frames [s_lo[q], s_lo[q + 1]): q(f) is monotone in f
        for (int f = 0; f < n; f++) {
            int qf = (f * strips + strips - 1) / per_xcd;
            if (qf > 7) qf = 7;
            while (q < qf) s_lo[++q] = f;
        }
        while (q < 8) s_lo[++q] = n;
        int longest = 0;
        for (q = 0; q < 8; q++) longest = max(longest, s_lo[q + 1] - s_lo[q]);
        int nrest = 0;
        for (int t = 0; t < longest; t++)
            for (q = 0; q < 8; q++)
                if (t < s_lo[q + 1] - s_lo[q]) {
                    const int b_ = t * 8 + q, v = s_lo[q] + t;
                    if (b_ < n) o[b_] = v;
                    else rest[nrest++] = v; // (slots t * 8 + q beyond n -> `rest`; slots left empty by short lists take them in order)
                }
        int r = 0;
        for (int b_ = 0; b_ < n; b_++)
            if (o[b_] < 0 && r < nrest) o[b_] = rest[r++];
        for (int b_ = 0; b_ < n; b_++)
            if (o[b_] >= 0) used[o[b_]] = 1;
        int nf = 0; // slots of short lists that `rest` did not fill: whatever frames are still unassigned (keeps the map a bijection)
        for (int b_ = 0; b_ < n; b_++)
            if (o[b_] < 0) {
                while (used[nf]) nf++;
                o[b_] = nf;
                used[nf] = 1;
            }
    }
    __threadfence_block();
    __syncthreads();
    if (in_lds)
        for (int i = tid; i < n; i += 256) order[i] = s_o[i];
}
} // namespace rmcv

namespace rmcv {
// holds a stream back for `ns` nanoseconds (one wavefront asleep; the constant-rate counter runs at 100 MHz)
__global__ void k_delay(unsigned long long ns)
{
    const unsigned long long t0 = wall_clock64();
    while ((wall_clock64() - t0) * 10ull < ns) __builtin_amdgcn_s_sleep(32);
}
hipError_t launch_delay(unsigned long long ns, hipStream_t s) { return launch(k_delay, dim3(1), dim3(64), 0, s, ns); }
} // namespace rmcv

// ---- binding a geometry: what is refused and what is recorded is bind_plan.h's; here are the HIP calls ----
int rmcv::check_layout(rmcv_ctx* c) { return refuse(c, layout_refusal(c->input)); }
// a frame pointer of 2-byte samples
int rmcv::check_sample_ptr(rmcv_ctx* c, const void* p)
{
    if (c->input.format && c->input.sample_bits == 16 && ((uintptr_t)p & 1))
        return fail(c, RMCV_ERR_BAD_ARG, "16-bit samples (RMCV_OPT_INPUT_SAMPLE_BITS): the frame pointer must be 2-byte aligned");
    return RMCV_OK;
}

// what per-frame detection keys refuse of the frames' format (fmt / enh: what they are read as), checked before anything of the context moves
static int check_frame_camps(rmcv_ctx* c, int fmt, int enh) { return refuse(c, pixel_refusal(fmt, enh, false, true, false)); }

// The extent in Geom (extent_fields) has been set.  When it changes the padded planes are zeroed (their pads must read 0) and the frame
// order is recomputed -- both ENQUEUED: on `as` when the caller (a pipeline) orders this context's work on its own streams and has
// already made `as` wait for the context's last batch; otherwise on the context's stream, behind a wait for everything the context has
// in flight and with a wait for them behind (the launches that follow may go to any stream of the caller's).
static int extent_apply(rmcv_ctx* c, hipStream_t as)
{
    const Geom& g = c->geom;
    const ExtentChange change = extent_change(c->geom_w, c->geom_h, c->order_n, c->order_h, g.w, g.h, g.n_frames);
    if (!change.planes && !change.order) return RMCV_OK;
    hipStream_t s = as ? as : c->stream;
    if (!as) { // the planes are re-zeroed and the frame order rewritten under the kernels' feet otherwise
        c->blocking_calls++;
        const int rcs = rmcv_batch_sync(c);
        if (rcs) return rcs;
    }
    if (change.planes) {
        const size_t plane = (size_t)(c->lim.max_height + 2) * ((c->lim.max_width + 63) / 64 + 2);
        HIPCHK(c, hipMemsetAsync(c->bufs.bits, 0, (size_t)c->lim.max_frames * plane * 8, s), "memset planes");
        if (c->n_sets > 1) HIPCHK(c, hipMemsetAsync(c->parked.bits, 0, (size_t)c->lim.max_frames * plane * 8, s), "memset planes");
        HIPCHK(c, hipMemsetAsync(c->bufs.lab, 0, (size_t)c->lim.max_frames * plane * 8, s), "memset planes");
        HIPCHK(c, hipMemsetAsync(c->bufs.neg, 0, (size_t)c->lim.max_frames * plane * 8, s), "memset planes");
        c->geom_w = g.w;
        c->geom_h = g.h;
        c->image = c->parked.image = IMAGE_STATE_UNKNOWN; // rows and frames of the byte image and of its mask now start elsewhere
        c->plane_sync = c->parked.plane_sync = 0;
    }
    if (change.order) {
        const int strips = (g.h + STRIP_ROWS - 1) / STRIP_ROWS;
        HIPCHK(c, launch(k_frame_order, dim3(1), dim3(256), 0, s, c->bufs.frame_order, c->order_scratch, g.n_frames, strips), "k_frame_order");
        c->order_n = g.n_frames;
        c->order_h = g.h;
    }
    if (!as) WAITCHK(c, wait_stream(c, s, "binding a geometry"));
    return RMCV_OK;
}

// win_w > 0: the frames are read through win_w x win_h windows
int rmcv::set_geom(rmcv_ctx* c, int n_frames, int w, int h, int stride, int64_t frame_pitch, hipStream_t as, int win_w, int win_h)
{
    int rc = refuse(c, binding_refusal(c->lim, c->input, n_frames, w, h, stride, frame_pitch, win_w, win_h));
    if (rc || (rc = ensure_mid(c, n_frames))) return rc;
    bind_geom(c->geom, c->input, n_frames, w, h, stride, frame_pitch, win_w, win_h);
    return extent_apply(c, as);
}

// The tail of every binder: `frames` are what the context reads from now on.  A new batch starts with every per-frame mode off
// (reset_modes), the host's pose matrices (an attitude step's were its batch's) and nothing of it run.
static int bound(rmcv_ctx* c, const void* frames)
{
    c->bufs.frames = (const uint8_t*)frames;
    reset_modes(c);
    c->bufs.pose_base2gripper = c->bufs.base2gripper;
    c->last_stages = 0;
    return RMCV_OK;
}

// ---- the shapes the batch setters and getters share ----

// A per-frame request table (window origins, camps, lower bounds, cameras) is the host's values, copied into the context's `own` table
// once nothing in flight reads it (`sync`: the caller has not waited already), or the caller's device memory, borrowed; both null: off.
// *req is what the runs read from then on; it changes only on success.
template <typename T>
static int set_request_table(rmcv_ctx* c, const T** req, T* own, const T* h_vals, const void* d_vals, bool sync, const char* what)
{
    if (h_vals) {
        if (sync) {
            if (const int rc = ctx_ready(c)) return rc; // the table about to be rewritten may still be read by a batch in flight
        }
        HIPCHK(c, hipMemcpy(own, h_vals, (size_t)c->geom.n_frames * sizeof(T), hipMemcpyHostToDevice), what);
    }
    *req = h_vals ? own : (const T*)d_vals;
    return RMCV_OK;
}

// An effective per-frame table as the last run left it, for the first `cap` frames bound (the context is ready: the caller has waited):
// d_eff's entries while the mode is on, `off` for every frame otherwise
template <typename T>
static int get_effective_table(rmcv_ctx* c, T* out, int cap, bool on, const T* d_eff, const T& off, const char* what)
{
    const int n = std::min(cap, c->geom.n_frames);
    if (n <= 0) return RMCV_OK;
    if (!on) std::fill_n(out, n, off);
    else HIPCHK(c, hipMemcpy(out, d_eff, (size_t)n * sizeof(T), hipMemcpyDeviceToHost), what);
    return RMCV_OK;
}

// the armour counts of the frames bound and their sum: what the gathers go by.  The detection kernels never leave a count beyond max_armours
// (they clamp and set RMCV_FRAME_OVF_ARMOURS), but a caller who writes the table through rmcv_batch_device_views may: the kernels behind it
// (k_pnp, the classifier, the harvest) then take rows 0 .. min(n, max_armours) - 1, and so do the gathers -- a frame's block has no more rows.
static int armour_counts(rmcv_ctx* c, std::vector<int32_t>& cnt, int64_t* total)
{
    cnt.resize(c->geom.n_frames);
    HIPCHK(c, hipMemcpy(cnt.data(), c->bufs.n_armours, cnt.size() * 4, hipMemcpyDeviceToHost), "D2H");
    *total = 0;
    for (int32_t& n : cnt) {
        n = n < 0 ? 0 : (n > c->lim.max_armours ? c->lim.max_armours : n);
        *total += n;
    }
    return RMCV_OK;
}
// the first cnt[f] rows of every frame's block of a device table [frame][max_armours], frame after frame
template <typename T>
static int gather_rows(rmcv_ctx* c, const T* d_table, const std::vector<int32_t>& cnt, T* out, const char* what)
{
    const size_t row_cap = (size_t)c->lim.max_armours;
    std::vector<T> all(cnt.size() * row_cap);
    HIPCHK(c, hipMemcpy(all.data(), d_table, all.size() * sizeof(T), hipMemcpyDeviceToHost), what);
    for (size_t f = 0; f < cnt.size(); f++) out = std::copy_n(all.data() + f * row_cap, cnt[f], out);
    return RMCV_OK;
}

// One run: the launches run_steps (bind_plan.h) decides on, in its order; `timed`: the events of rmcv_batch_run_timed between the stages
static int run_stages(rmcv_ctx* c, const rmcv_params* p, int stages, hipStream_t s, bool timed, const RunPlan& plan,
                      const rmcv_legacy_params* lp = nullptr, bool* lean = nullptr)
{
    const Geom& g = c->geom;
    const Bufs& b = c->bufs;
    const Limits& lim = c->lim;
    const RunSteps st = run_steps(stages, timed, lp != nullptr, g.input_format, g.enhance, g.win, g.keys, g.models);
    int k = 0;
    resident_none(c);
    int rc;
    // every argument check comes BEFORE the first enqueue (the callers': check_bound): an error return leaves the streams as they were
    if ((rc = refuse(c, st.refusal)) || (rc = order_begin(c, s))) return rc;
    if (c->test_delay_us) { // RMCV_OPT_TEST_DELAY_US: a stand-in for a kernel that does not finish in time (one shot)
        HIPCHK(c, launch_delay((unsigned long long)c->test_delay_us * 1000ull, s), "k_delay (RMCV_OPT_TEST_DELAY_US)");
        c->test_delay_us = 0;
    }
    if (timed) HIPCHK(c, hipEventRecord(c->ev[k++], s), "event");
    if (st.status_clear) HIPCHK(c, launch_status_clear(g, b, st.status_clear, s), "k_status_clear");
    if (lean) *lean = false;
    if (st.enhance_tables) HIPCHK(c, launch_enhance_tables(g, b, p->lower_bound, s), "k_frame_sums + k_enhance_table");
    if (st.window_origins) HIPCHK(c, launch_window_origins(g, b, s), "k_window_origins");
    if (st.frame_keys) HIPCHK(c, launch_frame_keys(g, b, p->lower_bound, s), "k_frame_keys");
    if (st.binary) {
        c->last_camp = p->camp;
        c->last_lower_bound = p->lower_bound;
        HIPCHK(c, launch_binary(g, b, p->camp, p->lower_bound, p->morph, st.image, plan, s, &c->image, &c->plane_sync), PIXEL_VARIANTS[geom_variant(g)].kernel);
    }
    if (timed) HIPCHK(c, hipEventRecord(c->ev[k++], s), "event");
    if (st.sparse) HIPCHK(c, launch_sparse(g, b, lim, *p, st.sparse_pairs, st.sparse_identity, plan, s, lean), "k_contours (fused)");
    if (st.contours) HIPCHK(c, launch_contours(g, b, lim, s), "k_contours");
    if (timed) HIPCHK(c, hipEventRecord(c->ev[k++], s), "event");
    if (st.match) HIPCHK(c, launch_match(g, b, lim, *p, *lp, 0, b.frames != nullptr, st.match_pairs, s), "k_match");
    if (st.blobs_armours) HIPCHK(c, launch_blobs_armours(g, b, lim, *p, s), "k_fit");
    if (st.blobs) HIPCHK(c, launch_blobs(g, b, lim, *p, s), "k_fit");
    if (timed) HIPCHK(c, hipEventRecord(c->ev[k++], s), "event");
    if (st.armours) HIPCHK(c, launch_armours(g, b, lim, *p, s), "k_armours");
    if (st.classify) HIPCHK(c, launch_classify(g, b, lim, s), "k_classify");
    if (st.pnp) HIPCHK(c, launch_pnp(g, b, lim, s), "k_pnp");
    if (timed) HIPCHK(c, hipEventRecord(c->ev[k++], s), "event");
    c->last_stages = next_last_stages(c->last_stages, stages);
    return order_end(c, s);
}

// everything rmcv_batch_run would refuse for this stage mask, WITHOUT enqueuing anything and before any frames are bound: the pipeline
// splits a batch into several runs on different streams and must not find out at the second one that the batch cannot run (a pixel
// kernel already enqueued, nothing ordered behind it), nor after its binding has enqueued a change of geometry
int rmcv::ctx_check_stages(rmcv_ctx* c, const rmcv_params* p, int stages)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    return refuse(c, stage_refusal(p, stages, c->bufs.svm_w != nullptr, c->bufs.pnp_cfg != nullptr));
}
// ... of the public entry points, which run on what the caller has bound
static int check_bound(rmcv_ctx* c, const rmcv_params* p, int stages)
{
    if (const int rc = ctx_check_stages(c, p, stages)) return rc;
    if ((c->geom.n_frames <= 0 || !c->bufs.frames) && (stages & RMCV_STAGE_BINARY)) return fail(c, RMCV_ERR_BAD_ARG, "no frames bound");
    return RMCV_OK;
}

extern "C" {

int rmcv_batch_upload(rmcv_ctx* c, const uint8_t* frames, int n_frames, int w, int h, int stride, int64_t frame_pitch)
{
    if (!c || !frames) return RMCV_ERR_BAD_ARG;
    int rc = ctx_ready(c); // the buffer about to be overwritten may still be read by a batch in flight
    if (rc) return rc;
    resident_none(c);
    if ((rc = check_layout(c)) || (rc = check_sample_ptr(c, frames))) return rc;
    const UploadLayout dev = upload_layout(ctx_pixel_bytes(c), w, h);
    if ((rc = refuse(c, dev.refusal(stride, frame_pitch))) || (rc = set_geom(c, n_frames, w, h, dev.stride, dev.pitch))) return rc;
    const size_t need = (size_t)dev.pitch * n_frames;
    rc = ensure_own_frames(c, need);
    if (rc) return rc;
    if (dev.same(stride, frame_pitch)) {
        HIPCHK(c, hipMemcpyAsync(c->own_frames, frames, need, hipMemcpyHostToDevice, c->stream), "H2D frames");
    } else {
        for (int f = 0; f < n_frames; f++)
            HIPCHK(c, hipMemcpy2DAsync(c->own_frames + (size_t)f * dev.pitch, dev.stride, frames + (size_t)f * frame_pitch, stride,
                                       (size_t)dev.row_bytes, h, hipMemcpyHostToDevice, c->stream),
                   "H2D frames 2D");
    }
    WAITCHK(c, wait_stream(c, c->stream, "H2D frames"));
    return bound(c, c->own_frames);
}

int rmcv_batch_set_device_frames(rmcv_ctx* c, const void* d_frames, int n_frames, int w, int h, int stride,
                                 int64_t frame_pitch)
{
    if (!c || !d_frames) return RMCV_ERR_BAD_ARG;
    hipSetDevice(c->device);
    resident_none(c);
    int rc = check_sample_ptr(c, d_frames);
    if (rc) return rc;
    rc = set_geom(c, n_frames, w, h, stride, frame_pitch);
    if (rc) return rc;
    return bound(c, d_frames);
}

} // extern "C"
namespace rmcv {
// rmcv_batch_set_device_frames for a pipeline: nothing blocks -- a change of geometry is enqueued on `s`, which the caller has made
// wait for the context's last batch
int ctx_bind_frames(rmcv_ctx* c, const void* d_frames, int n_frames, int w, int h, int stride, int64_t frame_pitch, hipStream_t s,
                    const void* d_origins, int win_w, int win_h, const void* d_camps, const void* d_lower_bounds)
{
    if (!c || !d_frames || !s) return RMCV_ERR_BAD_ARG;
    resident_none(c);
    int rc = check_sample_ptr(c, d_frames);
    if (rc) return rc;
    if (d_camps && (rc = check_frame_camps(c, c->input.format, c->input.enhance))) return rc;
    if (d_origins && win_w <= 0) return fail(c, RMCV_ERR_BAD_ARG, "window size out of range: win_w and win_h must be at least 1");
    rc = set_geom(c, n_frames, w, h, stride, frame_pitch, s, d_origins ? win_w : 0, win_h);
    if (rc || (rc = bound(c, d_frames))) return rc;
    c->bufs.win_req = (const rmcv_point*)d_origins; // (the run computes the effective origins in front of its pixel pass)
    c->geom.keys = d_camps != nullptr;              // (... and the effective keys)
    c->bufs.key_camps = (const int32_t*)d_camps;
    c->bufs.key_lbs = d_camps ? (const int32_t*)d_lower_bounds : nullptr;
    return RMCV_OK;
}
int ctx_check_modes(rmcv_ctx* c, bool keys, bool legacy) { return refuse(c, pixel_refusal(c->input.format, c->input.enhance, false, keys, legacy)); }
// what binding a batch would allocate, now (a pipeline does this for every context of its ring when it is created)
int ctx_prepare_ring(rmcv_ctx* c) { return ensure_mid(c, c->lim.max_frames); }
int ctx_prepare_pixel_sets(rmcv_ctx* c)
{
    if (c->n_sets > 1) return RMCV_OK;
    hipSetDevice(c->device);
    c->blocking_calls++;
    const size_t F = (size_t)c->lim.max_frames;
    const size_t plane = (size_t)(c->lim.max_height + 2) * ((c->lim.max_width + 63) / 64 + 2);
    rmcv_ctx::PixelSet& p = c->parked;
    HIPCHK(c, dalloc(c, &p.binary, F * c->lim.max_width * c->lim.max_height), "hipMalloc (second pixel set)");
    HIPCHK(c, dalloc(c, &p.bits, F * plane), "hipMalloc (second pixel set)");
    HIPCHK(c, dalloc(c, &p.rowmask, F * c->lim.max_height), "hipMalloc (second pixel set)");
    HIPCHK(c, dalloc(c, &p.imgmask, F * c->lim.max_height), "hipMalloc (second pixel set)");
    // (the planes' pads must read 0 for the geometry bound, if one is: the first set's were zeroed when it was bound)
    HIPCHK(c, hipMemset(p.bits, 0, F * plane * 8), "memset planes");
    p.image = IMAGE_STATE_UNKNOWN;
    p.plane_sync = 0;
    c->n_sets = 2;
    return RMCV_OK;
}
int ctx_run(rmcv_ctx* c, const rmcv_params* p, const rmcv_legacy_params* lp, int stages, hipStream_t s, const RunPlan& plan, bool* lean)
{
    const int rc = check_bound(c, p, stages);
    if (rc) return rc;
    return run_stages(c, p, stages, s, false, plan, lp, lean);
}
} // namespace rmcv
extern "C" {

int rmcv_batch_run(rmcv_ctx* c, const rmcv_params* p, int stages, void* hip_stream)
{
    int rc = check_bound(c, p, stages);
    if (rc) return rc;
    hipSetDevice(c->device);
    return run_stages(c, p, stages, hip_stream ? (hipStream_t)hip_stream : c->stream, false, ctx_plan(c));
}

int rmcv_batch_run_legacy(rmcv_ctx* c, const rmcv_params* p, const rmcv_legacy_params* lp, int stages, void* hip_stream)
{
    int rc = check_bound(c, p, stages);
    if (rc) return rc;
    if (!lp) return fail(c, RMCV_ERR_BAD_ARG, "null legacy params");
    // (the context's options as they are set now count beside what the frames were bound with; per-frame camps: run_stages)
    if ((rc = refuse(c, pixel_refusal(c->input.format | c->geom.input_format, c->input.enhance | c->geom.enhance, false, false, true)))) return rc;
    hipSetDevice(c->device);
    return run_stages(c, p, stages, hip_stream ? (hipStream_t)hip_stream : c->stream, false, ctx_plan(c), lp);
}

int rmcv_ctx_set_option(rmcv_ctx* c, int option, int value)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    const OptionRule* rule = option_rule(option); // the values each option takes: bind_plan.h
    if (!rule || !rule->accepts(value)) return fail(c, RMCV_ERR_BAD_ARG, "unknown option or value");
    switch (option) {
    case RMCV_OPT_SPARSE_WAVES: c->sparse_waves = value; break;
    case RMCV_OPT_RUN_AHEAD: c->chain.run_ahead = value; break;
    case RMCV_OPT_FRAME_UPLOAD: c->chain.frame_upload = value, c->chain.copy_up = {}; break;
    case RMCV_OPT_TEST_SLOW_US: c->chain.test_slow_us = value; break;
    case RMCV_OPT_PIXEL_HALO_NT: c->geom.pixel_halo_nt = value; break;
    case OPT_PIXEL_ROWQUAD: c->geom.pixel_rowquad = value; break; // k_binary's row-quad loader even where rows are contiguous (one pipeline, regions alternating)
    case RMCV_OPT_PIXEL_SHAPE: c->pixel_shape = value; break;
    case RMCV_OPT_OVERLOADS: c->geom.overloads = value, resident_none(c); break; // (results run ahead with the other setting are not this setting's)
    case RMCV_OPT_DENSE_DEFER: c->dense_defer = value; break;
    case RMCV_OPT_CONTOUR_TIER: c->geom.contour_tier = value; break;
    case RMCV_OPT_IMAGE_EXPORT: c->chain.image_export = value, c->chain.copy_img = {}; break;
    case RMCV_OPT_WAIT_TIMEOUT_MS: c->wait_timeout_ms = value; break;
    case RMCV_OPT_TEST_DELAY_US: c->test_delay_us = value; break;
    // the input options: frames bound before keep what they were bound with
    case RMCV_OPT_INPUT_FORMAT: c->input.format = value; break;
    case RMCV_OPT_INPUT_SAMPLE_BITS: c->input.sample_bits = value; break;
    case RMCV_OPT_INPUT_VALID_BIT: c->input.valid_bit = value; break;
    case RMCV_OPT_INPUT_ORIENT: c->input.orient = value; break;
    case RMCV_OPT_ENHANCE: c->input.enhance = value; break;
    case RMCV_OPT_PIXEL_GROUPS: c->pixel_groups = value; break;
    }
    return RMCV_OK;
}

int rmcv_ctx_check_guards(rmcv_ctx* c, int32_t* n_damaged)
{
    if (!c || !n_damaged) return RMCV_ERR_BAD_ARG;
    if (const int rc = ctx_ready(c)) return rc;
    std::vector<uint8_t> h;
    int bad = 0;
    c->err[0] = 0;
    for (const auto& g : c->guarded) {
        for (int side = 0; side < 2; side++) {
            const size_t n = side ? g.rear : GUARD;
            const uint8_t* src = side ? g.base + GUARD + g.bytes : g.base;
            h.resize(n);
            HIPCHK(c, hipMemcpy(h.data(), src, n, hipMemcpyDeviceToHost), "D2H guard zone");
            size_t first = n;
            for (size_t i = 0; i < n; i++)
                if (h[i] != GUARD_BYTE) { first = i; break; }
            if (first < n) {
                if (!bad) snprintf(c->err, sizeof(c->err), "guard zone %s %s damaged at byte %zu (buffer of %zu bytes)", side ? "behind" : "in front of", g.name, first, g.bytes);
                bad++;
            }
        }
    }
    *n_damaged = bad;
    return RMCV_OK;
}

int rmcv_batch_sync(rmcv_ctx* c)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    hipSetDevice(c->device);
    // the event sits behind everything this context enqueued, on whichever stream (a stream handle of the caller may be gone by now)
    if (c->external_order && c->ext_done) WAITCHK(c, wait_event(c, c->ext_done, "waiting for the context's last pipelined batch"));
    if (c->order_pending) WAITCHK(c, wait_event(c, c->ev_order, "waiting for the context's last launch"));
    WAITCHK(c, wait_stream(c, c->stream, "waiting for the context's stream"));
    c->timed_out = false;
    return RMCV_OK;
}

int rmcv_batch_run_timed(rmcv_ctx* c, const rmcv_params* p, int stages, void* hip_stream, float stage_ms[5])
{
    int rc = check_bound(c, p, stages);
    if (rc) return rc;
    if (!stage_ms) return fail(c, RMCV_ERR_BAD_ARG, "null stage_ms");
    hipSetDevice(c->device);
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    rc = run_stages(c, p, stages, s, true, ctx_plan(c));
    if (rc) return rc;
    WAITCHK(c, wait_stream(c, s, "waiting for the stream"));
    for (int i = 0; i < 4; i++) HIPCHK(c, hipEventElapsedTime(&stage_ms[i], c->ev[i], c->ev[i + 1]), "elapsed");
    HIPCHK(c, hipEventElapsedTime(&stage_ms[4], c->ev[0], c->ev[4]), "elapsed");
    return RMCV_OK;
}

int rmcv_batch_counts(rmcv_ctx* c, int32_t* n_contours, int32_t* n_points, int32_t* n_blobs, int32_t* n_armours,
                      int32_t* status)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    if (const int rc = ctx_ready(c)) return rc;
    const size_t n = (size_t)c->geom.n_frames * 4;
    if (n_contours) HIPCHK(c, hipMemcpy(n_contours, c->bufs.n_contours, n, hipMemcpyDeviceToHost), "D2H");
    if (n_points) HIPCHK(c, hipMemcpy(n_points, c->bufs.n_points, n, hipMemcpyDeviceToHost), "D2H");
    if (n_blobs) HIPCHK(c, hipMemcpy(n_blobs, c->bufs.n_blobs, n, hipMemcpyDeviceToHost), "D2H");
    if (n_armours) HIPCHK(c, hipMemcpy(n_armours, c->bufs.n_armours, n, hipMemcpyDeviceToHost), "D2H");
    if (status) HIPCHK(c, hipMemcpy(status, c->bufs.status, n, hipMemcpyDeviceToHost), "D2H");
    return RMCV_OK;
}

int rmcv_batch_get_binary(rmcv_ctx* c, int frame, uint8_t* out)
{
    if (!c || !out || frame < 0 || frame >= c->geom.n_frames) return RMCV_ERR_BAD_ARG;
    if (const int rc = ctx_ready(c)) return rc;
    const size_t sz = (size_t)c->geom.w * c->geom.h;
    HIPCHK(c, hipMemcpy(out, c->bufs.binary + (size_t)frame * sz, sz, hipMemcpyDeviceToHost), "D2H binary");
    return RMCV_OK;
}

int rmcv_batch_get_contours(rmcv_ctx* c, int frame, rmcv_point* pts_out, int pts_cap, int32_t* offs_out, int contours_cap,
                            int32_t* n_contours, int32_t* n_points)
{
    if (!c || frame < 0 || frame >= c->geom.n_frames) return RMCV_ERR_BAD_ARG;
    if (const int rc = ctx_ready(c)) return rc;
    hipStream_t s = c->stream;
    // pack this frame only: a one-frame view of the buffers
    Geom g1 = c->geom;
    g1.n_frames = 1;
    Bufs b1 = c->bufs;
    b1.points += (size_t)frame * c->lim.max_points;
    b1.cont_start += (size_t)frame * c->lim.max_contours;
    b1.cont_len += (size_t)frame * c->lim.max_contours;
    b1.n_contours += frame;
    HIPCHK(c, launch_pack_contours(g1, b1, c->lim, c->pack_pts, c->pack_offs, nullptr, s), "k_pack_contours");
    int32_t nc = 0, st = 0;
    HIPCHK(c, hipMemcpyAsync(&nc, c->bufs.n_contours + frame, 4, hipMemcpyDeviceToHost, s), "D2H");
    HIPCHK(c, hipMemcpyAsync(&st, c->bufs.status + frame, 4, hipMemcpyDeviceToHost, s), "D2H");
    WAITCHK(c, wait_stream(c, s, "waiting for the stream"));
    int32_t total = 0;
    HIPCHK(c, hipMemcpy(&total, c->pack_offs + nc, 4, hipMemcpyDeviceToHost), "D2H");
    if (n_contours) *n_contours = nc;
    if (n_points) *n_points = total;
    if (st & (RMCV_FRAME_OVF_CONTOURS | RMCV_FRAME_OVF_POINTS)) return fail(c, RMCV_ERR_CAPACITY, "context limits exceeded (max_contours/max_points)");
    if (nc > contours_cap || total > pts_cap) return fail(c, RMCV_ERR_CAPACITY, "output capacity exceeded");
    if (offs_out) HIPCHK(c, hipMemcpy(offs_out, c->pack_offs, (size_t)(nc + 1) * 4, hipMemcpyDeviceToHost), "D2H offs");
    if (pts_out && total) HIPCHK(c, hipMemcpy(pts_out, c->pack_pts, (size_t)total * sizeof(rmcv_point), hipMemcpyDeviceToHost), "D2H pts");
    return RMCV_OK;
}

int rmcv_batch_get_blobs(rmcv_ctx* c, int frame, rmcv_lightblob* blobs_out, int cap, int32_t* n_blobs, int32_t* blob_src)
{
    if (!c || frame < 0 || frame >= c->geom.n_frames) return RMCV_ERR_BAD_ARG;
    if (const int rc = ctx_ready(c)) return rc;
    int32_t nb = 0, st = 0;
    HIPCHK(c, hipMemcpy(&nb, c->bufs.n_blobs + frame, 4, hipMemcpyDeviceToHost), "D2H");
    HIPCHK(c, hipMemcpy(&st, c->bufs.status + frame, 4, hipMemcpyDeviceToHost), "D2H");
    if (n_blobs) *n_blobs = nb;
    if (st & RMCV_FRAME_OVF_BLOBS) return fail(c, RMCV_ERR_CAPACITY, "context limit exceeded (max_blobs)");
    if (nb > cap) return fail(c, RMCV_ERR_CAPACITY, "output capacity exceeded");
    if (blobs_out && nb)
        HIPCHK(c, hipMemcpy(blobs_out, c->bufs.blobs + (size_t)frame * c->lim.max_blobs, (size_t)nb * sizeof(rmcv_lightblob), hipMemcpyDeviceToHost), "D2H blobs");
    if (blob_src && nb)
        HIPCHK(c, hipMemcpy(blob_src, c->bufs.blob_src + (size_t)frame * c->lim.max_blobs, (size_t)nb * 4, hipMemcpyDeviceToHost), "D2H blob_src");
    return RMCV_OK;
}

int rmcv_batch_get_armours(rmcv_ctx* c, rmcv_armour* armours_out, int cap, int32_t* frame_offs, int32_t* n_total)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    const int nf = c->geom.n_frames;
    std::vector<int32_t> cnt, st(nf);
    int64_t total = 0;
    int rc = ctx_ready(c);
    if (rc || (rc = armour_counts(c, cnt, &total))) return rc;
    HIPCHK(c, hipMemcpy(st.data(), c->bufs.status, (size_t)nf * 4, hipMemcpyDeviceToHost), "D2H");
    int ovf = 0;
    int64_t off = 0;
    for (int f = 0; f < nf; f++) {
        if (frame_offs) frame_offs[f] = (int32_t)off;
        off += cnt[f];
        ovf |= st[f] & (RMCV_FRAME_OVF_CONTOURS | RMCV_FRAME_OVF_POINTS | RMCV_FRAME_OVF_BLOBS | RMCV_FRAME_OVF_ARMOURS);
    }
    if (frame_offs) frame_offs[nf] = (int32_t)total;
    if (n_total) *n_total = (int32_t)total;
    if (ovf) return fail(c, RMCV_ERR_CAPACITY, "context limits exceeded on at least one frame (see status)");
    if (total > cap) return fail(c, RMCV_ERR_CAPACITY, "output capacity exceeded");
    if (armours_out && total) return gather_rows(c, c->bufs.armours, cnt, armours_out, "D2H armours");
    return RMCV_OK;
}

int rmcv_batch_device_views(rmcv_ctx* c, void** d_armours, void** d_counts, int32_t* per_frame_cap, int32_t* n_frames)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    if (d_armours) *d_armours = c->bufs.armours;
    if (d_counts) *d_counts = c->bufs.n_armours;
    if (per_frame_cap) *per_frame_cap = c->lim.max_armours;
    if (n_frames) *n_frames = c->geom.n_frames;
    return RMCV_OK;
}

int rmcv_batch_compact_armours(rmcv_ctx* c, void* d_armours_out, int cap, void* d_frame_offs, void* hip_stream)
{
    if (!c || !d_armours_out || !d_frame_offs || cap < 0) return RMCV_ERR_BAD_ARG;
    hipSetDevice(c->device);
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    int rc = order_begin(c, s);
    if (rc) return rc;
    HIPCHK(c, launch_compact_armours(c->geom, c->bufs, c->lim, (rmcv_armour*)d_armours_out, cap, (int32_t*)d_frame_offs, s), "k_compact_armours");
    return order_end(c, s);
}

// The context's model table := models[0 .. n) (checked by the callers), per-frame selection off.  Entry 0 also goes into
// svm_w / svm_rho / svm_labels, which every single-model consumer reads.
static int load_model_table(rmcv_ctx* c, const rmcv_svm_model* models, int n)
{
    hipSetDevice(c->device);
    Bufs& b = c->bufs;
    if (!b.svm_w) {
        hipError_t e = dalloc(c, &b.svm_w, (size_t)28 * RMCV_SVM_FEATURES);
        if (e == hipSuccess) e = dalloc(c, &b.svm_rho, 28);
        if (e == hipSuccess) e = dalloc(c, &b.svm_labels, 8);
        if (e == hipSuccess) e = dalloc(c, &b.identity, (size_t)c->lim.max_frames * c->lim.max_armours);
        if (e == hipSuccess) e = dalloc(c, &b.icons, (size_t)c->lim.max_frames * c->lim.max_armours * RMCV_SVM_FEATURES);
        if (e == hipSuccess) e = dalloc(c, &b.svm_table, (size_t)RMCV_SVM_MAX_MODELS); // (the model table: behind the others, which stay where they were)
        if (e == hipSuccess) e = dalloc(c, &b.model_eff, (size_t)c->lim.max_frames);
        if (e == hipSuccess) e = dalloc(c, &c->model_own, (size_t)c->lim.max_frames);
        if (e == hipSuccess) e = hipMemset(b.model_eff, 0, (size_t)c->lim.max_frames * 4);
        if (e != hipSuccess) { b.svm_w = nullptr; return fail(c, RMCV_ERR_NOMEM, "svm buffers", e); }
    }
    const rmcv_svm_model& m0 = models[0];
    const int n_df = model_n_df(m0.n_class);
    HIPCHK(c, hipMemcpy(b.svm_w, m0.weights, (size_t)n_df * RMCV_SVM_FEATURES * sizeof(float), hipMemcpyHostToDevice), "H2D svm");
    HIPCHK(c, hipMemcpy(b.svm_rho, m0.rho, (size_t)n_df * sizeof(double), hipMemcpyHostToDevice), "H2D svm");
    HIPCHK(c, hipMemcpy(b.svm_labels, m0.labels, (size_t)m0.n_class * sizeof(int32_t), hipMemcpyHostToDevice), "H2D svm");
    b.svm_classes = m0.n_class;
    std::vector<SvmModelEntry> table((size_t)n);
    for (int m = 0; m < n; m++) {
        model_pack(models[m], &table[(size_t)m]);
        c->model_classes[m] = models[m].n_class;
    }
    HIPCHK(c, hipMemcpy(b.svm_table, table.data(), table.size() * sizeof(SvmModelEntry), hipMemcpyHostToDevice), "H2D model table");
    b.svm_models = n;
    b.model_idx = nullptr;
    c->geom.models = 0;
    return RMCV_OK;
}

// a table of one
int rmcv_svm_load(rmcv_ctx* c, const float* weights, const double* rho, const int32_t* labels, int n_class)
{
    if (!c || !weights || !rho || !labels || n_class < 2 || n_class > 8) return RMCV_ERR_BAD_ARG;
    const rmcv_svm_model one = {weights, rho, labels, n_class, 0};
    return load_model_table(c, &one, 1);
}

int rmcv_svm_load_models(rmcv_ctx* c, const rmcv_svm_model* models, int n_models)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    char msg[200];
    if (const int rc = refuse(c, models_refusal(models, n_models, msg))) return rc; // before any GPU work
    if (const int rc = ctx_ready(c)) return rc; // the table about to be rewritten may still be read by a batch in flight
    return load_model_table(c, models, n_models);
}

/* ---- per-frame models: every frame of the batch bound is classified with its own entry of the model table ---- */

// indices: the host's (validated, copied into the context's own table) or the caller's device memory (borrowed, any value); both null: model 0
static int set_frame_models(rmcv_ctx* c, const int32_t* h_idx, const void* d_idx)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    Geom& g = c->geom;
    Bufs& b = c->bufs;
    if (g.n_frames <= 0 || !b.frames) return fail(c, RMCV_ERR_BAD_ARG, "no frames bound: per-frame models are set after the frames");
    if ((h_idx || d_idx) && !b.svm_table) return fail(c, RMCV_ERR_BAD_ARG, "rmcv_svm_load_models first");
    char msg[200];
    if (h_idx)
        if (const int rc = refuse(c, frame_models_refusal(h_idx, g.n_frames, b.svm_models, msg))) return rc;
    const int rc = set_request_table(c, &b.model_idx, c->model_own, h_idx, d_idx, true, "H2D frame models");
    if (rc == RMCV_OK) g.models = b.model_idx != nullptr;
    return rc;
}

int rmcv_batch_set_frame_models(rmcv_ctx* c, const int32_t* idx) { return set_frame_models(c, idx, nullptr); }

int rmcv_batch_set_device_frame_models(rmcv_ctx* c, const void* d_idx) { return set_frame_models(c, nullptr, d_idx); }

int rmcv_batch_get_frame_models(rmcv_ctx* c, int32_t* out, int cap)
{
    if (!c || cap < 0 || (cap > 0 && !out)) return RMCV_ERR_BAD_ARG;
    if (const int rc = ctx_ready(c)) return rc;
    // selection off: model 0 for every frame
    return get_effective_table(c, out, cap, c->geom.models != 0, c->bufs.model_eff, int32_t{0}, "D2H frame models");
}

int rmcv_batch_get_identities(rmcv_ctx* c, int32_t* identity_out, int cap, int32_t* n_total)
{
    if (!c || !c->bufs.identity) return RMCV_ERR_BAD_ARG;
    std::vector<int32_t> cnt;
    int64_t total = 0;
    int rc = ctx_ready(c);
    if (rc || (rc = armour_counts(c, cnt, &total))) return rc;
    if (n_total) *n_total = (int32_t)total;
    if (total > cap) return fail(c, RMCV_ERR_CAPACITY, "output capacity exceeded");
    return gather_rows(c, c->bufs.identity, cnt, identity_out, "D2H identity");
}

int rmcv_batch_get_icons(rmcv_ctx* c, int frame, uint8_t* icons_out, int cap_armours, int32_t* n_armours)
{
    if (!c || !c->bufs.icons || !icons_out || frame < 0 || frame >= c->geom.n_frames) return RMCV_ERR_BAD_ARG;
    if (const int rc = ctx_ready(c)) return rc;
    int32_t na = 0;
    HIPCHK(c, hipMemcpy(&na, c->bufs.n_armours + frame, 4, hipMemcpyDeviceToHost), "D2H");
    if (n_armours) *n_armours = na;
    if (na > cap_armours) return fail(c, RMCV_ERR_CAPACITY, "output capacity exceeded");
    if (na)
        HIPCHK(c, hipMemcpy(icons_out, c->bufs.icons + (size_t)frame * c->lim.max_armours * RMCV_SVM_FEATURES,
                            (size_t)na * RMCV_SVM_FEATURES, hipMemcpyDeviceToHost), "D2H icons");
    return RMCV_OK;
}

// ---- armour pose ------------------------------------------------------------------------------------------
int rmcv_pnp_load(rmcv_ctx* c, const rmcv_pnp_config* cfg)
{
    if (!c || !cfg) return RMCV_ERR_BAD_ARG;
    hipSetDevice(c->device);
    Bufs& b = c->bufs;
    if (!b.pnp_cfg) {
        hipError_t e = dalloc(c, &b.pnp_cfg, 1);
        if (e == hipSuccess) e = dalloc(c, &b.base2gripper, (size_t)c->lim.max_frames * 16);
        if (e == hipSuccess) e = dalloc(c, &b.att_base2gripper, (size_t)c->lim.max_frames * 16);
        if (e == hipSuccess) e = dalloc(c, &b.poses, (size_t)c->lim.max_frames * c->lim.max_armours * 9);
        if (e == hipSuccess) e = dalloc(c, &b.cam_eff, (size_t)c->lim.max_frames); // (the camera table's indices: behind the others, which stay where they were)
        if (e == hipSuccess) e = dalloc(c, &c->cam_own, (size_t)c->lim.max_frames);
        if (e == hipSuccess) e = hipMemset(b.cam_eff, 0, (size_t)c->lim.max_frames * 4);
        if (e != hipSuccess) { b.pnp_cfg = nullptr; return fail(c, RMCV_ERR_NOMEM, "pnp buffers", e); }
        b.pose_base2gripper = b.base2gripper;
        std::vector<double> eye((size_t)c->lim.max_frames * 16, 0.0);
        for (int f = 0; f < c->lim.max_frames; f++)
            for (int k = 0; k < 4; k++) eye[(size_t)f * 16 + 5 * k] = 1.0;
        HIPCHK(c, hipMemcpy(b.base2gripper, eye.data(), eye.size() * sizeof(double), hipMemcpyHostToDevice), "H2D base2gripper");
    }
    HIPCHK(c, hipMemcpy(b.pnp_cfg, cfg, sizeof(*cfg), hipMemcpyHostToDevice), "H2D pnp config");
    // a table of one, per-frame selection off
    b.pnp_cams = b.pnp_cfg;
    b.n_cameras = 1;
    b.cam_req = nullptr;
    return RMCV_OK;
}

int rmcv_pnp_load_cameras(rmcv_ctx* c, const rmcv_pnp_config* cams, int n_cameras)
{
    if (!c || !cams) return RMCV_ERR_BAD_ARG;
    if (n_cameras < 1 || n_cameras > c->lim.max_frames) return fail(c, RMCV_ERR_BAD_ARG, "rmcv_pnp_load_cameras: n_cameras out of range (1 .. limits.max_frames)");
    int rc = ctx_ready(c); // the table about to be rewritten may still be read by a batch in flight
    if (rc || (rc = rmcv_pnp_load(c, &cams[0]))) return rc; // allocates what the pose stage needs on first use; selection off
    Bufs& b = c->bufs;
    if (!b.cam_table) {
        const hipError_t e = dalloc(c, &b.cam_table, (size_t)c->lim.max_frames);
        if (e != hipSuccess) { b.cam_table = nullptr; return fail(c, RMCV_ERR_NOMEM, "camera table", e); }
    }
    HIPCHK(c, hipMemcpy(b.cam_table, cams, (size_t)n_cameras * sizeof(*cams), hipMemcpyHostToDevice), "H2D camera table");
    b.pnp_cams = b.cam_table;
    b.n_cameras = n_cameras;
    return RMCV_OK;
}

/* ---- per-frame cameras: every frame of the batch bound is located through its own entry of the camera table ---- */

// indices: the host's (validated, copied into the context's own table) or the caller's device memory (borrowed, any value); both null: camera 0
static int set_frame_cameras(rmcv_ctx* c, const int32_t* h_idx, const void* d_idx)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    const Geom& g = c->geom;
    Bufs& b = c->bufs;
    if (g.n_frames <= 0 || !b.frames) return fail(c, RMCV_ERR_BAD_ARG, "no frames bound: per-frame cameras are set after the frames");
    if ((h_idx || d_idx) && !b.pnp_cams) return fail(c, RMCV_ERR_BAD_ARG, "rmcv_pnp_load_cameras first");
    for (int f = 0; h_idx && f < g.n_frames; f++)
        if (frame_camera_eff(h_idx[f], b.n_cameras) != h_idx[f]) {
            char msg[160];
            snprintf(msg, sizeof(msg), "rmcv_batch_set_frame_cameras: frame %d: camera %d is outside the table (0 .. %d)", f, (int)h_idx[f], b.n_cameras - 1);
            return fail(c, RMCV_ERR_BAD_ARG, msg);
        }
    return set_request_table(c, &b.cam_req, c->cam_own, h_idx, d_idx, true, "H2D frame cameras");
}

int rmcv_batch_set_frame_cameras(rmcv_ctx* c, const int32_t* idx) { return set_frame_cameras(c, idx, nullptr); }

int rmcv_batch_set_device_frame_cameras(rmcv_ctx* c, const void* d_idx) { return set_frame_cameras(c, nullptr, d_idx); }

int rmcv_batch_get_frame_cameras(rmcv_ctx* c, int32_t* out, int cap)
{
    if (!c || cap < 0 || (cap > 0 && !out)) return RMCV_ERR_BAD_ARG;
    if (const int rc = ctx_ready(c)) return rc;
    // selection off: camera 0 for every frame
    return get_effective_table(c, out, cap, c->bufs.cam_req != nullptr, c->bufs.cam_eff, int32_t{0}, "D2H frame cameras");
}

int rmcv_batch_set_base2gripper(rmcv_ctx* c, const double* mats, int n_frames)
{
    if (!c || !mats || n_frames < 1) return RMCV_ERR_BAD_ARG;
    if (!c->bufs.pnp_cfg) return fail(c, RMCV_ERR_BAD_ARG, "rmcv_pnp_load first");
    if (n_frames > c->lim.max_frames) return fail(c, RMCV_ERR_CAPACITY, "more frames than the context holds");
    if (const int rc = ctx_ready(c)) return rc;
    HIPCHK(c, hipMemcpy(c->bufs.base2gripper, mats, (size_t)n_frames * 16 * sizeof(double), hipMemcpyHostToDevice), "H2D base2gripper");
    c->bufs.pose_base2gripper = c->bufs.base2gripper;
    return RMCV_OK;
}

int rmcv_batch_get_base2gripper(rmcv_ctx* c, double* mats, int n_frames)
{
    if (!c || !mats || n_frames < 1) return RMCV_ERR_BAD_ARG;
    if (!c->bufs.pnp_cfg) return fail(c, RMCV_ERR_BAD_ARG, "rmcv_pnp_load first");
    if (n_frames > c->lim.max_frames) return fail(c, RMCV_ERR_CAPACITY, "more frames than the context holds");
    if (const int rc = ctx_ready(c)) return rc;
    HIPCHK(c, hipMemcpy(mats, c->bufs.pose_base2gripper, (size_t)n_frames * 16 * sizeof(double), hipMemcpyDeviceToHost), "D2H base2gripper");
    return RMCV_OK;
}

int rmcv_batch_get_poses(rmcv_ctx* c, double* rvecs, double* tvecs, double* positions, int cap, int32_t* n_total)
{
    if (!c || !c->bufs.poses) return RMCV_ERR_BAD_ARG;
    std::vector<int32_t> cnt;
    int64_t total = 0;
    int rc = ctx_ready(c);
    if (rc || (rc = armour_counts(c, cnt, &total))) return rc;
    if (n_total) *n_total = (int32_t)total;
    if (total > cap) return fail(c, RMCV_ERR_CAPACITY, "output capacity exceeded");
    std::vector<PoseRow> rows((size_t)total);
    if ((rc = gather_rows(c, reinterpret_cast<const PoseRow*>(c->bufs.poses), cnt, rows.data(), "D2H poses"))) return rc;
    for (size_t i = 0; i < rows.size(); i++) scatter_pose(rows[i], rvecs, tvecs, positions, i);
    return RMCV_OK;
}

} // extern "C"

extern "C" {

/* ---- exposure-adaptive detection: rm::CalcGamma / rm::AutoEnhance (src/imgproc.cpp:37-48, 77-98) ---- */

int rmcv_ctx_set_enhance_gains(rmcv_ctx* c, float max_gain, float min_gain)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    if (!gains_ok(max_gain, min_gain)) return fail(c, RMCV_ERR_BAD_ARG, "rmcv_ctx_set_enhance_gains: the gains must be finite and differ");
    c->input.max_gain = max_gain; // (like the option: frames bound before keep what they were bound with)
    c->input.min_gain = min_gain;
    return RMCV_OK;
}

int rmcv_ctx_get_enhance(const rmcv_ctx* c, int32_t* on, float* max_gain, float* min_gain)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    if (on) *on = c->input.enhance;
    if (max_gain) *max_gain = c->input.max_gain;
    if (min_gain) *min_gain = c->input.min_gain;
    return RMCV_OK;
}

int rmcv_batch_get_gammas(rmcv_ctx* c, float* gamma_out, int cap)
{
    if (!c || !gamma_out || cap < 0) return RMCV_ERR_BAD_ARG;
    if (const int rc = ctx_ready(c)) return rc;
    // without the option the frames are read as they are: gamma 1 is the identity table
    return get_effective_table(c, gamma_out, cap, c->geom.enhance != 0, c->bufs.enh_gamma, 1.0f, "D2H gammas");
}

/* ---- windowed detection: the frames bound are read through one window each (rm::utils::GetROI -> extract_color(image(roi))) ---- */

// origins: the host's (copied into the context's own table) or the caller's device memory (borrowed); win_w == 0: back to whole frames
static int set_windows(rmcv_ctx* c, const rmcv_point* h_origins, const void* d_origins, int win_w, int win_h)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    Geom& g = c->geom;
    if (g.n_frames <= 0 || !c->bufs.frames) return fail(c, RMCV_ERR_BAD_ARG, "no frames bound: windows are set after the frames");
    hipSetDevice(c->device);
    resident_none(c);
    if (win_w == 0) { // whole frames again
        if (!g.win) return RMCV_OK;
        g.win = 0;
        c->bufs.win_req = nullptr;
        extent_fields(g, g.frame_w, g.frame_h);
        return extent_apply(c, nullptr);
    }
    if (!h_origins && !d_origins) return fail(c, RMCV_ERR_BAD_ARG, "null origins");
    int rc = refuse(c, windows_refusal(c->lim, g.frame_w, g.frame_h, g.input_format, g.enhance, win_w, win_h));
    if (rc) return rc;
    // the tables about to be rewritten may still be read by a batch in flight: whichever origins they are, wait here
    if ((rc = rmcv_batch_sync(c)) || (rc = set_request_table(c, &c->bufs.win_req, c->win_own, h_origins, d_origins, false, "H2D window origins"))) return rc;
    g.win = 1;
    extent_fields(g, win_w, win_h);
    if ((rc = extent_apply(c, nullptr))) return rc;
    // the effective origins now (rmcv_batch_get_windows before the first run reads them); every run with the pixel pass computes them again
    if ((rc = order_begin(c, c->stream))) return rc;
    HIPCHK(c, launch_window_origins(g, c->bufs, c->stream), "k_window_origins");
    return order_end(c, c->stream);
}

int rmcv_batch_set_windows(rmcv_ctx* c, const rmcv_point* origins, int win_w, int win_h)
{
    if (c && win_w != 0 && !origins) return fail(c, RMCV_ERR_BAD_ARG, "null origins");
    return set_windows(c, origins, nullptr, win_w, win_h);
}

int rmcv_batch_set_device_windows(rmcv_ctx* c, const void* d_origins, int win_w, int win_h)
{
    if (c && win_w != 0 && !d_origins) return fail(c, RMCV_ERR_BAD_ARG, "null origins");
    return set_windows(c, nullptr, d_origins, win_w, win_h);
}

int rmcv_batch_get_windows(rmcv_ctx* c, rmcv_point* eff_out, int cap, int32_t* win_w, int32_t* win_h)
{
    if (!c || cap < 0 || (cap > 0 && !eff_out)) return RMCV_ERR_BAD_ARG;
    if (const int rc = ctx_ready(c)) return rc;
    const Geom& g = c->geom;
    if (win_w) *win_w = g.win ? g.w : 0;
    if (win_h) *win_h = g.win ? g.h : 0;
    // whole frames: every origin is (0, 0)
    return get_effective_table(c, eff_out, cap, g.win != 0, c->bufs.win_eff, rmcv_point{0, 0}, "D2H window origins");
}

int rmcv_batch_device_windows(rmcv_ctx* c, void** d_eff, int32_t* win_w, int32_t* win_h)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    if (d_eff) *d_eff = c->geom.win ? c->bufs.win_eff : nullptr;
    if (win_w) *win_w = c->geom.win ? c->geom.w : 0;
    if (win_h) *win_h = c->geom.win ? c->geom.h : 0;
    return RMCV_OK;
}

/* ---- per-frame detection keys: every frame of the batch bound has its own camp and lower bound (serial_package::target per frame) ---- */

// camps / lower bounds: the host's (copied into the context's own tables) or the caller's device memory (borrowed); both camps null: per-run keys
static int set_frame_camps(rmcv_ctx* c, const int32_t* h_camps, const int32_t* h_lbs, const void* d_camps, const void* d_lbs)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    Geom& g = c->geom;
    Bufs& b = c->bufs;
    if (g.n_frames <= 0 || !b.frames) return fail(c, RMCV_ERR_BAD_ARG, "no frames bound: per-frame camps are set after the frames");
    hipSetDevice(c->device);
    resident_none(c);
    const bool on = h_camps || d_camps;
    int rc = on ? check_frame_camps(c, g.input_format, g.enhance) : RMCV_OK;
    if (rc) return rc;
    // (the lower bounds go with the camps: behind the camps' wait, and null with null camps)
    if ((rc = set_request_table(c, &b.key_camps, c->key_own, h_camps, d_camps, true, "H2D frame camps")) ||
        (rc = set_request_table(c, &b.key_lbs, c->key_own + c->lim.max_frames, h_lbs, d_lbs, false, "H2D frame lower bounds")))
        return rc;
    g.keys = on;
    return RMCV_OK;
}

int rmcv_batch_set_frame_camps(rmcv_ctx* c, const int32_t* camps, const int32_t* lower_bounds)
{
    return set_frame_camps(c, camps, camps ? lower_bounds : nullptr, nullptr, nullptr);
}

int rmcv_batch_set_device_frame_camps(rmcv_ctx* c, const void* d_camps, const void* d_lower_bounds)
{
    return set_frame_camps(c, nullptr, nullptr, d_camps, d_camps ? d_lower_bounds : nullptr);
}

int rmcv_batch_get_frame_keys(rmcv_ctx* c, int32_t* keys_out, int cap)
{
    if (!c || cap < 0 || (cap > 0 && !keys_out)) return RMCV_ERR_BAD_ARG;
    if (const int rc = ctx_ready(c)) return rc;
    static_assert(sizeof(FrameKey) == 4 * sizeof(int32_t), "rmcv_batch_get_frame_keys hands the table out as [frame][4] int32");
    // per-run keys: the last run's, for every frame
    return get_effective_table(c, reinterpret_cast<FrameKey*>(keys_out), cap, c->geom.keys != 0, c->bufs.key_eff,
                               frame_key_eff(c->last_camp, c->last_lower_bound), "D2H frame keys");
}

int rmcv_batch_attitude(rmcv_ctx* c, rmcv_tracker* trk, const void* d_packets, void* hip_stream)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    hipSetDevice(c->device);
    return ctx_attitude(c, trk, d_packets, hip_stream ? (hipStream_t)hip_stream : c->stream);
}

int rmcv_batch_track(rmcv_ctx* c, rmcv_tracker* trk, int64_t timestamp, void* hip_stream)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    hipSetDevice(c->device);
    return ctx_track(c, trk, timestamp, c->last_stages, hip_stream ? (hipStream_t)hip_stream : c->stream);
}

} // extern "C"

namespace rmcv {
// the tracker's and the batch context's part of a loop record's launch (the recorder's: recorder_loop_begin)
static void loop_args_fill(LoopArgs& a, const TrackerView& v, const Geom& g, const Bufs& b, int stages, const void* d_packets, int64_t timestamp)
{
    a.n_streams = v.cfg.n_streams, a.trk_cap = v.cfg.track_cap, a.tb = v.b;
    a.aims = v.aims, a.aim_inputs = v.aim_inputs, a.aim_cfgs = v.aim_cfgs;
    a.attitudes = v.attitudes, a.packet_errors = v.packet_errors, a.stream_g2c = v.stream_g2c;
    a.has_aim = v.has_aim, a.has_att = v.has_att, a.has_camps = v.has_camps;
    a.packets = v.att_on ? static_cast<const uint8_t*>(d_packets) : nullptr; // (the batch's own, not a table of the tracker's: recorded where an attitude step read them)
    a.n_armours = b.n_armours, a.frame_status = b.status;
    a.win_eff = g.win ? b.win_eff : nullptr;
    a.key_eff = g.keys ? b.key_eff : nullptr;
    a.cam_eff = b.cam_req && (stages & RMCV_STAGE_POSE) ? b.cam_eff : nullptr;
    a.tcfg = v.cfg, a.aim_cfg = v.aim_cfg, a.att_cfg = v.att_cfg, a.timestamp = timestamp;
}

// one step of the device tracker behind the context's last run (every check before the first enqueue); never synchronises
int ctx_track(rmcv_ctx* c, rmcv_tracker* trk, int64_t timestamp, int stages, hipStream_t s, const LoopTicket* loop)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    if (!trk) return fail(c, RMCV_ERR_BAD_ARG, "null tracker");
    const Geom& g = c->geom;
    const TrackerView& v = tracker_view(trk);
    char msg[200];
    if (const char* no = step_refusal("rmcv_batch_track", true, v, step_batch(c), stages, msg)) return fail(c, RMCV_ERR_BAD_ARG, no);
    int rc;
    if ((rc = order_begin(c, s))) return rc;
    HIPCHK(c, tracker_order_begin(trk, s), "tracker: wait for its previous step");
    HIPCHK(c, launch_track(v.cfg, v.b, c->bufs, c->lim, (stages & RMCV_STAGE_IDENTITY) != 0, (stages & RMCV_STAGE_POSE) != 0,
                           g.win ? c->bufs.win_eff : nullptr, timestamp, s), "k_track");
    if (v.aim_on) HIPCHK(c, launch_aim(v, timestamp, s), "k_aim"); // the aim step reads the lists the step has just left
    // the recorder's loop records: the state the two steps have just left, in front of the tracker's event -- the next batch's
    // attitude step, which rewrites attitudes and aim inputs, waits for that event
    if (loop && loop->rec) {
        LoopArgs a{};
        if ((rc = recorder_loop_begin(*loop, trk, &a, s))) return fail(c, rc, rmcv_recorder_last_error(loop->rec));
        loop_args_fill(a, v, g, c->bufs, stages, loop->d_packets, timestamp);
        HIPCHK(c, launch_loop_record(a, s), "k_loop_record");
        if ((rc = recorder_loop_end(*loop, s))) return fail(c, rc, rmcv_recorder_last_error(loop->rec));
    }
    HIPCHK(c, tracker_order_end(trk, s), "tracker: record the step");
    return order_end(c, s);
}

// the attitude step in front of the bound batch's run (every check before the first enqueue); never synchronises.  It is a step of the
// tracker's like any other: behind the previous one (whose k_aim reads the inputs this one writes), recorded as the newest (the setters'
// and getters' wait covers it).
int ctx_attitude(rmcv_ctx* c, rmcv_tracker* trk, const void* d_packets, hipStream_t s)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    if (!trk) return fail(c, RMCV_ERR_BAD_ARG, "null tracker");
    const TrackerView& v = tracker_view(trk);
    char msg[200];
    if (const char* no = step_refusal("rmcv_batch_attitude", false, v, step_batch(c), 0, msg)) return fail(c, RMCV_ERR_BAD_ARG, no);
    int rc;
    if ((rc = order_begin(c, s))) return rc;
    HIPCHK(c, tracker_order_begin(trk, s), "attitude: wait for the tracker's previous step");
    HIPCHK(c, launch_attitude(v, d_packets, c->bufs.pnp_cfg ? c->bufs.att_base2gripper : nullptr, s), "k_attitude");
    if (c->bufs.pnp_cfg) c->bufs.pose_base2gripper = c->bufs.att_base2gripper;
    HIPCHK(c, tracker_order_end(trk, s), "attitude: record the step");
    return order_end(c, s);
}

// the dataset harvest behind the bound batch's last run: every check before the first enqueue; never synchronises.  An append
// is a step of the dataset's: behind its previous one, whatever stream that ran on, and recorded as its newest.
const char* ctx_harvest_refusal(int device, int n_frames, bool frames_bound, const rmcv_dataset* ds, int n_labels, int flags, int stages, int max_armours)
{
    if (!ds) return "harvest: null dataset";
    const DatasetView& v = dataset_view(ds);
    if (const char* no = harvest_refusal(frames_bound, stages, flags, device, v.device)) return no;
    if (n_frames > n_labels) return "harvest: the batch has more frames than the label table";
    if (v.ring_rows > 0 && n_frames > v.label_cap) return "harvest: the batch has more frames than the dataset has rings (its creating context's max_frames)";
    if (v.ring_rows > 0 && max_armours > v.keep_armours) return "harvest: max_armours is beyond that of the context the dataset with novelty was created on";
    return nullptr;
}
int ctx_harvest(rmcv_ctx* c, rmcv_dataset* ds, const int32_t* h_labels, const void* d_labels, int n_labels, int flags, uint64_t tag, int stages, hipStream_t s)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    if (!h_labels && !d_labels) return fail(c, RMCV_ERR_BAD_ARG, "harvest: null labels");
    const Geom& g = c->geom;
    if (h_labels && ds) { // host labels travel through the dataset's own table, rewritten behind its previous append
        n_labels = dataset_view(ds).label_cap;
        d_labels = dataset_view(ds).labels;
    }
    if (const char* no = ctx_harvest_refusal(c->device, g.n_frames, g.n_frames > 0 && c->bufs.frames, ds, n_labels, flags, stages, c->lim.max_armours)) return fail(c, RMCV_ERR_BAD_ARG, no);
    int rc;
    if ((rc = order_begin(c, s))) return rc;
    HIPCHK(c, dataset_order_begin(ds, s), "harvest: wait for the dataset's previous append");
    if (h_labels) HIPCHK(c, hipMemcpyAsync(const_cast<void*>(d_labels), h_labels, (size_t)g.n_frames * 4, hipMemcpyHostToDevice, s), "H2D harvest labels");
    HIPCHK(c, launch_harvest(g, c->bufs, c->lim, dataset_view(ds), static_cast<const int32_t*>(d_labels), flags, (stages & RMCV_STAGE_IDENTITY) != 0, tag, s),
           "k_harvest_plan + k_harvest_rows"); // (a dataset with novelty on: k_harvest_novel in front)
    HIPCHK(c, dataset_order_end(ds, s), "harvest: record the append");
    return order_end(c, s);
}
} // namespace rmcv
