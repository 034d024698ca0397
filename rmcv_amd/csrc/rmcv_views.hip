// rmcv_views.hip -- the entry points of include/rmcv_abi.h that render CHOSEN frames of the batch bound, and their stage-wise twins on the
// caller's own image: the operator's debug view, the source view (4p), the view labels (4q), the icon strip and the labeler's
// sheet (4r).  Those that measure chosen frames, the calibration capture, are rmcv_capture.hip.  Every family has the same three forms:
//   rmcv_batch_<x>s      n chosen frames into the caller's device memory, asynchronous: its checks (a *_plan.h), frame_list_begin, its
//                        launch, order_end
//   rmcv_batch_get_<x>   one frame onto the host: the same checks with a one-entry list, ctx_ready, the batch form into staging, a wait
//   rmcv_<x>             the caller's image and lists through the same kernels in a Scratch block of the call's own
// (frame_list_begin, Scratch and the block's packing: rmcv_ctx.h; the stage-wise rmcv_source_view alone is still rmcv_stagewise.hip's, see
// there).  What a pipeline needs of them are the ctx_* functions of rmcv_internal.h.  No kernel lives here.
#include <string.h>

#include <vector>

#include "rmcv_ctx.h"
#include "device_view.h"

using namespace rmcv;

// a getter of lists refuses a frame that exceeded a context limit: its tables are not its lists (behind ctx_ready)
static int frame_overflow_check(rmcv_ctx* c, int frame, const char* why)
{
    int32_t st = 0;
    HIPCHK(c, hipMemcpy(&st, c->bufs.status + frame, 4, hipMemcpyDeviceToHost), "D2H");
    if (st & (RMCV_FRAME_OVF_CONTOURS | RMCV_FRAME_OVF_POINTS | RMCV_FRAME_OVF_BLOBS | RMCV_FRAME_OVF_ARMOURS)) return fail(c, RMCV_ERR_BAD_ARG, why);
    return RMCV_OK;
}

// The block of a stage-wise view: `head` bytes of image or plane, ONE frame's lists as the caller has them (the negatives as CSR) and the
// counts -- so far uploaded --, then the overlay planes and the view.  (rmcv_debug_view's today; rmcv_source_view's layout is the same.)
namespace {
struct ViewBlock {
    int n_blobs, n_armours, n_neg, n_pts;
    size_t o_blobs, o_arm, o_pts, o_offs, o_cnt, in_bytes, o_ov, o_out, total;
    ViewBlock(size_t head, int nb, int na, const int32_t* neg_offs, int nn, size_t plane, int vw, int vh) : n_blobs(nb), n_armours(na), n_neg(nn), n_pts(nn ? neg_offs[nn] : 0)
    {
        o_blobs = up16(head), o_arm = o_blobs + up16((size_t)n_blobs * sizeof(rmcv_lightblob));
        o_pts = o_arm + up16((size_t)n_armours * sizeof(rmcv_armour)), o_offs = o_pts + up16((size_t)n_pts * sizeof(rmcv_point));
        o_cnt = o_offs + up16((size_t)(n_neg + 1) * 4), in_bytes = o_cnt + 16;
        o_ov = in_bytes, o_out = o_ov + up16(2 * plane * 8), total = o_out + (size_t)3 * vw * vh;
    }
    void pack(uint8_t* host, const rmcv_lightblob* blobs, const rmcv_armour* armours, const rmcv_point* neg_pts, const int32_t* neg_offs) const
    {
        if (n_blobs) memcpy(host + o_blobs, blobs, (size_t)n_blobs * sizeof(rmcv_lightblob));
        if (n_armours) memcpy(host + o_arm, armours, (size_t)n_armours * sizeof(rmcv_armour));
        if (n_pts) memcpy(host + o_pts, neg_pts, (size_t)n_pts * sizeof(rmcv_point));
        if (n_neg) memcpy(host + o_offs, neg_offs, (size_t)(n_neg + 1) * 4);
        const int32_t counts[4] = {n_blobs, n_armours, n_neg, 0};
        memcpy(host + o_cnt, counts, sizeof(counts));
    }
    // the job of the one view on the block at `d` (bits: the caller's)
    ViewJob job(uint8_t* d, int w, int h, int prow, size_t plane, int vw, int vh, int flags) const
    {
        const int32_t* cnt = reinterpret_cast<const int32_t*>(d + o_cnt);
        ViewJob j{};
        j.w = w; j.h = h; j.prow = prow; j.plane_pitch = (int64_t)plane;
        j.overlay = reinterpret_cast<uint64_t*>(d + o_ov); j.frames = nullptr;
        j.n = 1; j.vw = vw; j.vh = vh; j.flags = flags;
        j.out = d + o_out; j.out_stride = 3 * vw; j.out_pitch = (int64_t)3 * vw * vh;
        j.lists = ViewLists{reinterpret_cast<const rmcv_lightblob*>(d + o_blobs), cnt, reinterpret_cast<const rmcv_armour*>(d + o_arm), cnt + 1,
                            reinterpret_cast<const rmcv_point*>(d + o_pts), nullptr, nullptr, cnt + 3, nullptr, cnt + 2,
                            reinterpret_cast<const int32_t*>(d + o_offs), n_blobs, n_armours, n_pts, n_neg, 1};
        return j;
    }
};
} // namespace

/* ---- the operator's debug view (k_view.hip) and the source view (k_view_source.hip; 4p): the same entry points over
 * SRC(f), the planes are the same ---- */

namespace rmcv {

int ctx_view_check(rmcv_ctx* c, const int32_t* frames, int n, int n_frames, int stages, int vw, int vh, int flags, int out_stride, int64_t out_pitch)
{
    return refuse(c, debug_views_refusal(frames, n, n_frames, stages, view_stages_needed(flags), vw, vh, c->lim.max_width, c->lim.max_height, flags, out_stride, out_pitch));
}

int ctx_source_view_check(rmcv_ctx* c, const int32_t* frames, int n, int n_frames, int stages, int vw, int vh, int flags, int out_stride, int64_t out_pitch)
{
    return refuse(c, source_views_refusal(frames, n, n_frames, stages, view_stages_needed(flags & RMCV_VIEW_ALL), vw, vh, c->lim.max_width, c->lim.max_height, flags,
                                          out_stride, out_pitch));
}

int ctx_view_prepare(rmcv_ctx* c, int n)
{
    if (n <= c->view_cap) return RMCV_OK;
    // a handful of views, or every frame: at most two allocations in a context's life
    const int cap = n <= 8 && c->lim.max_frames > 8 ? 8 : c->lim.max_frames;
    const size_t plane = (size_t)(c->lim.max_height + 2) * ((c->lim.max_width + 63) / 64 + 2);
    uint64_t* p = nullptr;
    const hipError_t e = dalloc_named(c, &p, (size_t)cap * 2 * plane, "view_overlay");
    if (e != hipSuccess) return hip_failed(c, "allocating the debug views' planes", e);
    c->view_overlay = p;
    c->view_cap = cap;
    return RMCV_OK;
}

// the job of n views of the batch bound, the frame list already on the device
static ViewJob view_job(rmcv_ctx* c, const int32_t* d_frames, int n, int vw, int vh, int flags, void* d_out, int out_stride, int64_t out_pitch)
{
    const Geom& g = c->geom;
    const Bufs& b = c->bufs;
    ViewJob j{};
    j.w = g.w; j.h = g.h; j.prow = g.prow; j.plane_pitch = g.plane_pitch;
    j.bits = b.bits; j.overlay = c->view_overlay; j.frames = d_frames;
    j.n = n; j.vw = vw; j.vh = vh; j.flags = flags;
    j.out = (uint8_t*)d_out; j.out_stride = out_stride; j.out_pitch = out_pitch;
    j.lists = ViewLists{b.blobs, b.n_blobs, b.armours, b.n_armours, b.points, b.cont_start, b.cont_len, b.n_contours, b.neg_idx, b.n_neg, nullptr,
                        c->lim.max_blobs, c->lim.max_armours, c->lim.max_points, c->lim.max_contours, 0};
    return j;
}

int ctx_view_enqueue(rmcv_ctx* c, const int32_t* d_frames, int n, int vw, int vh, int flags, void* d_out, int out_stride, int64_t out_pitch, hipStream_t s)
{
    HIPCHK(c, launch_view(view_job(c, d_frames, n, vw, vh, flags, d_out, out_stride, out_pitch), s), "k_view_overlay + k_view_resize");
    return RMCV_OK;
}

int ctx_source_view_enqueue(rmcv_ctx* c, const int32_t* d_frames, int n, int vw, int vh, int flags, void* d_out, int out_stride, int64_t out_pitch, hipStream_t s)
{
    if (!c->bufs.frames) return fail(c, RMCV_ERR_BAD_ARG, SOURCE_VIEW_NOTHING_BOUND);
    const SourceViewJob sj{view_job(c, d_frames, n, vw, vh, flags, d_out, out_stride, out_pitch), frame_source_of(c->geom, c->bufs)};
    HIPCHK(c, launch_source_view(sj, s), "k_view_overlay + k_view_source");
    return RMCV_OK;
}

} // namespace rmcv

// rmcv_batch_debug_views / rmcv_batch_source_views behind their checks
typedef int (*ViewBatch)(rmcv_ctx*, const int32_t*, int, int, int, int, void*, int, int64_t, hipStream_t);
static int view_batch(rmcv_ctx* c, const int32_t* frames, int n, int vw, int vh, int flags, void* d_out, int out_stride, int64_t out_pitch, hipStream_t s)
{
    int rc = ctx_view_prepare(c, n);
    if (rc || (rc = frame_list_begin(c, frames, n, s, "H2D view frames"))) return rc;
    if ((rc = ctx_view_enqueue(c, c->frame_list, n, vw, vh, flags, d_out, out_stride, out_pitch, s))) return rc;
    return order_end(c, s);
}
static int source_view_batch(rmcv_ctx* c, const int32_t* frames, int n, int vw, int vh, int flags, void* d_out, int out_stride, int64_t out_pitch, hipStream_t s)
{
    if (!c->bufs.frames) return fail(c, RMCV_ERR_BAD_ARG, SOURCE_VIEW_NOTHING_BOUND); // (before anything is enqueued)
    int rc = ctx_view_prepare(c, n);
    if (rc || (rc = frame_list_begin(c, frames, n, s, "H2D view frames"))) return rc;
    if ((rc = ctx_source_view_enqueue(c, c->frame_list, n, vw, vh, flags, d_out, out_stride, out_pitch, s))) return rc;
    return order_end(c, s);
}

// rmcv_batch_get_debug_view / rmcv_batch_get_source_view behind their checks: one view through the context's staging onto the host
static int view_get(rmcv_ctx* c, ViewBatch batch, const char* overflow, const char* no_staging, const char* kernel, int frame, int vw, int vh, int flags,
                    uint8_t* out, int out_stride)
{
    int rc = ctx_ready(c);
    if (rc || (rc = frame_overflow_check(c, frame, overflow))) return rc;
    if ((rc = LAZY_TABLE(c, &c->view_out, (size_t)3 * c->lim.max_width * c->lim.max_height, no_staging))) return rc;
    const int32_t one = frame;
    if ((rc = batch(c, &one, 1, vw, vh, flags, c->view_out, 3 * vw, (int64_t)3 * vw * vh, c->stream))) return rc;
    WAITCHK(c, wait_stream(c, c->stream, kernel));
    HIPCHK(c, hipMemcpy2D(out, out_stride, c->view_out, (size_t)3 * vw, (size_t)3 * vw, vh, hipMemcpyDeviceToHost), "D2H view");
    return RMCV_OK;
}

extern "C" {

int rmcv_batch_debug_views(rmcv_ctx* c, const int32_t* frames, int n, int vw, int vh, int flags, void* d_out, int out_stride, int64_t out_pitch,
                           void* hip_stream)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    if (!d_out) return fail(c, RMCV_ERR_BAD_ARG, "rmcv_batch_debug_views: null output");
    if (const int rc = ctx_view_check(c, frames, n, c->geom.n_frames, c->last_stages, vw, vh, flags, out_stride, out_pitch)) return rc;
    hipSetDevice(c->device);
    return view_batch(c, frames, n, vw, vh, flags, d_out, out_stride, out_pitch, stream_of(c, hip_stream));
}

int rmcv_batch_get_debug_view(rmcv_ctx* c, int frame, int vw, int vh, int flags, uint8_t* out, int out_stride)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    if (!out) return fail(c, RMCV_ERR_BAD_ARG, "rmcv_batch_get_debug_view: null output");
    const int32_t one = frame;
    if (const int rc = ctx_view_check(c, &one, 1, c->geom.n_frames, c->last_stages, vw, vh, flags, out_stride, 0)) return rc;
    return view_get(c, view_batch, DEBUG_VIEW_OVERFLOW, "allocating the debug view's staging", "k_view_resize", frame, vw, vh, flags, out, out_stride);
}

int rmcv_batch_source_views(rmcv_ctx* c, const int32_t* frames, int n, int vw, int vh, int flags, void* d_out, int out_stride, int64_t out_pitch,
                            void* hip_stream)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    if (!d_out) return fail(c, RMCV_ERR_BAD_ARG, SOURCE_VIEW_NULL_OUTPUT);
    if (const int rc = ctx_source_view_check(c, frames, n, c->geom.n_frames, c->last_stages, vw, vh, flags, out_stride, out_pitch)) return rc;
    hipSetDevice(c->device);
    return source_view_batch(c, frames, n, vw, vh, flags, d_out, out_stride, out_pitch, stream_of(c, hip_stream));
}

int rmcv_batch_get_source_view(rmcv_ctx* c, int frame, int vw, int vh, int flags, uint8_t* out, int out_stride)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    if (!out) return fail(c, RMCV_ERR_BAD_ARG, SOURCE_VIEW_NULL_OUTPUT);
    const int32_t one = frame;
    if (const int rc = ctx_source_view_check(c, &one, 1, c->geom.n_frames, c->last_stages, vw, vh, flags, out_stride, 0)) return rc;
    return view_get(c, source_view_batch, SOURCE_VIEW_OVERFLOW, "allocating the source view's staging", "k_view_source", frame, vw, vh, flags, out, out_stride);
}

int rmcv_debug_view(rmcv_ctx* c, const uint8_t* binary, int w, int h, int stride, const rmcv_lightblob* blobs, int n_blobs, const rmcv_point* neg_pts,
                    const int32_t* neg_offs, int n_neg, const rmcv_armour* armours, int n_armours, int flags, int vw, int vh, uint8_t* out,
                    int out_stride)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    if (!binary || !out) return fail(c, RMCV_ERR_BAD_ARG, "rmcv_debug_view: null buffer");
    if (const int rc = refuse_as(c, "rmcv_debug_view", view_check_lists(w, h, stride, blobs, n_blobs, neg_pts, neg_offs, n_neg, armours, n_armours, flags, vw, vh, out_stride)))
        return rc;
    if (w > c->lim.max_width || h > c->lim.max_height || vw > c->lim.max_width || vh > c->lim.max_height)
        return fail(c, RMCV_ERR_BAD_ARG, "rmcv_debug_view: image or view beyond the context's max_width / max_height");
    if (const int rc = ctx_ready(c)) return rc;
    // one host block, one upload: the binary image as a bit plane, the lists
    const int prow = (w + 63) / 64 + 2;
    const size_t plane = (size_t)(h + 2) * prow;
    const ViewBlock B(plane * 8, n_blobs, n_armours, neg_offs, n_neg, plane, vw, vh);
    std::vector<uint8_t> host(B.in_bytes, 0);
    uint64_t* hp = reinterpret_cast<uint64_t*>(host.data());
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++)
            if (binary[(size_t)y * stride + x]) hp[(size_t)(y + 1) * prow + (x >> 6) + 1] |= 1ull << (x & 63);
    B.pack(host.data(), blobs, armours, neg_pts, neg_offs);
    auto launch = [&](uint8_t* d) {
        ViewJob j = B.job(d, w, h, prow, plane, vw, vh, flags);
        j.bits = reinterpret_cast<const uint64_t*>(d);
        return launch_view(j, c->stream);
    };
    return scratch_call(c, B.total, host.data(), B.in_bytes, launch, "k_view_overlay + k_view_resize", "k_view_resize", "rmcv_debug_view", [&](const uint8_t* d) {
        return hipMemcpy2D(out, out_stride, d + B.o_out, (size_t)3 * vw, (size_t)3 * vw, vh, hipMemcpyDeviceToHost);
    });
}

} // extern "C"

/* ---- the icon strip and the labeler's sheet (k_icon_strip.hip); the host-side entry points: k_icon_strip.hip ---- */

// rmcv_batch_icon_strips behind its checks
static int icon_strip_batch(rmcv_ctx* c, const int32_t* frames, int n, int side, int cap, void* d_out, int out_stride, int64_t out_pitch, int32_t* d_counts,
                            hipStream_t s)
{
    if (const int rc = frame_list_begin(c, frames, n, s, "H2D view frames")) return rc;
    HIPCHK(c, launch_icon_strip(c->geom, c->bufs, c->lim, c->frame_list, n, side, cap, cap * side, (uint8_t*)d_out, out_stride, out_pitch, d_counts, s), "k_icon_strip");
    return order_end(c, s);
}

static int icon_strip_check(rmcv_ctx* c, const int32_t* frames, int n, int side, int cap, int out_stride, int64_t out_pitch)
{
    if (!c->bufs.frames) return fail(c, RMCV_ERR_BAD_ARG, ICON_STRIP_NOTHING_BOUND);
    return refuse(c, icon_strips_refusal(frames, n, c->geom.n_frames, c->last_stages, side, cap, c->lim.max_armours, out_stride, out_pitch));
}

namespace rmcv {

int ctx_sheet_check(rmcv_ctx* c, const int32_t* frames, int n, int n_frames, int stages, int vw, int vh, int side, int flags, int out_stride, int64_t out_pitch)
{
    const int need = view_stages_needed(flags & RMCV_VIEW_ALL) | view_stages_needed(0) | RMCV_STAGE_ARMOURS;
    return refuse(c, sheets_refusal(frames, n, n_frames, stages, need, vw, vh, side, c->lim.max_width, c->lim.max_height, flags, out_stride, out_pitch));
}

// left pane, right pane, strip: the two view launches aimed at their sub-rectangles of the sheet, then k_icon_strip over its last rows
int ctx_sheet_enqueue(rmcv_ctx* c, const int32_t* d_frames, int n, int vw, int vh, int side, int flags, void* d_out, int out_stride, int64_t out_pitch, hipStream_t s)
{
    uint8_t* sheet = (uint8_t*)d_out;
    int rc = ctx_source_view_enqueue(c, d_frames, n, vw, vh, flags, sheet, out_stride, out_pitch, s);
    if (rc) return rc;
    if ((rc = ctx_view_enqueue(c, d_frames, n, vw, vh, 0, sheet + 3 * (size_t)vw, out_stride, out_pitch, s))) return rc;
    HIPCHK(c, launch_icon_strip(c->geom, c->bufs, c->lim, d_frames, n, side, sheet_cap(vw, side, c->lim.max_armours), 2 * vw, sheet + (size_t)vh * out_stride,
                                out_stride, out_pitch, nullptr, s),
           "k_icon_strip");
    return RMCV_OK;
}

} // namespace rmcv

// rmcv_batch_labeler_sheets behind its checks
static int sheet_batch(rmcv_ctx* c, const int32_t* frames, int n, int vw, int vh, int side, int flags, void* d_out, int out_stride, int64_t out_pitch, hipStream_t s)
{
    if (!c->bufs.frames) return fail(c, RMCV_ERR_BAD_ARG, SOURCE_VIEW_NOTHING_BOUND); // (before anything is enqueued)
    int rc = ctx_view_prepare(c, n);
    if (rc || (rc = frame_list_begin(c, frames, n, s, "H2D view frames"))) return rc;
    if ((rc = ctx_sheet_enqueue(c, c->frame_list, n, vw, vh, side, flags, d_out, out_stride, out_pitch, s))) return rc;
    return order_end(c, s);
}

extern "C" {

int rmcv_batch_icon_strips(rmcv_ctx* c, const int32_t* frames, int n, int side, int cap, void* d_out, int out_stride, int64_t out_pitch, int32_t* d_counts,
                           void* hip_stream)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    if (!d_out) return fail(c, RMCV_ERR_BAD_ARG, ICON_STRIP_NULL_OUTPUT);
    if (const int rc = icon_strip_check(c, frames, n, side, cap, out_stride, out_pitch)) return rc;
    hipSetDevice(c->device);
    return icon_strip_batch(c, frames, n, side, cap, d_out, out_stride, out_pitch, d_counts, stream_of(c, hip_stream));
}

int rmcv_batch_get_icon_strip(rmcv_ctx* c, int frame, int side, int cap, uint8_t* out, int out_stride, int32_t* n_icons)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    if (!out) return fail(c, RMCV_ERR_BAD_ARG, ICON_STRIP_NULL_OUTPUT);
    const int32_t one = frame;
    int rc = icon_strip_check(c, &one, 1, side, cap, out_stride, 0);
    if (rc || (rc = ctx_ready(c)) || (rc = frame_overflow_check(c, frame, ICON_STRIP_OVERFLOW))) return rc;
    // (staging of its own for this one call, 16 bytes in front for the count)
    const size_t row = (size_t)3 * cap * side;
    Scratch d;
    hipError_t e = d.alloc(16 + row * side);
    if (e != hipSuccess) return hip_failed(c, "allocating the icon strip's staging", e);
    if ((rc = icon_strip_batch(c, &one, 1, side, cap, d.d + 16, (int)row, (int64_t)row * side, reinterpret_cast<int32_t*>(d.d), c->stream))) return rc;
    WAITCHK(c, d.waited(wait_stream(c, c->stream, "k_icon_strip")));
    int32_t na = 0;
    e = hipMemcpy2D(out, out_stride, d.d + 16, row, row, side, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(&na, d.d, 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(c, RMCV_ERR_HIP, "D2H icon strip", e);
    if (n_icons) *n_icons = na;
    return RMCV_OK;
}

int rmcv_batch_labeler_sheets(rmcv_ctx* c, const int32_t* frames, int n, int vw, int vh, int side, int flags, void* d_out, int out_stride, int64_t out_pitch,
                              void* hip_stream)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    if (!d_out) return fail(c, RMCV_ERR_BAD_ARG, SHEET_NULL_OUTPUT);
    if (const int rc = ctx_sheet_check(c, frames, n, c->geom.n_frames, c->last_stages, vw, vh, side, flags, out_stride, out_pitch)) return rc;
    hipSetDevice(c->device);
    return sheet_batch(c, frames, n, vw, vh, side, flags, d_out, out_stride, out_pitch, stream_of(c, hip_stream));
}

int rmcv_batch_get_labeler_sheet(rmcv_ctx* c, int frame, int vw, int vh, int side, int flags, uint8_t* out, int out_stride)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    if (!out) return fail(c, RMCV_ERR_BAD_ARG, SHEET_NULL_OUTPUT);
    const int32_t one = frame;
    int rc = ctx_sheet_check(c, &one, 1, c->geom.n_frames, c->last_stages, vw, vh, side, flags, out_stride, 0);
    if (rc || (rc = ctx_ready(c)) || (rc = frame_overflow_check(c, frame, SHEET_OVERFLOW))) return rc;
    const size_t row = (size_t)6 * vw, rows = (size_t)vh + side;
    Scratch d;
    hipError_t e = d.alloc(row * rows);
    if (e != hipSuccess) return hip_failed(c, "allocating the sheet's staging", e);
    if ((rc = sheet_batch(c, &one, 1, vw, vh, side, flags, d.d, (int)row, (int64_t)(row * rows), c->stream))) return rc;
    WAITCHK(c, d.waited(wait_stream(c, c->stream, "k_icon_strip")));
    e = hipMemcpy2D(out, out_stride, d.d, row, row, rows, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(c, RMCV_ERR_HIP, "D2H sheet", e);
    return RMCV_OK;
}

int rmcv_icon_strip(rmcv_ctx* c, const uint8_t* bgr, int w, int h, int stride, const rmcv_armour* armours, int n, int side, int cap, uint8_t* out,
                    int out_stride)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    if (const int rc = refuse_as(c, "rmcv_icon_strip", icon_strip_image_refusal(bgr, out, w, h, stride, armours, n, side, cap, out_stride))) return rc;
    if (w > c->lim.max_width || h > c->lim.max_height || cap > c->lim.max_armours || n > c->lim.max_armours) return fail(c, RMCV_ERR_BAD_ARG, ICON_STRIP_BEYOND_LIMITS);
    if (const int rc = ctx_ready(c)) return rc;
    // one host block, one upload: the image, the armours, their count; the strip behind them
    const int dstride = bgr_row_bytes(w);
    const size_t o_arm = (size_t)dstride * h, o_cnt = o_arm + up16((size_t)n * sizeof(rmcv_armour)), in_bytes = o_cnt + 16;
    const size_t row = (size_t)3 * cap * side, o_out = in_bytes, total = o_out + row * side;
    std::vector<uint8_t> host(in_bytes, 0);
    pack_bgr(host.data(), bgr, w, h, stride);
    if (n) memcpy(&host[o_arm], armours, (size_t)n * sizeof(rmcv_armour));
    const int32_t count = n;
    memcpy(&host[o_cnt], &count, 4);
    auto launch = [&](uint8_t* d) {
        IconStripJob S{};
        S.frames = d, S.frame_pitch = (int64_t)dstride * h, S.stride = dstride, S.w = w, S.h = h, S.max_armours = n > 0 ? n : 1;
        S.armours = reinterpret_cast<const rmcv_armour*>(d + o_arm), S.n_armours = reinterpret_cast<const int32_t*>(d + o_cnt);
        S.n = 1, S.side = side, S.cap = cap, S.strip_w = cap * side, S.out = d + o_out, S.out_stride = (int)row, S.out_pitch = (int64_t)row * side;
        return launch_icon_strip(S, c->stream);
    };
    return scratch_call(c, total, host.data(), in_bytes, launch, "k_icon_strip", "k_icon_strip", "rmcv_icon_strip",
                        [&](const uint8_t* d) { return hipMemcpy2D(out, out_stride, d + o_out, row, row, side, hipMemcpyDeviceToHost); });
}

} // extern "C"

/* ---- view labels (k_view_text.hip); the host-side entry points and the stage-wise one: rmcv_labels.hip ---- */

namespace rmcv {

int ctx_label_check(rmcv_ctx* c, const char* who, rmcv_tracker* trk, const int32_t* frames, int n, int n_frames, int stages, int vw, int vh, int scale,
                    int out_stride, int64_t out_pitch)
{
    char msg[200];
    // (the views are finished ones: what their renderer refused of the list and the layout is refused here, whatever stages it needed)
    if (const int rc = ctx_view_check(c, frames, n, n_frames, ~0, vw, vh, 0, out_stride, out_pitch)) return rc;
    if (scale < 1 || scale > 8) {
        snprintf(msg, sizeof(msg), "%s: scale %d is outside 1 .. 8", who, scale);
        return fail(c, RMCV_ERR_BAD_ARG, msg);
    }
    if (trk) {
        if (const char* no = step_refusal(who, true, tracker_view(trk), step_batch(c), stages, msg)) return fail(c, RMCV_ERR_BAD_ARG, no);
    } else if (!(stages & RMCV_STAGE_ARMOURS)) {
        snprintf(msg, sizeof(msg), "%s: the last run had no RMCV_STAGE_ARMOURS: nothing to label", who);
        return fail(c, RMCV_ERR_BAD_ARG, msg);
    }
    return RMCV_OK;
}

int ctx_label_enqueue(rmcv_ctx* c, rmcv_tracker* trk, int what, int stages, const int32_t* d_frames, int n, int vw, int vh, int scale, void* d_views,
                      int out_stride, int64_t out_pitch, hipStream_t s)
{
    const Geom& g = c->geom;
    const Bufs& b = c->bufs;
    LabelJob j{};
    j.n = n, j.vw = vw, j.vh = vh, j.w = g.w, j.h = g.h, j.scale = scale, j.n_frames = g.n_frames;
    j.out = static_cast<uint8_t*>(d_views), j.out_stride = out_stride, j.out_pitch = out_pitch, j.frames = d_frames;
    if (what & RMCV_LABEL_ARMOURS) { // identity and position as the tracker's observations take them: from the run's stages, else -1 and zeros
        j.armours = b.armours, j.n_armours = b.n_armours, j.max_armours = c->lim.max_armours;
        j.identity = (stages & RMCV_STAGE_IDENTITY) ? b.identity : nullptr;
        j.positions = (stages & RMCV_STAGE_POSE) && b.poses ? b.poses + 6 : nullptr;
        j.pos_stride = 9;
    }
    const bool tracks = (what & RMCV_LABEL_TRACKS) && trk;
    if (tracks) {
        const TrackerView& v = tracker_view(trk);
        j.tracks = v.b.tracks, j.side = v.b.side, j.sel = v.b.sel, j.n_tracking = v.b.n_tracking;
        j.n_streams = v.cfg.n_streams, j.track_cap = v.cfg.track_cap;
        j.win_eff = g.win ? b.win_eff : nullptr;
        HIPCHK(c, tracker_order_begin(trk, s), "view labels: wait for the tracker's step");
    }
    HIPCHK(c, launch_view_text(j, s), "k_view_text");
    if (tracks) HIPCHK(c, tracker_order_end(trk, s), "view labels: record the read of the tracker's lists");
    return RMCV_OK;
}

} // namespace rmcv

// rmcv_batch_view_labels / rmcv_batch_view_tracks behind their checks
static int label_batch(rmcv_ctx* c, rmcv_tracker* trk, const int32_t* frames, int n, int vw, int vh, int scale, void* d_views, int stride, int64_t pitch, hipStream_t s)
{
    int rc = frame_list_begin(c, frames, n, s, "H2D view frames");
    if (rc) return rc;
    if ((rc = ctx_label_enqueue(c, trk, trk ? RMCV_LABEL_TRACKS : RMCV_LABEL_ARMOURS, c->last_stages, c->frame_list, n, vw, vh, scale, d_views, stride, pitch, s))) return rc;
    return order_end(c, s);
}

extern "C" {

int rmcv_batch_view_labels(rmcv_ctx* c, const int32_t* frames, int n, int vw, int vh, int scale, void* d_views, int stride, int64_t pitch, void* hip_stream)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    if (!d_views) return fail(c, RMCV_ERR_BAD_ARG, "rmcv_batch_view_labels: null views");
    if (const int rc = ctx_label_check(c, "rmcv_batch_view_labels", nullptr, frames, n, c->geom.n_frames, c->last_stages, vw, vh, scale, stride, pitch)) return rc;
    hipSetDevice(c->device);
    return label_batch(c, nullptr, frames, n, vw, vh, scale, d_views, stride, pitch, stream_of(c, hip_stream));
}

int rmcv_batch_view_tracks(rmcv_ctx* c, rmcv_tracker* trk, const int32_t* frames, int n, int vw, int vh, int scale, void* d_views, int stride, int64_t pitch,
                           void* hip_stream)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    if (!trk) return fail(c, RMCV_ERR_BAD_ARG, "rmcv_batch_view_tracks: null tracker");
    if (!d_views) return fail(c, RMCV_ERR_BAD_ARG, "rmcv_batch_view_tracks: null views");
    if (const int rc = ctx_label_check(c, "rmcv_batch_view_tracks", trk, frames, n, c->geom.n_frames, c->last_stages, vw, vh, scale, stride, pitch)) return rc;
    hipSetDevice(c->device);
    return label_batch(c, trk, frames, n, vw, vh, scale, d_views, stride, pitch, stream_of(c, hip_stream));
}

} // extern "C"
