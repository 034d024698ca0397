// frame_plan.h -- the host-side rules of the per-frame chain (rmcv_extract_color -> rmcv_filter_lightblobs -> rmcv_filter_armours,
// rmcv_frame.hip): which path a frame's two large copies take, the windows of the results that go home speculatively, the chunk bounds
// of the byte image's export and the parameter sets the chain runs ahead with.  Pure functions of plain values, without HIP types, so
// that a host compiler alone can check them (tests/test_frame_plan.py).
#pragma once

#include "pixel_plan.h"

namespace rmcv {

// ---- the adaptive copy path ----
// The runtime's pageable copies pin and unpin the caller's pages on every call; in some conditions (measured: for tens of seconds
// after a large GPU process has exited -- the driver's test suite in front of bench.py, every round) each such copy costs 120-250 us
// more, and the per-frame chain reads 0.28 ms (one of them slow) or 0.40 (both) instead of 0.18.  The library measures both copies on
// every frame with a `binary_out` and moves to its own paths -- pinned staging up, export kernel down -- after COPY_SLOW_FRAMES slow
// frames in a row, for COPY_HOLD_FRAMES frames, then tries the runtime's again.
// A path is 0 for the runtime's pageable copy, otherwise the library's own (upload: 1 pinned staging / 2 registered; image: 1 export).
struct CopyPathState {
    int slow; // consecutive slow frames on the runtime's path
    int hold; // frames left on the library's own path
};
struct CopyDirection {
    int adaptive;         // the option value that lets the library choose (any other value IS the path)
    double bytes_per_us;  // } a frame is slow when the copy took longer than bytes / bytes_per_us + slack_us
    double slack_us;      // }
};
// The constants were tuned at 1280x1024 on one box and have not been measured elsewhere.
static constexpr CopyDirection COPY_UPLOAD = {3, 45e3, 100.0}; // RMCV_OPT_FRAME_UPLOAD = 3; 45 GB/s + the pixel kernel + the waits' slack
static constexpr CopyDirection COPY_IMAGE = {2, 40e3, 60.0};   // RMCV_OPT_IMAGE_EXPORT = 2
static constexpr int COPY_SLOW_FRAMES = 3, COPY_HOLD_FRAMES = 512;

// the path the next frame takes (the image's only if mapped pinned memory is to be had: otherwise it takes 0 whatever this says)
RMCV_PLAN_FN int copy_path(const CopyDirection& d, int option, const CopyPathState& st)
{
    return option == d.adaptive ? (st.hold > 0 ? 1 : 0) : option;
}
// The state behind a frame with a `binary_out` (other frames leave it alone) that took `path`; us: what the copy cost as measured,
// RMCV_OPT_TEST_SLOW_US included; bytes: what it moved.  Setting the direction's option starts again from {0, 0}.
RMCV_PLAN_FN CopyPathState copy_path_step(const CopyDirection& d, int option, CopyPathState st, int path, double us, double bytes)
{
    if (path == 0) {
        st.slow = us > bytes / d.bytes_per_us + d.slack_us ? st.slow + 1 : 0;
        if (option == d.adaptive && st.slow >= COPY_SLOW_FRAMES) { st.hold = COPY_HOLD_FRAMES; st.slow = 0; }
    } else if (st.hold > 0) st.hold--;
    return st;
}

// ---- the result windows ----
// A header word + fixed windows of the results are copied back speculatively (a frame has ~1000 contour points, ~10 blobs, ~3 armours);
// what does not fit a window is fetched by a second copy.  Enqueue, export, finish and the second copies all read ONE FrameWindows.
static constexpr int SF_OFFS_WIN = 1024, SF_PTS_WIN = 8192, SF_BLOB_WIN = 64, SF_NEG_WIN = 1024, SF_ARM_WIN = 32;
struct FrameWindows {
    int offs, pts, blobs, neg, armours; // elements (offs: contours -- the CSR has one offset more)
};
RMCV_PLAN_FN FrameWindows frame_windows(int max_contours, int max_points, int max_blobs, int max_armours)
{
    return {SF_OFFS_WIN < max_contours ? SF_OFFS_WIN : max_contours, SF_PTS_WIN < max_points ? SF_PTS_WIN : max_points,
            SF_BLOB_WIN < max_blobs ? SF_BLOB_WIN : max_blobs, SF_NEG_WIN < max_contours ? SF_NEG_WIN : max_contours,
            SF_ARM_WIN < max_armours ? SF_ARM_WIN : max_armours};
}

// ---- the chunks of the byte image's export (k_image_export and the host loop that takes them) ----
constexpr int IMG_CHUNKS = 16, IMG_CHUNKS_DEFAULT = 8, IMG_GROUPS = 16; // IMG_CHUNKS: the flags' capacity.  Measured (1280x1024, from C, ms per chain; the runtime's copy: 0.186): 8 chunks x 16 workgroups 0.190, 4 x 8 0.189, 16 x 16 0.193, 8 x 8 0.195, 4 x 16 0.199, 8 x 32 0.200, 2 x 16 0.201, 1 x 16 0.207 (a fence per chunk and workgroup costs microseconds; all chunks at once leave the CPU copy nothing to overlap)
struct ImageChunk { long long lo, hi; };
// bytes [lo, hi) of chunk g of n_chunks: equal parts rounded up to 16 bytes (image_chunk_bytes), the last ones shorter or empty
RMCV_PLAN_FN long long image_chunk_bytes(long long bytes, int n_chunks) { return ((bytes + n_chunks - 1) / n_chunks + 15) & ~15ll; }
RMCV_PLAN_FN ImageChunk image_chunk_at(long long bytes, long long per, int g)
{
    const long long lo = (long long)g * per < bytes ? (long long)g * per : bytes;
    return {lo, lo + per < bytes ? lo + per : bytes};
}
RMCV_PLAN_FN ImageChunk image_chunk(long long bytes, int n_chunks, int g) { return image_chunk_at(bytes, image_chunk_bytes(bytes, n_chunks), g); }

// ---- the parameter sets ----
// what rmcv_filter_lightblobs / rmcv_filter_armours were asked for last, and the chain runs ahead with (FrameChain::last_lb, ::last_ar)
struct LbParams { float tilt_max, ratio_lo, ratio_hi; double area_lo, area_hi; int enemy; };
struct ArParams { float angle_diff_max, shear_max, length_ratio_max; int enemy; };
// the sets into `p`, which holds rmcv_default_params; an absent set leaves the defaults (both present: the chain has checked that they
// name the same enemy)
inline void chain_params(rmcv_params* p, const LbParams* lb, const ArParams* ar)
{
    if (ar) {
        p->angle_diff_max = ar->angle_diff_max;
        p->shear_max = ar->shear_max;
        p->length_ratio_max = ar->length_ratio_max;
        p->camp = ar->enemy;
    }
    if (lb) {
        p->tilt_max = lb->tilt_max;
        p->ratio_lo = lb->ratio_lo;
        p->ratio_hi = lb->ratio_hi;
        p->area_lo = lb->area_lo;
        p->area_hi = lb->area_hi;
        p->camp = lb->enemy;
    }
}

} // namespace rmcv
