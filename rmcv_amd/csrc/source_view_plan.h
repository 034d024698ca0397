// source_view_plan.h -- what the source view (k_view_source.hip) decides outside its kernels: which kind of source a batch is
// (what SRC(f) is computed from), every refusal of its entry points, the source span of an output tile, and whether a tile stages that span in
// LDS or gathers its taps through the caches.  Pure functions of plain values, without HIP types, so that a host compiler alone can check
// them (tests/test_source_view_plan.py); launch_source_view, the kernels and the entry points read the same functions.
#pragma once

#include <stdint.h>

#include "../../include/rmcv_abi.h"
#include "bind_plan.h"
#include "view_plan.h"

namespace rmcv {

// ---- the kind: what SRC(f), the BGR image a frame's results are defined on, is computed from ----
enum SourceKind {
    SOURCE_BGR = 0,    // BGR frames: the frame
    SOURCE_BGR_WIN,    // BGR frames read through windows: the crop at the frame's effective origin (Bufs::win_eff)
    SOURCE_MOSAIC,     // a plain 8-bit Bayer mosaic: D(m) (device_bayer.h: bayer_bgr)
    SOURCE_MOSAIC_RAW, // a mosaic in a sensor layout (16-bit samples, mirror, flip): D(T(r)) (bayer_bgr_raw)
    SOURCE_BGR_LUT,    // RMCV_OPT_ENHANCE: every byte through the frame's own table (Bufs::enh_lut)
    SOURCE_KINDS
};
static constexpr const char* SOURCE_KIND_NAMES[SOURCE_KINDS] = {"k_view_source<BGR>", "k_view_source<BGR_WIN>", "k_view_source<MOSAIC>", "k_view_source<MOSAIC_RAW>",
                                                                "k_view_source<BGR_LUT>"};
// (windows, a Bayer format and RMCV_OPT_ENHANCE exclude each other: pixel_refusal; the order below is pixel_variant's)
constexpr SourceKind source_kind(int input_format, int sample_bytes, int orient, int enhance, int win)
{
    return input_format != RMCV_INPUT_BGR ? ((sample_bytes == 1 && orient == 0) ? SOURCE_MOSAIC : SOURCE_MOSAIC_RAW)
           : enhance                      ? SOURCE_BGR_LUT
           : win                          ? SOURCE_BGR_WIN
                                          : SOURCE_BGR;
}
inline SourceKind source_kind(const Geom& g) { return source_kind(g.input_format, g.sample_bytes, g.orient, g.enhance, g.win); }

// ---- the refusals: the message an entry point fails with (RMCV_ERR_BAD_ARG), or null ----
// the batch entry points (rmcv_batch_source_views, rmcv_batch_get_source_view, rmcv_pipeline_set_source_views): rmcv_batch_debug_views' list.
// frames: host values; n_frames / stages: the batch the views are of and the stages it has been, or will be, through; need: view_stages_needed(flags)
static constexpr FrameListWords SOURCE_VIEW_FRAME_LIST = {nullptr, "source views: no frames chosen", "source views: more views than the batch has frames",
                                                          "source views: a frame index is outside the batch", "source views: a frame index is repeated"};
inline const char* source_views_refusal(const int32_t* frames, int n, int n_frames, int stages, int need, int vw, int vh, int max_width, int max_height, int flags,
                                        int out_stride, int64_t out_pitch)
{
    if (const FrameListFault bad = frame_count_fault(frames, n, n_frames)) return SOURCE_VIEW_FRAME_LIST[bad];
    if (flags < 0 || flags > RMCV_VIEW_ALL) return "source views: unknown view flags";
    if (vw < 1 || vh < 1 || vw > max_width || vh > max_height) return "source views: the view size must be 1 .. max_width x 1 .. max_height";
    if (out_stride < 3 * (int64_t)vw) return "source views: out_stride < 3 vw";
    if (n > 1 && out_pitch < (int64_t)out_stride * (vh - 1) + 3 * (int64_t)vw) return "source views: out_pitch < out_stride (vh - 1) + 3 vw";
    if (const FrameListFault bad = frame_index_fault(frames, n, n_frames)) return SOURCE_VIEW_FRAME_LIST[bad];
    if ((stages & need) != need) return "source views: the batch's run lacked a stage the view flags need";
    return nullptr;
}
static constexpr const char* SOURCE_VIEW_NULL_OUTPUT = "source views: null output";
static constexpr const char* SOURCE_VIEW_NOTHING_BOUND = "source views: no frames are bound";
static constexpr const char* SOURCE_VIEW_OVERFLOW = "rmcv_batch_get_source_view: the frame exceeded a context limit (see its status): its tables are not its lists";
static constexpr const char* SOURCE_VIEW_FEWER_FRAMES = "the batch has fewer frames than the source views name (rmcv_pipeline_set_source_views)";
static constexpr const char* SOURCE_VIEW_FEWER_STAGES = "the batch's stages lack what the source views' flags need (rmcv_pipeline_set_source_views)";
// the image of the stage-wise and the host form (their lists: device_view.h, view_check_lists)
inline const char* source_image_refusal(const void* bgr, const void* out, int w, int h, int stride)
{
    if (!bgr || !out) return "null buffer";
    if (w < 1 || h < 1) return "the image needs w >= 1 and h >= 1";
    if (stride < 3 * (int64_t)w) return "stride < 3 w";
    return nullptr;
}
static constexpr const char* SOURCE_VIEW_BEYOND_LIMITS = "rmcv_source_view: image or view beyond the context's max_width / max_height";

// ---- a tile: 64 x 16 output pixels of one view, a 256-thread workgroup ----
static constexpr int SOURCE_TILE_X = 64, SOURCE_TILE_Y = 16;
// The source span of a tile, from its first and last taps (taps are monotone in the output coordinate): columns c0 .. c1 of rows r0 .. r1
struct SourceSpan {
    int r0, c0, rows, cols;
};
RMCV_PLAN_FN SourceSpan source_span(int first_col_s0, int last_col_s1, int first_row_s0, int last_row_s1)
{
    return {first_row_s0, first_col_s0, last_row_s1 - first_row_s0 + 1, last_col_s1 - first_col_s0 + 1};
}
// A staged span lies in LDS as B, G, R triples, row after row.  A BGR row is copied as the aligned dwords that hold it, so its first byte
// sits 0 .. 3 bytes into its LDS row: bytes between the LDS rows of a span of `cols` pixels (a multiple of 4)
RMCV_PLAN_FN int source_span_pitch(int cols) { return (3 * cols + 6) & ~3; }
// The rule, a byte budget: a tile stages its span when the span's LDS rows fit SOURCE_STAGE_BYTES and -- a plain mosaic, which is demosaiced
// from a staged copy of the span's mosaic bytes plus one ring -- that copy fits SOURCE_RING_BYTES.  Otherwise its taps are gathered.
// 24 KiB hold the span of every view down to about 1 : 2.8 (1280 x 1024 -> 1024 x 768: 82 x 24 pixels, 6 KiB; the exact half: 128 x 32,
// 12 KiB); with the ring, the tile on its way out, the taps and a gamma table that is 39 KiB of static LDS, four workgroups on a CU's
// 160 KiB.  A thumbnail (1 : 8) would need 512 x 128 pixels, of which it reads one in sixteen: it gathers.
static constexpr int SOURCE_STAGE_BYTES = 24576, SOURCE_RING_BYTES = 10240;
RMCV_PLAN_FN bool source_tile_staged(int kind, int rows, int cols)
{
    if ((int64_t)rows * source_span_pitch(cols) > SOURCE_STAGE_BYTES) return false;
    return kind != SOURCE_MOSAIC || (int64_t)(rows + 2) * (cols + 2) <= SOURCE_RING_BYTES;
}

} // namespace rmcv
