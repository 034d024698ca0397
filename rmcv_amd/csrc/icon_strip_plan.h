// icon_strip_plan.h -- what the icon strip and the labeler's sheet (k_icon_strip.hip) decide outside their kernel: every
// refusal of their entry points, the sheet's extent and its strip's capacity.  Pure functions of plain values, without HIP types, so that a
// host compiler alone can check them (tests/test_icon_strip_plan.py); the entry points read the same functions.
#pragma once

#include <stdint.h>

#include "../../include/rmcv_abi.h"
#include "source_view_plan.h"

namespace rmcv {

static constexpr int ICON_SIDE_MAX = RMCV_ICON_SIDE_MAX; // icon_image's largest output side (device_icon_image.h: ICON_IMAGE_MAX)

// ---- rm::affine_correction on the host (rmcv_affine_correction_host) ----
inline const char* affine_host_refusal(const void* bgr, const void* icon, const void* out, int w, int h, int stride, int ow, int oh, int out_stride)
{
    if (!bgr || !icon || !out) return "null buffer";
    if (w < 1 || h < 1) return "the image needs w >= 1 and h >= 1";
    if (stride < 3 * (int64_t)w) return "stride < 3 w";
    if (ow < 1 || oh < 1 || ow > ICON_SIDE_MAX || oh > ICON_SIDE_MAX) return "the output size must be 1 .. 256 x 1 .. 256";
    if (out_stride < 3 * ow) return "out_stride < 3 ow";
    return nullptr;
}

// ---- the strip of one host image (rmcv_icon_strip_host; rmcv_icon_strip adds the context's limits below) ----
inline const char* icon_strip_image_refusal(const void* bgr, const void* out, int w, int h, int stride, const void* armours, int n, int side, int cap,
                                            int out_stride)
{
    if (const char* bad = source_image_refusal(bgr, out, w, h, stride)) return bad;
    if (n < 0 || (n > 0 && !armours)) return "n armours without a list";
    if (side < 1 || side > ICON_SIDE_MAX) return "side must be 1 .. 256";
    if (cap < 1 || cap > RMCV_ICON_STRIP_CAP_MAX) return "cap must be 1 .. RMCV_ICON_STRIP_CAP_MAX";
    if (out_stride < 3 * (int64_t)cap * side) return "out_stride < 3 cap side";
    return nullptr;
}
static constexpr const char* ICON_STRIP_BEYOND_LIMITS = "rmcv_icon_strip: image beyond the context's max_width / max_height, or cap or n beyond its max_armours";

// ---- the batch entry points (rmcv_batch_icon_strips, rmcv_batch_get_icon_strip) ----
// frames: host values; n_frames / stages: the batch the strips are of and the stages it has been, or will be, through
static constexpr FrameListWords ICON_STRIP_FRAME_LIST = {nullptr, "icon strips: no frames chosen", "icon strips: more strips than the batch has frames",
                                                         "icon strips: a frame index is outside the batch", "icon strips: a frame index is repeated"};
inline const char* icon_strips_refusal(const int32_t* frames, int n, int n_frames, int stages, int side, int cap, int max_armours, int out_stride, int64_t out_pitch)
{
    if (const FrameListFault bad = frame_count_fault(frames, n, n_frames)) return ICON_STRIP_FRAME_LIST[bad];
    if (side < 1 || side > ICON_SIDE_MAX) return "icon strips: side must be 1 .. 256";
    if (cap < 1 || cap > max_armours) return "icon strips: cap must be 1 .. max_armours";
    if (out_stride < 3 * (int64_t)cap * side) return "icon strips: out_stride < 3 cap side";
    if (n > 1 && out_pitch < (int64_t)out_stride * (side - 1) + 3 * (int64_t)cap * side) return "icon strips: out_pitch < out_stride (side - 1) + 3 cap side";
    if (const FrameListFault bad = frame_index_fault(frames, n, n_frames)) return ICON_STRIP_FRAME_LIST[bad];
    if (!(stages & RMCV_STAGE_ARMOURS)) return "icon strips: the batch's run lacked RMCV_STAGE_ARMOURS";
    return nullptr;
}
static constexpr const char* ICON_STRIP_NULL_OUTPUT = "icon strips: null output";
static constexpr const char* ICON_STRIP_NOTHING_BOUND = "icon strips: no frames are bound";
static constexpr const char* ICON_STRIP_OVERFLOW = "rmcv_batch_get_icon_strip: the frame exceeded a context limit (see its status): its tables are not its lists";

// ---- the sheet (executable/svm/labeler.cpp:113-119 at view size): 2 vw x (vh + side) pixels ----
inline const char* sheet_size_refusal(int vw, int vh, int side)
{
    if (vw < 1 || vh < 1) return "labeler sheet: the view size must be at least 1 x 1";
    if (side < 1 || side > ICON_SIDE_MAX) return "labeler sheet: side must be 1 .. 256";
    if (side > 2 * (int64_t)vw) return "labeler sheet: side > 2 vw";
    if (vw > (1 << 20) || vh > (1 << 20)) return "labeler sheet: the view size is beyond 2^20";
    return nullptr;
}
// icons the sheet's strip holds: as many as fit its 2 vw pixels, at most `most` (a context's max_armours; the host form: RMCV_ICON_STRIP_CAP_MAX)
inline int sheet_cap(int vw, int side, int most)
{
    const int fit = 2 * vw / side;
    return fit < most ? fit : most;
}
// the batch entry points (rmcv_batch_labeler_sheets, rmcv_batch_get_labeler_sheet, rmcv_pipeline_set_sheets): what either view refuses, the
// strip's stage, and the sheet's own layout.  need: view_stages_needed(flags) | view_stages_needed(0) | RMCV_STAGE_ARMOURS
inline const char* sheets_refusal(const int32_t* frames, int n, int n_frames, int stages, int need, int vw, int vh, int side, int max_width, int max_height,
                                  int flags, int out_stride, int64_t out_pitch)
{
    if (const char* bad = sheet_size_refusal(vw, vh, side)) return bad;
    if (out_stride < 6 * (int64_t)vw) return "labeler sheet: out_stride < 6 vw";
    if (n > 1 && out_pitch < (int64_t)out_stride * (vh + side - 1) + 6 * (int64_t)vw) return "labeler sheet: out_pitch < out_stride (vh + side - 1) + 6 vw";
    // (the panes' own layout, out_stride >= 3 vw and out_pitch >= out_stride (vh - 1) + 3 vw, follows from the two lines above)
    return source_views_refusal(frames, n, n_frames, stages, need, vw, vh, max_width, max_height, flags, out_stride, out_pitch);
}
static constexpr const char* SHEET_NULL_OUTPUT = "labeler sheet: null output";
static constexpr const char* SHEET_OVERFLOW = "rmcv_batch_get_labeler_sheet: the frame exceeded a context limit (see its status): its tables are not its lists";
static constexpr const char* SHEET_FEWER_FRAMES = "the batch has fewer frames than the sheets name (rmcv_pipeline_set_sheets)";
static constexpr const char* SHEET_FEWER_STAGES = "the batch's stages lack what the sheets need (rmcv_pipeline_set_sheets)";

} // namespace rmcv
