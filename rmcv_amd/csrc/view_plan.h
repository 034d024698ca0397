// view_plan.h -- the frame-list rule of every entry point that renders or measures CHOSEN frames of the batch bound (the debug and source
// views, their labels, the labeler's sheet, the icon strips, the corner refinement, the chessboard detector), and every refusal of the debug
// view's batch entry points.  Pure functions of plain values, without HIP types, so that a host compiler alone can check them
// (tests/test_view_plan.py); the entry points read the same functions.
#pragma once

#include <stdint.h>

#include "../../include/rmcv_abi.h"

namespace rmcv {

// ---- the frame list: host values; a list there is, 1 <= n <= n_frames, every index inside the batch, none twice ----
enum FrameListFault { FRAME_LIST_OK = 0, FRAME_LIST_NONE, FRAME_LIST_TOO_MANY, FRAME_LIST_OUTSIDE, FRAME_LIST_REPEATED };
// A family's words for the faults, indexed by the fault.  The rule comes in two halves because the views and the strips check their layout
// between them: the count, which reads no entry of the list ...
typedef const char* const FrameListWords[5];
inline FrameListFault frame_count_fault(const int32_t* frames, int n, int n_frames)
{
    if (!frames || n < 1) return FRAME_LIST_NONE;
    if (n > n_frames) return FRAME_LIST_TOO_MANY;
    return FRAME_LIST_OK;
}
// ... and the entries of a list whose count holds, in list order: the first one outside the batch or equal to one in front of it
// (quadratic: n <= max_frames, and a call names a handful of frames or every frame once)
inline FrameListFault frame_index_fault(const int32_t* frames, int n, int n_frames)
{
    for (int k = 0; k < n; k++) {
        if (frames[k] < 0 || frames[k] >= n_frames) return FRAME_LIST_OUTSIDE;
        for (int q = 0; q < k; q++)
            if (frames[q] == frames[k]) return FRAME_LIST_REPEATED;
    }
    return FRAME_LIST_OK;
}
inline FrameListFault frame_list_fault(const int32_t* frames, int n, int n_frames)
{
    const FrameListFault bad = frame_count_fault(frames, n, n_frames);
    return bad ? bad : frame_index_fault(frames, n, n_frames);
}

// ---- the debug view's batch entry points (rmcv_batch_debug_views, rmcv_batch_get_debug_view, rmcv_pipeline_set_views; the labels check
// their views with these too): the message an entry point fails with (RMCV_ERR_BAD_ARG), or null ----
static constexpr FrameListWords DEBUG_VIEW_FRAME_LIST = {nullptr, "debug views: no frames chosen", "debug views: more views than the batch has frames",
                                                         "debug views: a frame index is outside the batch", "debug views: a frame index is repeated"};
// frames: host values; n_frames / stages: the batch the views are of and the stages it has been, or will be, through; need: view_stages_needed(flags)
inline const char* debug_views_refusal(const int32_t* frames, int n, int n_frames, int stages, int need, int vw, int vh, int max_width, int max_height, int flags,
                                       int out_stride, int64_t out_pitch)
{
    if (const FrameListFault bad = frame_count_fault(frames, n, n_frames)) return DEBUG_VIEW_FRAME_LIST[bad];
    if (flags < 0 || flags > RMCV_VIEW_ALL) return "debug views: unknown view flags";
    if (vw < 1 || vh < 1 || vw > max_width || vh > max_height) return "debug views: the view size must be 1 .. max_width x 1 .. max_height";
    if (out_stride < 3 * (int64_t)vw) return "debug views: out_stride < 3 vw";
    if (n > 1 && out_pitch < (int64_t)out_stride * (vh - 1) + 3 * (int64_t)vw) return "debug views: out_pitch < out_stride (vh - 1) + 3 vw";
    if (const FrameListFault bad = frame_index_fault(frames, n, n_frames)) return DEBUG_VIEW_FRAME_LIST[bad];
    if ((stages & need) != need) return "debug views: the batch's run lacked a stage the view flags need";
    return nullptr;
}
static constexpr const char* DEBUG_VIEW_OVERFLOW = "rmcv_batch_get_debug_view: the frame exceeded a context limit (see its status): its tables are not its lists";

} // namespace rmcv
