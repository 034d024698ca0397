// corner_plan.h -- what the corner refinement (k_corner.hip, device_corner.h) decides outside its kernel: the limits, every
// refusal of its entry points, the LDS a workgroup needs and the launch shape.  Pure functions of plain values, without HIP types, so that a
// host compiler alone can check them (tests/test_corner_plan.py); the entry points and launch_corner read the same functions.
#pragma once

#include <stdint.h>

#include "../../include/rmcv_abi.h"
#include "source_view_plan.h"

namespace rmcv {

// ---- the refusals: the message an entry point fails with (RMCV_ERR_BAD_ARG), or null ----
// the rule's parameters, the same for every entry point
inline const char* corner_params_refusal(int win_x, int win_y, int zero_x, int zero_y, int max_iters, double eps)
{
    if (win_x < 1 || win_y < 1 || win_x > RMCV_CORNER_WIN_MAX || win_y > RMCV_CORNER_WIN_MAX) return "corners: win_x and win_y must be 1 .. 15";
    if (!(zero_x == -1 && zero_y == -1) && !(zero_x >= 0 && zero_x < win_x && zero_y >= 0 && zero_y < win_y))
        return "corners: the zero zone must be (-1, -1) or 0 <= zero_x < win_x and 0 <= zero_y < win_y";
    if (max_iters < 1 || max_iters > RMCV_CORNER_ITERS_MAX) return "corners: max_iters must be 1 .. 100";
    if (!(eps >= 0.0) || !(eps <= 1.79769313486231570815e308)) return "corners: eps must be finite and >= 0";
    return nullptr;
}
// the image of the host and the stage-wise form
inline const char* corner_image_refusal(const void* bgr, const void* corners, int w, int h, int stride, int n)
{
    if (!bgr || (n > 0 && !corners)) return "null buffer";
    if (w < 1 || h < 1) return "the image needs w >= 1 and h >= 1";
    if (stride < 3 * (int64_t)w) return "stride < 3 w";
    if (n < 0) return "corners: n < 0";
    return nullptr;
}
static constexpr const char* CORNER_PER_FRAME = "corners: per_frame must be 1 .. 1024";
static constexpr const char* CORNER_BEYOND_LIMITS = "rmcv_corner_subpix: image beyond the context's max_width / max_height";
static constexpr const char* CORNER_NULL_TABLE = "corners: null corner table";
static constexpr const char* CORNER_NOTHING_BOUND = "corners: no frames are bound";
static constexpr const char* CORNER_NEEDS_RUN = "corners: a windowed or enhanced batch is read behind a run with RMCV_STAGE_BINARY (its origins / tables)";
// the batch entry points (rmcv_batch_refine_corners, rmcv_batch_get_refined_corners): the frame-list rule in the source views' words, then the
// table and the parameters.  kind: source_kind of the batch; stages: those of its last run
inline const char* corners_refusal(const int32_t* frames, int n, int n_frames, int kind, int stages, const void* d_corners, int per_frame, int win_x, int win_y,
                                   int zero_x, int zero_y, int max_iters, double eps)
{
    if (const FrameListFault bad = frame_list_fault(frames, n, n_frames)) return SOURCE_VIEW_FRAME_LIST[bad];
    if (!d_corners) return CORNER_NULL_TABLE;
    if (per_frame < 1 || per_frame > RMCV_CORNER_PER_FRAME_MAX) return CORNER_PER_FRAME;
    if (const char* why = corner_params_refusal(win_x, win_y, zero_x, zero_y, max_iters, eps)) return why;
    if ((kind == SOURCE_BGR_WIN || kind == SOURCE_BGR_LUT) && !(stages & RMCV_STAGE_BINARY)) return CORNER_NEEDS_RUN;
    return nullptr;
}

// ---- the launch shape: one wavefront per (chosen frame, corner), four per workgroup ----
static constexpr int CORNER_WAVES = 4;
RMCV_PLAN_FN int corner_win_w(int win_x) { return 2 * win_x + 1; }
RMCV_PLAN_FN int64_t corner_workgroups(int n, int per_frame) { return ((int64_t)n * per_frame + CORNER_WAVES - 1) / CORNER_WAVES; }
// ---- the LDS budget.  Per wavefront: the (win_w + 3) x (win_h + 3) gray bytes (rounded up to a dword) and the (win_w + 2) x (win_h + 2)
// float patch; per workgroup: the win_w x win_h float mask once.  Sized for the largest window, static: 1156 + 4356 bytes per wavefront and
// 3844 for the mask, 25 892 bytes a workgroup -- six workgroups on a CU's 160 KiB.
static constexpr int CORNER_WIN_W_MAX = 2 * RMCV_CORNER_WIN_MAX + 1;
RMCV_PLAN_FN int corner_gray_bytes(int win_w, int win_h) { return ((win_w + 3) * (win_h + 3) + 3) & ~3; }
RMCV_PLAN_FN int corner_patch_bytes(int win_w, int win_h) { return (win_w + 2) * (win_h + 2) * 4; }
RMCV_PLAN_FN int corner_mask_bytes(int win_w, int win_h) { return win_w * win_h * 4; }
RMCV_PLAN_FN int corner_lds_bytes(int win_w, int win_h)
{
    return CORNER_WAVES * (corner_gray_bytes(win_w, win_h) + corner_patch_bytes(win_w, win_h)) + corner_mask_bytes(win_w, win_h);
}
static constexpr int CORNER_GRAY_MAX = ((CORNER_WIN_W_MAX + 3) * (CORNER_WIN_W_MAX + 3) + 3) & ~3;
static constexpr int CORNER_PATCH_MAX = (CORNER_WIN_W_MAX + 2) * (CORNER_WIN_W_MAX + 2);
static constexpr int CORNER_MASK_MAX = CORNER_WIN_W_MAX * CORNER_WIN_W_MAX;

} // namespace rmcv
