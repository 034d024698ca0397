// calib_plan.h -- what the calibration solve (k_calib.hip, device_calib.h) decides outside its kernels: the limits, every
// refusal of its entry points, the LDS and workspace budgets and the launch shapes.  Pure functions of plain values, without HIP types, so
// that a host compiler alone can check them (tests/test_calib_plan.py); the entry points and launch_calib read the same functions.
#pragma once

#include <stdint.h>

#include "../../include/rmcv_abi.h"
#include "pixel_plan.h"

namespace rmcv {

static constexpr int CALIB_POINTS_MIN = 4, CALIB_VIEWS_MIN = 3, CALIB_VIEWS_PER_CAMERA_MAX = RMCV_CALIB_VIEWS_PER_CAMERA_MAX;
static constexpr int CALIB_ITERS_MAX = 100, CALIB_FIX_ALL = 511, CALIB_JACOBI_SWEEPS = 30;

inline rmcv_calib_params calib_default_params() { return {30, 0, 2.2204460492503131e-16}; }

inline bool calib_plan_finite(double v) { return v - v == 0.0; }

// ---- the refusals: the message an entry point fails with (RMCV_ERR_BAD_ARG), or null ----
// the pattern, the extents and the rule's parameters: the same for every entry point
inline const char* calib_params_refusal(int per_frame, int n_views, int cols, int rows, double square, int w, int h, const rmcv_calib_params& p)
{
    if (n_views < 1 || n_views > RMCV_CALIB_VIEWS_MAX) return "calibration: n_views must be 1 .. 4096";
    if (cols < 1 || rows < 1 || (int64_t)cols * rows < CALIB_POINTS_MIN || (int64_t)cols * rows > RMCV_CORNER_PER_FRAME_MAX)
        return "calibration: a cols x rows pattern of 4 .. 1024 corners";
    if (per_frame < cols * rows || per_frame > RMCV_CORNER_PER_FRAME_MAX) return "calibration: per_frame must be cols * rows .. 1024";
    if (!calib_plan_finite(square) || !(square > 0.0)) return "calibration: square must be finite and > 0";
    if (w < 1 || h < 1) return "calibration: the image needs w >= 1 and h >= 1";
    if (p.max_iters < 1 || p.max_iters > CALIB_ITERS_MAX) return "calibration: max_iters must be 1 .. 100";
    if (p.fix_mask < 0 || p.fix_mask > CALIB_FIX_ALL) return "calibration: fix_mask must be 0 .. 511";
    if (!calib_plan_finite(p.eps) || !(p.eps >= 0.0)) return "calibration: eps must be finite and >= 0";
    return nullptr;
}
// a table of guesses (nullable): every entry in use (fx != 0) is finite with positive focal lengths
inline const char* calib_guess_refusal(const rmcv_calib_guess* g, int n)
{
    for (int k = 0; g && k < n; k++) {
        if (g[k].camera_matrix[0] == 0.0) continue;
        for (int i = 0; i < 9; i++)
            if (!calib_plan_finite(g[k].camera_matrix[i])) return "calibration: a guess is not finite";
        for (int i = 0; i < 5; i++)
            if (!calib_plan_finite(g[k].dist[i])) return "calibration: a guess is not finite";
        if (!(g[k].camera_matrix[0] > 0.0) || !(g[k].camera_matrix[4] > 0.0)) return "calibration: a guess needs focal lengths > 0";
    }
    return nullptr;
}
static constexpr const char* CALIB_NULL_TABLE = "calibration: null corner, count, result or view table";
static constexpr const char* CALIB_CAMERAS = "calibration: n_cameras must be 1 .. 64";
// every entry point: the tables, the cameras, then the parameters and the guesses
inline const char* calib_refusal(const void* corners, const void* counts, const void* results, const void* views, int per_frame, int n_views, int n_cameras, int cols,
                                 int rows, double square, int w, int h, const rmcv_calib_params& p, const rmcv_calib_guess* guesses)
{
    if (!corners || !counts || !results || !views) return CALIB_NULL_TABLE;
    if (n_cameras < 1 || n_cameras > RMCV_CALIB_CAMERAS_MAX) return CALIB_CAMERAS;
    if (const char* why = calib_params_refusal(per_frame, n_views, cols, rows, square, w, h, p)) return why;
    return calib_guess_refusal(guesses, n_cameras);
}

// ---- the workspace: one row of doubles per view, in the context's memory (allocated on first use for RMCV_CALIB_VIEWS_MAX views), and one int32 ----
// H (9) | q, t (7) | the trial's q, t (7) | cost, the trial's cost, |db|^2, |q|^2 + |t|^2, the pivot flag | T (45), e (9) | Y (54) | z (6)
static constexpr int CV_H = 0, CV_Q = 9, CV_T = 13, CV_QT = 16, CV_TT = 20, CV_COST = 23, CV_COSTT = 24, CV_DN = 25, CV_PN = 26, CV_BAD = 27, CV_RED = 28, CV_Y = 82,
                     CV_Z = 136, CALIB_VIEW_WS = 144;
static_assert(CV_Z + 6 <= CALIB_VIEW_WS && CV_RED + 54 == CV_Y && CV_Y + 54 == CV_Z, "a view's workspace row");
RMCV_PLAN_FN int64_t calib_ws_doubles(int n_views) { return (int64_t)n_views * CALIB_VIEW_WS; }

// ---- k_calib_homography: one wavefront per view, four per workgroup; LDS per wavefront: A and V of the Jacobi, 2 x 81 doubles ----
// ---- k_calib_solve: one workgroup per camera.  LDS per wavefront: a view's blocks (120 + 15 + 1 sums) and the factor of V (36); per
// workgroup: the camera's state and its list of views.  A pass of the per-view sums holds at most CALIB_PASS_MAX doubles per lane.
static constexpr int CALIB_HOMOGRAPHY_WAVES = 4, CALIB_SOLVE_WAVES = 4, CALIB_WAVE_LDS = 172, CALIB_PASS_MAX = 33;
static_assert(CALIB_WAVE_LDS >= 162 && CALIB_WAVE_LDS >= 136 + 36, "a wavefront's LDS holds the Jacobi's matrices or a view's blocks");
RMCV_PLAN_FN int calib_homography_workgroups(int n_views) { return (n_views + CALIB_HOMOGRAPHY_WAVES - 1) / CALIB_HOMOGRAPHY_WAVES; }
static constexpr int CALIB_CAM_STATE_BYTES = (9 + 9 + 9 + 81 + 9 + 6) * 8 + 5 * 4 + 4;
static constexpr int CALIB_HOMOGRAPHY_LDS_BYTES = CALIB_HOMOGRAPHY_WAVES * CALIB_WAVE_LDS * 8;
static constexpr int CALIB_SOLVE_LDS_BYTES = CALIB_SOLVE_WAVES * CALIB_WAVE_LDS * 8 + CALIB_CAM_STATE_BYTES + CALIB_VIEWS_PER_CAMERA_MAX * 4;
// the guide's budgets: 512 registers per lane (a workgroup of 4 wavefronts: one per SIMD), 160 KiB of LDS per workgroup
static constexpr int CALIB_VGPR_BUDGET = 512, CALIB_LDS_BUDGET = 160 * 1024;
static_assert(2 * CALIB_PASS_MAX + 2 * 32 + 64 <= CALIB_VGPR_BUDGET, "a pass's sums, a point's Jacobian and temporaries fit a lane's registers");
static_assert(CALIB_SOLVE_LDS_BYTES <= CALIB_LDS_BUDGET && CALIB_HOMOGRAPHY_LDS_BYTES <= CALIB_LDS_BUDGET, "LDS");

} // namespace rmcv
