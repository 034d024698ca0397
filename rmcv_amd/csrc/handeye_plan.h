// handeye_plan.h -- what the hand-eye solve (k_handeye.hip, device_handeye.h) decides outside its kernel: the limits, every
// refusal of its entry points, the LDS budget and the launch shape.  Pure functions of plain values, without HIP types, so that a host
// compiler alone can check them (tests/test_handeye_plan.py); the entry points and launch_handeye read the same functions.
#pragma once

#include <stdint.h>

#include "../../include/rmcv_abi.h"
#include "calib_plan.h"

namespace rmcv {

static constexpr int HANDEYE_VIEWS_MIN = 3;

inline rmcv_handeye_params handeye_default_params() { return {0.5, {0, 0}}; }

// ---- the refusals: the message an entry point fails with (RMCV_ERR_BAD_ARG), or null ----
static constexpr const char* HANDEYE_NULL_TABLE = "hand-eye: null view, attitude, result or view-output table";
static constexpr const char* HANDEYE_VIEWS = "hand-eye: n_views must be 1 .. 4096";
static constexpr const char* HANDEYE_CAMERAS = "hand-eye: n_cameras must be 1 .. 64";
static constexpr const char* HANDEYE_MIN_W = "hand-eye: min_w must be finite and in [0, 1)";
// every entry point: the tables (the gripper translations and the camera indices may be null), the extents, then the parameter
inline const char* handeye_refusal(const void* views, const void* attitudes, const void* results, const void* views_out, int n_views, int n_cameras,
                                   const rmcv_handeye_params& p)
{
    if (!views || !attitudes || !results || !views_out) return HANDEYE_NULL_TABLE;
    if (n_views < 1 || n_views > RMCV_CALIB_VIEWS_MAX) return HANDEYE_VIEWS;
    if (n_cameras < 1 || n_cameras > RMCV_CALIB_CAMERAS_MAX) return HANDEYE_CAMERAS;
    if (!calib_plan_finite(p.min_w) || !(p.min_w >= 0.0) || !(p.min_w < 1.0)) return HANDEYE_MIN_W;
    return nullptr;
}

// ---- the pairs of n used views: all i < j in lexicographic order; pair index p counts them from 0 ----
RMCV_PLAN_FN constexpr int handeye_pairs(int n) { return n * (n - 1) / 2; }
// (i, j) -> the pair `step` places further on; i == n - 1 behind the last.  From (0, 1) that is pair `step` itself.
RMCV_PLAN_FN void handeye_pair_advance(int& i, int& j, int step, int n)
{
    j += step;
    while (i < n - 1 && j >= n) {
        i++;
        j = j - n + i + 1;
    }
}

// ---- k_handeye: one workgroup of HANDEYE_THREADS per camera, no workspace.  LDS: a used view's staged row -- B (9), q_g (4), q_c (4),
// t_c (3), t_g (3) -- the list of used views, the cross-wavefront partials of a sum, and the camera's state (HandEyeCam, device_handeye.h)
static constexpr int HANDEYE_WAVES = 4, HANDEYE_THREADS = 64 * HANDEYE_WAVES, HANDEYE_SUMS_MAX = 12;
static constexpr int HV_B = 0, HV_QG = 9, HV_QC = 13, HV_TC = 17, HV_TG = 20, HANDEYE_VIEW_LDS = 23;
static constexpr int HANDEYE_CAM_STATE_BYTES = (16 + 16 + 9 + 3 + 4 + 9 + 3 + 16 + 3 + 4 + 3 + 2) * 8 + 6 * 4;
static constexpr int HANDEYE_LDS_BYTES = CALIB_VIEWS_PER_CAMERA_MAX * (HANDEYE_VIEW_LDS * 8 + 4) + HANDEYE_WAVES * HANDEYE_SUMS_MAX * 8 + HANDEYE_CAM_STATE_BYTES;
// the guide's budgets: 160 KiB of LDS per workgroup; the staged views take 46 KiB of it
static_assert(CALIB_VIEWS_PER_CAMERA_MAX * HANDEYE_VIEW_LDS * 8 == 47104 && HANDEYE_LDS_BYTES <= 64 * 1024 && HANDEYE_LDS_BYTES <= CALIB_LDS_BUDGET, "LDS");
static_assert(handeye_pairs(CALIB_VIEWS_PER_CAMERA_MAX) == 32640, "the cap's pairs");
RMCV_PLAN_FN int handeye_workgroups(int n_cameras) { return n_cameras; }

} // namespace rmcv
