// rmcv_handeye.hip -- the hand-eye solve behind the ABI: the host-side functions, which need no context and no device
// (rmcv_handeye_defaults, rmcv_calibrate_hand_eye_host, rmcv_handeye_to_pnp_config, rmcv_handeye_to_attitude_config), the fleet call on
// device tables (rmcv_calibrate_hand_eyes) and the stage-wise rmcv_calibrate_hand_eye, the same kernel on host tables in a Scratch block of
// its own.  The rule is device_handeye.h, every refusal handeye_plan.h, the kernel k_handeye.hip; the fleet call takes its place in the
// context's order as every batch call does (rmcv_ctx.h: order_begin / order_end).  No kernel lives here.
#include <string.h>

#include <vector>

#include "device_handeye.h"
#include "rmcv_ctx.h"

using namespace rmcv;

static HandEyeJob handeye_job(const void* views, const void* attitudes, const void* gripper_t, int n_views, const void* view_camera, int n_cameras,
                              const rmcv_handeye_params& p, void* results, void* views_out)
{
    HandEyeJob j{};
    j.views = (const rmcv_calib_view*)views; j.att = (const rmcv_attitude*)attitudes; j.gripper_t = (const double*)gripper_t;
    j.view_camera = (const int32_t*)view_camera; j.results = (rmcv_handeye_result*)results; j.views_out = (rmcv_handeye_view*)views_out;
    j.min_w = p.min_w; j.n_views = n_views; j.n_cameras = n_cameras;
    return j;
}

// the matrix of a result the converters accept, or null
static const double* handeye_matrix(const rmcv_handeye_result* r, int allow_rotation_only)
{
    if (!r) return nullptr;
    if (r->status & RMCV_HANDEYE_OK) return r->cam2gripper;
    return ((r->status & RMCV_HANDEYE_T_UNOBSERVABLE) && allow_rotation_only) ? r->cam2gripper : nullptr;
}

extern "C" {

void rmcv_handeye_defaults(rmcv_handeye_params* p)
{
    if (p) *p = handeye_default_params();
}

int rmcv_calibrate_hand_eye_host(const rmcv_calib_view* views, const rmcv_attitude* attitudes, const double* gripper_t, int n_views,
                                 const rmcv_handeye_params* params, rmcv_handeye_result* result, rmcv_handeye_view* views_out)
{
    const rmcv_handeye_params prm = params ? *params : handeye_default_params();
    if (handeye_refusal(views, attitudes, result, views_out, n_views, 1, prm)) return RMCV_ERR_BAD_ARG;
    std::vector<double> stage((size_t)CALIB_VIEWS_PER_CAMERA_MAX * HANDEYE_VIEW_LDS);
    handeye_solve_host(handeye_job(views, attitudes, gripper_t, n_views, nullptr, 1, prm, result, views_out), stage.data());
    return RMCV_OK;
}

int rmcv_handeye_to_pnp_config(const rmcv_handeye_result* r, rmcv_pnp_config* cfg, int allow_rotation_only)
{
    const double* m = handeye_matrix(r, allow_rotation_only);
    if (!m || !cfg) return RMCV_ERR_BAD_ARG;
    memcpy(cfg->gripper2camera, m, sizeof(cfg->gripper2camera));
    return RMCV_OK;
}

int rmcv_handeye_to_attitude_config(const rmcv_handeye_result* r, rmcv_attitude_config* cfg, int allow_rotation_only)
{
    const double* m = handeye_matrix(r, allow_rotation_only);
    if (!m || !cfg) return RMCV_ERR_BAD_ARG;
    memcpy(cfg->gripper2camera, m, sizeof(cfg->gripper2camera));
    return RMCV_OK;
}

int rmcv_calibrate_hand_eyes(rmcv_ctx* c, const void* d_views, const void* d_attitudes, const void* d_gripper_t, int n_views, const void* d_view_camera,
                             int n_cameras, const rmcv_handeye_params* params, void* d_results, void* d_views_out, void* hip_stream)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    const rmcv_handeye_params prm = params ? *params : handeye_default_params();
    int rc = refuse(c, handeye_refusal(d_views, d_attitudes, d_results, d_views_out, n_views, n_cameras, prm));
    if (rc) return rc;
    hipSetDevice(c->device);
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    if ((rc = order_begin(c, s))) return rc;
    HIPCHK(c, launch_handeye(handeye_job(d_views, d_attitudes, d_gripper_t, n_views, d_view_camera, n_cameras, prm, d_results, d_views_out), s), "k_handeye");
    return order_end(c, s);
}

int rmcv_calibrate_hand_eye(rmcv_ctx* c, const rmcv_calib_view* views, const rmcv_attitude* attitudes, const double* gripper_t, int n_views,
                            const rmcv_handeye_params* params, rmcv_handeye_result* result, rmcv_handeye_view* views_out)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    const rmcv_handeye_params prm = params ? *params : handeye_default_params();
    int rc = refuse_as(c, "rmcv_calibrate_hand_eye", handeye_refusal(views, attitudes, result, views_out, n_views, 1, prm));
    if (rc || (rc = ctx_ready(c))) return rc;
    // (a stage-wise helper: buffers of its own) -- the views | the attitudes | the gripper translations | the result | the view rows
    const size_t b_views = (size_t)n_views * sizeof(rmcv_calib_view), b_att = (size_t)n_views * sizeof(rmcv_attitude), b_gt = (size_t)n_views * 24;
    const size_t b_out = (size_t)n_views * sizeof(rmcv_handeye_view);
    const size_t o_att = b_views, o_gt = o_att + b_att, o_res = o_gt + b_gt, o_out = o_res + sizeof(rmcv_handeye_result), total = o_out + b_out;
    Scratch blk;
    hipError_t e = blk.alloc(total);
    uint8_t* const d = blk.d;
    if (e == hipSuccess) e = hipMemcpyAsync(d, views, b_views, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_att, attitudes, b_att, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && gripper_t) e = hipMemcpyAsync(d + o_gt, gripper_t, b_gt, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_res, result, sizeof(rmcv_handeye_result), hipMemcpyHostToDevice, c->stream);   // (rows not written keep the caller's bytes)
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_out, views_out, b_out, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = launch_handeye(handeye_job(d, d + o_att, gripper_t ? d + o_gt : nullptr, n_views, nullptr, 1, prm, d + o_res, d + o_out), c->stream);
    c->last_what = "k_handeye";
    int rcw = 0;
    if (e == hipSuccess) rcw = blk.waited(wait_stream(c, c->stream, "k_handeye"));
    if (e == hipSuccess && rcw == 0) e = hipMemcpy(result, d + o_res, sizeof(rmcv_handeye_result), hipMemcpyDeviceToHost);
    if (e == hipSuccess && rcw == 0) e = hipMemcpy(views_out, d + o_out, b_out, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(c, e == hipErrorOutOfMemory ? RMCV_ERR_NOMEM : RMCV_ERR_HIP, "rmcv_calibrate_hand_eye", e);
    return rcw;
}

} // extern "C"
