// rmcv_calib.hip -- the calibration solve behind the ABI: the host-side functions, which need no context and no device
// (rmcv_calib_defaults, rmcv_calibrate_camera_host, rmcv_calib_to_pnp_config), the fleet call on device tables (rmcv_calibrate_cameras) and
// the stage-wise rmcv_calibrate_camera, the same kernels on host tables in a Scratch block of its own.  The rule is device_calib.h, every
// refusal calib_plan.h, the kernels k_calib.hip; the fleet call takes its place in the context's order as every batch call does (rmcv_ctx.h:
// order_begin / order_end).  No kernel lives here.
#include <string.h>

#include <vector>

#include "device_calib.h"
#include "rmcv_ctx.h"

using namespace rmcv;

static CalibJob calib_job(const void* corners, int per_frame, const void* counts, int n_views, const void* view_camera, int n_cameras, int cols, int rows, double square,
                          int w, int h, const rmcv_calib_params& p)
{
    CalibJob j{};
    j.corners = (const float*)corners; j.per_frame = per_frame; j.counts = (const int32_t*)counts; j.n_views = n_views;
    j.view_camera = (const int32_t*)view_camera; j.n_cameras = n_cameras;
    j.cols = cols; j.rows = rows; j.square = square; j.w = w; j.h = h;
    j.max_iters = p.max_iters; j.fix_mask = p.fix_mask; j.eps = p.eps;
    return j;
}

extern "C" {

void rmcv_calib_defaults(rmcv_calib_params* p)
{
    if (p) *p = calib_default_params();
}

int rmcv_calibrate_camera_host(const float* corners, int per_frame, const int32_t* counts, int n_views, int cols, int rows, double square, int w, int h,
                               const rmcv_calib_params* params, const rmcv_calib_guess* guess, rmcv_calib_result* result, rmcv_calib_view* views_out)
{
    const rmcv_calib_params prm = params ? *params : calib_default_params();
    if (calib_refusal(corners, counts, result, views_out, per_frame, n_views, 1, cols, rows, square, w, h, prm, guess)) return RMCV_ERR_BAD_ARG;
    std::vector<double> ws((size_t)calib_ws_doubles(n_views));
    std::vector<int32_t> vcam((size_t)n_views);
    CalibJob j = calib_job(corners, per_frame, counts, n_views, nullptr, 1, cols, rows, square, w, h, prm);
    j.guesses = guess; j.ws = ws.data(); j.vcam = vcam.data(); j.results = result; j.views = views_out;
    calib_solve_host(j);
    return RMCV_OK;
}

int rmcv_calib_to_pnp_config(const rmcv_calib_result* r, rmcv_pnp_config* cfg)
{
    if (!r || !cfg || !(r->status & (RMCV_CALIB_CONVERGED | RMCV_CALIB_MAX_ITERS | RMCV_CALIB_STALLED))) return RMCV_ERR_BAD_ARG;
    memcpy(cfg->camera_matrix, r->camera_matrix, sizeof(cfg->camera_matrix));
    memcpy(cfg->dist, r->dist, sizeof(cfg->dist));
    return RMCV_OK;
}

int rmcv_calibrate_cameras(rmcv_ctx* c, const void* d_corners, int per_frame, const void* d_counts, int n_views, const void* d_view_camera, int n_cameras, int cols,
                           int rows, double square, int w, int h, const rmcv_calib_params* params, const rmcv_calib_guess* guesses, void* d_results, void* d_views,
                           void* hip_stream)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    const rmcv_calib_params prm = params ? *params : calib_default_params();
    int rc = refuse(c, calib_refusal(d_corners, d_counts, d_results, d_views, per_frame, n_views, n_cameras, cols, rows, square, w, h, prm, guesses));
    if (rc) return rc;
    hipSetDevice(c->device);
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    hipError_t e = hipSuccess;
    if (!c->calib_ws) e = dalloc(c, &c->calib_ws, (size_t)calib_ws_doubles(RMCV_CALIB_VIEWS_MAX));
    if (e == hipSuccess && !c->calib_vcam) e = dalloc(c, &c->calib_vcam, (size_t)RMCV_CALIB_VIEWS_MAX);
    if (e == hipSuccess && !c->calib_guesses) e = dalloc(c, &c->calib_guesses, (size_t)RMCV_CALIB_CAMERAS_MAX);
    if (e != hipSuccess) return fail(c, e == hipErrorOutOfMemory ? RMCV_ERR_NOMEM : RMCV_ERR_HIP, "allocating the calibration solve's workspace", e);
    if ((rc = order_begin(c, s))) return rc;
    CalibJob j = calib_job(d_corners, per_frame, d_counts, n_views, d_view_camera, n_cameras, cols, rows, square, w, h, prm);
    if (guesses) {
        HIPCHK(c, hipMemcpyAsync(c->calib_guesses, guesses, (size_t)n_cameras * sizeof(rmcv_calib_guess), hipMemcpyHostToDevice, s), "H2D calibration guesses");
        j.guesses = c->calib_guesses;
    }
    j.ws = c->calib_ws; j.vcam = c->calib_vcam; j.results = (rmcv_calib_result*)d_results; j.views = (rmcv_calib_view*)d_views;
    HIPCHK(c, launch_calib(j, s), "k_calib");
    return order_end(c, s);
}

int rmcv_calibrate_camera(rmcv_ctx* c, const float* corners, int per_frame, const int32_t* counts, int n_views, int cols, int rows, double square, int w, int h,
                          const rmcv_calib_params* params, const rmcv_calib_guess* guess, rmcv_calib_result* result, rmcv_calib_view* views_out)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    const rmcv_calib_params prm = params ? *params : calib_default_params();
    int rc = refuse_as(c, "rmcv_calibrate_camera", calib_refusal(corners, counts, result, views_out, per_frame, n_views, 1, cols, rows, square, w, h, prm, guess));
    if (rc || (rc = ctx_ready(c))) return rc;
    // (a stage-wise helper: buffers of its own) -- the workspace | the result | the views | the guess | the corners | the counts | the flags
    const size_t b_ws = (size_t)calib_ws_doubles(n_views) * 8, b_views = (size_t)n_views * sizeof(rmcv_calib_view), b_cor = (size_t)n_views * per_frame * 8;
    const size_t o_res = b_ws, o_views = o_res + sizeof(rmcv_calib_result), o_guess = o_views + b_views, o_cor = o_guess + sizeof(rmcv_calib_guess);
    const size_t o_cnt = o_cor + b_cor, o_vcam = o_cnt + (size_t)n_views * 4, total = o_vcam + (size_t)n_views * 4;
    Scratch blk;
    hipError_t e = blk.alloc(total);
    uint8_t* const d = blk.d;
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_res, result, sizeof(rmcv_calib_result), hipMemcpyHostToDevice, c->stream);   // (rows not written keep the caller's bytes)
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_views, views_out, b_views, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && guess) e = hipMemcpyAsync(d + o_guess, guess, sizeof(rmcv_calib_guess), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_cor, corners, b_cor, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_cnt, counts, (size_t)n_views * 4, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        CalibJob j = calib_job(d + o_cor, per_frame, d + o_cnt, n_views, nullptr, 1, cols, rows, square, w, h, prm);
        j.guesses = guess ? reinterpret_cast<const rmcv_calib_guess*>(d + o_guess) : nullptr;
        j.ws = reinterpret_cast<double*>(d);
        j.vcam = reinterpret_cast<int32_t*>(d + o_vcam);
        j.results = reinterpret_cast<rmcv_calib_result*>(d + o_res);
        j.views = reinterpret_cast<rmcv_calib_view*>(d + o_views);
        e = launch_calib(j, c->stream);
    }
    c->last_what = "k_calib";
    int rcw = 0;
    if (e == hipSuccess) rcw = blk.waited(wait_stream(c, c->stream, "k_calib"));
    if (e == hipSuccess && rcw == 0) e = hipMemcpy(result, d + o_res, sizeof(rmcv_calib_result), hipMemcpyDeviceToHost);
    if (e == hipSuccess && rcw == 0) e = hipMemcpy(views_out, d + o_views, b_views, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(c, e == hipErrorOutOfMemory ? RMCV_ERR_NOMEM : RMCV_ERR_HIP, "rmcv_calibrate_camera", e);
    return rcw;
}

} // extern "C"
