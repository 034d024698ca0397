// rmcv_capture.hip -- the calibration capture behind the ABI: the entry points of include/rmcv_abi.h that MEASURE chosen frames of the batch
// bound, and their stage-wise twins on the caller's own image -- the corner refinement and the chessboard detector (4t).  The
// same three forms as the views of rmcv_views.hip (the batch call, the one-frame getter through the context's staging, the stage-wise helper
// in a Scratch block of the call's own), on the same shared pieces (rmcv_ctx.h: frame_list_begin, Scratch, pack_bgr).  Every refusal is
// corner_plan.h's or chess_plan.h's.  No kernel lives here.
#include <string.h>

#include <vector>

#include "rmcv_ctx.h"
#include "device_corner.h"

using namespace rmcv;

/* ---- corner refinement (k_corner.hip); the host-side entry points: k_corner.hip ---- */

// rmcv_batch_refine_corners behind its checks
static int corner_batch(rmcv_ctx* c, const int32_t* frames, int n, void* d_corners, int per_frame, const void* d_counts, int win_x, int win_y, int zero_x,
                        int zero_y, int max_iters, double eps, void* d_status, hipStream_t s)
{
    int rc = LAZY_TABLE(c, &c->corner_mask, (size_t)CORNER_MASK_MAX, "allocating the corner refinement's tables");
    if (rc || (rc = frame_list_begin(c, frames, n, s, "H2D corner frames"))) return rc;
    const int nel = (2 * win_x + 1) * (2 * win_y + 1);
    corner_mask(win_x, win_y, zero_x, zero_y, c->corner_mask_host);
    HIPCHK(c, hipMemcpyAsync(c->corner_mask, c->corner_mask_host, (size_t)nel * 4, hipMemcpyHostToDevice, s), "H2D corner mask");
    CornerJob j{};
    j.src = frame_source_of(c->geom, c->bufs);
    j.frames = c->frame_list; j.n = n; j.per_frame = per_frame;
    j.corners = (float*)d_corners; j.counts = (const int32_t*)d_counts; j.status = (int32_t*)d_status;
    j.mask = c->corner_mask;
    j.win_x = win_x; j.win_y = win_y; j.max_iters = max_iters; j.eps = eps;
    HIPCHK(c, launch_corner(j, s), "k_corner_subpix");
    return order_end(c, s);
}

static int corner_check(rmcv_ctx* c, const int32_t* frames, int n, const void* d_corners, int per_frame, int win_x, int win_y, int zero_x, int zero_y,
                        int max_iters, double eps)
{
    if (!c->bufs.frames) return fail(c, RMCV_ERR_BAD_ARG, CORNER_NOTHING_BOUND);
    return refuse(c, corners_refusal(frames, n, c->geom.n_frames, source_kind(c->geom), c->last_stages, d_corners, per_frame, win_x, win_y, zero_x, zero_y,
                                     max_iters, eps));
}

extern "C" {

int rmcv_batch_refine_corners(rmcv_ctx* c, const int32_t* frames, int n, void* d_corners, int per_frame, const void* d_counts, int win_x, int win_y,
                              int zero_x, int zero_y, int max_iters, double eps, void* d_status, void* hip_stream)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    if (const int rc = corner_check(c, frames, n, d_corners, per_frame, win_x, win_y, zero_x, zero_y, max_iters, eps)) return rc;
    hipSetDevice(c->device);
    return corner_batch(c, frames, n, d_corners, per_frame, d_counts, win_x, win_y, zero_x, zero_y, max_iters, eps, d_status, stream_of(c, hip_stream));
}

int rmcv_batch_get_refined_corners(rmcv_ctx* c, int frame, float* corners, int n, int win_x, int win_y, int zero_x, int zero_y, int max_iters, double eps,
                                   int32_t* status_out)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    if (!corners) return fail(c, RMCV_ERR_BAD_ARG, CORNER_NULL_TABLE);
    const int32_t one = frame;
    int rc = corner_check(c, &one, 1, corners, n, win_x, win_y, zero_x, zero_y, max_iters, eps);
    if (rc || (rc = ctx_ready(c))) return rc;
    if ((rc = LAZY_TABLE(c, &c->corner_tab, (size_t)3 * RMCV_CORNER_PER_FRAME_MAX, "allocating the corner refinement's staging"))) return rc;
    int32_t* d_status = c->corner_tab + 2 * RMCV_CORNER_PER_FRAME_MAX;
    HIPCHK(c, hipMemcpy(c->corner_tab, corners, (size_t)n * 8, hipMemcpyHostToDevice), "H2D corners");
    if ((rc = corner_batch(c, &one, 1, c->corner_tab, n, nullptr, win_x, win_y, zero_x, zero_y, max_iters, eps, d_status, c->stream))) return rc;
    WAITCHK(c, wait_stream(c, c->stream, "k_corner_subpix"));
    HIPCHK(c, hipMemcpy(corners, c->corner_tab, (size_t)n * 8, hipMemcpyDeviceToHost), "D2H corners");
    if (status_out) HIPCHK(c, hipMemcpy(status_out, d_status, (size_t)n * 4, hipMemcpyDeviceToHost), "D2H corner status");
    return RMCV_OK;
}

int rmcv_corner_subpix(rmcv_ctx* c, const uint8_t* bgr, int w, int h, int stride, float* corners, int n, int win_x, int win_y, int zero_x, int zero_y,
                       int max_iters, double eps, int32_t* status_out)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    const char* bad = corner_image_refusal(bgr, corners, w, h, stride, n);
    if (!bad && (n < 1 || n > RMCV_CORNER_PER_FRAME_MAX)) bad = CORNER_PER_FRAME;
    if (!bad) bad = corner_params_refusal(win_x, win_y, zero_x, zero_y, max_iters, eps);
    if (const int rc = refuse_as(c, "rmcv_corner_subpix", bad)) return rc;
    if (w > c->lim.max_width || h > c->lim.max_height) return fail(c, RMCV_ERR_BAD_ARG, CORNER_BEYOND_LIMITS);
    if (const int rc = ctx_ready(c)) return rc;
    // one host block, one upload: the image, the corners, the mask; the status words behind them
    const int dstride = bgr_row_bytes(w), nel = (2 * win_x + 1) * (2 * win_y + 1);
    const size_t o_cor = (size_t)dstride * h, o_mask = o_cor + up16((size_t)n * 8), in_bytes = o_mask + up16((size_t)nel * 4);
    const size_t o_st = in_bytes, total = o_st + (size_t)n * 4;
    std::vector<uint8_t> host(in_bytes, 0);
    pack_bgr(host.data(), bgr, w, h, stride);
    memcpy(&host[o_cor], corners, (size_t)n * 8);
    corner_mask(win_x, win_y, zero_x, zero_y, reinterpret_cast<float*>(&host[o_mask]));
    auto launch = [&](uint8_t* d) {
        CornerJob j{};
        j.src = frame_source_packed(d, w, h, dstride);
        j.frames = nullptr; j.n = 1; j.per_frame = n;
        j.corners = reinterpret_cast<float*>(d + o_cor); j.counts = nullptr; j.status = reinterpret_cast<int32_t*>(d + o_st);
        j.mask = reinterpret_cast<const float*>(d + o_mask);
        j.win_x = win_x; j.win_y = win_y; j.max_iters = max_iters; j.eps = eps;
        return launch_corner(j, c->stream);
    };
    return scratch_call(c, total, host.data(), in_bytes, launch, "k_corner_subpix", "k_corner_subpix", "rmcv_corner_subpix", [&](const uint8_t* d) {
        const hipError_t e = hipMemcpy(corners, d + o_cor, (size_t)n * 8, hipMemcpyDeviceToHost);
        return e == hipSuccess && status_out ? hipMemcpy(status_out, d + o_st, (size_t)n * 4, hipMemcpyDeviceToHost) : e;
    });
}

} // extern "C"

/* ---- the chessboard detector (k_chess.hip); the host-side entry points: k_chess.hip ---- */

// rmcv_batch_find_chessboards behind its checks
static int chess_batch(rmcv_ctx* c, const int32_t* frames, int n, int cols, int rows, const rmcv_chess_params& prm, void* d_corners, int per_frame, void* d_counts,
                       void* d_status, void* d_cand, void* d_cand_n, hipStream_t s)
{
    int rc = LAZY_TABLE(c, &c->chess_lists, (size_t)c->lim.max_frames * (1 + CHESS_LIST_WORDS), "allocating the chessboard detector's tables");
    if (rc || (rc = frame_list_begin(c, frames, n, s, "H2D chessboard frames"))) return rc;
    ChessJob j{};
    j.src = frame_source_of(c->geom, c->bufs);
    j.frames = c->frame_list; j.n = n;
    j.cols = cols; j.rows = rows; j.prm = prm;
    j.lists = c->chess_lists;
    j.corners = (float*)d_corners; j.per_frame = per_frame; j.counts = (int32_t*)d_counts; j.status = (int32_t*)d_status;
    j.cand = (int32_t*)d_cand; j.cand_n = (int32_t*)d_cand_n;
    HIPCHK(c, launch_chess(j, s), "k_chess");
    return order_end(c, s);
}

static int chess_check(rmcv_ctx* c, const int32_t* frames, int n, const void* d_corners, const void* d_counts, int per_frame, int cols, int rows,
                       const rmcv_chess_params& prm)
{
    if (!c->bufs.frames) return fail(c, RMCV_ERR_BAD_ARG, CHESS_NOTHING_BOUND);
    return refuse(c, chessboards_refusal(frames, n, c->geom.n_frames, source_kind(c->geom), c->last_stages, d_corners, d_counts, per_frame, cols, rows, prm));
}

extern "C" {

int rmcv_batch_find_chessboards(rmcv_ctx* c, const int32_t* frames, int n, int cols, int rows, const rmcv_chess_params* params, void* d_corners, int per_frame,
                                void* d_counts, void* d_status, void* hip_stream)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    const rmcv_chess_params prm = params ? *params : chess_default_params();
    if (const int rc = chess_check(c, frames, n, d_corners, d_counts, per_frame, cols, rows, prm)) return rc;
    hipSetDevice(c->device);
    return chess_batch(c, frames, n, cols, rows, prm, d_corners, per_frame, d_counts, d_status, nullptr, nullptr, stream_of(c, hip_stream));
}

int rmcv_batch_get_chessboard(rmcv_ctx* c, int frame, int cols, int rows, const rmcv_chess_params* params, float* corners_out, int32_t* status_out,
                              int32_t* cand_out, int32_t* cand_n_out)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    const rmcv_chess_params prm = params ? *params : chess_default_params();
    const int32_t one = frame;
    int rc = chess_check(c, &one, 1, corners_out, corners_out, RMCV_CORNER_PER_FRAME_MAX, cols, rows, prm);
    if (rc || (rc = ctx_ready(c))) return rc;
    constexpr int CAP = RMCV_CHESS_CAND_MAX, O_WORDS = 2 * RMCV_CORNER_PER_FRAME_MAX, O_CAND = O_WORDS + 4;   // corners | count, status, candidates, - | (x, y, R)
    if ((rc = LAZY_TABLE(c, &c->chess_tab, (size_t)O_CAND + 3 * CAP, "allocating the chessboard detector's staging"))) return rc;
    int32_t* t = c->chess_tab;
    if ((rc = chess_batch(c, &one, 1, cols, rows, prm, t, RMCV_CORNER_PER_FRAME_MAX, t + O_WORDS, t + O_WORDS + 1, t + O_CAND, t + O_WORDS + 2, c->stream))) return rc;
    WAITCHK(c, wait_stream(c, c->stream, "k_chess"));
    int32_t words[3];
    HIPCHK(c, hipMemcpy(words, t + O_WORDS, sizeof(words), hipMemcpyDeviceToHost), "D2H chessboard words");
    if (words[0] > 0) HIPCHK(c, hipMemcpy(corners_out, t, (size_t)words[0] * 8, hipMemcpyDeviceToHost), "D2H chessboard corners");
    if (cand_out && words[2] > 0) HIPCHK(c, hipMemcpy(cand_out, t + O_CAND, (size_t)words[2] * 12, hipMemcpyDeviceToHost), "D2H chessboard candidates");
    if (status_out) *status_out = words[1];
    if (cand_n_out) *cand_n_out = words[2];
    return RMCV_OK;
}

int rmcv_find_chessboard(rmcv_ctx* c, const uint8_t* bgr, int w, int h, int stride, int cols, int rows, const rmcv_chess_params* params, float* corners_out,
                         int32_t* status_out, int32_t* cand_out, int32_t* cand_n_out)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    const rmcv_chess_params prm = params ? *params : chess_default_params();
    const char* bad = chess_image_refusal(bgr, corners_out, w, h, stride);
    if (!bad) bad = chess_params_refusal(cols, rows, prm);
    if (const int rc = refuse_as(c, "rmcv_find_chessboard", bad)) return rc;
    if (w > c->lim.max_width || h > c->lim.max_height) return fail(c, RMCV_ERR_BAD_ARG, CHESS_BEYOND_LIMITS);
    if (const int rc = ctx_ready(c)) return rc;
    // the image is all that is uploaded; behind it the words (count, status, candidates, -), the corners, the sorted candidates and the list
    // between the two kernels
    constexpr size_t CAP = RMCV_CHESS_CAND_MAX;
    const int dstride = bgr_row_bytes(w), want = cols * rows;
    const size_t o_words = (size_t)dstride * h, o_cor = o_words + 16, o_cand = o_cor + (size_t)want * 8, o_list = o_cand + 12 * CAP;
    const size_t total = o_list + 4 * (1 + (size_t)CHESS_LIST_WORDS);
    std::vector<uint8_t> host(o_words, 0);
    pack_bgr(host.data(), bgr, w, h, stride);
    auto launch = [&](uint8_t* d) {
        ChessJob j{};
        j.src = frame_source_packed(d, w, h, dstride);
        j.frames = nullptr; j.n = 1;
        j.cols = cols; j.rows = rows; j.prm = prm;
        j.lists = reinterpret_cast<uint32_t*>(d + o_list);
        j.corners = reinterpret_cast<float*>(d + o_cor); j.per_frame = want;
        int32_t* words = reinterpret_cast<int32_t*>(d + o_words);
        j.counts = words; j.status = words + 1; j.cand_n = words + 2;
        j.cand = reinterpret_cast<int32_t*>(d + o_cand);
        return launch_chess(j, c->stream);
    };
    int32_t words[3] = {0, 0, 0};
    const int rc = scratch_call(c, total, host.data(), o_words, launch, "k_chess", "k_chess", "rmcv_find_chessboard", [&](const uint8_t* d) {
        hipError_t e = hipMemcpy(words, d + o_words, sizeof(words), hipMemcpyDeviceToHost);
        if (e == hipSuccess && words[0] == want) e = hipMemcpy(corners_out, d + o_cor, (size_t)want * 8, hipMemcpyDeviceToHost);
        if (e == hipSuccess && cand_out && words[2] > 0 && words[2] <= (int)CAP) e = hipMemcpy(cand_out, d + o_cand, (size_t)words[2] * 12, hipMemcpyDeviceToHost);
        return e;
    });
    if (rc) return rc;
    if (status_out) *status_out = words[1];
    if (cand_n_out) *cand_n_out = words[2];
    return RMCV_OK;
}

} // extern "C"

