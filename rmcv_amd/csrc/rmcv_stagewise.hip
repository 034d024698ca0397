// rmcv_stagewise.hip -- the stage-wise helpers of include/rmcv_abi.h: one stage of the path on the CALLER's own data (an image, a
// contour, a list of armours), through the same kernels the batch path launches.  They use a context for its device, stream, limits and
// loaded models; what they bind or allocate is their own, so that nothing the caller has bound to the context moves unless said.  The
// stage-wise debug view and icon strip stand with their batch forms in rmcv_views.hip, the corner refinement and the chessboard detector in
// rmcv_capture.hip, the stage-wise calibration solve in rmcv_calib.hip.  rmcv_source_view stays here, in the text it had before those units
// existed: its move onto their shared pieces (ViewBlock, pack_bgr, scratch_call) met a GPU fault in
// tests/test_gpu_source_view.py::test_stagewise_view_equals_the_reference[640x400-40x25] whose cause has not been found, and it goes there
// only once that cause is known.
#include <string.h>

#include <cmath>

#include "rmcv_ctx.h"
#include "device_bayer.h"
#include "device_view.h"

using namespace rmcv;

extern "C" {

int rmcv_classify_armours(rmcv_ctx* c, const uint8_t* bgr, int w, int h, int stride, rmcv_armour* armours, int n,
                          int32_t* identity_out, uint8_t* icons_out)
{
    if (!c || !bgr || (n > 0 && (!armours || !identity_out)) || n < 0) return RMCV_ERR_BAD_ARG;
    if (!c->bufs.svm_w) return fail(c, RMCV_ERR_BAD_ARG, "rmcv_svm_load first");
    if (n > c->lim.max_armours) return fail(c, RMCV_ERR_CAPACITY, "too many armours for this context");
    int rc = rmcv_batch_upload(c, bgr, 1, w, h, stride, (int64_t)stride * h); // syncs the context first
    if (rc) return rc;
    if (n == 0) return RMCV_OK;
    HIPCHK(c, hipMemcpy(c->bufs.armours, armours, (size_t)n * sizeof(rmcv_armour), hipMemcpyHostToDevice), "H2D armours");
    HIPCHK(c, hipMemcpy(c->bufs.n_armours, &n, 4, hipMemcpyHostToDevice), "H2D");
    if (c->geom.enhance) HIPCHK(c, launch_enhance_tables(c->geom, c->bufs, 1, c->stream), "k_frame_sums + k_enhance_table"); // the icon is cut from E(f)
    HIPCHK(c, launch_classify(c->geom, c->bufs, c->lim, c->stream), "k_classify");
    WAITCHK(c, wait_stream(c, c->stream, "waiting for the context's stream"));
    HIPCHK(c, hipMemcpy(armours, c->bufs.armours, (size_t)n * sizeof(rmcv_armour), hipMemcpyDeviceToHost), "D2H armours");
    HIPCHK(c, hipMemcpy(identity_out, c->bufs.identity, (size_t)n * 4, hipMemcpyDeviceToHost), "D2H identity");
    if (icons_out) HIPCHK(c, hipMemcpy(icons_out, c->bufs.icons, (size_t)n * RMCV_SVM_FEATURES, hipMemcpyDeviceToHost), "D2H icons");
    return RMCV_OK;
}

int rmcv_locate_armours(rmcv_ctx* c, const rmcv_armour* armours, int n, const double* base2gripper, double* rvecs, double* tvecs,
                        double* positions)
{
    if (!c || n < 0 || (n > 0 && !armours)) return RMCV_ERR_BAD_ARG;
    if (!c->bufs.pnp_cfg) return fail(c, RMCV_ERR_BAD_ARG, "rmcv_pnp_load first");
    if (n > c->lim.max_armours) return fail(c, RMCV_ERR_CAPACITY, "too many armours for this context");
    if (n == 0) return RMCV_OK;
    if (const int rc = ctx_ready(c)) return rc;
    resident_none(c);
    static const double eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    HIPCHK(c, hipMemcpy(c->bufs.armours, armours, (size_t)n * sizeof(rmcv_armour), hipMemcpyHostToDevice), "H2D armours");
    HIPCHK(c, hipMemcpy(c->bufs.n_armours, &n, 4, hipMemcpyHostToDevice), "H2D");
    HIPCHK(c, hipMemcpy(c->bufs.base2gripper, base2gripper ? base2gripper : eye, sizeof(eye), hipMemcpyHostToDevice), "H2D base2gripper");
    Geom g1 = c->geom;
    g1.n_frames = 1;
    g1.win = 0; // (the caller's armours, the default ROI: whatever windows the batch bound to the context has)
    Bufs b1 = c->bufs;
    b1.pose_base2gripper = b1.base2gripper; // (... and the caller's matrix, whatever attitude step ran in front of that batch)
    b1.cam_req = nullptr;                   // (... and camera 0, whatever cameras its frames have)
    HIPCHK(c, launch_pnp(g1, b1, c->lim, c->stream), "k_pnp");
    WAITCHK(c, wait_stream(c, c->stream, "waiting for the context's stream"));
    std::vector<PoseRow> all((size_t)n);
    HIPCHK(c, hipMemcpy(all.data(), c->bufs.poses, all.size() * sizeof(PoseRow), hipMemcpyDeviceToHost), "D2H poses");
    for (int a = 0; a < n; a++) scatter_pose(all[a], rvecs, tvecs, positions, (size_t)a);
    return RMCV_OK;
}

// ---- legacy per-contour matcher --------------------------------------------------------------------------
static int match_one(rmcv_ctx* c, const rmcv_point* pts, int n, const rmcv_legacy_params& lp, int mode, rmcv_rrect* box, int32_t* matched)
{
    int32_t offs[2] = {0, n};
    hipSetDevice(c->device);
    int rc = load_contours(c, pts, offs, 1);
    if (rc) return rc;
    rmcv_params p;
    rmcv_default_params(&p);
    const Geom g1 = one_frame_geom(c);
    HIPCHK(c, launch_match(g1, c->bufs, c->lim, p, lp, mode, false, false, c->stream), "k_match");
    WAITCHK(c, wait_stream(c, c->stream, "waiting for the context's stream"));
    int32_t nb = 0, st = 0;
    HIPCHK(c, hipMemcpy(&nb, c->bufs.n_blobs, 4, hipMemcpyDeviceToHost), "D2H");
    HIPCHK(c, hipMemcpy(&st, c->bufs.status, 4, hipMemcpyDeviceToHost), "D2H");
    if (st & RMCV_FRAME_HULL)
        return fail(c, RMCV_ERR_BAD_ARG, "minAreaRect: not a closed border (a column of the bounding box is empty) or wider than the context's max_width");
    *matched = nb == 1;
    if (nb == 1) HIPCHK(c, hipMemcpy(box, c->bufs.ellipses, sizeof(rmcv_rrect), hipMemcpyDeviceToHost), "D2H box");
    return RMCV_OK;
}

int rmcv_min_area_rect(rmcv_ctx* c, const rmcv_point* pts, int n, rmcv_rrect* out)
{
    if (!c || !pts || !out || n < 1) return RMCV_ERR_BAD_ARG;
    rmcv_legacy_params lp = {0, 0, 0, 0, 0, 0};
    int32_t m = 0;
    int rc = match_one(c, pts, n, lp, 1, out, &m);
    if (rc) return rc;
    return m ? RMCV_OK : fail(c, RMCV_ERR_HIP, "minAreaRect produced no result");
}

int rmcv_match_lightblob(rmcv_ctx* c, const rmcv_point* pts, int n, const rmcv_legacy_params* lp, rmcv_rrect* box_out, int32_t* matched)
{
    if (!c || !lp || !box_out || !matched || n < 0 || (n > 0 && !pts)) return RMCV_ERR_BAD_ARG;
    *matched = 0;
    if (n < 6) return RMCV_OK; // src/objdetect.cpp:12
    return match_one(c, pts, n, *lp, 0, box_out, matched);
}

// rmcv_demosaic / rmcv_demosaic_raw: the arguments are checked, then D(T(r)) of the buffer in layout `lay` (0: a plain 8-bit mosaic)
static int demosaic_body(rmcv_ctx* c, const uint8_t* raw, int w, int h, int stride, int pattern, int lay, uint8_t* bgr_out, int out_stride)
{
    const int sb = rmcv::lay_bytes(lay);
    if (const int rc = ctx_ready(c)) return rc;
    // (a stage-wise helper: buffers of its own, so that nothing bound to the context moves)
    Scratch d_raw, d_out;
    const size_t in_bytes = (size_t)sb * w * h, out_bytes = (size_t)3 * w * h;
    hipError_t e = d_raw.alloc(in_bytes);
    if (e == hipSuccess) e = d_out.alloc(out_bytes);
    if (e == hipSuccess) e = hipMemcpy2DAsync(d_raw.d, (size_t)sb * w, raw, stride, (size_t)sb * w, h, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = launch_demosaic(d_raw.d, sb * w, w, h, pattern, lay, d_out.d, 3 * w, c->stream);
    c->last_what = "k_demosaic";
    int rcw = 0;
    if (e == hipSuccess) rcw = d_raw.waited(d_out.waited(wait_stream(c, c->stream, "k_demosaic")));
    if (e == hipSuccess && rcw == 0) e = hipMemcpy2D(bgr_out, out_stride, d_out.d, 3 * w, 3 * w, h, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(c, e == hipErrorOutOfMemory ? RMCV_ERR_NOMEM : RMCV_ERR_HIP, "rmcv_demosaic", e);
    return rcw;
}

int rmcv_demosaic(rmcv_ctx* c, const uint8_t* raw, int w, int h, int stride, int pattern, uint8_t* bgr_out, int out_stride)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    if (!raw || !bgr_out) return fail(c, RMCV_ERR_BAD_ARG, "rmcv_demosaic: null buffer");
    if (w < 3 || h < 3) return fail(c, RMCV_ERR_BAD_ARG, "rmcv_demosaic: a mosaic needs w >= 3 and h >= 3");
    if (stride < w) return fail(c, RMCV_ERR_BAD_ARG, "rmcv_demosaic: stride < w");
    if (out_stride < 3 * w) return fail(c, RMCV_ERR_BAD_ARG, "rmcv_demosaic: out_stride < 3 w");
    if (pattern < RMCV_BAYER_RG || pattern > RMCV_BAYER_BG) return fail(c, RMCV_ERR_BAD_ARG, "rmcv_demosaic: unknown Bayer pattern");
    return demosaic_body(c, raw, w, h, stride, pattern, 0, bgr_out, out_stride);
}

int rmcv_demosaic_raw(rmcv_ctx* c, const void* raw, int w, int h, int stride, int pattern, int sample_bits, int valid_bit, int orient,
                      uint8_t* bgr_out, int out_stride)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    if (!raw || !bgr_out) return fail(c, RMCV_ERR_BAD_ARG, "rmcv_demosaic_raw: null buffer");
    if (w < 3 || h < 3) return fail(c, RMCV_ERR_BAD_ARG, "rmcv_demosaic_raw: a mosaic needs w >= 3 and h >= 3");
    if (sample_bits != 8 && sample_bits != 16) return fail(c, RMCV_ERR_BAD_ARG, "rmcv_demosaic_raw: sample_bits is 8 or 16");
    if (valid_bit < 0 || valid_bit > 4) return fail(c, RMCV_ERR_BAD_ARG, "rmcv_demosaic_raw: valid_bit is 0 .. 4");
    if (orient < 0 || orient > (RMCV_ORIENT_MIRROR | RMCV_ORIENT_FLIP)) return fail(c, RMCV_ERR_BAD_ARG, "rmcv_demosaic_raw: unknown orientation bits");
    if (stride < sample_bits / 8 * w) return fail(c, RMCV_ERR_BAD_ARG, sample_bits == 16 ? "rmcv_demosaic_raw: stride < 2 w" : "rmcv_demosaic_raw: stride < w");
    if (sample_bits == 16 && (stride & 1)) return fail(c, RMCV_ERR_BAD_ARG, "rmcv_demosaic_raw: odd stride with 16-bit samples");
    if (sample_bits == 16 && ((uintptr_t)raw & 1)) return fail(c, RMCV_ERR_BAD_ARG, "rmcv_demosaic_raw: 16-bit samples need a 2-byte aligned buffer");
    if (out_stride < 3 * w) return fail(c, RMCV_ERR_BAD_ARG, "rmcv_demosaic_raw: out_stride < 3 w");
    if (pattern < RMCV_BAYER_RG || pattern > RMCV_BAYER_BG) return fail(c, RMCV_ERR_BAD_ARG, "rmcv_demosaic_raw: unknown Bayer pattern");
    return demosaic_body(c, (const uint8_t*)raw, w, h, stride, pattern, rmcv::raw_layout(sample_bits, valid_bit, orient), bgr_out, out_stride);
}

// rmcv_calc_gamma / rmcv_auto_enhance: a host image of `rows` rows of `row_bytes` bytes through a table, on the device.  A stage-wise
// helper like rmcv_demosaic: buffers of its own, so that nothing bound to the context moves.  auto_w > 0: the image is a BGR frame of
// auto_w pixels per row and the table is that of ITS gamma (sums and table on the device); otherwise the table of `gamma`.
static int bytemap_body(rmcv_ctx* c, const uint8_t* src, int row_bytes, int rows, int src_stride, float gamma, int auto_w, float max_gain, float min_gain,
                        uint8_t* dst, int dst_stride, float* gamma_out, const char* who)
{
    if (const int rc = ctx_ready(c)) return rc;
    const int dstride = (row_bytes + 15) & ~15;
    const size_t img = (size_t)dstride * rows;
    // [image | sums 3 x 8 | gamma 4 + pad 4 | table 256 | threshold table 512]
    Scratch blk;
    hipError_t e = blk.alloc(img + 32 + 256 + 512);
    uint8_t* const d = blk.d;
    hipStream_t s = c->stream;
    if (e == hipSuccess && dstride != row_bytes) e = hipMemsetAsync(d, 0, img, s); // (the pad bytes go through the table too: keep them defined)
    if (e == hipSuccess) e = hipMemcpy2DAsync(d, dstride, src, src_stride, (size_t)row_bytes, rows, hipMemcpyHostToDevice, s);
    uint8_t* d_lut = d + img + 32;
    if (e == hipSuccess) {
        if (auto_w > 0) {
            Geom g1 = c->geom;
            g1.n_frames = 1; g1.w = auto_w; g1.h = rows; g1.stride = dstride; g1.frame_pitch = (int64_t)img;
            g1.enh_max_gain = max_gain; g1.enh_min_gain = min_gain;
            Bufs b1{};
            b1.frames = d;
            b1.enh_sums = reinterpret_cast<uint64_t*>(d + img);
            b1.enh_gamma = reinterpret_cast<float*>(d + img + 24);
            b1.enh_lut = d_lut;
            b1.enh_m = reinterpret_cast<uint16_t*>(d + img + 32 + 256);
            e = launch_enhance_tables(g1, b1, 1, s);
        } else e = launch_gamma_lut(gamma, d_lut, s);
    }
    if (e == hipSuccess) e = launch_bytemap(d, d, (int64_t)(img / 16), d_lut, c->geom.n_cu, s);
    c->last_what = auto_w > 0 ? "k_frame_sums, k_enhance_table, k_bytemap" : "k_gamma_lut, k_bytemap";
    int rcw = 0;
    if (e == hipSuccess) rcw = blk.waited(wait_stream(c, s, who));
    if (e == hipSuccess && rcw == 0) e = hipMemcpy2D(dst, dst_stride, d, dstride, (size_t)row_bytes, rows, hipMemcpyDeviceToHost);
    if (e == hipSuccess && rcw == 0 && gamma_out && auto_w > 0) e = hipMemcpy(gamma_out, d + img + 24, sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(c, e == hipErrorOutOfMemory ? RMCV_ERR_NOMEM : RMCV_ERR_HIP, who, e);
    return rcw;
}

int rmcv_calc_gamma(rmcv_ctx* c, const uint8_t* src, int row_bytes, int rows, int src_stride, float gamma, uint8_t* dst, int dst_stride)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    if (!src || !dst) return fail(c, RMCV_ERR_BAD_ARG, "rmcv_calc_gamma: null buffer");
    if (row_bytes < 1 || rows < 1 || src_stride < row_bytes || dst_stride < row_bytes) return fail(c, RMCV_ERR_BAD_ARG, "rmcv_calc_gamma: bad size or stride");
    if (!(gamma >= 0.0f) || !std::isfinite(gamma)) return fail(c, RMCV_ERR_BAD_ARG, "rmcv_calc_gamma: gamma must be finite and not negative");
    return bytemap_body(c, src, row_bytes, rows, src_stride, gamma, 0, 0.0f, 0.0f, dst, dst_stride, nullptr, "rmcv_calc_gamma");
}

int rmcv_auto_enhance(rmcv_ctx* c, const uint8_t* bgr, int w, int h, int stride, float max_gain, float min_gain, uint8_t* out, int out_stride,
                      float* gamma_out)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    if (!bgr || !out) return fail(c, RMCV_ERR_BAD_ARG, "rmcv_auto_enhance: null buffer");
    if (w < 1 || h < 1 || w > 65536 || h > 65536 || stride < 3 * w || out_stride < 3 * w) return fail(c, RMCV_ERR_BAD_ARG, "rmcv_auto_enhance: bad size or stride");
    if (!gains_ok(max_gain, min_gain)) return fail(c, RMCV_ERR_BAD_ARG, "rmcv_auto_enhance: the gains must be finite and differ");
    return bytemap_body(c, bgr, 3 * w, h, stride, 0.0f, w, max_gain, min_gain, out, out_stride, gamma_out, "rmcv_auto_enhance");
}

int rmcv_find_lightblobs(rmcv_ctx* c, const uint8_t* bgr, int w, int h, int stride, const rmcv_point* pts, const int32_t* offs,
                         int n_contours, const rmcv_legacy_params* lp, rmcv_lightblob* blobs_out, int blobs_cap, int32_t* n_blobs,
                         int32_t* blob_src, rmcv_rrect* boxes_out)
{
    if (!c || !bgr || !lp || (n_contours > 0 && (!pts || !offs))) return RMCV_ERR_BAD_ARG;
    int rc = refuse(c, pixel_refusal(c->input.format, c->input.enhance, false, false, true));
    if (rc) return rc;
    hipSetDevice(c->device);
    rc = rmcv_batch_upload(c, bgr, 1, w, h, stride, (int64_t)stride * h); // source.channels() == 3 is the ABI's only format
    if (rc) return rc;
    rc = load_contours(c, pts, offs, n_contours);
    if (rc) return rc;
    for (int i = 0; i < (n_contours ? offs[n_contours] : 0); i++)
        if (pts[i].x < 0 || pts[i].x >= w || pts[i].y < 0 || pts[i].y >= h) return fail(c, RMCV_ERR_BAD_ARG, "contour point outside the frame");
    rmcv_params p;
    rmcv_default_params(&p);
    HIPCHK(c, launch_match(c->geom, c->bufs, c->lim, p, *lp, 0, true, false, c->stream), "k_match");
    int32_t nb = 0;
    rc = rmcv_batch_get_blobs(c, 0, blobs_out, blobs_cap, &nb, blob_src);
    if (rc) return rc;
    if (n_blobs) *n_blobs = nb;
    int32_t st = 0;
    HIPCHK(c, hipMemcpy(&st, c->bufs.status, 4, hipMemcpyDeviceToHost), "D2H");
    if (st & RMCV_FRAME_HULL) return fail(c, RMCV_ERR_BAD_ARG, "minAreaRect: a contour is not a closed border or exceeds the hull tables");
    if (boxes_out && nb) HIPCHK(c, hipMemcpy(boxes_out, c->bufs.ellipses, (size_t)nb * sizeof(rmcv_rrect), hipMemcpyDeviceToHost), "D2H boxes");
    return RMCV_OK;
}

int rmcv_source_view(rmcv_ctx* c, const uint8_t* bgr, int w, int h, int stride, const rmcv_lightblob* blobs, int n_blobs, const rmcv_point* neg_pts,
                     const int32_t* neg_offs, int n_neg, const rmcv_armour* armours, int n_armours, int flags, int vw, int vh, uint8_t* out,
                     int out_stride)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    const char* bad = rmcv::source_image_refusal(bgr, out, w, h, stride);
    if (!bad) bad = view_check_lists(w, h, w, blobs, n_blobs, neg_pts, neg_offs, n_neg, armours, n_armours, flags, vw, vh, out_stride);
    if (bad) {
        char msg[160];
        snprintf(msg, sizeof(msg), "rmcv_source_view: %s", bad);
        return fail(c, RMCV_ERR_BAD_ARG, msg);
    }
    if (w > c->lim.max_width || h > c->lim.max_height || vw > c->lim.max_width || vh > c->lim.max_height) return fail(c, RMCV_ERR_BAD_ARG, rmcv::SOURCE_VIEW_BEYOND_LIMITS);
    if (const int rc = ctx_ready(c)) return rc;
    // (a stage-wise helper: buffers of its own, so that nothing bound to the context moves) -- one host block, one upload; the image
    // packed to rows of 3 w bytes rounded up to 16
    const int prow = (w + 63) / 64 + 2, n_pts = n_neg ? neg_offs[n_neg] : 0, dstride = (3 * w + 15) & ~15;
    const size_t plane = (size_t)(h + 2) * prow;
    auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t o_blobs = (size_t)dstride * h, o_arm = o_blobs + up16((size_t)n_blobs * sizeof(rmcv_lightblob));
    const size_t o_pts = o_arm + up16((size_t)n_armours * sizeof(rmcv_armour)), o_offs = o_pts + up16((size_t)n_pts * sizeof(rmcv_point));
    const size_t o_cnt = o_offs + up16((size_t)(n_neg + 1) * 4), in_bytes = o_cnt + 16;
    const size_t o_ov = in_bytes, o_out = o_ov + up16(2 * plane * 8), total = o_out + (size_t)3 * vw * vh;
    std::vector<uint8_t> host(in_bytes, 0);
    for (int y = 0; y < h; y++) memcpy(&host[(size_t)y * dstride], bgr + (size_t)y * stride, (size_t)3 * w);
    if (n_blobs) memcpy(&host[o_blobs], blobs, (size_t)n_blobs * sizeof(rmcv_lightblob));
    if (n_armours) memcpy(&host[o_arm], armours, (size_t)n_armours * sizeof(rmcv_armour));
    if (n_pts) memcpy(&host[o_pts], neg_pts, (size_t)n_pts * sizeof(rmcv_point));
    if (n_neg) memcpy(&host[o_offs], neg_offs, (size_t)(n_neg + 1) * 4);
    const int32_t counts[4] = {n_blobs, n_armours, n_neg, 0};
    memcpy(&host[o_cnt], counts, sizeof(counts));
    uint8_t* d = nullptr;
    hipError_t e = hipMalloc((void**)&d, total);
    if (e == hipSuccess) e = hipMemcpyAsync(d, host.data(), in_bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        const int32_t* cnt = reinterpret_cast<const int32_t*>(d + o_cnt);
        SourceViewJob sj{};
        ViewJob& j = sj.view;
        j.w = w; j.h = h; j.prow = prow; j.plane_pitch = (int64_t)plane;
        j.bits = nullptr; j.overlay = reinterpret_cast<uint64_t*>(d + o_ov); j.frames = nullptr;
        j.n = 1; j.vw = vw; j.vh = vh; j.flags = flags;
        j.out = d + o_out; j.out_stride = 3 * vw; j.out_pitch = (int64_t)3 * vw * vh;
        j.lists = ViewLists{reinterpret_cast<const rmcv_lightblob*>(d + o_blobs), cnt, reinterpret_cast<const rmcv_armour*>(d + o_arm), cnt + 1,
                            reinterpret_cast<const rmcv_point*>(d + o_pts), nullptr, nullptr, cnt + 3, nullptr, cnt + 2,
                            reinterpret_cast<const int32_t*>(d + o_offs), n_blobs, n_armours, n_pts, n_neg, 1};
        sj.src = frame_source_packed(d, w, h, dstride);
        e = launch_source_view(sj, c->stream);
    }
    c->last_what = "k_view_overlay + k_view_source";
    int rcw = 0;
    if (e == hipSuccess) rcw = wait_stream(c, c->stream, "k_view_source");
    if (e == hipSuccess && rcw == 0) e = hipMemcpy2D(out, out_stride, d + o_out, (size_t)3 * vw, (size_t)3 * vw, vh, hipMemcpyDeviceToHost);
    if ((rcw == 0 || e != hipSuccess) && d) hipFree(d); // (after a wait that ran out the kernels may still be using it)
    if (e != hipSuccess) return fail(c, e == hipErrorOutOfMemory ? RMCV_ERR_NOMEM : RMCV_ERR_HIP, "rmcv_source_view", e);
    return rcw;
}

} // extern "C"
