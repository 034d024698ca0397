// device_corner.h -- sub-pixel corner refinement: the library's pinned statement of cv::cornerSubPix as
// executable/calibration/hand_eye.cpp:121 calls it, one source for rmcv_corner_subpix_host (the sequential form, this file) and
// k_corner_subpix (k_corner.hip), which agree bit for bit.  OpenCV is not the reference here: this text is, and DESIGN.md 4s lists where it
// knowingly departs.  Built with -ffp-contract=off; every float expression is evaluated left to right in float, every sum in double.
//
// Gray.   (1868 B + 9617 G + 4899 R + 8192) >> 14 of SRC(f), the BGR image a frame's results are defined on (source_view_plan.h).
// Mask.   win_w = 2 win_x + 1, win_h = 2 win_y + 1; mask[i][j] = (float)(vy * exp(-(x x))), x = (float)(j - win_x) / win_x,
//         y = (float)(i - win_y) / win_y, vy = exp(-(y y)); both exp are pm_exp of the double promoted from the float product.  A zero zone
//         (zx, zy) zeroes rows win_y - zy .. win_y + zy in columns win_x - zx .. win_x + zx.  Built once per call on the host.
// Patch.  (win_w + 2) x (win_h + 2) floats around the iterate c: cx = c.x - (win_w + 1) * 0.5f, fx = floor(cx), a = max(cx - fx, 0.0001f);
//         likewise cy, fy, b = cy - fy (no lower bound); a11 = (1-a)(1-b), a12 = a(1-b), a21 = (1-a)b, a22 = ab;
//         p[r][c] = g(ix+c, iy+r) a11 + g(ix+c+1, iy+r) a12 + g(ix+c, iy+r+1) a21 + g(ix+c+1, iy+r+1) a22, g = gray as float with both
//         indices clamped into the image; ix = (int)fx where that lies in -64 .. w + 64 and that bound otherwise (every tap of such a patch is
//         clamped to the same edge column whichever it is), likewise iy.
// Window element k = i win_w + j:  tgx = p[i+1][j+2] - p[i+1][j], tgy = p[i+2][j+1] - p[i][j+1]; gxx = tgx tgx m, gxy = tgx tgy m,
//         gyy = tgy tgy m; px = j - win_x, py = i - win_y; a += gxx, b += gxy, c += gyy, bb1 += gxx px + gxy py, bb2 += gxy px + gyy py (the
//         last two terms in float, then widened).
// Order.  What a wavefront does: partial sum l (0 .. 63) takes the elements k % 64 == l in ascending k, then acc[l] = acc[l] + acc[l ^ s] for
//         s = 32, 16, 8, 4, 2, 1, all 64 at once per s.  Every l ends with the same five sums (a + b == b + a).
// Solve.  det = a c - b b; |det| <= DBL_EPSILON^2 (or not a number): DET_ZERO, stop, keep c.  Else scale = 1.0 / det,
//         x' = (float)(c.x + c scale bb1 - b scale bb2), y' = (float)(c.y - b scale bb1 + a scale bb2), err = (x'-c.x)^2 + (y'-c.y)^2 in
//         float, c = (x', y').  c outside [0, w) x [0, h): LEFT_IMAGE, stop.  err <= eps eps (double): CONVERGED, stop.  Stop after max_iters.
//         Afterwards |c.x - in.x| > win_x or |c.y - in.y| > win_y: REVERTED, the result is the input.  A non-finite input: BAD_INPUT, untouched.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "../../include/rmcv_abi.h"
#include "pinned_math.h"
#include "source_view_plan.h"

#if defined(__HIPCC__)
#include "frame_source.h"
#define CORNER_FN __host__ __device__ static inline
#else
#define CORNER_FN static inline
#endif

namespace rmcv {

CORNER_FN int corner_gray(int b, int g, int r) { return (1868 * b + 9617 * g + 4899 * r + 8192) >> 14; }

CORNER_FN bool corner_finite(float v)
{
    uint32_t u;
    __builtin_memcpy(&u, &v, 4);
    return (u & 0x7F800000u) != 0x7F800000u;
}

// one entry of the mask (zero zone apart)
CORNER_FN float corner_mask_entry(int i, int j, int win_x, int win_y)
{
    const float x = (float)(j - win_x) / (float)win_x, y = (float)(i - win_y) / (float)win_y;
    const float xx = x * x, yy = y * y;
    const double vy = pm_exp(-(double)yy);
    return (float)(vy * pm_exp(-(double)xx));
}
// the whole mask, win_h rows of win_w floats (the parameters have been checked: corner_plan.h)
static inline void corner_mask(int win_x, int win_y, int zero_x, int zero_y, float* mask)
{
    const int win_w = 2 * win_x + 1, win_h = 2 * win_y + 1;
    for (int i = 0; i < win_h; i++)
        for (int j = 0; j < win_w; j++) mask[i * win_w + j] = corner_mask_entry(i, j, win_x, win_y);
    if (zero_x >= 0 && zero_y >= 0)
        for (int i = win_y - zero_y; i <= win_y + zero_y; i++)
            for (int j = win_x - zero_x; j <= win_x + zero_x; j++) mask[i * win_w + j] = 0.0f;
}

// where the patch around (x, y) lies and its four weights
struct CornerPatch {
    int ix, iy;
    float a11, a12, a21, a22;
};
CORNER_FN int corner_origin(float f, int extent)
{
    const float hi = (float)(extent + 64);
    return (int)(f < -64.0f ? -64.0f : (f > hi ? hi : f));
}
CORNER_FN CornerPatch corner_patch(float x, float y, int win_w, int win_h, int w, int h)
{
    const float cx = x - (float)(win_w + 1) * 0.5f, cy = y - (float)(win_h + 1) * 0.5f;
    const float fx = floorf(cx), fy = floorf(cy);
    float a = cx - fx;
    const float b = cy - fy;
    a = a < 0.0001f ? 0.0001f : a;
    CornerPatch P;
    P.ix = corner_origin(fx, w);
    P.iy = corner_origin(fy, h);
    P.a11 = (1.0f - a) * (1.0f - b);
    P.a12 = a * (1.0f - b);
    P.a21 = (1.0f - a) * b;
    P.a22 = a * b;
    return P;
}
CORNER_FN int corner_clamp(int v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); }
CORNER_FN float corner_patch_px(int g00, int g01, int g10, int g11, const CornerPatch& P)
{
    return (float)g00 * P.a11 + (float)g01 * P.a12 + (float)g10 * P.a21 + (float)g11 * P.a22;
}

struct CornerSums {
    double a, b, c, bb1, bb2;
};
CORNER_FN CornerSums corner_zero_sums() { return {0.0, 0.0, 0.0, 0.0, 0.0}; }
CORNER_FN CornerSums corner_add(const CornerSums& p, const CornerSums& q) { return {p.a + q.a, p.b + q.b, p.c + q.c, p.bb1 + q.bb1, p.bb2 + q.bb2}; }
// window element (i, j) of a patch of rows `pw` = win_w + 2 floats apart, weighted m, into s
template <class Patch>
CORNER_FN void corner_element(const Patch& p, int pw, int i, int j, float m, int win_x, int win_y, CornerSums& s)
{
    const float tgx = p[(i + 1) * pw + j + 2] - p[(i + 1) * pw + j];
    const float tgy = p[(i + 2) * pw + j + 1] - p[i * pw + j + 1];
    const float gxx = tgx * tgx * m, gxy = tgx * tgy * m, gyy = tgy * tgy * m;
    const float px = (float)(j - win_x), py = (float)(i - win_y);
    s.a += (double)gxx;
    s.b += (double)gxy;
    s.c += (double)gyy;
    s.bb1 += (double)(gxx * px + gxy * py);
    s.bb2 += (double)(gxy * px + gyy * py);
}

// one step from the sums: false = singular (x, y, err untouched)
CORNER_FN bool corner_solve(const CornerSums& s, float& x, float& y, float& err)
{
    const double det = s.a * s.c - s.b * s.b;
    if (!(pm_fabs(det) > DBL_EPSILON * DBL_EPSILON)) return false;
    const double scale = 1.0 / det;
    const float nx = (float)((double)x + s.c * scale * s.bb1 - s.b * scale * s.bb2);
    const float ny = (float)((double)y - s.b * scale * s.bb1 + s.a * scale * s.bb2);
    const float dx = nx - x, dy = ny - y;
    err = dx * dx + dy * dy;
    x = nx;
    y = ny;
    return true;
}

// The iteration of one corner.  sums(x, y): the five sums of the window around (x, y) in the pinned order -- the host's below, the
// wavefront's in k_corner.hip, where every lane calls this with the same values and leaves the loop in the same pass.
template <class Sums>
CORNER_FN void corner_refine(float& x, float& y, int32_t& status, int w, int h, int win_x, int win_y, int max_iters, double eps, Sums sums)
{
    const float x0 = x, y0 = y;
    if (!corner_finite(x0) || !corner_finite(y0)) {
        status = RMCV_CORNER_BAD_INPUT;
        return;
    }
    const double eps2 = eps * eps;
    float cx = x0, cy = y0, err = 0.0f;
    int iters = 0, st = 0;
    for (;;) {
        iters++;
        const CornerSums s = sums(cx, cy);
        if (!corner_solve(s, cx, cy, err)) { st |= RMCV_CORNER_DET_ZERO; break; }
        if (!(cx >= 0.0f && cx < (float)w && cy >= 0.0f && cy < (float)h)) { st |= RMCV_CORNER_LEFT_IMAGE; break; }
        if (!((double)err > eps2)) { st |= RMCV_CORNER_CONVERGED; break; }
        if (iters >= max_iters) break;
    }
    const float ddx = cx - x0, ddy = cy - y0;
    if (!((ddx < 0 ? -ddx : ddx) <= (float)win_x) || !((ddy < 0 ? -ddy : ddy) <= (float)win_y)) {
        cx = x0;
        cy = y0;
        st |= RMCV_CORNER_REVERTED;
    }
    x = cx;
    y = cy;
    status = iters | st;
}

// ---- the host form: a BGR image, rows `stride` bytes apart; the sequential statement of the rule ----
static inline int corner_gray_host_at(const uint8_t* bgr, int w, int h, int stride, int x, int y)
{
    const uint8_t* q = bgr + (int64_t)corner_clamp(y, h) * stride + 3 * (int64_t)corner_clamp(x, w);
    return corner_gray(q[0], q[1], q[2]);
}
static inline void corner_subpix_host(const uint8_t* bgr, int w, int h, int stride, float* corners, int n, int win_x, int win_y, int zero_x, int zero_y,
                                      int max_iters, double eps, int32_t* status_out)
{
    const int win_w = 2 * win_x + 1, win_h = 2 * win_y + 1, gw = win_w + 3, gh = win_h + 3, pw = win_w + 2, ph = win_h + 2;
    float* mask = new float[win_w * win_h];
    uint8_t* gray = new uint8_t[gw * gh];
    float* patch = new float[pw * ph];
    corner_mask(win_x, win_y, zero_x, zero_y, mask);
    auto sums = [&](float x, float y) {
        const CornerPatch P = corner_patch(x, y, win_w, win_h, w, h);
        for (int r = 0; r < gh; r++)
            for (int c = 0; c < gw; c++) gray[r * gw + c] = (uint8_t)corner_gray_host_at(bgr, w, h, stride, P.ix + c, P.iy + r);
        for (int r = 0; r < ph; r++)
            for (int c = 0; c < pw; c++) {
                const uint8_t* g = gray + r * gw + c;
                patch[r * pw + c] = corner_patch_px(g[0], g[1], g[gw], g[gw + 1], P);
            }
        CornerSums acc[64], nxt[64];
        for (int l = 0; l < 64; l++) acc[l] = corner_zero_sums();
        for (int k = 0; k < win_w * win_h; k++) corner_element(patch, pw, k / win_w, k % win_w, mask[k], win_x, win_y, acc[k & 63]);
        for (int s = 32; s >= 1; s >>= 1) {
            for (int l = 0; l < 64; l++) nxt[l] = corner_add(acc[l], acc[l ^ s]);
            for (int l = 0; l < 64; l++) acc[l] = nxt[l];
        }
        return acc[0];
    };
    for (int q = 0; q < n; q++) {
        int32_t st = 0;
        corner_refine(corners[2 * q], corners[2 * q + 1], st, w, h, win_x, win_y, max_iters, eps, sums);
        if (status_out) status_out[q] = st;
    }
    delete[] patch;
    delete[] gray;
    delete[] mask;
}

#if defined(__HIPCC__)
// ---- the device's gray accessor: gray of SRC(f) at (x, y), both clamped into w x h, by the kind of source (source_view_plan.h) -- what
// k_view_source and the icon paths read -- of the frame frame_pixels (frame_source.h) has resolved
template <int SRC>
__device__ inline int corner_gray_at(const FramePixels& s, int x, int y)
{
    x = corner_clamp(x, s.w);
    y = corner_clamp(y, s.h);
    if constexpr (SRC == SOURCE_MOSAIC || SRC == SOURCE_MOSAIC_RAW) {
        int o[3];
        if constexpr (SRC == SOURCE_MOSAIC) bayer_bgr(s.frame, s.stride, s.w, s.h, s.rx, s.ry, x, y, o);
        else bayer_bgr_raw(s.frame, s.stride, s.w, s.h, s.rx, s.ry, s.lay, x, y, o);
        return corner_gray(o[0], o[1], o[2]);
    } else {
        const uint8_t* q = s.frame + (int64_t)y * s.stride + 3 * (int64_t)x;
        if constexpr (SRC == SOURCE_BGR_LUT) return corner_gray(s.lut[q[0]], s.lut[q[1]], s.lut[q[2]]);
        else return corner_gray(q[0], q[1], q[2]);
    }
}
#endif

} // namespace rmcv
