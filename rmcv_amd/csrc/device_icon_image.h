// device_icon_image.h -- one armour's icon at any output size: rm::affine_correction(frame, tmp, armour.icon, {ow, oh}) as the
// labeler calls it (executable/svm/labeler.cpp:100, {80, 80}), by one wavefront.  It is icon_row (device_classify.h) with the output extent
// as run-time values.  The setup up to the inverted map is restated here, not shared with icon_row: factoring it out of icon_row changed the
// register allocation of every kernel that instantiates icon_row (profiles/icon_strip_isa_identity.txt compares them as they are now), so
// icon_row is left as it was and tests/test_gpu_icon_strip.py holds the two against each other at 20 x 20.
#pragma once
#include "device_classify.h"

namespace rmcv {

// icon_row's rule up to the inverted map (imgproc.cpp:11-28): clamp, integer box, getAffineTransform.  ic: the
// clamped quadrilateral (every lane has it); W: the warp of the box (W.bw x W.bh pixels at W.roi) as warp_px reads it.  Returns whether the
// box is degenerate (the icon is then zeros).  A is only read.
template <int BAYER>
__device__ __forceinline__ bool icon_setup(const uint8_t* frame, int f, int lane, const rmcv_armour* A, int w, int h, int stride, int pattern, int lay,
                                           const uint8_t* luts, float ic[4][2], WarpCtx& W)
{
    {
        // ---- imgproc.cpp:11-15 clamp (in place, like the reference), :17 integer bounding box
        int minx = 0, maxx = 0, miny = 0, maxy = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const float vx0 = A->icon[i][0], vy0 = A->icon[i][1];
            // std::max(0.0f, std::min(v, lim)): min(a, b) is b when b < a, max(a, b) is b when a < b -- so NaN and -0 both end as +0
            const float vx = (float)w - 1 < vx0 ? (float)w - 1 : vx0, vy = (float)h - 1 < vy0 ? (float)h - 1 : vy0;
            ic[i][0] = 0.0f < vx ? vx : 0.0f;
            ic[i][1] = 0.0f < vy ? vy : 0.0f;
            const int px = cv_round_f(ic[i][0]), py = cv_round_f(ic[i][1]);
            if (i == 0 || px < minx) minx = px;
            if (i == 0 || px > maxx) maxx = px;
            if (i == 0 || py < miny) miny = py;
            if (i == 0 || py > maxy) maxy = py;
        }
        const int bx = minx, by = miny, bw = maxx - minx + 1, bh = maxy - miny + 1;
        const bool degenerate = (bw <= 0 || bh <= 0 || bx < 0 || by < 0 || bx + bw > w || by + bh > h);
        // ---- :18-28 getAffineTransform: 6x6 LU with partial pivoting, matrix kept across the lanes
        W.roi = frame + (int64_t)by * stride + 3 * bx;
        W.stride = stride;
        W.bw = bw;
        W.bh = bh;
        if constexpr (BAYER == 2) W.lut = luts + (int64_t)f * 256;
        if constexpr (BAYER == 1) {
            W.frame = frame;
            W.fw = w;
            W.fh = h;
            W.bx = bx;
            W.by = by;
            W.rx = raw_rx(pattern, lay, w);
            W.ry = raw_ry(pattern, lay, h);
            W.lay = lay;
        }
        {
            const float src[3][2] = {{ic[1][0] - (float)bx, ic[1][1] - (float)by},
                                     {ic[2][0] - (float)bx, ic[2][1] - (float)by},
                                     {ic[0][0] - (float)bx, ic[0][1] - (float)by}};
            const float dst[3][2] = {{0, 0}, {(float)bw, 0}, {0, (float)bh}};
            LaneVec Am(lane), bv(lane);
            { // row 2i: [x y 1 0 0 0], row 2i+1: [0 0 0 x y 1]   (selects, not lane-dependent subscripts: those put the arrays in scratch memory)
                const int r = lane / 6, c = lane - 6 * r, i = r >> 1;
                const float sxi = i == 0 ? src[0][0] : (i == 1 ? src[1][0] : src[2][0]);
                const float syi = i == 0 ? src[0][1] : (i == 1 ? src[1][1] : src[2][1]);
                double v = 0.0;
                if (lane < 36) {
                    const int cc = (r & 1) ? c - 3 : c;
                    if (cc >= 0 && cc < 3) v = cc == 0 ? (double)sxi : (cc == 1 ? (double)syi : 1.0);
                }
                Am.reg = v;
                // b = (dst0.x, dst0.y, dst1.x, dst1.y, dst2.x, dst2.y) = (0, 0, bw, 0, 0, bh)
                bv.reg = lane == 2 ? (double)dst[1][0] : (lane == 5 ? (double)dst[2][1] : 0.0);
            }
            bool ok = true;
            for (int i = 0; i < 6 && ok; i++) {
                int k = i;
                for (int j = i + 1; j < 6; j++)
                    if (dabs(Am[j * 6 + i]) > dabs(Am[k * 6 + i])) k = j;
                if (dabs(Am[k * 6 + i]) < DBL_EPSILON * 100) { ok = false; break; }
                if (k != i) {
                    for (int j = i; j < 6; j++) { const double t = Am[i * 6 + j]; Am[i * 6 + j] = (double)Am[k * 6 + j]; Am[k * 6 + j] = t; }
                    const double t = bv[i]; bv[i] = (double)bv[k]; bv[k] = t;
                }
                const double d = -1 / (double)Am[i * 6 + i];
                for (int j = i + 1; j < 6; j++) {
                    const double alpha = (double)Am[j * 6 + i] * d;
                    for (int kk = i + 1; kk < 6; kk++) Am[j * 6 + kk] += alpha * (double)Am[i * 6 + kk];
                    bv[j] += alpha * (double)bv[i];
                }
            }
            if (ok)
                for (int i = 5; i >= 0; i--) {
                    double s = bv[i];
                    for (int k = i + 1; k < 6; k++) s -= (double)Am[i * 6 + k] * (double)bv[k];
                    bv[i] = s / (double)Am[i * 6 + i];
                }
            double M[6];
#pragma unroll
            for (int i = 0; i < 6; i++) M[i] = ok ? bv.get(i) : 0.0;
            // warpAffine inverts the map (no WARP_INVERSE_MAP)
            double D = M[0] * M[4] - M[1] * M[3];
            D = D != 0 ? 1. / D : 0;
            const double A11 = M[4] * D, A22 = M[0] * D;
            M[0] = A11; M[1] *= -D;
            M[3] *= -D; M[4] = A22;
            const double b1 = -M[0] * M[2] - M[1] * M[5];
            const double b2 = -M[3] * M[2] - M[4] * M[5];
            M[2] = b1; M[5] = b2;
#pragma unroll
            for (int i = 0; i < 6; i++) W.M[i] = M[i];
        }
        return degenerate;
    }
}

static constexpr int ICON_IMAGE_MAX = 256; // the largest side of icon_image's output (icon_strip_plan.h refuses more)

// One armour's icon at ow x oh (1 .. ICON_IMAGE_MAX each) by one wavefront: icon_row with the output extent as run-time values -- the same
// clamp, box, LU and inverse map (icon_setup), warp_px on demand, the same fixed-point resize with the scales bw / ow and bh / oh, the exact
// 2:1 box average when bw == 2 ow && bh == 2 oh.  An upscale (a 30-pixel box to 80 x 80) takes the same tap rule: the left clamp and the edge
// columns are monotone in dx for any scale.  put(o, res): called by the lane that owns output pixel o = dy * ow + dx; A is only read.
// (The labeler's rm::affine_correction(frame, tmp, armour.icon, {80, 80}), executable/svm/labeler.cpp:100)
template <int BAYER, class Put>
__device__ __forceinline__ void icon_image(const uint8_t* frame, int f, int lane, const rmcv_armour* A, int w, int h, int stride, int pattern, int lay,
                                           const uint8_t* luts, int ow, int oh, float ic[4][2], Put put)
{
    WarpCtx W;
    const bool degenerate = icon_setup<BAYER>(frame, f, lane, A, w, h, stride, pattern, lay, luts, ic, W);
    const int bw = W.bw, bh = W.bh;
    const bool area = (bw == 2 * ow && bh == 2 * oh);
    const double scale_x = (double)bw / ow, scale_y = (double)bh / oh;
    for (int o = lane; o < ow * oh; o += 64) {
        const int dy = o / ow, dx = o - dy * ow;
        int res[3] = {0, 0, 0};
        if (!degenerate) {
            if (area) {
                int p00[3], p01[3], p10[3], p11[3];
                warp_px<BAYER>(W, 2 * dx, 2 * dy, p00);
                warp_px<BAYER>(W, 2 * dx + 1, 2 * dy, p01);
                warp_px<BAYER>(W, 2 * dx, 2 * dy + 1, p10);
                warp_px<BAYER>(W, 2 * dx + 1, 2 * dy + 1, p11);
#pragma unroll
                for (int c = 0; c < 3; c++) res[c] = (p00[c] + p01[c] + p10[c] + p11[c] + 2) >> 2;
            } else {
                float fx = (float)((dx + 0.5) * scale_x - 0.5);
                int sx = cv_floor_f(fx);
                fx -= sx;
                if (sx < 0) { fx = 0; sx = 0; }
                bool edge = false; // dx >= xmax: single tap weighted 2048
                if (sx + 1 >= bw) {
                    edge = true;
                    if (sx >= bw - 1) { fx = 0; sx = bw - 1; }
                }
                const int a0 = (short)cv_round_f((1.f - fx) * 2048), a1 = (short)cv_round_f(fx * 2048);
                float fy = (float)((dy + 0.5) * scale_y - 0.5);
                const int sy = cv_floor_f(fy);
                fy -= sy;
                const int b0 = (short)cv_round_f((1.f - fy) * 2048), b1 = (short)cv_round_f(fy * 2048);
                int sy0 = sy, sy1 = sy + 1;
                sy0 = sy0 < 0 ? 0 : (sy0 > bh - 1 ? bh - 1 : sy0);
                sy1 = sy1 < 0 ? 0 : (sy1 > bh - 1 ? bh - 1 : sy1);
                int p00[3], p01[3] = {0, 0, 0}, p10[3], p11[3] = {0, 0, 0};
                warp_px<BAYER>(W, sx, sy0, p00);
                warp_px<BAYER>(W, sx, sy1, p10);
                if (!edge) {
                    warp_px<BAYER>(W, sx + 1, sy0, p01);
                    warp_px<BAYER>(W, sx + 1, sy1, p11);
                }
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const int r0 = edge ? p00[c] * 2048 : p00[c] * a0 + p01[c] * a1;
                    const int r1 = edge ? p10[c] * 2048 : p10[c] * a0 + p11[c] * a1;
                    const int v = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2;
                    res[c] = v < 0 ? 0 : (v > 255 ? 255 : v);
                }
            }
        }
        put(o, res);
    }
}

} // namespace rmcv
