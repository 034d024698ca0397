// icon_host.h -- rm::affine_correction (src/imgproc.cpp:9-35) at any output size on the CPU, the strip of a frame's icons and the labeler's
// sheet (executable/svm/labeler.cpp:93-119) composed from it.  The sequential statement of the rule icon_image runs on the
// device (device_icon_image.h): clamp, integer box, getAffineTransform by a 6 x 6 LU with the first maximum as pivot, the inverted map,
// warpAffine INTER_LINEAR / BORDER_CONSTANT 0 of the box in OpenCV's fixed point, then resize INTER_LINEAR (the exact 2:1 case as the 2 x 2 box
// average) -- here as the reference runs it, the whole box warped first and resized afterwards.  Plain C++ without HIP types: a host compiler
// alone builds it (tests/icon_strip_san_main.cpp, the shim's rm::affine_correction).  Build with -ffp-contract=off: the map is double
// arithmetic that must not be contracted.
#pragma once

#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/rmcv_abi.h"
#include "device_view.h"

namespace rmcv {

inline int icon_round_d(double v) { return (int)nearbyint(v); } // cvRound: half to even (the default rounding mode)
inline int icon_round_f(float v) { return (int)nearbyintf(v); }
inline int icon_floor_f(float v) { int i = (int)v; return i - (i > v); }

// the clamped quadrilateral's integer box and the inverted map of its warp
struct IconMap {
    int bx, by, bw, bh;
    bool degenerate;
    double M[6];
};

// imgproc.cpp:11-28: icon is clamped in place to (w, h); the box; getAffineTransform of ([1], [2], [0]) -> ((0, 0), (bw, 0), (0, bh)), inverted
inline IconMap icon_map(float icon[4][2], int w, int h)
{
    IconMap m{};
    int minx = 0, maxx = 0, miny = 0, maxy = 0;
    for (int i = 0; i < 4; i++) {
        // std::max(0.0f, std::min(v, lim)): min(a, b) is b when b < a, max(a, b) is b when a < b -- so NaN and -0 both end as +0
        const float vx0 = icon[i][0], vy0 = icon[i][1];
        const float vx = (float)w - 1 < vx0 ? (float)w - 1 : vx0, vy = (float)h - 1 < vy0 ? (float)h - 1 : vy0;
        icon[i][0] = 0.0f < vx ? vx : 0.0f;
        icon[i][1] = 0.0f < vy ? vy : 0.0f;
        const int px = icon_round_f(icon[i][0]), py = icon_round_f(icon[i][1]);
        if (i == 0 || px < minx) minx = px;
        if (i == 0 || px > maxx) maxx = px;
        if (i == 0 || py < miny) miny = py;
        if (i == 0 || py > maxy) maxy = py;
    }
    m.bx = minx, m.by = miny, m.bw = maxx - minx + 1, m.bh = maxy - miny + 1;
    m.degenerate = m.bw <= 0 || m.bh <= 0 || m.bx < 0 || m.by < 0 || m.bx + m.bw > w || m.by + m.bh > h;
    const float src[3][2] = {{icon[1][0] - (float)m.bx, icon[1][1] - (float)m.by},
                             {icon[2][0] - (float)m.bx, icon[2][1] - (float)m.by},
                             {icon[0][0] - (float)m.bx, icon[0][1] - (float)m.by}};
    double a[6][6] = {}, b[6] = {0, 0, (double)(float)m.bw, 0, 0, (double)(float)m.bh};
    for (int i = 0; i < 3; i++) { // row 2i: [x y 1 0 0 0], row 2i + 1: [0 0 0 x y 1]
        a[2 * i][0] = a[2 * i + 1][3] = src[i][0];
        a[2 * i][1] = a[2 * i + 1][4] = src[i][1];
        a[2 * i][2] = a[2 * i + 1][5] = 1.0;
    }
    bool ok = true; // cv::solve(DECOMP_LU): partial pivoting, the first maximum; alpha = a[j][i] * (-1 / pivot)
    for (int i = 0; i < 6 && ok; i++) {
        int k = i;
        for (int j = i + 1; j < 6; j++)
            if (fabs(a[j][i]) > fabs(a[k][i])) k = j;
        if (fabs(a[k][i]) < DBL_EPSILON * 100) { ok = false; break; }
        if (k != i) {
            for (int j = i; j < 6; j++) { const double t = a[i][j]; a[i][j] = a[k][j]; a[k][j] = t; }
            const double t = b[i]; b[i] = b[k]; b[k] = t;
        }
        const double d = -1 / a[i][i];
        for (int j = i + 1; j < 6; j++) {
            const double alpha = a[j][i] * d;
            for (int kk = i + 1; kk < 6; kk++) a[j][kk] += alpha * a[i][kk];
            b[j] += alpha * b[i];
        }
    }
    if (ok)
        for (int i = 5; i >= 0; i--) {
            double s = b[i];
            for (int k = i + 1; k < 6; k++) s -= a[i][k] * b[k];
            b[i] = s / a[i][i];
        }
    double M[6];
    for (int i = 0; i < 6; i++) M[i] = ok ? b[i] : 0.0;
    // warpAffine inverts the map (no WARP_INVERSE_MAP)
    double D = M[0] * M[4] - M[1] * M[3];
    D = D != 0 ? 1. / D : 0;
    const double A11 = M[4] * D, A22 = M[0] * D;
    M[0] = A11; M[1] *= -D;
    M[3] *= -D; M[4] = A22;
    const double b1 = -M[0] * M[2] - M[1] * M[5];
    const double b2 = -M[3] * M[2] - M[4] * M[5];
    M[2] = b1; M[5] = b2;
    for (int i = 0; i < 6; i++) m.M[i] = M[i];
    return m;
}

// cv::warpAffine(roi, dst, M, roi.size()) INTER_LINEAR, BORDER_CONSTANT 0, CV_8UC3: the box's bw x bh pixels, 3 bw bytes a row
inline void icon_warp_box(const uint8_t* bgr, int stride, const IconMap& m, std::vector<uint8_t>& warped)
{
    const int AB_SCALE = 1 << 10, round_delta = 16, bw = m.bw, bh = m.bh;
    const uint8_t* roi = bgr + (size_t)m.by * stride + 3 * (size_t)m.bx;
    warped.assign((size_t)3 * bw * bh, 0);
    std::vector<int> adelta(bw), bdelta(bw);
    for (int x = 0; x < bw; x++) {
        adelta[x] = icon_round_d(m.M[0] * x * AB_SCALE);
        bdelta[x] = icon_round_d(m.M[3] * x * AB_SCALE);
    }
    for (int y = 0; y < bh; y++) {
        const int X0 = icon_round_d((m.M[1] * y + m.M[2]) * AB_SCALE) + round_delta;
        const int Y0 = icon_round_d((m.M[4] * y + m.M[5]) * AB_SCALE) + round_delta;
        for (int x = 0; x < bw; x++) {
            const int X = (X0 + adelta[x]) >> 5, Y = (Y0 + bdelta[x]) >> 5;
            int sx = X >> 5, sy = Y >> 5;
            sx = sx > 32767 ? 32767 : (sx < -32768 ? -32768 : sx);
            sy = sy > 32767 ? 32767 : (sy < -32768 ? -32768 : sy);
            const int fx = X & 31, fy = Y & 31;
            // the 2 x 2 weights of (fx, fy) / 32 in 2^15: the table entry's closed form (the one weight above a short is cut, the sum kept)
            int w00 = (32 - fx) * (32 - fy) * 32, w01 = fx * (32 - fy) * 32, w10 = (32 - fx) * fy * 32, w11 = fx * fy * 32;
            if (w00 > 32767) { w00 = 32767; w11 += 1; }
            const bool y0ok = sy >= 0 && sy < bh, y1ok = sy + 1 >= 0 && sy + 1 < bh;
            const bool x0ok = sx >= 0 && sx < bw, x1ok = sx + 1 >= 0 && sx + 1 < bw;
            for (int c = 0; c < 3; c++) {
                auto tap = [&](bool ok, int tx, int ty) { return ok ? (int)roi[(ptrdiff_t)ty * stride + 3 * tx + c] : 0; };
                const int v = (tap(y0ok && x0ok, sx, sy) * w00 + tap(y0ok && x1ok, sx + 1, sy) * w01 + tap(y1ok && x0ok, sx, sy + 1) * w10 +
                               tap(y1ok && x1ok, sx + 1, sy + 1) * w11 + (1 << 14)) >> 15;
                warped[((size_t)y * bw + x) * 3 + c] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
            }
        }
    }
}

// cv::resize(src, dst, {ow, oh}) INTER_LINEAR on CV_8UC3 (src: sw x sh pixels, 3 sw bytes a row)
inline void icon_resize(const std::vector<uint8_t>& src, int sw, int sh, int ow, int oh, uint8_t* out, int out_stride)
{
    auto at = [&](int x, int y, int c) { return (int)src[((size_t)y * sw + x) * 3 + c]; };
    if (sw == 2 * ow && sh == 2 * oh) { // the exact 2:1 case is computed as the 2 x 2 box average
        for (int dy = 0; dy < oh; dy++)
            for (int dx = 0; dx < ow; dx++)
                for (int c = 0; c < 3; c++)
                    out[(size_t)dy * out_stride + 3 * dx + c] =
                        (uint8_t)((at(2 * dx, 2 * dy, c) + at(2 * dx + 1, 2 * dy, c) + at(2 * dx, 2 * dy + 1, c) + at(2 * dx + 1, 2 * dy + 1, c) + 2) >> 2);
        return;
    }
    const double scale_x = (double)sw / ow, scale_y = (double)sh / oh;
    std::vector<int> xo(ow), xa0(ow), xa1(ow);
    for (int dx = 0; dx < ow; dx++) {
        float fx = (float)((dx + 0.5) * scale_x - 0.5);
        int sx = icon_floor_f(fx);
        fx -= sx;
        if (sx < 0) { fx = 0; sx = 0; }
        if (sx >= sw - 1) { fx = 0; sx = sw - 1; } // from xmax on: a single tap weighted 2048
        xo[dx] = sx;
        xa0[dx] = (short)icon_round_f((1.f - fx) * 2048);
        xa1[dx] = (short)icon_round_f(fx * 2048);
    }
    for (int dy = 0; dy < oh; dy++) {
        float fy = (float)((dy + 0.5) * scale_y - 0.5);
        const int sy = icon_floor_f(fy);
        fy -= sy;
        const int b0 = (short)icon_round_f((1.f - fy) * 2048), b1 = (short)icon_round_f(fy * 2048);
        const int sy0 = sy < 0 ? 0 : (sy > sh - 1 ? sh - 1 : sy), sy1 = sy + 1 < 0 ? 0 : (sy + 1 > sh - 1 ? sh - 1 : sy + 1);
        for (int dx = 0; dx < ow; dx++) {
            const int sx = xo[dx], sx1 = sx + 1 < sw ? sx + 1 : sw - 1; // (a clamped column's second tap has weight 0)
            for (int c = 0; c < 3; c++) {
                const int r0 = at(sx, sy0, c) * xa0[dx] + at(sx1, sy0, c) * xa1[dx];
                const int r1 = at(sx, sy1, c) * xa0[dx] + at(sx1, sy1, c) * xa1[dx];
                const int v = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2;
                out[(size_t)dy * out_stride + 3 * dx + c] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
            }
        }
    }
}

// rm::affine_correction(bgr, out, icon, {ow, oh}): icon is clamped in place; a degenerate box leaves `out` zero-filled.  Returns whether it was.
// Every argument has been checked by the caller (icon_strip_plan.h: affine_host_refusal).
inline bool icon_affine_host(const uint8_t* bgr, int w, int h, int stride, float icon[4][2], int ow, int oh, uint8_t* out, int out_stride)
{
    const IconMap m = icon_map(icon, w, h);
    if (m.degenerate) {
        for (int y = 0; y < oh; y++) memset(out + (size_t)y * out_stride, 0, (size_t)3 * ow);
        return true;
    }
    std::vector<uint8_t> warped;
    icon_warp_box(bgr, stride, m, warped);
    icon_resize(warped, m.bw, m.bh, ow, oh, out, out_stride);
    return false;
}

// labeler.cpp:93-106: the icons of armours 0 .. min(n, cap) - 1 side by side at columns [j side, (j + 1) side) of `side` rows of strip_w >=
// cap * side pixels; every other byte of the strip's 3 strip_w bytes a row is zero (the labeler's Mat::zeros; its uninitialised tail is not
// mirrored).  The armours are only read.  Returns the icons rendered.
inline int icon_strip_host(const uint8_t* bgr, int w, int h, int stride, const rmcv_armour* armours, int n, int side, int cap, int strip_w, uint8_t* out,
                           int out_stride)
{
    const int na = n < cap ? (n < 0 ? 0 : n) : cap;
    for (int y = 0; y < side; y++) memset(out + (size_t)y * out_stride, 0, (size_t)3 * strip_w);
    for (int j = 0; j < na; j++) {
        float ic[4][2];
        memcpy(ic, armours[j].icon, sizeof(ic));
        icon_affine_host(bgr, w, h, stride, ic, side, side, out + (size_t)3 * j * side, out_stride);
    }
    return na;
}

// labeler.cpp:113-119 at view size: the source view with `flags` | the plain binary as BGR (the debug view with flags 0) over the strip of
// cap = min(floor(2 vw / side), cap_most) icons: 2 vw x (vh + side) pixels.  Every argument has been checked by the caller.
inline void labeler_sheet_host(const uint8_t* bgr, int w, int h, int stride, const uint8_t* binary, int binary_stride, const rmcv_lightblob* blobs, int n_blobs,
                               const rmcv_point* neg_pts, const int32_t* neg_offs, int n_neg, const rmcv_armour* armours, int n_armours, int vw, int vh,
                               int side, int cap_most, int flags, uint8_t* out, int out_stride)
{
    source_view_host(bgr, w, h, stride, blobs, n_blobs, neg_pts, neg_offs, n_neg, armours, n_armours, flags, vw, vh, out, out_stride);
    view_host(binary, w, h, binary_stride, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, 0, vw, vh, out + (size_t)3 * vw, out_stride);
    const int fit = 2 * vw / side, cap = fit < cap_most ? fit : cap_most;
    icon_strip_host(bgr, w, h, stride, armours, n_armours, side, cap, 2 * vw, out + (size_t)vh * out_stride, out_stride);
}

} // namespace rmcv
