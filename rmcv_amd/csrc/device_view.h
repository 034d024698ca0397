/*
 * device_view.h -- the operator's debug view of ONE frame, host and device from the same source:
 *     V = resize( draw_armours( draw_lightblobs( GRAY2BGR(binary) ) ), (vw, vh), INTER_LINEAR ),  8UC3
 *   the loop's debug image          executable/main.cpp:200-207, shown at 1024x768 by :90-100
 *   rm::debug::draw_lightblobs      src/debug.cpp:72-93
 *   rm::debug::draw_armours         src/debug.cpp:43-70   (cv::putText, :53-57, is NOT rendered: no glyph tables)
 * The OpenCV side is [OCV-recall] (4.8.0): Point2f -> Point, drawContours(thickness 1, LINE_8) -> ThickLine -> Line ->
 * LineIterator(leftToRight) behind clipLine, and the 8-bit INTER_LINEAR resize as device_classify.h states it for the icon.
 *
 * Here: the conversion of a vertex, the clip, the line iterator (every pixel handed to a functor: the host writes a BGR canvas in draw
 * order, the device sets bits of two colour planes), the colours, and the resize taps with their fixed-point mix.  Integer arithmetic
 * but for the clip's one double expression and the taps' float coefficients; compile with -ffp-contract=off, no fast-math.
 */
#ifndef RMCV_DEVICE_VIEW_H
#define RMCV_DEVICE_VIEW_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/rmcv_abi.h"

#if defined(__HIPCC__)
#define VIEW_FN __host__ __device__ static inline
#else
#define VIEW_FN static inline
#endif

/* colours as channel masks, bit 0 = B, 1 = G, 2 = R (every channel of the view's source is 0 or 255) */
#define VIEW_BLACK 0
#define VIEW_WHITE 7
#define VIEW_GREEN 2  /* (0, 255, 0):   a positive blob whose target is CAMP_RED, debug.cpp:82 */
#define VIEW_RED 4    /* (0, 0, 255):   every other positive blob                             */
#define VIEW_YELLOW 6 /* (0, 255, 255): negatives (:92), armours' vertices and icons (:69)    */
VIEW_FN int view_blob_colour(int32_t target) { return target == RMCV_CAMP_RED ? VIEW_GREEN : VIEW_RED; }

#define VIEW_COORD_LIMIT 1073741824 /* 2^30: an endpoint of this magnitude (or not finite) and its segment is skipped -- a recorded deviation */

/* cv::Point(Point2f) = cvRound per coordinate: round half to even.  0: the coordinate is not finite or too large (the segment is skipped) */
VIEW_FN int view_coord(float v, int* out)
{
    if (!(__builtin_fabsf(v) < (float)VIEW_COORD_LIMIT)) return 0; /* NaN compares false */
    *out = (int)__builtin_rintf(v);
    return 1;
}
VIEW_FN int view_coord_i(int32_t v) { return v > -VIEW_COORD_LIMIT && v < VIEW_COORD_LIMIT; }

/* cv::clipLine(Size, Point&, Point&) on 64-bit coordinates: Cohen-Sutherland codes, y first, then x; 0: nothing of the segment is inside */
VIEW_FN int view_clip_line(int w, int h, int64_t* px1, int64_t* py1, int64_t* px2, int64_t* py2)
{
    int64_t x1 = *px1, y1 = *py1, x2 = *px2, y2 = *py2;
    const int64_t right = (int64_t)w - 1, bottom = (int64_t)h - 1;
    if (w <= 0 || h <= 0) return 0;
    int c1 = (x1 < 0) + (x1 > right) * 2 + (y1 < 0) * 4 + (y1 > bottom) * 8;
    int c2 = (x2 < 0) + (x2 > right) * 2 + (y2 < 0) * 4 + (y2 > bottom) * 8;
    if ((c1 & c2) == 0 && (c1 | c2) != 0) {
        int64_t a;
        if (c1 & 12) {
            a = c1 < 8 ? 0 : bottom;
            x1 += (int64_t)((double)(a - y1) * (double)(x2 - x1) / (double)(y2 - y1));
            y1 = a;
            c1 = (x1 < 0) + (x1 > right) * 2;
        }
        if (c2 & 12) {
            a = c2 < 8 ? 0 : bottom;
            x2 += (int64_t)((double)(a - y2) * (double)(x2 - x1) / (double)(y2 - y1));
            y2 = a;
            c2 = (x2 < 0) + (x2 > right) * 2;
        }
        if ((c1 & c2) == 0 && (c1 | c2) != 0) {
            if (c1) {
                a = c1 == 1 ? 0 : right;
                y1 += (int64_t)((double)(a - x1) * (double)(y2 - y1) / (double)(x2 - x1));
                x1 = a;
                c1 = 0;
            }
            if (c2) {
                a = c2 == 1 ? 0 : right;
                y2 += (int64_t)((double)(a - x2) * (double)(y2 - y1) / (double)(x2 - x1));
                x2 = a;
                c2 = 0;
            }
        }
    }
    *px1 = x1; *py1 = y1; *px2 = x2; *py2 = y2;
    return (c1 | c2) == 0;
}

/* cv::LineIterator(img, p1, p2, 8, leftToRight = true) as Line() walks it: put(x, y) for each of its `count` pixels, in its order */
template <typename Put>
VIEW_FN void view_line(int w, int h, int x1, int y1, int x2, int y2, Put put)
{
    if ((unsigned)x1 >= (unsigned)w || (unsigned)x2 >= (unsigned)w || (unsigned)y1 >= (unsigned)h || (unsigned)y2 >= (unsigned)h) {
        int64_t a = x1, b = y1, c = x2, d = y2;
        if (!view_clip_line(w, h, &a, &b, &c, &d)) return; /* count = 0 */
        x1 = (int)a; y1 = (int)b; x2 = (int)c; y2 = (int)d;
    }
    int step_x = 1, step_y = 1;
    int dx = x2 - x1, dy = y2 - y1;
    if (dx < 0) { /* leftToRight: the endpoints swap, AFTER clipping */
        dx = -dx;
        dy = -dy;
        x1 = x2;
        y1 = y2;
    }
    if (dy < 0) {
        dy = -dy;
        step_y = -1;
    }
    const int vert = dy > dx;
    if (vert) {
        const int t = dx; dx = dy; dy = t;
    }
    int err = dx - (dy + dy);
    const int plus_delta = dx + dx, minus_delta = -(dy + dy), count = dx + 1;
    int x = x1, y = y1;
    for (int i = 0; i < count; i++) {
        put(x, y);
        const int mask = err < 0 ? -1 : 0;
        err += minus_delta + (plus_delta & mask);
        if (vert) {
            y += step_y;
            x += step_x & mask;
        } else {
            x += step_x;
            y += step_y & mask;
        }
    }
}

/* one edge of a polygon drawn by drawContours(thickness 1, LINE_8), from float vertices (a blob's, an armour's) or from contour points */
template <typename Put>
VIEW_FN void view_edge_f(int w, int h, const float* p, const float* q, Put put)
{
    int x1, y1, x2, y2;
    if (!view_coord(p[0], &x1) || !view_coord(p[1], &y1) || !view_coord(q[0], &x2) || !view_coord(q[1], &y2)) return;
    view_line(w, h, x1, y1, x2, y2, put);
}
template <typename Put>
VIEW_FN void view_edge_i(int w, int h, rmcv_point p, rmcv_point q, Put put)
{
    if (!view_coord_i(p.x) || !view_coord_i(p.y) || !view_coord_i(q.x) || !view_coord_i(q.y)) return;
    view_line(w, h, p.x, p.y, q.x, q.y, put);
}

/* ---- resize: cv::resize(src, dst, dsize, 0, 0, INTER_LINEAR) on 8UC3 ------------------------------------------------------------ */
VIEW_FN int view_floor_f(float v)
{
    const int i = (int)v;
    return i - (i > v);
}
VIEW_FN int view_round_f(float v) { return (int)__builtin_rintf(v); }

#define VIEW_COPY 0   /* equal size: a copy                                                        */
#define VIEW_AREA 1   /* exactly half in both directions: INTER_LINEAR becomes the 2x2 area mean   */
#define VIEW_LINEAR 2
VIEW_FN int view_resize_mode(int w, int h, int vw, int vh)
{
    if (vw == w && vh == h) return VIEW_COPY;
    if (w == 2 * vw && h == 2 * vh) return VIEW_AREA;
    return VIEW_LINEAR;
}

/* the two source positions of an output coordinate and their weights (short, 11 fractional bits) */
struct view_tap {
    int s0, s1, c0, c1;
};
/* horizontal: fx from (dx + 0.5) scale - 0.5; clamped at both ends, where one tap carries the whole weight */
VIEW_FN view_tap view_tap_x(int mode, int d, int n_src, int n_dst)
{
    view_tap t;
    if (mode == VIEW_COPY) { t.s0 = t.s1 = d; t.c0 = 2048; t.c1 = 0; return t; }
    if (mode == VIEW_AREA) { t.s0 = 2 * d; t.s1 = 2 * d + 1; t.c0 = t.c1 = 0; return t; }
    const double scale = (double)n_src / n_dst;
    float f = (float)((d + 0.5) * scale - 0.5);
    int s = view_floor_f(f);
    f -= s;
    if (s < 0) { f = 0; s = 0; }
    if (s >= n_src - 1) { f = 0; s = n_src - 1; } /* dx >= xmax: the single tap weighted 2048 */
    t.s0 = s;
    t.s1 = s + 1 < n_src ? s + 1 : s;
    t.c0 = (short)view_round_f((1.f - f) * 2048);
    t.c1 = (short)view_round_f(f * 2048);
    return t;
}
/* vertical: the rows clamp, the weights do not */
VIEW_FN view_tap view_tap_y(int mode, int d, int n_src, int n_dst)
{
    view_tap t;
    if (mode != VIEW_LINEAR) return view_tap_x(mode, d, n_src, n_dst);
    const double scale = (double)n_src / n_dst;
    float f = (float)((d + 0.5) * scale - 0.5);
    const int s = view_floor_f(f);
    f -= s;
    t.s0 = s < 0 ? 0 : (s > n_src - 1 ? n_src - 1 : s);
    t.s1 = s + 1 < 0 ? 0 : (s + 1 > n_src - 1 ? n_src - 1 : s + 1);
    t.c0 = (short)view_round_f((1.f - f) * 2048);
    t.c1 = (short)view_round_f(f * 2048);
    return t;
}
/* one channel of one output pixel from its four source values (row 0: p00 p01, row 1: p10 p11) */
VIEW_FN int view_mix(int mode, int p00, int p01, int p10, int p11, const view_tap& tx, const view_tap& ty)
{
    if (mode == VIEW_COPY) return p00;
    if (mode == VIEW_AREA) return (p00 + p01 + p10 + p11 + 2) >> 2;
    const int r0 = p00 * tx.c0 + p01 * tx.c1, r1 = p10 * tx.c0 + p11 * tx.c1;
    const int v = (((ty.c0 * (r0 >> 4)) >> 16) + ((ty.c1 * (r1 >> 4)) >> 16) + 2) >> 2;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

/* ---- the host side: what rmcv_debug_view / rmcv_debug_view_host refuse of their arguments (null: nothing), and the sequential restatement ---- */
#include <vector>

static inline const char* view_check_lists(int w, int h, int stride, const rmcv_lightblob* blobs, int n_blobs, const rmcv_point* neg_pts, const int32_t* neg_offs,
                             int n_neg, const rmcv_armour* armours, int n_armours, int flags, int vw, int vh, int out_stride)
{
    if (w < 1 || h < 1) return "the image needs w >= 1 and h >= 1";
    if (stride < w) return "stride < w";
    if (n_blobs < 0 || n_neg < 0 || n_armours < 0) return "negative list length";
    if ((n_blobs && !blobs) || (n_armours && !armours) || (n_neg && !neg_offs)) return "null list";
    if (flags < 0 || flags > RMCV_VIEW_ALL) return "unknown view flags";
    if (vw < 1 || vh < 1) return "the view needs vw >= 1 and vh >= 1";
    if (out_stride < 3 * (int64_t)vw) return "out_stride < 3 vw";
    if (n_neg) {
        if (neg_offs[0] < 0) return "negative contour offset";
        for (int i = 0; i < n_neg; i++)
            if (neg_offs[i + 1] < neg_offs[i]) return "contour offsets must not decrease";
        if (neg_offs[n_neg] > 0 && !neg_pts) return "null contour points";
    }
    return nullptr;
}

// what both sequential restatements share behind their canvas's initialisation: the draws on the full-resolution BGR canvas (3 w bytes a
// row) in the reference's call order, then the resize pixel by pixel
static inline void view_canvas_finish(std::vector<uint8_t>& canvas, int w, int h, const rmcv_lightblob* blobs, int n_blobs, const rmcv_point* neg_pts,
               const int32_t* neg_offs, int n_neg, const rmcv_armour* armours, int n_armours, int flags, int vw, int vh, uint8_t* out, int out_stride)
{
    int colour = VIEW_YELLOW;
    auto put = [&](int x, int y) {
        uint8_t* p = &canvas[((size_t)y * w + x) * 3];
        for (int c = 0; c < 3; c++) p[c] = (colour >> c & 1) ? 255 : 0;
    };
    const int nb = (flags & RMCV_VIEW_BLOBS) ? n_blobs : 0, nn = (flags & RMCV_VIEW_NEGATIVES) ? n_neg : 0;
    if (nb || nn) { // draw_lightblobs: debug.cpp:75
        for (int i = 0; i < nb; i++) {
            colour = view_blob_colour(blobs[i].target);
            for (int e = 0; e < 4; e++) view_edge_f(w, h, blobs[i].vertices[e], blobs[i].vertices[(e + 1) & 3], put);
        }
        colour = VIEW_YELLOW;
        for (int i = 0; i < nn; i++) {
            const int start = neg_offs[i], len = neg_offs[i + 1] - start;
            for (int e = 0; e < len; e++) view_edge_i(w, h, neg_pts[start + e], neg_pts[start + (e + 1 == len ? 0 : e + 1)], put);
        }
    }
    if ((flags & RMCV_VIEW_ARMOURS) && n_armours) { // draw_armours: debug.cpp:45
        colour = VIEW_YELLOW;
        for (int i = 0; i < n_armours; i++) {
            for (int e = 0; e < 4; e++) view_edge_f(w, h, armours[i].vertices[e], armours[i].vertices[(e + 1) & 3], put);
            for (int e = 0; e < 4; e++) view_edge_f(w, h, armours[i].icon[e], armours[i].icon[(e + 1) & 3], put);
        }
    }
    const int mode = view_resize_mode(w, h, vw, vh);
    for (int dy = 0; dy < vh; dy++) {
        const view_tap ty = view_tap_y(mode, dy, h, vh);
        for (int dx = 0; dx < vw; dx++) {
            const view_tap tx = view_tap_x(mode, dx, w, vw);
            for (int c = 0; c < 3; c++) {
                auto px = [&](int x, int y) { return (int)canvas[((size_t)y * w + x) * 3 + c]; };
                out[(size_t)dy * out_stride + 3 * dx + c] =
                    (uint8_t)view_mix(mode, px(tx.s0, ty.s0), px(tx.s1, ty.s0), px(tx.s0, ty.s1), px(tx.s1, ty.s1), tx, ty);
            }
        }
    }
}

// the sequential restatement: a full-resolution BGR canvas drawn in the reference's call order, then resized pixel by pixel
static inline void view_host(const uint8_t* binary, int w, int h, int stride, const rmcv_lightblob* blobs, int n_blobs, const rmcv_point* neg_pts,
               const int32_t* neg_offs, int n_neg, const rmcv_armour* armours, int n_armours, int flags, int vw, int vh, uint8_t* out, int out_stride)
{
    std::vector<uint8_t> canvas((size_t)3 * w * h);
    for (int y = 0; y < h; y++) // cvtColor(GRAY2BGR) of a 0 / 255 image (any other non-zero byte counts as 255)
        for (int x = 0; x < w; x++) {
            const uint8_t g = binary[(size_t)y * stride + x] ? 255 : 0;
            uint8_t* p = &canvas[((size_t)y * w + x) * 3];
            p[0] = p[1] = p[2] = g;
        }
    view_canvas_finish(canvas, w, h, blobs, n_blobs, neg_pts, neg_offs, n_neg, armours, n_armours, flags, vw, vh, out, out_stride);
}

// the source view's: the canvas starts as the BGR image itself (labeler.cpp:108 copies the camera frame), stride >= 3 w
static inline void source_view_host(const uint8_t* bgr, int w, int h, int stride, const rmcv_lightblob* blobs, int n_blobs, const rmcv_point* neg_pts,
               const int32_t* neg_offs, int n_neg, const rmcv_armour* armours, int n_armours, int flags, int vw, int vh, uint8_t* out, int out_stride)
{
    std::vector<uint8_t> canvas((size_t)3 * w * h);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < 3 * w; x++) canvas[(size_t)y * 3 * w + x] = bgr[(size_t)y * stride + x];
    view_canvas_finish(canvas, w, h, blobs, n_blobs, neg_pts, neg_offs, n_neg, armours, n_armours, flags, vw, vh, out, out_stride);
}

#endif /* RMCV_DEVICE_VIEW_H */
