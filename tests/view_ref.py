"""The debug image of the reference's loop (executable/main.cpp:200-207, shown resized by :90-100), restated literally in numpy and plain
Python for the tests -- independent of rmcv_amd/csrc/device_view.h, with which it shares no code:
    V = resize( draw_armours( draw_lightblobs( GRAY2BGR(binary) ) ), (vw, vh), INTER_LINEAR )
It draws on a full-resolution BGR canvas in the reference's call order (src/debug.cpp:72-93, then 43-70; no putText), walks every line pixel
by pixel the way cv::LineIterator does behind cv::clipLine, and resizes in two separable passes, rows then columns, as cv::resize does for
8-bit images.  OpenCV 4.8.0 as recalled."""
import math

import numpy as np

from rmcv_amd.abi import CAMP_RED

GREEN, RED, YELLOW = (0, 255, 0), (0, 0, 255), (0, 255, 255)
VIEW_BLOBS, VIEW_NEGATIVES, VIEW_ARMOURS, VIEW_ALL = 1, 2, 4, 7
LIMIT = 2 ** 30


def to_point(x, y):
    """cv::Point(cv::Point2f): cvRound, half to even; None where the segment is to be skipped"""
    out = []
    for v in (x, y):
        v = float(np.float32(v))
        if not math.isfinite(v) or abs(v) >= LIMIT:
            return None
        n = math.floor(v)
        d = v - n
        if d > 0.5 or (d == 0.5 and n % 2 == 1):
            n += 1
        out.append(int(n))
    return tuple(out)


def clip_line(w, h, p1, p2):
    """cv::clipLine: (inside, p1, p2)"""
    x1, y1 = p1
    x2, y2 = p2
    right, bottom = w - 1, h - 1

    def code(x, y):
        return (x < 0) + (x > right) * 2 + (y < 0) * 4 + (y > bottom) * 8
    c1, c2 = code(x1, y1), code(x2, y2)
    if (c1 & c2) == 0 and (c1 | c2) != 0:
        if c1 & 12:
            a = 0 if c1 < 8 else bottom
            x1 += int(float(a - y1) * float(x2 - x1) / float(y2 - y1))
            y1 = a
            c1 = (x1 < 0) + (x1 > right) * 2
        if c2 & 12:
            a = 0 if c2 < 8 else bottom
            x2 += int(float(a - y2) * float(x2 - x1) / float(y2 - y1))
            y2 = a
            c2 = (x2 < 0) + (x2 > right) * 2
        if (c1 & c2) == 0 and (c1 | c2) != 0:
            if c1:
                a = 0 if c1 == 1 else right
                y1 += int(float(a - x1) * float(y2 - y1) / float(x2 - x1))
                x1 = a
                c1 = 0
            if c2:
                a = 0 if c2 == 1 else right
                y2 += int(float(a - x2) * float(y2 - y1) / float(x2 - x1))
                x2 = a
                c2 = 0
    return (c1 | c2) == 0, (x1, y1), (x2, y2)


def line_pixels(w, h, p1, p2):
    """the pixels cv::line(img, p1, p2, colour, 1, LINE_8) sets, in order: LineIterator(img, p1, p2, 8, leftToRight=True)"""
    inside = lambda p: 0 <= p[0] < w and 0 <= p[1] < h
    if not (inside(p1) and inside(p2)):
        ok, p1, p2 = clip_line(w, h, p1, p2)
        if not ok:
            return []
    dx, dy = p2[0] - p1[0], p2[1] - p1[1]
    if dx < 0:
        dx, dy, p1 = -dx, -dy, p2
    sy = 1
    if dy < 0:
        dy, sy = -dy, -1
    x, y = p1
    out = []
    if dy > dx:  # the major axis is y
        err, plus, minus = dy - 2 * dx, 2 * dy, -2 * dx
        for _ in range(dy + 1):
            out.append((x, y))
            neg = err < 0
            err += minus + (plus if neg else 0)
            y += sy
            x += 1 if neg else 0
    else:
        err, plus, minus = dx - 2 * dy, 2 * dx, -2 * dy
        for _ in range(dx + 1):
            out.append((x, y))
            neg = err < 0
            err += minus + (plus if neg else 0)
            x += 1
            y += sy if neg else 0
    return out


def draw_polygon(canvas, pts, colour):
    """drawContours(canvas, {pts}, -1, colour, 1): the closed polygon, edges j -> j + 1, last -> 0"""
    h, w, _ = canvas.shape
    n = len(pts)
    for j in range(n):
        a, b = pts[j], pts[(j + 1) % n]
        if a is None or b is None:
            continue
        for x, y in line_pixels(w, h, a, b):
            canvas[y, x] = colour


def int_point(p):
    x, y = int(p[0]), int(p[1])
    return None if abs(x) >= LIMIT or abs(y) >= LIMIT else (x, y)


def draw(binary, blobs, negatives, armours, flags=VIEW_ALL):
    """the full-resolution debug image, (h, w, 3) uint8 BGR"""
    g = np.where(np.asarray(binary) != 0, 255, 0).astype(np.uint8)
    canvas = np.stack([g, g, g], 2)  # cvtColor(GRAY2BGR)
    positive = list(blobs) if flags & VIEW_BLOBS else []
    negative = list(negatives) if flags & VIEW_NEGATIVES else []
    if positive or negative:  # draw_lightblobs, debug.cpp:75
        for lb in positive:
            draw_polygon(canvas, [to_point(v[0], v[1]) for v in lb["vertices"]], GREEN if int(lb["target"]) == CAMP_RED else RED)
        if negative:
            for c in negative:
                draw_polygon(canvas, [int_point(p) for p in c], YELLOW)
    if flags & VIEW_ARMOURS and len(armours):  # draw_armours, debug.cpp:45
        contours = []
        for ar in armours:
            contours.append([to_point(v[0], v[1]) for v in ar["vertices"]])
            contours.append([to_point(v[0], v[1]) for v in ar["icon"]])
        for c in contours:
            draw_polygon(canvas, c, YELLOW)
    return canvas


def cv_floor(f):
    return int(math.floor(float(f)))


def cv_round(f):
    return int(np.rint(np.float32(f)))


def resize_linear(src, vw, vh):
    """cv::resize(src, dst, (vw, vh), 0, 0, INTER_LINEAR) for 8UC3"""
    h, w, _ = src.shape
    if (vw, vh) == (w, h):
        return src.copy()
    s = src.astype(np.int32)
    if w == 2 * vw and h == 2 * vh:  # is_area_fast with both scales 2: the 2x2 mean
        return ((s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    scale_x, scale_y = w / vw, h / vh
    # horizontal pass over every source row: xofs, alpha, and xmax, from where on one tap carries ONE = 2048
    xofs, alpha, xmax = np.zeros(vw, np.int64), np.zeros((vw, 2), np.int32), vw
    for dx in range(vw):
        fx = np.float32((dx + 0.5) * scale_x - 0.5)
        sx = cv_floor(fx)
        fx = np.float32(fx - np.float32(sx))
        if sx < 0:
            fx, sx = np.float32(0), 0
        if sx + 1 >= w:
            xmax = min(xmax, dx)
            if sx >= w - 1:
                fx, sx = np.float32(0), w - 1
        xofs[dx] = sx
        alpha[dx] = cv_round(np.float32(np.float32(1) - fx) * np.float32(2048)), cv_round(fx * np.float32(2048))
    rows = np.empty((h, vw, 3), np.int32)
    body = slice(0, xmax)
    rows[:, body] = s[:, xofs[body]] * alpha[body, 0][None, :, None] + s[:, np.minimum(xofs[body] + 1, w - 1)] * alpha[body, 1][None, :, None]
    rows[:, xmax:] = s[:, xofs[xmax:]] * 2048
    # vertical pass
    out = np.empty((vh, vw, 3), np.uint8)
    for dy in range(vh):
        fy = np.float32((dy + 0.5) * scale_y - 0.5)
        sy = cv_floor(fy)
        fy = np.float32(fy - np.float32(sy))
        b0, b1 = cv_round(np.float32(np.float32(1) - fy) * np.float32(2048)), cv_round(fy * np.float32(2048))
        r0, r1 = rows[min(max(sy, 0), h - 1)], rows[min(max(sy + 1, 0), h - 1)]
        v = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2
        out[dy] = np.clip(v, 0, 255)
    return out


def view(binary, blobs, negatives, armours, size, flags=VIEW_ALL):
    """V at size = (vw, vh): (vh, vw, 3) uint8"""
    return resize_linear(draw(binary, blobs, negatives, armours, flags), int(size[0]), int(size[1]))
