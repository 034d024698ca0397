"""Independent restatement, in plain Python, of the two rules windowed detection adds (tests only; nothing under rmcv_amd/ imports it):
  * rm::utils::GetROI, the reference's src/core.cpp:224-263, statement by statement;
  * the effective origin of a window: x_eff = clamp(x, 0, frame_w - win_w) & ~15, y_eff = clamp(y, 0, frame_h - win_h).
Written from the reference's text and the contract, not from the library's code: float32 minima / maxima through numpy scalars, C's
int arithmetic as Python integers (the tests keep every value far from 2^31), (int) casts as truncation towards zero."""
import math

import numpy as np


def bounding_rect_f32(points):
    """cv::boundingRect on float points: minima and maxima in float, x = floor(min), w = floor(max) - x + 1; no points: the empty rect"""
    pts = np.asarray(points, np.float32).reshape(-1, 2)
    if len(pts) == 0:
        return 0, 0, 0, 0
    minx, miny = np.float32(pts[0, 0]), np.float32(pts[0, 1])
    maxx, maxy = minx, miny
    for px, py in pts[1:]:
        minx, maxx = min(minx, px), max(maxx, px)
        miny, maxy = min(miny, py), max(maxy, py)
    x, y = math.floor(float(minx)), math.floor(float(miny))
    return x, y, math.floor(float(maxx)) - x + 1, math.floor(float(maxy)) - y + 1


def get_roi(points, scale=(1.0, 1.0), frame_size=(-1, -1), previous=(0, 0, 0, 0)):
    """-> (x, y, w, h)"""
    x, y, w, h = bounding_rect_f32(points)
    x += int(previous[0])
    y += int(previous[1])
    sw, sh = float(np.float32(scale[0])), float(np.float32(scale[1]))       # cv::Size2f holds floats
    if sw != 1.0 or sh != 1.0:
        mw = int(float(w) * sw / 2.0)                                        # (int)((double)width * scaleFactor.width / 2.0)
        mh = int(float(h) * sh / 2.0)
        x -= mw
        y -= mh
        w += mw * 2
        h += mw * 2                                                          # core.cpp:238 adds scale.width to the height
    if x < 0:
        x = 0
    if y < 0:
        y = 0
    if x + w >= frame_size[0]:
        w = frame_size[0] - x - 1
    if y + h >= frame_size[1]:
        h = frame_size[1] - y - 1
    if w < 0 or h < 0:
        return 0, 0, 0, 0
    return x, y, w, h


def window_origin(rect, win_w, win_h):
    """the requested origin of a window centred on rect: centre minus half the window, C integer division (operands are not negative
    in the divisions: sizes)"""
    x, y, w, h = (int(v) for v in rect)
    return x + w // 2 - win_w // 2, y + h // 2 - win_h // 2


def effective_origin(x, y, frame_w, frame_h, win_w, win_h):
    xe = min(max(int(x), 0), frame_w - win_w)
    ye = min(max(int(y), 0), frame_h - win_h)
    return xe - xe % 16, ye


def effective_origins(origins, frame_w, frame_h, win_w, win_h):
    o = np.asarray(origins).reshape(-1, 2)
    return np.array([effective_origin(x, y, frame_w, frame_h, win_w, win_h) for x, y in o], np.int32).reshape(-1, 2)


def crop(frame, origin_eff, win_w, win_h):
    x, y = int(origin_eff[0]), int(origin_eff[1])
    return np.ascontiguousarray(frame[y:y + win_h, x:x + win_w])
