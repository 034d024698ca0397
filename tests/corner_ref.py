"""numpy restatements of the corner refinement's rule, written from the text at the head of rmcv_amd/csrc/device_corner.h, not
from its code: (a) `subpix(..., pinned=True)`, the pinned summation order -- 64 partial sums, then the butterfly --, which
rmcv_corner_subpix_host has to equal byte for byte; (b) `pinned=False`, the same with OpenCV's sequential row-major double sums.  Every
float expression is float32 left to right (every constant an np.float32), every sum and the solve are Python floats (double)."""
import math

import numpy as np

F = np.float32
DET_ZERO, LEFT_IMAGE, REVERTED, CONVERGED, BAD_INPUT = 1 << 8, 1 << 9, 1 << 10, 1 << 11, 1 << 12
DBL_EPS = 2.0 ** -52


def gray(bgr):
    """(1868 B + 9617 G + 4899 R + 8192) >> 14"""
    b = bgr.astype(np.int64)
    return ((1868 * b[..., 0] + 9617 * b[..., 1] + 4899 * b[..., 2] + 8192) >> 14).astype(np.uint8)


def mask(win_x, win_y, zero=(-1, -1), exp=math.exp):
    """(win_h, win_w) float32; exp: the double exponential (the header's is pm_exp; the entries are rounded to float behind the product)"""
    win_w, win_h = 2 * win_x + 1, 2 * win_y + 1
    m = np.zeros((win_h, win_w), F)
    for i in range(win_h):
        y = F(i - win_y) / F(win_y)
        vy = exp(-float(y * y))
        for j in range(win_w):
            x = F(j - win_x) / F(win_x)
            m[i, j] = F(vy * exp(-float(x * x)))
    zx, zy = zero
    if zx >= 0 and zy >= 0:
        m[win_y - zy:win_y + zy + 1, win_x - zx:win_x + zx + 1] = 0
    return m


def _origin(f, extent):
    return int(min(max(f, F(-64)), F(extent + 64)))


def _sums(g, x, y, m, win_x, win_y, pinned):
    h, w = g.shape
    win_w, win_h = 2 * win_x + 1, 2 * win_y + 1
    cx, cy = x - F(win_w + 1) * F(0.5), y - F(win_h + 1) * F(0.5)
    fx, fy = np.floor(cx), np.floor(cy)
    a, b = cx - fx, cy - fy
    a = F(0.0001) if a < F(0.0001) else a
    one = F(1)
    a11, a12, a21, a22 = (one - a) * (one - b), a * (one - b), (one - a) * b, a * b
    ix, iy = _origin(fx, w), _origin(fy, h)
    cols = np.clip(ix + np.arange(win_w + 3), 0, w - 1)
    rows = np.clip(iy + np.arange(win_h + 3), 0, h - 1)
    s = g[np.ix_(rows, cols)].astype(F)
    p = s[:-1, :-1] * a11 + s[:-1, 1:] * a12 + s[1:, :-1] * a21 + s[1:, 1:] * a22      # (win_h + 2, win_w + 2), float32 left to right
    tgx = p[1:-1, 2:] - p[1:-1, :-2]
    tgy = p[2:, 1:-1] - p[:-2, 1:-1]
    gxx, gxy, gyy = tgx * tgx * m, tgx * tgy * m, tgy * tgy * m
    px = np.arange(-win_x, win_x + 1).astype(F)[None, :]
    py = np.arange(-win_y, win_y + 1).astype(F)[:, None]
    terms = np.stack([gxx, gxy, gyy, gxx * px + gxy * py, gxy * px + gyy * py]).reshape(5, -1)
    assert terms.dtype == F
    terms = terms.astype(np.float64)
    n = terms.shape[1]
    if not pinned:
        return [float(np.add.accumulate(np.concatenate(([0.0], t)))[-1]) for t in terms]  # ((0 + t0) + t1) + ..., row-major
    acc = np.zeros((5, 64))
    for r in range(0, n, 64):
        k = min(64, n - r)
        acc[:, :k] = acc[:, :k] + terms[:, r:r + k]
    lanes = np.arange(64)
    for sft in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ sft]
    return [float(v) for v in acc[:, 0]]


def subpix(bgr, corners, win, zero=(-1, -1), max_iters=40, eps=0.001, pinned=True, exp=math.exp):
    """-> (corners (n, 2) float32, status (n,) int32)"""
    with np.errstate(all="ignore"):  # (an iterate far outside the image may overflow a float: it has then left the image)
        return _subpix(bgr, corners, win, zero, max_iters, eps, pinned, exp)


def _subpix(bgr, corners, win, zero, max_iters, eps, pinned, exp):
    g = gray(np.asarray(bgr))
    h, w = g.shape
    win_x, win_y = win
    m = mask(win_x, win_y, zero, exp)
    out = np.array(corners, F).reshape(-1, 2)
    status = np.zeros(len(out), np.int32)
    eps2 = float(eps) * float(eps)
    for q in range(len(out)):
        x0, y0 = out[q]
        if not (np.isfinite(x0) and np.isfinite(y0)):
            status[q] = BAD_INPUT
            continue
        x, y, iters, st = x0, y0, 0, 0
        while True:
            iters += 1
            a, b, c, bb1, bb2 = _sums(g, x, y, m, win_x, win_y, pinned)
            det = a * c - b * b
            if not abs(det) > DBL_EPS * DBL_EPS:
                st |= DET_ZERO
                break
            scale = 1.0 / det
            nx = F(float(x) + c * scale * bb1 - b * scale * bb2)
            ny = F(float(y) - b * scale * bb1 + a * scale * bb2)
            dx, dy = nx - x, ny - y
            err = dx * dx + dy * dy
            x, y = nx, ny
            if not (x >= 0 and x < F(w) and y >= 0 and y < F(h)):
                st |= LEFT_IMAGE
                break
            if not float(err) > eps2:
                st |= CONVERGED
                break
            if iters >= max_iters:
                break
        if not abs(x - x0) <= F(win_x) or not abs(y - y0) <= F(win_y):
            x, y = x0, y0
            st |= REVERTED
        out[q] = (x, y)
        status[q] = iters | st
    return out, status
