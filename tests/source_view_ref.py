"""The labeler's picture (executable/svm/labeler.cpp:108-111: the camera frame copied, armours and light blobs drawn on it), resized as the
loop's debug thread resizes its image -- the source view of DESIGN.md 4p, restated for the tests independently of rmcv_amd/csrc:
    S = resize( draw_armours( draw_lightblobs( SRC ) ), (vw, vh), INTER_LINEAR )
canvas = SRC.copy(), then tests/view_ref.py's polygons in the order its draw() has, then its resize.  SRC of a batch's frame is composed from
the references the other contracts already have: bayer_ref / raw_ref (D(T(r))), enhance_ref (E(f)), window_ref (the crop)."""
import numpy as np

import bayer_ref as BR
import enhance_ref as ER
import raw_ref as RR
import view_ref as R
import window_ref as WR
from rmcv_amd.abi import CAMP_RED

VIEW_BLOBS, VIEW_NEGATIVES, VIEW_ARMOURS, VIEW_ALL = R.VIEW_BLOBS, R.VIEW_NEGATIVES, R.VIEW_ARMOURS, R.VIEW_ALL


def draw(src, blobs, negatives, armours, flags=VIEW_ALL):
    """the full-resolution picture, (h, w, 3) uint8 BGR: a set overlay pixel replaces the source pixel"""
    canvas = np.array(src, np.uint8, copy=True)
    assert canvas.ndim == 3 and canvas.shape[2] == 3
    positive = list(blobs) if flags & VIEW_BLOBS else []
    negative = list(negatives) if flags & VIEW_NEGATIVES else []
    if positive or negative:  # draw_lightblobs, debug.cpp:75
        for lb in positive:
            R.draw_polygon(canvas, [R.to_point(v[0], v[1]) for v in lb["vertices"]], R.GREEN if int(lb["target"]) == CAMP_RED else R.RED)
        for c in negative:
            R.draw_polygon(canvas, [R.int_point(p) for p in c], R.YELLOW)
    if flags & VIEW_ARMOURS and len(armours):  # draw_armours, debug.cpp:45: per armour `vertices`, then `icon`
        for ar in armours:
            R.draw_polygon(canvas, [R.to_point(v[0], v[1]) for v in ar["vertices"]], R.YELLOW)
            R.draw_polygon(canvas, [R.to_point(v[0], v[1]) for v in ar["icon"]], R.YELLOW)
    return canvas


def view(src, blobs, negatives, armours, size, flags=VIEW_ALL):
    """S at size = (vw, vh): (vh, vw, 3) uint8"""
    return R.resize_linear(draw(src, blobs, negatives, armours, flags), int(size[0]), int(size[1]))


# ---- SRC(f) of a batch's frame, by what the batch is ----
def src_bgr(frame):
    return np.asarray(frame, np.uint8)


def src_bayer(delivered, pattern, valid_bit=0, mirror=False, flip=False):
    """D(T(r)): `pattern` is the buffer's as delivered (what the context is told)"""
    m = RR.T(delivered, valid_bit, mirror, flip)
    h, w = m.shape
    return BR.demosaic(m, RR.derived_pattern(pattern, w, h, mirror, flip))


def src_enhanced(frame, max_gain=100.0, min_gain=50.0):
    """(E(f), the frame's table)"""
    g = ER.gamma_of(frame, max_gain, min_gain)
    table = ER.lut(g)
    return table[frame], table


def src_window(frame, origin, win_w, win_h):
    h, w, _ = frame.shape
    return WR.crop(frame, WR.effective_origin(origin[0], origin[1], w, h, win_w, win_h), win_w, win_h)
