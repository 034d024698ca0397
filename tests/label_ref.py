"""The label pass over a finished view, restated in numpy and plain Python for the tests from the text of include/rmcv_abi.h
("view labels") -- placement, scaling, clipping and the two-phase order.  It shares no code with rmcv_amd/csrc/device_text.h: it takes
only the glyph rows and the strings from the library (the strings have their own independent reference, Python's "%f"); a vertex's rounding,
the clip and the line iterator are tests/view_ref.py's literal restatements of OpenCV's."""
import numpy as np

import view_ref as VR

YELLOW, MAGENTA = (0, 255, 255), (255, 0, 255)


def floor_div(a, b):
    return a // b   # Python's // is the true floor for negatives


def anchor(vertex, origin, w, h, vw, vh):
    """a float vertex -> its view position, or None where it is not drawable"""
    p = VR.to_point(vertex[0], vertex[1])
    if p is None:
        return None
    return floor_div((p[0] - origin[0]) * vw, w), floor_div((p[1] - origin[1]) * vh, h)


def blit(img, text, at, scale, colour, glyph):
    """text with its bottom-left at `at`: a set bit of character k at column c, row r fills the scale x scale block at
    x = ax + (6 k + c) scale, y = ay - (7 - r) scale; clipped; only set bits write.  glyph(ch) -> 7 row bytes, the left column in bit 4"""
    vh, vw, _ = img.shape
    ax, ay = at
    for k, ch in enumerate(text):
        rows = glyph(ch)
        for r in range(7):
            for c in range(5):
                if not (int(rows[r]) >> (4 - c)) & 1:
                    continue
                x0, y0 = ax + (6 * k + c) * scale, ay - (7 - r) * scale
                xa, xb, ya, yb = max(x0, 0), min(x0 + scale, vw), max(y0, 0), min(y0 + scale, vh)
                if xa < xb and ya < yb:
                    img[ya:yb, xa:xb] = colour


def labels(view, geometry, scale, armours, armour_texts, track_texts, sides, origin, glyph):
    """view: (vh, vw, 3) uint8, drawn in place and returned.  armour_texts / track_texts: the lines, one per armour / track"""
    vh, vw, _ = view.shape
    w, h = geometry
    for text, quad in zip(track_texts, sides):   # everything of the tracks first
        pts = [anchor(v, origin, w, h, vw, vh) for v in quad]
        if all(p is not None for p in pts):
            for j in range(4):
                for x, y in VR.line_pixels(vw, vh, pts[j], pts[(j + 1) % 4]):
                    view[y, x] = MAGENTA
        if pts[0] is not None:
            blit(view, text, pts[0], scale, MAGENTA, glyph)
    for text, a in zip(armour_texts, armours):   # then the armours' lines
        at = anchor(a["vertices"][0], (0, 0), w, h, vw, vh)
        if at is not None:
            blit(view, text, at, scale, YELLOW, glyph)
    return view


def texts_of(case):
    """the lines of a case of tests/label_cases.py, from the library: (one per armour, one per track)"""
    import rmcv_amd
    n = len(case["armours"])
    ids = case["identities"] if case["identities"] is not None else [-1] * n
    pos = case["positions"] if case["positions"] is not None else [None] * n
    return ([rmcv_amd.label_text(int(ids[i]), pos[i]) for i in range(n)],
            [rmcv_amd.track_label_text(case["tracks"][t:t + 1]) for t in range(len(case["tracks"]))])


def expected(case, scale):
    """(the flat buffer the pass must leave of a case's background, the one it started from)"""
    import label_cases as K
    import rmcv_amd
    stride = case["stride"]
    start = K.background(stride)
    want = start.copy()
    img = K.rows_of(want, stride).reshape(K.VH, K.VW, 3).copy()
    at, tt = texts_of(case)
    labels(img, case["geometry"], scale, case["armours"], at, tt, case["side"], case["origin"], rmcv_amd.view_glyph)
    K.rows_of(want, stride)[:] = img.reshape(K.VH, 3 * K.VW)
    return want, start
