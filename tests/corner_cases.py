"""The corner refinement's cases: one named list, used by the CPU tests, the sanitized program and the GPU tests alike.
Images of 96 x 80 and 160 x 128 with boards of 5 x 4 squares (12 inner corners) from rmcv_amd.synth.chessboard, guesses perturbed by up to
+-2.5 px from a fixed seed, and single-corner cases for every branch of the rule."""
import collections

import numpy as np

from rmcv_amd import synth

Case = collections.namedtuple("Case", "name image corners win zero max_iters eps")

# 9, 49, 81, 289, 961, 119 and 115 elements: below one wavefront, just below, a ragged second round, the reference's, the largest, rectangular
WINDOWS = [(1, 1), (3, 3), (4, 4), (8, 8), (15, 15), (8, 3), (2, 11)]
ZERO_ZONES = [(-1, -1), (0, 0), (2, 1)]

# The affine boards have integer coefficients and offsets at .5 / .0: every inner corner lies on a pixel centre or a pixel corner in each
# axis, so the rendered board is point-symmetric about it and the rule's fixed point is the analytic corner up to rounding (a box-sampled
# step edge at any other phase moves the fixed point by up to 0.1 px, which is the method's, not an error).
H_AFFINE_96 = [[14, 2, 14.5], [-1, 13, 16.0], [0, 0, 1]]
H_AFFINE_160 = [[24, 3, 20.5], [-2, 22, 25.0], [0, 0, 1]]
H_PERSP_160 = [[24.3, 3.1, 20.3], [-2.2, 22.4, 24.7], [2.0e-4, 3.0e-4, 1]]
H_EDGE_160 = [[20.2, 1.1, 5.2], [0.6, 19.3, 5.4], [0, 0, 1]]       # the board's corner 5 px from the image's top-left corner


def _boards():
    rng = np.random.default_rng(20241021)
    out = {}
    for name, (w, h, H) in (("affine96", (96, 80, H_AFFINE_96)), ("affine160", (160, 128, H_AFFINE_160)), ("persp160", (160, 128, H_PERSP_160)),
                            ("edge160", (160, 128, H_EDGE_160))):
        img, truth = synth.chessboard(w, h, H, 5, 4, ss=4, lo=40, hi=215)
        out[name] = (img, truth)
    img, truth = out["affine96"]
    noise = rng.integers(-6, 7, img.shape)
    out["noise96"] = (np.clip(img.astype(np.int64) + noise, 0, 255).astype(np.uint8), truth)
    out["flat96"] = (np.full((80, 96, 3), 128, np.uint8), np.zeros((0, 2)))
    return out, rng


BOARDS, _rng = _boards()
ACCURACY_BOARDS = ("affine96", "affine160")   # clean, affine: the refined corner is compared with the analytic one
IMAGES = {k: v[0] for k, v in BOARDS.items()}
TRUTH = {k: v[1] for k, v in BOARDS.items()}


def _guesses(name):
    t = TRUTH[name]
    return (t + _rng.uniform(-2.5, 2.5, t.shape)).astype(np.float32)


def _cases():
    cases = []
    for name in ("affine96", "affine160", "persp160", "edge160", "noise96"):
        g = _guesses(name)
        for win in WINDOWS:
            cases.append(Case("%s-win%dx%d" % (name, win[0], win[1]), name, g, win, (-1, -1), 40, 0.001))
    for name in ("affine96", "persp160"):
        g = _guesses(name)
        for win in ((3, 3), (8, 8), (8, 3), (2, 11), (15, 15)):
            for zero in ZERO_ZONES[1:]:
                if zero[0] < win[0] and zero[1] < win[1]:
                    cases.append(Case("%s-win%dx%d-zero%dx%d" % (name, win[0], win[1], zero[0], zero[1]), name, g, win, zero, 40, 0.001))
    t = TRUTH["affine96"]
    one = lambda x, y: np.array([[x, y]], np.float32)
    cases += [
        Case("flat-det-zero", "flat96", one(40.3, 30.7), (8, 8), (-1, -1), 40, 0.001),
        Case("far-flat-window", "affine160", one(TRUTH["affine160"][5][0] + 7.5, TRUTH["affine160"][5][1] + 7.5), (3, 3), (-1, -1), 40, 0.001),   # inside a square
        Case("reverted", "affine96", one(t[5][0] + 3.0, t[5][1] + 0.9), (3, 3), (-1, -1), 40, 0.001),
        Case("clamped-taps", "edge160", one(1.2, 1.4), (8, 8), (-1, -1), 40, 0.001),
        Case("leaves-image-far", "edge160", one(4.191999435424805, 12.5349702835083), (1, 1), (-1, -1), 40, 0.001),       # ... and is reverted
        Case("leaves-image-near", "noise96", one(6.418604373931885, 2.280351161956787), (3, 3), (-1, -1), 40, 0.001),      # ... by less than win: kept
        Case("nan", "affine96", np.array([[np.nan, 10.0], [12.0, np.inf]], np.float32), (8, 8), (-1, -1), 40, 0.001),
        Case("max-iters-1", "affine96", one(t[0][0] + 1.7, t[0][1] - 1.2), (8, 8), (-1, -1), 1, 0.001),
        Case("eps-0", "affine96", one(t[0][0] + 1.7, t[0][1] - 1.2), (8, 8), (-1, -1), 40, 0.0),
    ]
    return cases


CASES = _cases()
