"""The chessboard detector's cases: a seeded list of named frames drawn with synth.chessboard, each with its pattern, its
parameters and what is known of it beforehand -- whether a board is found and, where one is, its analytic inner corners in the order the rule
returns them (expected_order applies the rule's orientation choice to the analytic corners and insists on a margin, so that half a pixel of
detection error cannot change the choice).  Shared by the CPU tests, the sanitized program and the GPU tests; nothing here is changed by them.
Cases with gpu=False have frames beyond the 320 x 256 the GPU tests keep to."""
from collections import namedtuple

import numpy as np

from rmcv_amd import synth

Case = namedtuple("Case", "name image cols rows params analytic found clean gpu")
IMAGES, CASES = {}, []


def expected_order(analytic, cols, rows):
    """the analytic corners (row-major, rows x cols) in the right-handed orientation whose first corner has the smallest x + y"""
    G = np.asarray(analytic, np.float64).reshape(rows, cols, 2)
    options = []
    for swap in (False, True):
        grid = G.transpose(1, 0, 2) if swap else G
        if grid.shape[:2] != (rows, cols):
            continue
        for flip_i in (False, True):
            for flip_j in (False, True):
                g = grid[::-1 if flip_j else 1, ::-1 if flip_i else 1]
                a, b = g[0, 1] - g[0, 0], g[1, 0] - g[0, 0]
                if a[0] * b[1] - a[1] * b[0] > 0:
                    options.append((g[0, 0].sum(), g[0, 0, 1], g))
    options.sort(key=lambda o: o[:2])
    assert len(options) >= 2 and options[1][0] - options[0][0] > 6, "the orientation choice of this board has no margin"
    return np.ascontiguousarray(options[0][2].reshape(-1, 2))


def rot(angle, side, cx, cy, nx, ny):
    """squares of `side` pixels rotated by `angle` about the board's middle, which lands on (cx, cy)"""
    c, s = np.cos(angle) * side, np.sin(angle) * side
    return [[c, -s, cx - (c * nx - s * ny) / 2], [s, c, cy - (s * nx + c * ny) / 2], [0, 0, 1]]


def add(name, w, h, H, cols, rows, noise=0, seed=0, found=True, params=None, crop=None, gpu=None):
    img, an = synth.chessboard(w, h, H, cols + 1, rows + 1)
    if crop:
        img, w, h = np.ascontiguousarray(img[:crop[1], :crop[0]]), crop[0], crop[1]
    if noise:
        rng = np.random.default_rng(seed)
        img = np.clip(img.astype(np.int64) + rng.integers(-noise, noise + 1, img.shape), 0, 255).astype(np.uint8)   # (each channel its own)
    IMAGES[name] = img
    CASES.append(Case(name, name, cols, rows, dict(params or {}), expected_order(an, cols, rows) if found else None, found, found and not noise,
                      (w <= 320 and h <= 256) if gpu is None else gpu))
    return img, an


P1 = [[30, 2, 40.5], [1, 28, 30.5], [.0006, .0004, 1]]
P2 = [[30, 4, 60.5], [-3, 26, 50.5], [.0015, .0008, 1]]
SHEAR = [[18, 0.3 * 18, 30.5], [0, 18, 30.5], [0, 0, 1]]

# the boards the rule was prototyped on
add("upright-5x4", 160, 128, [[20, 0, 20.5], [0, 20, 14.5], [0, 0, 1]], 5, 4)
add("rot0.17-5x4", 160, 128, rot(0.17, 18, 80.2, 64.4, 6, 5), 5, 4)
add("rot0.52-5x4", 200, 200, rot(0.52, 18, 100.3, 99.1, 6, 5), 5, 4)
add("rot1.4-5x4", 200, 200, rot(1.4, 18, 100.3, 99.1, 6, 5), 5, 4)
add("shear0.3-5x4", 200, 160, SHEAR, 5, 4)
add("persp1-8x6", 320, 256, P1, 8, 6)
add("persp1-8x6-noise8", 320, 256, P1, 8, 6, noise=8, seed=11)
add("persp2-8x6", 400, 320, P2, 8, 6)
add("rot0.7-6x6", 240, 240, rot(0.7, 20, 120.4, 119.7, 7, 7), 6, 6)
add("squares13-11x8", 176, 128, [[13, 0, 10.5], [0, 13, 5.5], [0, 0, 1]], 11, 8)
add("squares14-11x8-noise6", 200, 160, [[14, 0, 16.5], [0, 14, 17.0], [0, 0, 1]], 11, 8, noise=6, seed=12)
add("persp2-8x6-cropped", 400, 320, P2, 8, 6, found=False, crop=(320, 256))          # one corner lost: 47 candidates
# the smallest and the longest pattern, a small square one, a half turn, a mirror image
add("upright-2x2", 160, 128, [[24, 0, 44.5], [0, 24, 28.0], [0, 0, 1]], 2, 2)
# (two rows of 11-pixel squares: the knight's segment from one row to the other passes the edge test there, so the distance range excludes it)
add("long-32x2", 320, 256, rot(0.6, 11, 160.3, 128.4, 33, 3), 32, 2, params=dict(dist_max=14))
add("rot0.3-4x4", 160, 160, rot(0.3, 20, 80.3, 79.6, 5, 5), 4, 4)
add("rot3.14-5x4", 200, 160, rot(np.pi, 18, 100.3, 80.2, 6, 5), 5, 4)
add("mirror-5x4", 200, 160, [[-18, 2, 160.5], [1, 18, 30.5], [0, 0, 1]], 5, 4)
# a board with one corner, its rightmost, in the border where R is 0: 19 candidates
add("corner-outside-5x4", 160, 128, rot(0.3, 18, 116.2, 64.4, 6, 5), 5, 4, found=False)


def two_boards():
    """two 3 x 3 boards side by side, the right one higher: its first candidate comes first in row-major order, so it is the board"""
    left, _ = synth.chessboard(160, 128, [[20, 0, 40.5], [0, 20, 34.5], [0, 0, 1]], 4, 4)
    right, an = synth.chessboard(160, 128, [[20, 0, 30.5], [0, 20, 14.5], [0, 0, 1]], 4, 4)
    IMAGES["two-boards-3x3"] = np.ascontiguousarray(np.concatenate([left, right], axis=1))
    CASES.append(Case("two-boards-3x3", "two-boards-3x3", 3, 3, {}, expected_order(an + [160.0, 0.0], 3, 3), True, True, True))


two_boards()
IMAGES["blank"] = np.full((128, 160, 3), 215, np.uint8)
CASES.append(Case("blank", "blank", 5, 4, {}, None, False, False, True))
IMAGES["noise"] = np.random.default_rng(13).integers(0, 256, (256, 320, 3), dtype=np.uint8)
CASES.append(Case("noise-overflow", "noise", 5, 4, dict(threshold=0, nms=1), None, False, False, True))
# the same board through other parameters: a wide suppression window, a tight distance range that still holds its 20-pixel squares
CASES.append(Case("upright-5x4-nms7", "upright-5x4", 5, 4, dict(nms=7, dist_min=15, dist_max=25, contrast=40), CASES[0].analytic, True, True, True))
CASES.append(Case("upright-5x4-too-far", "upright-5x4", 5, 4, dict(dist_max=19), None, False, False, True))
CASES.append(Case("upright-5x4-as-4x5", "upright-5x4", 4, 5, {}, expected_order(synth.chessboard(160, 128, [[0, 20, 20.5], [20, 0, 14.5], [0, 0, 1]], 5, 6)[1], 4, 5),
                  True, True, True))

# clean affine boards by the corner refinement's recipe (tests/corner_cases.py: integer coefficients, offsets at .5 / .0, squares >= 14 px): after
# find -> refine the corners lie within the refinement's bound of the analytic ones
ACCURACY_BOUND = 0.0081
add("affine96-4x3", 96, 80, [[14, 2, 14.5], [-1, 13, 16.0], [0, 0, 1]], 4, 3)
add("affine160-4x3", 160, 128, [[24, 3, 20.5], [-2, 22, 25.0], [0, 0, 1]], 4, 3)
add("affine200-11x8", 200, 160, [[14, 1, 10.5], [-1, 14, 28.0], [0, 0, 1]], 11, 8)
ACCURACY = ("affine96-4x3", "affine160-4x3", "affine200-11x8")
ACCURACY_WINDOWS = ((8, 8), (5, 5))

BY_NAME = {c.name: c for c in CASES}
