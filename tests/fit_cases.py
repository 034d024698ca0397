"""Seeded contours for every branch of fit_ellipse_wave (rmcv_amd/csrc/wave_detect.h), shared by tests/test_fit_cases_cpu.py (the oracle's
branch census: every case reaches the branch it is named for), tests/test_gpu_fit_cases.py (the device through every call site of the fit
against the oracle's bytes), tests/fit_unit_cases.py (the scalar tails' inputs harvested from these fits) and tests/fit_ref.py.

A case is a point list -- cv::fitEllipseDirect takes any point list of six or more points, a border or not -- or a binary image whose
external borders are the contours.  Everything is deterministic: no random numbers at all.

`expect` names census counters of oracle/rmcv_oracle.c (orc_census_read) that the case's fit must increment, `path` what
orc_fit_ellipse_direct returns (0: the direct solution, 1: the general fit).  The 2^24 branch of the device has no counterpart in the
oracle (whose sums are the reference's sequential ones); its cases carry `sums`, the relation of their coordinate sums to 2^24, which the
CPU test checks on the points themselves."""
import math
from collections import namedtuple

import numpy as np

POINT = np.dtype([("x", "<i4"), ("y", "<i4")])
TWO24 = 1 << 24

Case = namedtuple("Case", "name pts path expect sums")
ImageCase = namedtuple("ImageCase", "name mask expect")


def P(xy):
    a = np.zeros(len(xy), POINT)
    a["x"] = [int(p[0]) for p in xy]
    a["y"] = [int(p[1]) for p in xy]
    return a


def ellipse_samples(n, cx, cy, a, b, deg):
    """n samples of an ellipse's outline, rounded to the pixel grid, in order of the parameter (duplicates stay: a contour may repeat points)"""
    th = math.radians(deg)
    t = np.arange(n) * (2.0 * math.pi / n)
    x = cx + a * np.cos(t) * math.cos(th) - b * np.sin(t) * math.sin(th)
    y = cy + a * np.cos(t) * math.sin(th) + b * np.sin(t) * math.cos(th)
    return P(list(zip(np.rint(x).astype(np.int64), np.rint(y).astype(np.int64))))


def rect_border(x0, y0, w, h):
    """the closed outer border of a filled w x h rectangle, 2 (w + h) - 4 points, walked down the left side first"""
    pts = [(x0, y) for y in range(y0, y0 + h)] + [(x, y0 + h - 1) for x in range(x0 + 1, x0 + w)]
    pts += [(x0 + w - 1, y) for y in range(y0 + h - 2, y0 - 1, -1)] + [(x, y0) for x in range(x0 + w - 2, x0, -1)]
    return P(pts)


def zigzag_bar(n, x0, y0):
    """n points of a two-pixel-wide vertical bar, alternating between its columns: aspect far beyond 30 for n >= 127, so the general fit"""
    return P([(x0 + (i & 1), y0 + i // 2) for i in range(n)])


def with_sum_x(base, total):
    """the point list `base` moved along x so that its coordinate sum is exactly `total`: a common shift, then +1 on the first few points"""
    n = len(base)
    s0 = int(base["x"].astype(np.int64).sum())
    shift = (total - s0) // n
    p = base.copy()
    p["x"] += shift
    rem = total - int(p["x"].astype(np.int64).sum())
    assert 0 <= rem < n
    p["x"][:rem] += 1
    assert int(p["x"].astype(np.int64).sum()) == total
    return p


def swap_xy(p):
    q = p.copy()
    q["x"], q["y"] = p["y"], p["x"]
    return q


# the chunk edges of seq_sum_terms / seq_sum_terms2 (64 points) and seq_sum_products_two (32 points), the smallest contour the gate
# admits, and one beyond 2048
COUNTS = (6, 7, 31, 32, 33, 63, 64, 65, 127, 128, 129, 2500)


def point_cases():
    c = []

    def add(name, pts, path, expect, sums=None):
        c.append(Case(name, pts, path, tuple(expect), sums))

    # ---- direct path, first attempt, at every point count
    # (the scaled coordinates are 100 (x - cx) / s with s ~ n times the size, so the 3 x 3 determinant falls with the twelfth power of n,
    # whatever the size: 3e-6 .. 1.5e-9 for these outlines up to 129 points, 1e-22 at 2 500.  Neither attempt can pass |det| > 1e-10
    # beyond 2048 points, so the long outline of this list belongs to the general path, below.)
    for n in COUNTS:
        if n < 2048:
            add("direct_first_n%d" % n, ellipse_samples(n, 700, 600, 40, 15, 17), 0, ["direct_attempt0"])
    for deg in (0, 60, 90, 133):
        add("direct_first_tilt%d" % deg, ellipse_samples(60, 300, 200, 30, 10, deg), 0, ["direct_attempt0"])
    add("direct_first_circle", ellipse_samples(48, 50, 50, 12, 12, 0), 0, ["direct_attempt0"])
    add("direct_good_box_bar4", rect_border(100, 100, 4, 60), 0, ["direct_attempt0", "direct_swap"])
    add("direct_square_pv1_zero", rect_border(100, 100, 5, 5), 0, ["direct_attempt0", "theta_pv1_zero_0"])
    # ---- direct path, jittered attempt: two adjacent rows of 20 points (det0 = 2.9e-18, det1 = 1e-4); the box is wild -> general fit
    add("direct_jittered_two_rows", P([(x, 50) for x in range(20)] + [(x, 51) for x in range(19, -1, -1)]), 1,
        ["direct_attempt1", "direct_bad_box", "general_no_retry"])
    add("direct_jittered_diagonal", P([(x, x + 3) for x in range(20)]), 1, ["direct_attempt1", "direct_bad_box", "general_jitter_retry"])
    # ---- neither attempt (the determinant is NaN or tiny both times)
    add("direct_none_collinear_horizontal", P([(x, 50) for x in range(10, 30)]), 1, ["direct_none", "general_jitter_retry"])
    add("direct_none_all_equal", P([(7, 9)] * 12), 1, ["direct_none", "centre_det_zero", "finish_rp2_below", "finish_rp3_below"])
    add("direct_none_bar3", rect_border(100, 100, 3, 200), 1, ["direct_none", "general_no_retry", "general_no_swap"])
    add("direct_none_bar2", rect_border(100, 100, 2, 90), 1, ["direct_none", "general_no_retry", "general_swap"])
    # ---- a first attempt whose box is wild (aspect beyond 30): the general fit replaces it
    add("direct_wild_box", P([(x + 20, (x * x * x) // 4 + 200) for x in range(-9, 8)]), 1, ["direct_attempt0", "direct_bad_box"])
    # ---- a jittered attempt whose box is good: a row of 12 points and one point beside it
    add("direct_jittered_good_box", P([(x, 50) for x in range(12)] + [(5, 51)]), 0, ["direct_attempt1"])
    # ---- the eigenvector choice of direct_finish: the THIRD vector has the largest 4ac - b^2 (found by a seeded search over small lists)
    add("direct_cond_pick2", P([(9, 6), (4, 10), (4, 10), (8, 7), (7, 5), (8, 7)]), 1, ["direct_attempt0", "cond_pick2", "direct_bad_box"])
    add("direct_none_n2500", ellipse_samples(2500, 700, 600, 400, 150, 17), 1, ["direct_none", "general_fit"])
    # ---- general path at every point count (par_sum_products / normal_refine: lane-strided sums, n below, at and above 64)
    for n in COUNTS:
        add("general_n%d" % n, zigzag_bar(n, 100, 50) if n > 6 else P([(x, 50) for x in range(6)]), 1, ["general_fit"])
    # ---- coordinate sums: the 2^24 branch (general fit: the float centroid; direct fit: seq_sum_terms in place of the paired walk)
    bar = rect_border(5990, 10, 20, 1482)              # 3000 points, aspect 74: the general fit
    ell = ellipse_samples(129, 140000, 300, 40, 15, 30)   # the direct solution: a small outline far out (the entry points take any int32)
    add("sum_x_over_general", bar, 1, ["general_fit"], ("over", "under"))
    add("sum_y_over_general", swap_xy(bar), 1, ["general_fit"], ("under", "over"))
    add("sum_both_over_general", rect_border(5990, 5800, 20, 1482), 1, ["general_fit"], ("over", "over"))
    add("sum_x_over_direct", ell, 0, ["direct_attempt0"], ("over", "under"))
    add("sum_y_over_direct", swap_xy(ell), 0, ["direct_attempt0"], ("under", "over"))
    add("sum_both_over_direct", ellipse_samples(129, 140000, 150000, 40, 15, 30), 0, ["direct_attempt0"], ("over", "over"))
    thin = rect_border(0, 10, 6, 1000)                 # 2008 points, aspect 167
    add("sum_x_2p24_minus_1_general", with_sum_x(thin, TWO24 - 1), 1, ["general_fit"], ("last_under", "under"))
    add("sum_x_2p24_general", with_sum_x(thin, TWO24), 1, ["general_fit"], ("first_over", "under"))
    small = ellipse_samples(128, 0, 300, 40, 15, 40)
    add("sum_x_2p24_minus_1_direct", with_sum_x(small, TWO24 - 1), 0, ["direct_attempt0"], ("last_under", "under"))
    add("sum_x_2p24_direct", with_sum_x(small, TWO24), 0, ["direct_attempt0"], ("first_over", "under"))
    return c


# the degenerate results (zero width: ratio = inf; 0 / 0: ratio = NaN) by name: what goes through the gates with ratio_hi = +inf
DEGENERATE = ("direct_none_collinear_horizontal", "direct_none_all_equal", "direct_jittered_two_rows")


def _disc(mask, cx, cy, a, b, deg):
    h, w = mask.shape
    yy, xx = np.mgrid[0:h, 0:w]
    th = math.radians(deg)
    u = (xx - cx) * math.cos(th) + (yy - cy) * math.sin(th)
    v = -(xx - cx) * math.sin(th) + (yy - cy) * math.cos(th)
    mask[(u / a) ** 2 + (v / b) ** 2 <= 1.0] = 255


def shapes_mask():
    """one small frame of real borders: discs of several tilts (direct fits; the tall pairs make armours), bars two to four pixels wide
    (general fits, a good direct box), one-pixel lines (collinear borders walked there and back), specks below the six-point gate"""
    m = np.zeros((240, 480), np.uint8)
    for k, x in enumerate((40, 110, 180, 250)):   # two pairs of tall light bars
        _disc(m, x, 70, 7, 30, 3 if k & 1 else -2)
    _disc(m, 330, 60, 40, 12, 25)
    _disc(m, 420, 70, 20, 20, 0)
    _disc(m, 60, 180, 35, 6, 160)
    m[130:230, 140:142] = 255                    # 2 wide
    m[130:230, 160:163] = 255                    # 3 wide
    m[130:230, 180:184] = 255                    # 4 wide
    m[130:230, 200] = 255                        # 1 wide: vertical line
    m[200, 230:330] = 255                        # horizontal line
    for i in range(60):
        m[130 + i, 350 + i] = 255                # diagonal line
    m[150, 440] = 255                            # a speck: 1 point
    m[160:162, 440:442] = 255                    # 4 points
    m[170:173, 440:443] = 255                    # 8 points
    return m


def comb_mask():
    """the fused path at the 2^24 branch within the default limits: a 1920 x 1200 frame, 8 one-pixel teeth from x = 1900, rows 100 .. 1099,
    (every second column), joined along the bottom row -- one border of 15 998 points whose x sum is 30 508 186.  Its area is 0, so the
    frame is run with the area gate open"""
    m = np.zeros((1200, 1920), np.uint8)
    for k in range(8):
        m[100:1100, 1900 + 2 * k] = 255
    m[1099, 1900:1915] = 255
    return m


def image_cases():
    return [ImageCase("shapes", shapes_mask(), ("direct_attempt0", "direct_none", "general_fit", "general_no_retry")),
            ImageCase("comb_2p24", comb_mask(), ("general_fit",))]


def frame_of(mask):
    """the BGR frame whose CAMP_BLUE binary image (lower bound 80, no morphology) is `mask`"""
    f = np.zeros(mask.shape + (3,), np.uint8)
    f[..., 0] = mask
    return f
