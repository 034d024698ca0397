"""SURVEY 8f-1 / VERDICT r2 #8: a second opinion for the [OCV] fixed-point pieces of the icon path (warpAffine + resize on 8-bit
BGR, getAffineTransform), which so far had ONE restatement (oracle/rmcv_oracle.c, mirrored by k_classify).  tests/independent_icon.py
restates them a second time, table-driven and vectorised, from the published structure; here the two are compared bit for bit on
more than a thousand regions.  Neither is pinned against real OpenCV (absent here); agreement removes slips of one author's one
restatement, not shared misconceptions."""
import numpy as np

import independent_icon as ind
import oracle_lib as O
from icon_cases import random_icon, scene


def test_warp_resize_second_opinion_on_1200_regions():
    rng = np.random.default_rng(20241008)
    n = same = clamped = area = 0
    for s in range(24):
        h, w = int(rng.integers(60, 400)), int(rng.integers(60, 500))
        img = scene(rng, h, w)
        for _ in range(50):
            icon = random_icon(rng, h, w)
            a, ia, ra = O.affine_correction(img, icon)
            b, ib, rb = ind.affine_correction(img, icon)
            assert ra == rb and np.array_equal(ia, ib), (s, icon.tolist())
            assert np.array_equal(a, b), (s, icon.tolist(), int(np.abs(a.astype(int) - b.astype(int)).max()))
            n += 1
            same += ra == 0
            clamped += not np.array_equal(ia, icon)
            area += (ia[:, 0].max() - ia[:, 0].min() == 39) and (ia[:, 1].max() - ia[:, 1].min() == 39)
    assert n == 1200 and same > 1100 and clamped > 100 and area > 100


def test_weight_table_is_the_closed_form_except_where_shorts_saturate():
    """the table built OpenCV's way equals 32 (32 - fx)(32 - fy) ... everywhere but at (0, 0), where 2^15 does not fit a short:
    32767 there, and the missing 1 goes to the LAST tap -- what the oracle's closed form does with `w11 += 1`"""
    t = ind.bilinear_table()
    for fy in range(32):
        for fx in range(32):
            cf = [[(32 - fx) * (32 - fy) * 32, fx * (32 - fy) * 32], [(32 - fx) * fy * 32, fx * fy * 32]]
            if fx == 0 and fy == 0:
                assert t[0, 0].tolist() == [[32767, 0], [0, 1]]
            else:
                assert t[fy, fx].tolist() == cf, (fx, fy)


def test_synthetic_stream_icons_second_opinion():
    """the icons the benchmark's own C5 frames produce (every armour of 24 frames at 1920x1200)"""
    from rmcv_amd import synth
    O.set_math_mode(0)
    n = 0
    for i in range(24):
        fr = synth.frame(120000 + i, 1920, 1200)
        for a in O.detect_frame(fr)["armours"]:
            x, ic, rc = O.affine_correction(fr, a["icon"])
            y, ic2, rc2 = ind.affine_correction(fr, a["icon"])
            assert rc == rc2 and np.array_equal(ic, ic2) and np.array_equal(x, y)
            n += 1
    assert n > 40
