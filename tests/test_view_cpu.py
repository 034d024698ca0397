"""The operator's debug view on the CPU: rmcv_debug_view_host -- the sequential restatement in rmcv_amd/csrc/device_view.h of
executable/main.cpp:200-207 -- equals tests/view_ref.py, the independent literal restatement, byte for byte, on the case list of
tests/view_cases.py at every size there; hand-checked lines make sure the two do not merely share an error.  No GPU."""
import numpy as np
import pytest

import view_cases as K
import view_ref as R
from rmcv_amd import abi, debug_view_host
from rmcv_amd.abi import ERR_BAD_ARG, VIEW_ALL, VIEW_ARMOURS, VIEW_BLOBS, VIEW_NEGATIVES, RmcvError


def both(case, binary, size, flags=VIEW_ALL):
    got = debug_view_host(binary, case["blobs"], case["negatives"], case["armours"], size, flags)
    want = R.view(binary, case["blobs"], case["negatives"], case["armours"], size, flags)
    return got, want


@pytest.mark.parametrize("src,dst", K.SIZES, ids=["%dx%d-%dx%d" % (s + d) for s, d in K.SIZES])
def test_host_view_equals_the_reference_on_every_case(src, dst):
    binary = K.binary(*src)
    drawn = 0
    for case in K.cases(*src):
        got, want = both(case, binary, dst)
        assert got.shape == (dst[1], dst[0], 3)
        assert np.array_equal(got, want), case["name"]
        full = R.draw(binary, case["blobs"], case["negatives"], case["armours"])
        drawn += int((full != R.draw(binary, [], [], [])).any())
    assert drawn >= 9  # (the cases do draw: an empty overlay would pass nothing)


@pytest.mark.parametrize("flags", [0, VIEW_BLOBS, VIEW_NEGATIVES, VIEW_ARMOURS, VIEW_BLOBS | VIEW_ARMOURS])
def test_each_flag_alone(flags):
    src, dst = K.SIZES[0]
    binary = K.binary(*src)
    views = []
    for case in K.cases(*src):
        if case["name"] in ("crossing", "random", "clipped"):
            got, want = both(case, binary, dst, flags)
            assert np.array_equal(got, want), case["name"]
            views.append(got)
    if flags:
        plain = debug_view_host(binary, None, None, None, dst, VIEW_ALL)
        assert any((v != plain).any() for v in views)


def test_draw_order_between_blob_colours():
    """the later blob's colour where two cross, whichever comes first"""
    w, h = 96, 64
    cases = {c["name"]: c for c in K.cases(w, h)}
    black = np.zeros((h, w), np.uint8)
    a = debug_view_host(black, cases["red_then_blue"]["blobs"], None, None, (w, h))
    b = debug_view_host(black, cases["blue_then_red"]["blobs"][:2], None, None, (w, h))
    assert (a != b).any()
    cx, cy, r = w // 2, h // 2, min(w, h) // 3
    assert tuple(a[cy - 5, cx - 5]) == R.RED and tuple(b[cy - 5, cx - 5]) == R.GREEN   # both polygons pass through this pixel
    assert tuple(a[cy - 5, cx - r]) == R.GREEN and tuple(b[cy - 5, cx - r]) == R.RED   # only the first one does


def lit(view):
    ys, xs = np.nonzero(view.any(axis=2))
    return sorted(zip(xs.tolist(), ys.tolist()))


@pytest.mark.parametrize("size,contour,pixels", [
    # worked by hand from LineIterator's recurrence (err = dx - 2 dy, +2 dx when negative): tests/view_ref.py has the same answers
    ((8, 6), [(1, 1), (4, 2)], [(1, 1), (2, 1), (3, 2), (4, 2)]),                    # shallow; the way back (dx < 0) swaps the ends: same pixels
    ((8, 6), [(2, 5), (3, 1)], [(2, 5), (2, 4), (2, 3), (3, 2), (3, 1)]),            # steep, upwards: the minor step comes after the third pixel
    ((8, 6), [(0, 0), (3, 3)], [(0, 0), (1, 1), (2, 2), (3, 3)]),                    # the diagonal: dy > dx is false, x is the major axis
    ((8, 6), [(-3, 0), (6, 4)], [(0, 1), (1, 1), (2, 2), (3, 2), (4, 3), (5, 3), (6, 4)]),  # clipped at x = 0: y1 += (int)(3 * 4 / 9.0) = 1
])
def test_known_answers(size, contour, pixels):
    w, h = size
    black = np.zeros((h, w), np.uint8)
    got = debug_view_host(black, None, [contour], None, (w, h))
    assert lit(got) == sorted(pixels)
    assert all(tuple(got[y, x]) == R.YELLOW for x, y in pixels)
    assert lit(R.view(black, [], [np.asarray(contour)], [], (w, h))) == sorted(pixels)


def test_known_answer_resize():
    """one white pixel (1, 1) of a 4 x 4 image, at 3 x 3, by hand.  scale = 4/3: dx = 0 -> fx = 1/6, taps 0, 1 weighted 1707, 341; dx = 1 -> fx = 1.5,
    taps 1, 2 weighted 1024, 1024; dx = 2 -> taps 2, 3.  Row sums of source row 1: 255 * 341 = 86955, 255 * 1024 = 261120, 0; >> 4: 5434, 16320.
    dy = 0 (rows 0, 1 weighted 1707, 341): ((341 * 5434) >> 16) = 28 -> (28 + 2) >> 2 = 7;  ((341 * 16320) >> 16) = 84 -> 21.
    dy = 1 (rows 1, 2 weighted 1024, 1024): ((1024 * 5434) >> 16) = 84 -> 21;  ((1024 * 16320) >> 16) = 255 -> (255 + 2) >> 2 = 64.  dy = 2: rows 2, 3: 0."""
    b = np.zeros((4, 4), np.uint8)
    b[1, 1] = 255
    got = debug_view_host(b, None, None, None, (3, 3))
    want = np.array([[7, 21, 0], [21, 64, 0], [0, 0, 0]])
    for c in range(3):
        assert np.array_equal(got[:, :, c], want)
    assert np.array_equal(R.view(b, [], [], [], (3, 3))[:, :, 0], want)


def test_refusals():
    L = abi.lib()
    b = np.zeros((8, 8), np.uint8)
    out = np.zeros((8, 8, 3), np.uint8)
    offs = np.array([0, 2], np.int32)
    pts = np.zeros(2, abi.POINT)
    blobs = np.zeros(1, abi.LIGHTBLOB)

    def call(binary=b, w=8, h=8, stride=8, bl=None, nb=0, p=pts, o=offs, nn=1, ar=None, na=0, flags=VIEW_ALL, vw=8, vh=8, dst=out, ostride=24):
        return L.rmcv_debug_view_host(abi.ptr(binary), w, h, stride, abi.ptr(bl), nb, abi.ptr(p), abi.ptr(o), nn, abi.ptr(ar), na, flags, vw, vh, abi.ptr(dst), ostride)
    assert call() == 0
    for bad in (dict(binary=None), dict(dst=None), dict(w=0), dict(h=0), dict(stride=7), dict(nb=-1), dict(nb=1), dict(na=1), dict(nn=-1), dict(o=None),
                dict(p=None), dict(flags=8), dict(flags=-1), dict(vw=0), dict(vh=0), dict(ostride=23), dict(o=np.array([2, 0], np.int32)),
                dict(o=np.array([-1, 2], np.int32))):
        assert call(**bad) == ERR_BAD_ARG, bad
    assert call(bl=blobs, nb=1) == 0
    with pytest.raises(RmcvError):
        debug_view_host(b, None, None, None, (0, 4))
