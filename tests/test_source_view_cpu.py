"""The source view on the CPU: rmcv_source_view_host -- the sequential restatement in rmcv_amd/csrc/device_view.h of the
labeler's picture (executable/svm/labeler.cpp:108-111), resized -- equals tests/source_view_ref.py, the independent restatement, byte for
byte on the case list of tests/view_cases.py at every size of tests/source_view_cases.py.  The frames are not 0 / 255: this is what pins
view_mix on values in between.  rmcv_debug_view_host, whose body was factored for it, still equals tests/view_ref.py.  No GPU."""
import numpy as np
import pytest

import source_view_cases as SK
import source_view_ref as SR
import view_cases as K
import view_ref as R
from rmcv_amd import abi, debug_view_host, source_view_host
from rmcv_amd.abi import ERR_BAD_ARG, VIEW_ALL, VIEW_ARMOURS, VIEW_BLOBS, VIEW_NEGATIVES, RmcvError

IDS = ["%dx%d-%dx%d" % (s + d) for s, d in SK.SIZES]


@pytest.mark.parametrize("src,dst", SK.SIZES, ids=IDS)
def test_host_source_view_equals_the_reference_on_every_case(src, dst):
    frame = SK.frame(*src)
    plain = SR.view(frame, [], [], [], dst)
    differ = 0
    for case in K.cases(*src):
        got = source_view_host(frame, case["blobs"], case["negatives"], case["armours"], dst)
        want = SR.view(frame, case["blobs"], case["negatives"], case["armours"], dst)
        assert got.shape == (dst[1], dst[0], 3)
        assert np.array_equal(got, want), case["name"]
        differ += int((SR.draw(frame, case["blobs"], case["negatives"], case["armours"]) != frame).any())
    assert differ >= 9  # (the cases do draw: an empty overlay would pass nothing)
    # the frame is what is under the overlays: channels differ, and values other than 0 / 255 reach the mix
    assert len(np.unique(plain)) > 2 or dst == (1, 1)
    assert (plain[..., 0] != plain[..., 1]).any() or dst == (1, 1)


@pytest.mark.parametrize("flags", [0, VIEW_BLOBS, VIEW_NEGATIVES, VIEW_ARMOURS])
def test_each_flag_alone(flags):
    src, dst = SK.SIZES[0]
    frame = SK.frame(*src)
    views = []
    for case in K.cases(*src):
        if case["name"] in ("crossing", "random", "clipped"):
            got = source_view_host(frame, case["blobs"], case["negatives"], case["armours"], dst, flags)
            assert np.array_equal(got, SR.view(frame, case["blobs"], case["negatives"], case["armours"], dst, flags)), case["name"]
            views.append(got)
    plain = source_view_host(frame, None, None, None, dst, VIEW_ALL)
    if flags:
        assert any((v != plain).any() for v in views)
    else:  # flags 0: the plain resized frame, whatever the lists
        assert all(np.array_equal(v, plain) for v in views)
        assert np.array_equal(plain, R.resize_linear(frame, *dst))


def test_copy_size_is_the_frame_with_the_overlay_pixels_replaced():
    w, h = 96, 64
    frame = SK.frame(w, h)
    case = {c["name"]: c for c in K.cases(w, h)}["crossing"]
    got = source_view_host(frame, case["blobs"], case["negatives"], case["armours"], (w, h))
    drawn = R.draw(np.zeros((h, w), np.uint8), case["blobs"], case["negatives"], case["armours"])  # the same polygons over black
    mask = drawn.any(axis=2)
    assert mask.any() and np.array_equal(got[~mask], frame[~mask]) and np.array_equal(got[mask], drawn[mask])


def test_strided_rows():
    w, h, dst = 50, 30, (31, 17)
    frame = SK.frame(w, h)
    padded = np.full((h, 3 * w + 7), 0xEE, np.uint8)
    padded[:, :3 * w] = frame.reshape(h, 3 * w)
    out = np.zeros((dst[1], 3 * dst[0] + 5), np.uint8)
    rc = abi.lib().rmcv_source_view_host(abi.ptr(padded), w, h, 3 * w + 7, None, 0, None, abi.ptr(np.zeros(1, np.int32)), 0, None, 0, VIEW_ALL, dst[0], dst[1],
                                         abi.ptr(out), 3 * dst[0] + 5)
    assert rc == 0
    assert np.array_equal(out[:, :3 * dst[0]].reshape(dst[1], dst[0], 3), R.resize_linear(frame, *dst)) and not out[:, 3 * dst[0]:].any()


def test_refusals():
    L = abi.lib()
    b = np.zeros((8, 8, 3), np.uint8)
    out = np.zeros((8, 8, 3), np.uint8)
    offs = np.array([0, 2], np.int32)
    pts = np.zeros(2, abi.POINT)
    blobs = np.zeros(1, abi.LIGHTBLOB)

    def call(bgr=b, w=8, h=8, stride=24, bl=None, nb=0, p=pts, o=offs, nn=1, ar=None, na=0, flags=VIEW_ALL, vw=8, vh=8, dst=out, ostride=24):
        return L.rmcv_source_view_host(abi.ptr(bgr), w, h, stride, abi.ptr(bl), nb, abi.ptr(p), abi.ptr(o), nn, abi.ptr(ar), na, flags, vw, vh, abi.ptr(dst), ostride)
    assert call() == 0
    for bad in (dict(bgr=None), dict(dst=None), dict(w=0), dict(h=0), dict(stride=23), dict(nb=-1), dict(nb=1), dict(na=1), dict(nn=-1), dict(o=None),
                dict(p=None), dict(flags=8), dict(flags=-1), dict(vw=0), dict(vh=0), dict(ostride=23), dict(o=np.array([2, 0], np.int32)),
                dict(o=np.array([-1, 2], np.int32))):
        assert call(**bad) == ERR_BAD_ARG, bad
    assert call(bl=blobs, nb=1) == 0
    with pytest.raises(RmcvError):
        source_view_host(b, None, None, None, (0, 4))


@pytest.mark.parametrize("src,dst", K.SIZES, ids=["%dx%d-%dx%d" % (s + d) for s, d in K.SIZES])
def test_debug_view_host_is_unchanged(src, dst):
    binary = K.binary(*src)
    for case in K.cases(*src):
        got = debug_view_host(binary, case["blobs"], case["negatives"], case["armours"], dst)
        assert np.array_equal(got, R.view(binary, case["blobs"], case["negatives"], case["armours"], dst)), case["name"]
