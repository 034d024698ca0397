"""The icon at any output size on the CPU (rmcv_amd/csrc/icon_host.h): rmcv_affine_correction_host equals the second opinion
(tests/independent_icon.py) byte for byte on tests/icon_strip_cases.py at every side and at two rectangular sizes, and the oracle at 20 x 20;
rmcv_icon_strip_host's layout and zero slots and rmcv_labeler_sheet_host's three parts equal numpy restatements; the case list reaches the
branches it is there for.  No GPU."""
import time

import numpy as np
import pytest

import icon_cases as K
import icon_strip_cases as S
import independent_icon as ind
import oracle_lib as O
import source_view_cases as SK
import view_cases as VK
from rmcv_amd import RmcvError, VIEW_ALL, VIEW_ARMOURS, affine_correction_host, icon_strip_host, labeler_sheet_host, sheet_size
from rmcv_amd import abi

SIZES = [(s, s) for s in S.SIDES] + list(S.RECT_SIZES)


@pytest.mark.parametrize("ow,oh", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_host_icon_equals_the_second_opinion(ow, oh):
    img = K.frame()
    want = S.expected(ow, oh)
    for (name, q), (out, clamped, deg) in zip(S.list_for(ow, oh), want):
        got, ic, d = affine_correction_host(img, q, (ow, oh))
        assert np.array_equal(got, out), name
        assert ic.tobytes() == clamped.tobytes(), name     # clamped in place, imgproc.cpp:11-15 (bit for bit: -0 and NaN end as +0)
        assert d == bool(deg), name


def test_square_sizes_are_the_second_opinions_own_function():
    """expected() composes the second opinion's pieces so that it can state ow != oh; for squares that is affine_correction(img, icon, side)"""
    img = K.frame()
    for side in (7, 80):
        for (name, q), (out, clamped, deg) in list(zip(S.list_for(side, side), S.expected(side, side)))[::9]:
            o2, c2, d2 = ind.affine_correction(img, q, side)
            assert np.array_equal(out, o2) and clamped.tobytes() == c2.tobytes() and deg == d2, name


def test_side_20_equals_the_oracle():
    img = K.frame()
    differ = 0
    for (name, q), (out, clamped, deg) in zip(S.list_for(20, 20), S.expected(20, 20)):
        ref, ric, rc = O.affine_correction(img, q)
        differ += not (np.array_equal(ref, out) and ric.tobytes() == clamped.tobytes() and bool(rc) == bool(deg))
        got, ic, d = affine_correction_host(img, q, (20, 20))
        assert np.array_equal(got, ref) and ic.tobytes() == ric.tobytes() and d == bool(rc), name
    assert differ == 0   # the restatement and the oracle differ on 0 cases


def test_the_case_list_reaches_its_branches():
    for side in S.SIDES:
        boxes = [S.box_of(q) for _, q in S.cases(side)]
        live = [(bw, bh) for _, _, bw, bh, deg in boxes if not deg]
        area = any(bw == 2 * side and bh == 2 * side for bw, bh in live)
        assert area == (side in (1, 7, 20, 33)), side                     # the exact 2:1 branch where the double box fits the frame
        if side > 1:
            assert any(bw < side and bh < side for bw, bh in live), side  # an upscale in both directions
            # a downscale by the tap rule: in both directions where the 120-row frame has room for one, in x alone at side 128
            assert any(bw > side and (bh > side or side >= S.H) and not (bw == 2 * side and bh == 2 * side) for bw, bh in live), side
            assert any(bw == side and bh == min(side, S.H) for bw, bh in live), side  # scale 1: every fraction zero
    names = {n for side in S.SIDES for n, _ in S.cases(side)}
    assert not names & set(S.LEFT_OUT) and {"double_%d" % s for s in (1, 7, 20, 33)} <= names


@pytest.mark.parametrize("side", S.SIDES)
def test_named_icons_on_the_restatement(side):
    """the 142 named icons: none degenerate, no all-zero picture, the whole list in under a second"""
    img = K.frame()
    named = K.named_icons(S.W, S.H)
    assert len(named) == 142
    t0 = time.perf_counter()
    outs = [ind.affine_correction(img, q, side) for _, q in named]
    took = time.perf_counter() - t0
    assert sum(rc for _, _, rc in outs) == 0
    assert sum(not o.any() for o, _, _ in outs) == 0
    assert took < 1.0, took


def test_strip_layout_and_zero_slots():
    img = K.frame()
    icons = [q for _, q in S.cases(20)[:9]]
    arm = S.armours_of(icons)
    before = arm.tobytes()
    for side in (1, 7, 20, 33):
        for cap in (1, 4, 9, 12):                                        # fewer slots than armours, as many, and more
            got = icon_strip_host(img, arm, side, cap)
            assert got.shape == (side, cap * side, 3)
            assert np.array_equal(got, S.strip_ref(img, icons, side, cap)), (side, cap)
            if cap > len(icons):
                assert not got[:, len(icons) * side:].any()
    assert arm.tobytes() == before                                       # the armours are only read
    assert not icon_strip_host(img, None, 7, 3).any()                    # no armours: zeros
    # padded rows: bytes behind 3 cap side of a row are not the function's to write
    side, cap = 7, 4
    buf = np.full((side, 3 * cap * side + 5), 0xEE, np.uint8)
    rc = abi.lib().rmcv_icon_strip_host(abi.ptr(img), S.W, S.H, 3 * S.W, abi.ptr(arm), len(arm), side, cap, abi.ptr(buf), buf.shape[1])
    assert rc == 0 and (buf[:, 3 * cap * side:] == 0xEE).all()
    assert np.array_equal(buf[:, :3 * cap * side].reshape(side, cap * side, 3), S.strip_ref(img, icons, side, cap))


def test_an_image_whose_rows_are_padded():
    """stride > 3 w: the host function reads rows `stride` apart"""
    img = K.frame()
    padded = np.full((S.H, 3 * S.W + 7), 0x77, np.uint8)
    padded[:, :3 * S.W] = img.reshape(S.H, 3 * S.W)
    for name, q in S.cases(33)[::17]:
        ic = np.array(q, np.float32).copy()
        out = np.empty((33, 33, 3), np.uint8)
        deg = np.zeros(1, np.int32)
        assert abi.lib().rmcv_affine_correction_host(abi.ptr(padded), S.W, S.H, padded.shape[1], abi.ptr(ic), 33, 33, abi.ptr(out), 99, abi.ptr(deg)) == 0
        assert np.array_equal(out, S.affine_any(img, q, 33, 33)[0]), name


def test_sheet_equals_its_three_parts():
    src, dst = (200, 136), (100, 68)
    img, binary = SK.frame(*src), VK.binary(*src)
    for case in VK.cases(*src):
        if not len(case["armours"]) and case["name"] not in ("octants", "clipped"):
            continue
        for size, side, flags in ((dst, 20, VIEW_ALL), (src, 80, VIEW_ARMOURS), ((50, 34), 33, 0)):
            got = labeler_sheet_host(img, binary, case["blobs"], case["negatives"], case["armours"], size, side, flags)
            assert got.shape == (size[1] + side, 2 * size[0], 3) == sheet_size(size, side)[::-1] + (3,)
            want = S.sheet_ref(img, binary, case["blobs"], case["negatives"], case["armours"], size, side, flags, abi.ICON_STRIP_CAP_MAX)
            assert np.array_equal(got, want), (case["name"], size, side, flags)
    assert sum(len(c["armours"]) > 0 for c in VK.cases(*src)) >= 2
    # a strip with fewer slots than the frame has armours, and a remainder behind the last slot: 2 * 50 // 33 = 3 slots, 1 pixel over
    many = VK.armours(*[VK.armour(K.box(5, 5, 30, 30), K.box(10 + 9 * k, 8 + 5 * k, 60 + 9 * k, 50 + 5 * k)) for k in range(5)])
    got = labeler_sheet_host(img, binary, None, None, many, (50, 34), 33, VIEW_ALL)
    assert np.array_equal(got, S.sheet_ref(img, binary, VK.blobs(), [], many, (50, 34), 33, VIEW_ALL, abi.ICON_STRIP_CAP_MAX))
    assert got[34:, :99].any() and not got[34:, 99:].any()


def test_host_refusals():
    L, p = abi.lib(), abi.ptr
    img = np.ascontiguousarray(K.frame())
    ic = np.array(K.QUAD, np.float32)
    out = np.zeros((256, 256 * 3), np.uint8)

    def affine(bgr=img, w=S.W, h=S.H, stride=3 * S.W, icon=ic, ow=20, oh=20, o=out, ostride=768):
        return L.rmcv_affine_correction_host(p(bgr), w, h, stride, p(icon), ow, oh, p(o), ostride, None)
    assert affine() == 0
    for bad in (dict(bgr=None), dict(icon=None), dict(o=None), dict(w=0), dict(h=0), dict(stride=3 * S.W - 1), dict(ow=0), dict(oh=0), dict(ow=257), dict(oh=257),
                dict(ow=-1), dict(ostride=59)):
        assert affine(**bad) == abi.ERR_BAD_ARG, bad
    assert affine(ow=256, oh=256) == 0 and affine(ow=1, oh=256, ostride=3) == 0
    arm = S.armours_of([np.array(K.QUAD, np.float32)])

    def strip(bgr=img, w=S.W, h=S.H, stride=3 * S.W, a=arm, n=1, side=20, cap=2, o=out, ostride=768):
        return L.rmcv_icon_strip_host(p(bgr), w, h, stride, p(a), n, side, cap, p(o), ostride)
    assert strip() == 0
    for bad in (dict(bgr=None), dict(o=None), dict(a=None), dict(n=-1), dict(w=0), dict(h=0), dict(stride=3), dict(side=0), dict(side=257), dict(cap=0),
                dict(cap=abi.ICON_STRIP_CAP_MAX + 1), dict(ostride=119)):
        assert strip(**bad) == abi.ERR_BAD_ARG, bad
    for size, side in (((0, 5), 4), ((5, 0), 4), ((5, 5), 0), ((5, 5), 11), ((200, 5), 257)):
        with pytest.raises(RmcvError):
            sheet_size(size, side)
    assert sheet_size((5, 7), 10) == (10, 17)
    binary = VK.binary(S.W, S.H)
    with pytest.raises(RmcvError):
        labeler_sheet_host(img, binary, size=(5, 5), side=11)
    with pytest.raises(RmcvError):
        labeler_sheet_host(img, binary, size=(50, 50), side=20, flags=8)
