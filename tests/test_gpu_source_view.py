"""The source view on the GPU (k_view_source.hip): the device's views equal tests/source_view_ref.py -- the labeler's picture
(executable/svm/labeler.cpp:108-111) over SRC(f), resized -- byte for byte: the stage-wise helper on the CPU case list at every size (staged
and gathered tiles), batches of synthetic frames with real detections (BGR at every flag, borrowed frames with odd strides, Bayer in all
four patterns and in a sensor layout, through the gamma tables of dimmed frames, windowed), a pipeline's per-slot views, the refusals."""
import functools

import numpy as np
import pytest

import bayer_ref as BR
import enhance_ref as ER
import raw_ref as RR
import source_view_cases as SK
import source_view_ref as SR
import view_cases as K
import view_ref as R
from rmcv_amd import (CAMP_BLUE, STAGE_ALL, STAGE_BINARY, STAGE_CONTOURS, STAGE_NO_IMAGE, VIEW_ALL, VIEW_ARMOURS, VIEW_BLOBS, VIEW_NEGATIVES, Context, Pipeline,
                      RmcvError, default_params, source_view_host, synth)
from rmcv_amd import abi

pytestmark = pytest.mark.gpu

TILT = 10.0  # makes negatives of the synthetic stream's tilted bars
LIMITS = dict(max_frames=8, max_width=640, max_height=400)


@functools.lru_cache(maxsize=None)
def case_refs(k):
    """(frame, cases, reference views) of size pair k: computed once, shared"""
    src, dst = SK.SIZES[k]
    frame = SK.frame(*src)
    cases = K.cases(*src)
    return frame, cases, [SR.view(frame, c["blobs"], c["negatives"], c["armours"], dst) for c in cases]


@pytest.fixture(scope="module")
def small():
    c = Context(device=0, **LIMITS)
    yield c
    c.close()


@pytest.mark.parametrize("k", range(len(SK.SIZES)), ids=["%dx%d-%dx%d" % (s + d) for s, d in SK.SIZES])
def test_stagewise_view_equals_the_reference(small, k):
    frame, cases, refs = case_refs(k)
    for case, want in zip(cases, refs):
        got = small.source_view_of(frame, case["blobs"], case["negatives"], case["armours"], SK.SIZES[k][1])
        assert np.array_equal(got, want), case["name"]


@pytest.mark.parametrize("flags", [0, VIEW_BLOBS, VIEW_NEGATIVES, VIEW_ARMOURS])
def test_stagewise_flags(small, flags):
    frame, cases, _ = case_refs(0)
    for case in cases:
        if case["name"] in ("crossing", "random", "blue_then_red"):
            got = small.source_view_of(frame, case["blobs"], case["negatives"], case["armours"], SK.SIZES[0][1], flags)
            assert np.array_equal(got, SR.view(frame, case["blobs"], case["negatives"], case["armours"], SK.SIZES[0][1], flags)), case["name"]


def frames_of(w, h, special):
    """8 synthetic frames; `special` = (position, index, variant) entries replace the plain run of indices"""
    out = np.stack([synth.frame(i, w, h, CAMP_BLUE, 0) for i in range(8)])
    for pos, index, variant in special:
        out[pos] = synth.frame(index, w, h, CAMP_BLUE, variant)
    return out


def lists_of(c, oracle, f, arm, offs):
    """frame f's lists from the batch getters (the negative contours through the oracle's filter: no getter hands them out)"""
    pts, co = c.contours(f)
    blobs, _ = c.blobs(f)
    ob, _, neg = oracle.filter_lightblobs(pts, co, oracle.default_params(tilt_max=TILT))
    assert ob.tobytes() == blobs.tobytes()
    negatives = [np.stack([pts["x"][co[i]:co[i + 1]], pts["y"][co[i]:co[i + 1]]], 1) for i in neg]
    return blobs, negatives, arm[offs[f]:offs[f + 1]]


def batch_lists(c, oracle, n=8):
    c.sync()
    arm, offs = c.armours()
    return [lists_of(c, oracle, f, arm, offs) for f in range(n)]


def check_views(c, srcs, lists, dst, flags=VIEW_ALL, chosen=None):
    chosen = list(range(len(srcs))) if chosen is None else chosen
    got = c.source_views(chosen, size=dst, flags=flags)
    assert got.shape == (len(chosen), dst[1], dst[0], 3)
    for k, f in enumerate(chosen):
        assert np.array_equal(got[k], SR.view(srcs[f], *lists[f], dst, flags)), (dst, flags, f)
    return got


SPECIAL = [(0, 3, 0), (3, 1000, 1)]
# the frame's own size (copy), the exact half, a general downscale with tile seams, a thumbnail (gathered)
DSTS_200 = [(200, 136), (100, 68), (160, 102), (25, 17)]


def test_batch_bgr_views(small, oracle):
    w, h = 200, 136
    c = small
    frames = frames_of(w, h, SPECIAL)
    p = default_params(tilt_max=TILT)
    c.upload(frames)
    c.run(p, STAGE_ALL)
    lists = batch_lists(c, oracle)
    assert sum(len(b) >= 1 and len(n) >= 1 and len(a) >= 1 for b, n, a in lists) >= 1  # (a view of empty overlays would prove little)
    for dst in DSTS_200:
        full = check_views(c, frames, lists, dst)
        assert np.array_equal(source_view_host(frames[3], *lists[3], dst), full[3])
    dst = DSTS_200[2]
    for flags in (0, VIEW_BLOBS, VIEW_NEGATIVES, VIEW_ARMOURS):
        check_views(c, frames, lists, dst, flags)
    want = [SR.view(frames[f], *lists[f], dst) for f in range(8)]
    for chosen in ([0, 3, 7], [5]):
        check_views(c, frames, lists, dst, VIEW_ALL, chosen)
    assert np.array_equal(c.source_view(3, dst), want[3])
    # a caller's device buffer with padded rows and views
    import torch
    stride, pitch = 3 * dst[0] + 20, (3 * dst[0] + 20) * dst[1] + 64
    buf = torch.zeros(3 * pitch, dtype=torch.uint8, device="cuda")
    c._chk(abi.lib().rmcv_batch_source_views(c._h, abi.ptr(np.array([7, 0, 3], np.int32)), 3, dst[0], dst[1], VIEW_ALL, buf.data_ptr(), stride, pitch, None))
    c.sync()
    host = buf.cpu().numpy()
    for k, f in enumerate([7, 0, 3]):
        v = host[k * pitch:k * pitch + stride * dst[1]].reshape(dst[1], stride)
        assert np.array_equal(v[:, :3 * dst[0]].reshape(dst[1], dst[0], 3), want[f]) and not v[:, 3 * dst[0]:].any()
    # an unaligned destination: the byte-wise stores
    odd = torch.zeros(3 * dst[0] * dst[1] + 1, dtype=torch.uint8, device="cuda")
    c.source_views([3], dst=odd.data_ptr() + 1, size=dst)
    c.sync()
    assert np.array_equal(odd.cpu().numpy()[1:].reshape(dst[1], dst[0], 3), want[3])
    # without the byte image the views are the same: they never read it
    c.run(p, STAGE_ALL | STAGE_NO_IMAGE)
    check_views(c, frames, lists, dst)
    assert c.check_guards()[0] == 0


def test_borrowed_frames_with_odd_strides(small, oracle):
    """rows that start at every byte phase, the first frame one byte into its buffer and the last ending with the buffer: the aligned dword
    loads mask their heads and tails, and none reaches outside what is bound"""
    import torch
    w, h = 200, 136
    c = small
    frames = frames_of(w, h, SPECIAL)
    stride, pitch = 3 * w + 1, (3 * w + 1) * h + 3
    total = 1 + 7 * pitch + stride * (h - 1) + 3 * w
    host = np.full(total, 0x5A, np.uint8)
    for f in range(8):
        rows = np.lib.stride_tricks.as_strided(host[1 + f * pitch:], (h, 3 * w), (stride, 1))
        rows[:] = frames[f].reshape(h, 3 * w)
    dev = torch.from_numpy(host).cuda()
    c.bind_device_frames(dev.data_ptr() + 1, 8, h, w, stride=stride, frame_pitch=pitch, keepalive=dev)
    c.run(default_params(tilt_max=TILT), STAGE_ALL)
    lists = batch_lists(c, oracle)
    for dst in DSTS_200:
        check_views(c, frames, lists, dst)
    c.upload(frames)  # (the borrowed buffer is let go)


@pytest.mark.parametrize("pattern", BR.PATTERNS)
def test_bayer_plain_views(oracle, pattern):
    w, h = 200, 136  # (a width that is no multiple of 16)
    frames = frames_of(w, h, SPECIAL)
    m = BR.mosaic(frames, pattern)
    c = Context(device=0, **LIMITS)
    try:
        c.set_input_format(pattern)
        c.upload(m)
        c.run(default_params(tilt_max=TILT), STAGE_ALL)
        lists = batch_lists(c, oracle)
        srcs = [SR.src_bayer(m[f], pattern) for f in range(8)]
        assert not np.array_equal(srcs[0], frames[0])  # (D of the mosaic, not the frame it was sampled from)
        for dst in DSTS_200:  # the copy first: D's clamped border rows and columns are in the view
            check_views(c, srcs, lists, dst)
        check_views(c, srcs, lists, DSTS_200[2], 0, [2, 6])
        assert np.array_equal(c.source_view(1, (w, h)), SR.view(srcs[1], *lists[1], (w, h)))
        assert c.check_guards()[0] == 0
    finally:
        c.close()


def test_bayer_sensor_layout_views(oracle):
    """16-bit samples with the pixel at bits 2 .. 9, mirrored and flipped, an odd width"""
    w, h, pattern = 203, 136, BR.GB
    frames = frames_of(w, h, SPECIAL)
    oriented = RR.derived_pattern(pattern, w, h, True, True)
    m = BR.mosaic(frames, oriented)
    r = RR.delivered(m, 16, 2, True, True, np.random.default_rng(3))
    c = Context(device=0, **LIMITS)
    try:
        c.set_input_format(pattern)
        c.set_input_layout(16, 2, True, True)
        c.upload(r)
        c.run(default_params(tilt_max=TILT), STAGE_ALL)
        lists = batch_lists(c, oracle)
        srcs = [SR.src_bayer(r[f], pattern, 2, True, True) for f in range(8)]
        assert np.array_equal(srcs[0], BR.demosaic(m[0], oriented))
        for dst in [(w, h), (160, 102), (25, 17)]:
            check_views(c, srcs, lists, dst)
        # 8-bit samples, mirrored only: the layout path without the narrowing
        c.set_input_layout(8, 0, True, False)
        o2 = RR.derived_pattern(pattern, w, h, True, False)
        r2 = RR.delivered(BR.mosaic(frames, o2), 8, 0, True, False)
        c.upload(r2)
        c.run(default_params(tilt_max=TILT), STAGE_ALL)
        lists = batch_lists(c, oracle)
        check_views(c, [SR.src_bayer(r2[f], pattern, 0, True, False) for f in range(8)], lists, (160, 102))
        assert c.check_guards()[0] == 0
    finally:
        c.close()


def test_enhanced_views(oracle):
    w, h = 200, 136
    frames = ER.dim(frames_of(w, h, SPECIAL), 96)
    c = Context(device=0, **LIMITS)
    try:
        c.set_enhance(True)
        c.upload(frames)
        c.run(default_params(tilt_max=TILT), STAGE_ALL)
        lists = batch_lists(c, oracle)
        srcs, tables = zip(*[SR.src_enhanced(frames[f]) for f in range(8)])
        assert any((t != np.arange(256)).any() for t in tables)  # the gamma is not 1: a missed lookup shows
        assert any((s != f).any() for s, f in zip(srcs, frames))
        for dst in DSTS_200:
            check_views(c, srcs, lists, dst)
        check_views(c, srcs, lists, DSTS_200[2], VIEW_BLOBS, [4])
        assert c.check_guards()[0] == 0
    finally:
        c.close()


def test_windowed_views(small, oracle):
    fw, fh, ww, wh = 320, 256, 128, 96
    c = small
    frames = frames_of(fw, fh, [(0, 0, 0), (3, 1001, 1)])
    # negatives and values beyond the frame (clamped), x that is no multiple of 16 (snapped), and the window at the right and bottom edge
    origins = np.array([(-20, -5), (400, 300), (fw - ww, fh - wh), (100, 50), (33, 200), (319, 0), (0, 255), (150, 100)], np.int32)
    c.upload(frames)
    c.set_windows(origins, ww, wh)
    try:
        c.run(default_params(tilt_max=TILT), STAGE_ALL)
        lists = batch_lists(c, oracle)
        eff = c.windows()[0]
        srcs = [SR.src_window(frames[f], origins[f], ww, wh) for f in range(8)]
        assert eff.tolist() == [[0, 0], [192, 160], [192, 160], [96, 50], [32, 160], [192, 0], [0, 160], [144, 100]]
        assert all(s.shape == (wh, ww, 3) for s in srcs)
        for dst in [(ww, wh), (64, 48), (96, 72), (16, 12)]:
            check_views(c, srcs, lists, dst)
    finally:
        c.set_windows(None, 0, 0)


def test_pipeline_source_views(small):
    import torch
    w, h, dst, chosen = 200, 136, (160, 102), [0, 3, 7]
    p = default_params(tilt_max=TILT)
    sets = [frames_of(w, h, [(0, 3, 0), (3, 1000, 1)]), frames_of(w, h, [(0, 40, 0), (7, 1003, 1)]), frames_of(w, h, [(3, 77, 0)])[::-1].copy()]
    want, want_bin = [], []
    for fr in sets:  # the context path (equal to the reference: test_batch_bgr_views)
        small.upload(fr)
        small.run(p, STAGE_ALL)
        want.append(small.source_views(chosen, size=dst))
        want_bin.append(small.debug_views(chosen, dst))
    assert any((a != b).any() for a, b in zip(want[:-1], want[1:])) and (want[0] != want_bin[0]).any()
    dev = [torch.from_numpy(fr).cuda() for fr in sets]
    pl = Pipeline(device=0, depth=2, **LIMITS)
    try:
        pl.set_views(chosen, dst, source=True)
        tickets = []
        for k in range(3):
            tickets.append(pl.submit(dev[k].data_ptr(), 8, h, w, p, STAGE_ALL))
            if k >= 1:  # ticket k - 1: its record, and its views, live until ticket k + 1 is submitted
                pl.wait(tickets[k - 1])
                v = pl.views(tickets[k - 1])
                assert tuple(v.shape) == (3, dst[1], dst[0], 3) and v.dtype == torch.uint8
                assert np.array_equal(v.cpu().numpy(), want[k - 1]), k - 1
        pl.wait(tickets[2])
        assert np.array_equal(pl.views(tickets[2]).cpu().numpy(), want[2])
        assert pl.get_info().host_blocking_calls == 0
        with pytest.raises(RmcvError):  # fewer frames than the views name; stages that lack what the flags need
            pl.submit(dev[0].data_ptr(), 4, h, w, p, STAGE_ALL)
        with pytest.raises(RmcvError):
            pl.submit(dev[0].data_ptr(), 8, h, w, p, STAGE_BINARY | STAGE_CONTOURS)
        # one kind at a time, the one set last: the binary's view, and back
        pl.set_views(chosen, dst)
        t = pl.submit(dev[1].data_ptr(), 8, h, w, p, STAGE_ALL)
        pl.wait(t)
        assert np.array_equal(pl.views(t).cpu().numpy(), want_bin[1])
        pl.set_views(chosen, dst, flags=VIEW_BLOBS, source=True)
        t = pl.submit(dev[1].data_ptr(), 8, h, w, p, STAGE_ALL)
        pl.wait(t)
        small.upload(sets[1])
        small.run(p, STAGE_ALL)
        assert np.array_equal(pl.views(t).cpu().numpy(), small.source_views(chosen, size=dst, flags=VIEW_BLOBS))
        # n == 0: off
        pl.set_views(None, source=True)
        t = pl.submit(dev[0].data_ptr(), 8, h, w, p, STAGE_ALL)
        pl.wait(t)
        with pytest.raises(RmcvError):
            pl.views(t)
        assert pl.get_info().host_blocking_calls == 0
    finally:
        pl.close()


def test_refusals_on_the_device_paths(small):
    c = small
    w, h, dst = 200, 136, (160, 102)
    frames = frames_of(w, h, [])
    c.upload(frames)
    with pytest.raises(RmcvError):  # nothing run yet: not even the binary's stage
        c.source_views([0], size=dst, flags=0)
    c.run(default_params(), STAGE_BINARY | STAGE_CONTOURS)
    with pytest.raises(RmcvError):  # the run lacked the stages the flags need
        c.source_views([0], size=dst)
    assert np.array_equal(c.source_views([0], size=dst, flags=0)[0], R.resize_linear(frames[0], *dst))  # flags 0: the thumbnail
    c.run(default_params(), STAGE_ALL)
    for bad in ([8], [-1], [0, 0], [], list(range(8)) + [0]):
        with pytest.raises(RmcvError):
            c.source_views(bad, size=dst)
    for size in ((0, 10), (10, 0), (641, 10), (10, 401)):
        with pytest.raises(RmcvError):
            c.source_views([0], size=size)
        with pytest.raises(RmcvError):
            c.source_view(0, size)
    for flags in (8, -1):
        with pytest.raises(RmcvError):
            c.source_views([0], size=dst, flags=flags)
    L = abi.lib()
    one = np.zeros(1, np.int32)
    import torch
    buf = torch.zeros(2 * 3 * dst[0] * dst[1], dtype=torch.uint8, device="cuda")
    assert L.rmcv_batch_source_views(c._h, abi.ptr(one), 1, dst[0], dst[1], VIEW_ALL, buf.data_ptr(), 3 * dst[0] - 1, 0, None) == abi.ERR_BAD_ARG
    assert L.rmcv_batch_source_views(c._h, abi.ptr(np.array([0, 1], np.int32)), 2, dst[0], dst[1], VIEW_ALL, buf.data_ptr(), 3 * dst[0], 3 * dst[0] * dst[1] - 1, None) == abi.ERR_BAD_ARG
    assert L.rmcv_batch_source_views(c._h, abi.ptr(one), 1, dst[0], dst[1], VIEW_ALL, None, 3 * dst[0], 0, None) == abi.ERR_BAD_ARG
    assert not buf.any().item()  # refused before anything was enqueued
    # the existing entry points keep refusing what they refused
    with pytest.raises(RmcvError):
        c.debug_views([0], dst, flags=8)
    # a frame that exceeded a limit: the batch call renders what the tables hold, the one-frame getter refuses
    tiny = Context(device=0, max_contours=1, **LIMITS)
    try:
        tiny.upload(frames)
        tiny.run(default_params(), STAGE_ALL)
        st = tiny.counts()["status"]
        over = [f for f in range(8) if st[f] & abi.FRAME_OVF_CONTOURS]
        assert over
        with pytest.raises(RmcvError):
            tiny.source_view(over[0], dst)
        assert tiny.source_views(over[:1], size=dst).shape == (1, dst[1], dst[0], 3)
        assert tiny.check_guards()[0] == 0
    finally:
        tiny.close()
    with pytest.raises(RmcvError):  # the stage-wise helper's
        c.source_view_of(np.zeros((8, 8, 3), np.uint8), size=(0, 3))
    with pytest.raises(RmcvError):
        c.source_view_of(np.zeros((8, 700, 3), np.uint8), size=(4, 4))
    # the context still works
    assert c.source_views([1], size=dst).shape == (1, dst[1], dst[0], 3)
