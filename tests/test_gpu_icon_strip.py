"""The icon strip and the labeler's sheet on the GPU (k_icon_strip.hip): the device's strips equal rmcv_icon_strip_host and the
numpy restatement (tests/icon_strip_cases.py over tests/independent_icon.py) byte for byte -- the stage-wise helper on the 160 x 120 case
list at every side, batches of synthetic frames with real detections (BGR, borrowed frames with an odd stride, Bayer in all four patterns and
in a sensor layout, through the gamma tables of dimmed frames, windowed) --, slot j at 20 x 20 equals row j of Context.icons; the sheets equal
their three parts; a pipeline's per-slot sheets; the refusals."""
import functools

import numpy as np
import pytest

import bayer_ref as BR
import enhance_ref as ER
import icon_cases as K
import icon_strip_cases as S
import raw_ref as RR
import source_view_ref as SR
from rmcv_amd import (CAMP_BLUE, LABEL_ARMOURS, STAGE_ALL, STAGE_ARMOURS, STAGE_BINARY, STAGE_BLOBS, STAGE_CONTOURS, STAGE_IDENTITY, VIEW_ALL, VIEW_ARMOURS, Context,
                      Pipeline, RmcvError, default_params, icon_strip_host, labeler_sheet_host, synth)
from rmcv_amd import abi

pytestmark = pytest.mark.gpu

TILT = 10.0
LIMITS = dict(max_frames=8, max_width=640, max_height=400)
SPECIAL = [(0, 3, 0), (3, 1000, 1)]
W, H = 200, 136
DETECT = STAGE_BINARY | STAGE_CONTOURS | STAGE_BLOBS | STAGE_ARMOURS
CHUNK = 97   # icons per stage-wise strip (<= max_armours; no multiple of a workgroup's four wavefronts: the last workgroup is partly idle)


@pytest.fixture(scope="module")
def small():
    c = Context(device=0, **LIMITS)
    yield c
    c.close()


def frames_of(w, h, special):
    """8 synthetic frames as tests/test_gpu_source_view.py builds them"""
    out = np.stack([synth.frame(i, w, h, CAMP_BLUE, 0) for i in range(8)])
    for pos, index, variant in special:
        out[pos] = synth.frame(index, w, h, CAMP_BLUE, variant)
    return out


def armours_of(c, n=8):
    c.sync()
    arm, offs = c.armours()
    return [arm[offs[f]:offs[f + 1]] for f in range(n)]


@functools.lru_cache(maxsize=None)
def want_strip(key, f, side, cap):
    """the restated strip of frame f of the registered batch `key`: computed once, shared"""
    srcs, arms = BATCHES[key]
    return S.strip_ref(srcs[f], list(arms[f]["icon"]), side, cap)


BATCHES = {}


def check_strips(c, key, srcs, arms, side, cap, chosen=None):
    BATCHES[key] = (srcs, arms)
    chosen = list(range(len(srcs))) if chosen is None else chosen
    got = c.icon_strips(chosen, side, cap)
    assert got.shape == (len(chosen), side, cap * side, 3)
    for k, f in enumerate(chosen):
        assert np.array_equal(got[k], want_strip(key, f, side, cap)), (key, side, cap, f)
    return got


@pytest.mark.parametrize("side", S.SIDES)
def test_stagewise_strips_equal_the_host_and_the_restatement(small, side):
    assert CHUNK <= small.limits.max_armours
    img = K.frame()
    cases, want = S.cases(side), S.expected(side, side)
    for a in range(0, len(cases), CHUNK):
        icons = [q for _, q in cases[a:a + CHUNK]]
        arm = S.armours_of(icons)
        before = arm.tobytes()
        got = small.icon_strip_of(img, arm, side, len(icons))
        assert arm.tobytes() == before
        assert np.array_equal(got, icon_strip_host(img, arm, side, len(icons))), (side, a)
        for j in range(len(icons)):
            assert np.array_equal(got[:, j * side:(j + 1) * side], want[a + j][0]), cases[a + j][0]
    # more slots than armours: zeros behind them; fewer: the first cap
    arm = S.armours_of([q for _, q in cases[:5]])
    for cap in (3, 5, 8):
        got = small.icon_strip_of(img, arm, side, cap)
        assert np.array_equal(got, S.strip_ref(img, [q for _, q in cases[:5]], side, cap)), (side, cap)
    assert not small.icon_strip_of(img, None, side, 2).any()


def test_batch_bgr_strips(small):
    import torch
    c = small
    frames = frames_of(W, H, SPECIAL)
    p = default_params(tilt_max=TILT)
    c.upload(frames)
    c.run(p, DETECT)
    arms = armours_of(c)
    counts = [len(a) for a in arms]
    assert max(counts) >= 2 and min(counts) == 0, counts
    small_cap, large_cap = 4, max(counts) + 1
    assert small_cap < max(counts) < large_cap <= c.limits.max_armours
    table = c.armours()[0].tobytes()
    first = {}
    for side in (20, 80):
        for cap in (small_cap, large_cap):
            first[side, cap] = check_strips(c, "bgr", frames, arms, side, cap)
        check_strips(c, "bgr", frames, arms, side, small_cap, [6, 1, 2])
        f = int(np.argmax(counts))
        one, n = c.icon_strip(f, side, small_cap)
        assert n == small_cap and np.array_equal(one, want_strip("bgr", f, side, small_cap))
        assert np.array_equal(one, icon_strip_host(frames[f], arms[f], side, small_cap))
    assert c.armours()[0].tobytes() == table                              # the armour table's bytes are unchanged by the calls
    # d_counts, and a caller's buffer with padded rows and strips: the padding is not the kernel's to write
    side, cap, chosen = 20, small_cap, [2, 0, 1, 7]
    stride, pitch = 3 * cap * side + 20, (3 * cap * side + 20) * side + 64
    buf = torch.full((len(chosen) * pitch,), 0xEE, dtype=torch.uint8, device="cuda")
    cnt = torch.full((len(chosen),), -1, dtype=torch.int32, device="cuda")
    c._chk(abi.lib().rmcv_batch_icon_strips(c._h, abi.ptr(np.array(chosen, np.int32)), len(chosen), side, cap, buf.data_ptr(), stride, pitch, cnt.data_ptr(), None))
    c.sync()
    assert cnt.cpu().tolist() == [min(counts[f], cap) for f in chosen]
    host = buf.cpu().numpy()
    for k, f in enumerate(chosen):
        v = host[k * pitch:k * pitch + stride * side].reshape(side, stride)
        assert np.array_equal(v[:, :3 * cap * side].reshape(side, cap * side, 3), want_strip("bgr", f, side, cap)) and (v[:, 3 * cap * side:] == 0xEE).all()
        assert (host[k * pitch + stride * side:(k + 1) * pitch] == 0xEE).all()
    # with the classifier's stage: the same strips (the clamp it writes back is idempotent), and slot j at 20 x 20 is row j of Context.icons
    c.svm_load(np.zeros((1, abi.SVM_FEATURES), np.float32), np.zeros(1), np.array([3, 5], np.int32))
    c.run(p, DETECT | STAGE_IDENTITY)
    with_identity = armours_of(c)
    assert any(a.tobytes() != b.tobytes() for a, b in zip(arms, with_identity))   # (the stage clamped an icon in the table: the strips still agree)
    for side in (20, 80):
        for cap in (small_cap, large_cap):
            assert np.array_equal(c.icon_strips(list(range(8)), side, cap), first[side, cap]), (side, cap)
    for f in range(8):
        rows = c.icons(f)
        assert len(rows) == counts[f]
        for j in range(counts[f]):
            assert np.array_equal(first[20, large_cap][f][:, 20 * j:20 * j + 20], rows[j]), (f, j)
    assert c.check_guards()[0] == 0


def test_borrowed_frames_with_an_odd_stride(small):
    import torch
    c = small
    frames = frames_of(W, H, SPECIAL)
    stride, pitch = 3 * W + 1, (3 * W + 1) * H + 3
    total = 1 + 7 * pitch + stride * (H - 1) + 3 * W
    host = np.full(total, 0x5A, np.uint8)
    for f in range(8):
        rows = np.lib.stride_tricks.as_strided(host[1 + f * pitch:], (H, 3 * W), (stride, 1))
        rows[:] = frames[f].reshape(H, 3 * W)
    dev = torch.from_numpy(host).cuda()
    c.bind_device_frames(dev.data_ptr() + 1, 8, H, W, stride=stride, frame_pitch=pitch, keepalive=dev)
    c.run(default_params(tilt_max=TILT), DETECT)
    arms = armours_of(c)
    assert sum(len(a) for a in arms) >= 2
    for side in (20, 80):
        check_strips(c, "bgr", frames, arms, side, 4)
    c.upload(frames)  # (the borrowed buffer is let go)


@pytest.mark.parametrize("pattern", BR.PATTERNS)
def test_bayer_plain_strips(pattern):
    frames = frames_of(W, H, SPECIAL)
    m = BR.mosaic(frames, pattern)
    c = Context(device=0, **LIMITS)
    try:
        c.set_input_format(pattern)
        c.upload(m)
        c.run(default_params(tilt_max=TILT), DETECT)
        arms = armours_of(c)
        assert sum(len(a) for a in arms) >= 2
        srcs = [SR.src_bayer(m[f], pattern) for f in range(8)]
        for side in (20, 80):
            check_strips(c, ("bayer", pattern), srcs, arms, side, 4)
        assert c.check_guards()[0] == 0
    finally:
        c.close()


def test_bayer_sensor_layout_strips():
    """16-bit samples with the pixel at bits 2 .. 9, mirrored and flipped, an odd width"""
    w, h, pattern = 203, 136, BR.GB
    frames = frames_of(w, h, SPECIAL)
    oriented = RR.derived_pattern(pattern, w, h, True, True)
    r = RR.delivered(BR.mosaic(frames, oriented), 16, 2, True, True, np.random.default_rng(3))
    c = Context(device=0, **LIMITS)
    try:
        c.set_input_format(pattern)
        c.set_input_layout(16, 2, True, True)
        c.upload(r)
        c.run(default_params(tilt_max=TILT), DETECT)
        arms = armours_of(c)
        assert sum(len(a) for a in arms) >= 2
        srcs = [SR.src_bayer(r[f], pattern, 2, True, True) for f in range(8)]
        for side in (20, 80):
            check_strips(c, "layout", srcs, arms, side, 4)
        assert c.check_guards()[0] == 0
    finally:
        c.close()


def test_enhanced_strips():
    frames = ER.dim(frames_of(W, H, SPECIAL), 96)
    c = Context(device=0, **LIMITS)
    try:
        c.set_enhance(True)
        c.upload(frames)
        c.run(default_params(tilt_max=TILT), DETECT)
        arms = armours_of(c)
        assert sum(len(a) for a in arms) >= 2
        srcs, tables = zip(*[SR.src_enhanced(frames[f]) for f in range(8)])
        assert any((t != np.arange(256)).any() for t in tables)  # the gamma is not 1: a missed lookup shows
        for side in (20, 80):
            got = check_strips(c, "enhanced", srcs, arms, side, 4)
            BATCHES["dim"] = (frames, arms)
            assert any((got[f] != want_strip("dim", f, side, 4)).any() for f in range(8))   # (not the strip of the frame as delivered)
        assert c.check_guards()[0] == 0
    finally:
        c.close()


def test_windowed_strips(small):
    ww, wh = 96, 64
    c = small
    frames = frames_of(W, H, SPECIAL)
    origins = np.array([(55, 22), (51, 30), (64, 41), (30, 57), (54, 30), (79, 48), (31, 45), (50, 35)], np.int32)   # around the frames' armours
    c.upload(frames)
    c.set_windows(origins, ww, wh)
    try:
        c.run(default_params(tilt_max=TILT), DETECT)
        arms = armours_of(c)
        assert sum(len(a) for a in arms) >= 4
        icons = np.concatenate([a["icon"].reshape(-1, 2) for a in arms if len(a)])
        # icons leave the window above and below, at rows that lie inside the 136-row frame: they clamp to the window, not to the frame
        assert icons[:, 1].min() < 0 and wh - 1 < icons[:, 1].max() < H - 1
        srcs = [SR.src_window(frames[f], origins[f], ww, wh) for f in range(8)]
        assert all(s.shape == (wh, ww, 3) for s in srcs)
        for side in (20, 80):
            check_strips(c, "window", srcs, arms, side, 4)
    finally:
        c.set_windows(None, 0, 0)


def lists_of(c, oracle, f, arm):
    pts, co = c.contours(f)
    blobs, _ = c.blobs(f)
    ob, _, neg = oracle.filter_lightblobs(pts, co, oracle.default_params(tilt_max=TILT))
    assert ob.tobytes() == blobs.tobytes()
    return blobs, [np.stack([pts["x"][co[i]:co[i + 1]], pts["y"][co[i]:co[i + 1]]], 1) for i in neg], arm


def test_sheets(small, oracle):
    import torch
    c = small
    frames = frames_of(W, H, SPECIAL)
    c.upload(frames)
    c.run(default_params(tilt_max=TILT), DETECT)
    arms = armours_of(c)
    chosen = [2, 0, 1]
    lists = {f: lists_of(c, oracle, f, arms[f]) for f in chosen}
    binaries = {f: c.binary(f) for f in chosen}
    for size in ((200, 136), (100, 68)):
        for side in (20, 80):
            got = c.labeler_sheets(chosen, size, side, VIEW_ALL)
            assert got.shape == (3, size[1] + side, 2 * size[0], 3)
            left, right = c.source_views(chosen, size=size, flags=VIEW_ALL), c.debug_views(chosen, size, 0)
            for k, f in enumerate(chosen):
                assert np.array_equal(got[k], labeler_sheet_host(frames[f], binaries[f], *lists[f], size, side, VIEW_ALL)), (size, side, f)
                assert np.array_equal(got[k], S.sheet_ref(frames[f], binaries[f], *lists[f], size, side, VIEW_ALL, c.limits.max_armours)), (size, side, f)
                assert np.array_equal(got[k][:size[1], :size[0]], left[k]) and np.array_equal(got[k][:size[1], size[0]:], right[k])
            assert np.array_equal(c.labeler_sheet(2, size, side, VIEW_ARMOURS), S.sheet_ref(frames[2], binaries[2], *lists[2], size, side, VIEW_ARMOURS, c.limits.max_armours))
    # a poisoned output with padded rows and sheets: the padding bytes are untouched
    size, side = (100, 68), 20
    rows, stride = size[1] + side, 6 * size[0] + 10
    pitch = stride * rows + 32
    buf = torch.full((len(chosen) * pitch,), 0xEE, dtype=torch.uint8, device="cuda")
    c._chk(abi.lib().rmcv_batch_labeler_sheets(c._h, abi.ptr(np.array(chosen, np.int32)), len(chosen), size[0], size[1], side, VIEW_ALL, buf.data_ptr(), stride, pitch, None))
    c.sync()
    host = buf.cpu().numpy()
    want = c.labeler_sheets(chosen, size, side, VIEW_ALL)
    for k in range(len(chosen)):
        v = host[k * pitch:k * pitch + stride * rows].reshape(rows, stride)
        assert np.array_equal(v[:, :6 * size[0]].reshape(rows, 2 * size[0], 3), want[k]) and (v[:, 6 * size[0]:] == 0xEE).all()
        assert (host[k * pitch + stride * rows:(k + 1) * pitch] == 0xEE).all()
    assert c.check_guards()[0] == 0


def test_pipeline_sheets(small):
    import torch
    dst, side, chosen = (100, 68), 20, [0, 2, 7]
    p = default_params(tilt_max=TILT)
    sets = [frames_of(W, H, SPECIAL), frames_of(W, H, [(0, 40, 0), (7, 1003, 1)]), frames_of(W, H, [(3, 77, 0)])[::-1].copy()]
    want, want_src, want_bin, want_lab = [], [], [], []
    for fr in sets:  # the context path (equal to the restatement: test_sheets)
        small.upload(fr)
        small.run(p, STAGE_ALL)
        want.append(small.labeler_sheets(chosen, dst, side, VIEW_ALL))
        want_src.append(small.source_views(chosen, size=dst))
        want_bin.append(small.debug_views(chosen, dst))
        lab = torch.from_numpy(want_src[-1]).cuda()                      # the labels over the source view alone
        small.batch_view_labels(chosen, lab.data_ptr(), dst, 1)
        small.sync()
        want_lab.append(lab.cpu().numpy())
    assert any((a != b).any() for a, b in zip(want[:-1], want[1:])) and any((a != b).any() for a, b in zip(want_src, want_lab))
    dev = [torch.from_numpy(fr).cuda() for fr in sets]
    pl = Pipeline(device=0, depth=2, **LIMITS)
    try:
        pl.set_views(chosen, dst)
        t = pl.submit(dev[1].data_ptr(), 8, H, W, p, STAGE_ALL)
        pl.wait(t)
        before_bin = pl.views(t).cpu().numpy()
        assert np.array_equal(before_bin, want_bin[1])
        pl.set_sheets(chosen, dst, side, VIEW_ALL)
        tickets = []
        for k in range(3):
            tickets.append(pl.submit(dev[k].data_ptr(), 8, H, W, p, STAGE_ALL))
            if k >= 1:  # ticket k - 1: its record, and its sheets, live until ticket k + 1 is submitted
                pl.wait(tickets[k - 1])
                v = pl.views(tickets[k - 1])
                assert tuple(v.shape) == (3, dst[1] + side, 2 * dst[0], 3) and v.dtype == torch.uint8
                assert np.array_equal(v.cpu().numpy(), want[k - 1]), k - 1
        pl.wait(tickets[2])
        assert np.array_equal(pl.views(tickets[2]).cpu().numpy(), want[2])
        assert pl.get_info().host_blocking_calls == 0
        # with the view labels on, the left pane is the labels over the source view; the other parts are as they were
        pl.set_view_labels(LABEL_ARMOURS, 1)
        t = pl.submit(dev[0].data_ptr(), 8, H, W, p, STAGE_ALL)
        pl.wait(t)
        v = pl.views(t).cpu().numpy()
        assert np.array_equal(v[:, :dst[1], :dst[0]], want_lab[0])
        assert np.array_equal(v[:, :dst[1], dst[0]:], want[0][:, :dst[1], dst[0]:]) and np.array_equal(v[:, dst[1]:], want[0][:, dst[1]:])
        pl.set_view_labels(0)
        with pytest.raises(RmcvError):  # fewer frames than the sheets name; stages that lack the armours
            pl.submit(dev[0].data_ptr(), 4, H, W, p, STAGE_ALL)
        with pytest.raises(RmcvError):
            pl.submit(dev[0].data_ptr(), 8, H, W, p, STAGE_BINARY | STAGE_CONTOURS | STAGE_BLOBS)
        with pytest.raises(RmcvError):  # side > 2 vw
            pl.set_sheets(chosen, (9, 68), 20)
        # the latest setter wins: the binary's views are what they were before any sheet was set
        pl.set_sheets(chosen, dst, side, VIEW_ARMOURS)
        pl.set_views(chosen, dst)
        t = pl.submit(dev[1].data_ptr(), 8, H, W, p, STAGE_ALL)
        pl.wait(t)
        assert np.array_equal(pl.views(t).cpu().numpy(), before_bin)
        pl.set_sheets(chosen, dst, side, VIEW_ALL)
        pl.set_sheets(None)  # n == 0: off
        t = pl.submit(dev[0].data_ptr(), 8, H, W, p, STAGE_ALL)
        pl.wait(t)
        with pytest.raises(RmcvError):
            pl.views(t)
        pl.set_views(chosen, dst, source=True)
        t = pl.submit(dev[2].data_ptr(), 8, H, W, p, STAGE_ALL)
        pl.wait(t)
        assert np.array_equal(pl.views(t).cpu().numpy(), want_src[2])
        assert pl.get_info().host_blocking_calls == 0
    finally:
        pl.close()


def test_refusals_on_the_device_paths(small):
    import torch
    c = small
    frames = frames_of(W, H, [])
    c.upload(frames)
    with pytest.raises(RmcvError):  # nothing run yet
        c.icon_strips([0], 20, 4)
    c.run(default_params(), STAGE_BINARY | STAGE_CONTOURS | STAGE_BLOBS)
    with pytest.raises(RmcvError) as e:  # the run lacked the armours
        c.icon_strips([0], 20, 4)
    assert "RMCV_STAGE_ARMOURS" in str(e.value)
    with pytest.raises(RmcvError):
        c.labeler_sheets([0], (100, 68), 20, 0)
    c.run(default_params(), DETECT)
    L, one, two = abi.lib(), np.zeros(1, np.int32), np.array([0, 1], np.int32)
    buf = torch.zeros(2 * 3 * 4 * 20 * 20 + 64, dtype=torch.uint8, device="cuda")
    cnt = torch.full((2,), -1, dtype=torch.int32, device="cuda")

    def strips(fr=one, n=1, side=20, cap=4, out=buf.data_ptr(), stride=240, pitch=4800):
        return L.rmcv_batch_icon_strips(c._h, abi.ptr(fr) if fr is not None else None, n, side, cap, out, stride, pitch, cnt.data_ptr(), None)
    for bad, word in ((dict(fr=None), "no frames"), (dict(n=0), "no frames"), (dict(fr=np.array([8], np.int32)), "outside"), (dict(fr=np.array([-1], np.int32)), "outside"),
                      (dict(fr=np.array([1, 1], np.int32), n=2), "repeated"), (dict(fr=np.arange(9, dtype=np.int32), n=9), "more strips"), (dict(side=0), "side"),
                      (dict(side=257), "side"), (dict(cap=0), "cap"), (dict(cap=c.limits.max_armours + 1), "cap"), (dict(stride=239), "out_stride"),
                      (dict(fr=two, n=2, pitch=4799), "out_pitch"), (dict(out=None), "null output")):
        assert strips(**bad) == abi.ERR_BAD_ARG, bad
        assert word in L.rmcv_last_error(c._h).decode(), (bad, L.rmcv_last_error(c._h).decode())
    c.sync()
    assert not buf.any().item() and cnt.cpu().tolist() == [-1, -1]      # refused before anything was enqueued
    assert strips(fr=two, n=2) == 0
    out = np.zeros((20, 80, 3), np.uint8)
    assert L.rmcv_batch_get_icon_strip(c._h, 0, 20, 4, None, 240, None) == abi.ERR_BAD_ARG
    assert L.rmcv_batch_get_icon_strip(c._h, 8, 20, 4, abi.ptr(out), 240, None) == abi.ERR_BAD_ARG
    assert L.rmcv_batch_get_icon_strip(c._h, 0, 20, 4, abi.ptr(out), 239, None) == abi.ERR_BAD_ARG
    # the sheets: what the views refuse, and their own
    big = torch.zeros(2 * 600 * 88 + 64, dtype=torch.uint8, device="cuda")

    def sheets(fr=one, n=1, vw=100, vh=68, side=20, flags=VIEW_ALL, out=big.data_ptr(), stride=600, pitch=600 * 88):
        return L.rmcv_batch_labeler_sheets(c._h, abi.ptr(fr) if fr is not None else None, n, vw, vh, side, flags, out, stride, pitch, None)
    for bad, word in ((dict(fr=None), "no frames"), (dict(fr=np.array([8], np.int32)), "outside"), (dict(fr=np.array([1, 1], np.int32), n=2), "repeated"),
                      (dict(vw=0), "view size"), (dict(vw=641, stride=3846), "view size"), (dict(vh=401), "view size"), (dict(flags=8), "flags"), (dict(side=0), "side"),
                      (dict(side=257, vw=200, stride=1200), "side"), (dict(vw=9, stride=54), "side > 2 vw"), (dict(stride=599), "out_stride"),
                      (dict(fr=two, n=2, pitch=600 * 88 - 1), "out_pitch"), (dict(out=None), "null output")):
        assert sheets(**bad) == abi.ERR_BAD_ARG, bad
        assert word in L.rmcv_last_error(c._h).decode(), (bad, L.rmcv_last_error(c._h).decode())
    c.sync()
    assert not big.any().item()
    assert sheets(fr=two, n=2) == 0
    c.sync()
    for size, side in (((0, 10), 4), ((10, 0), 4), ((10, 10), 21), ((10, 10), 0)):
        with pytest.raises(RmcvError):
            c.labeler_sheet(0, size, side)
    # a frame that exceeded a limit: the batch calls render what the tables hold, the one-frame getters refuse
    tiny = Context(device=0, max_contours=1, **LIMITS)
    try:
        tiny.upload(frames)
        tiny.run(default_params(), DETECT)
        st = tiny.counts()["status"]
        over = [f for f in range(8) if st[f] & abi.FRAME_OVF_CONTOURS]
        assert over
        with pytest.raises(RmcvError):
            tiny.icon_strip(over[0], 20, 4)
        with pytest.raises(RmcvError):
            tiny.labeler_sheet(over[0], (100, 68), 20)
        assert tiny.icon_strips(over[:1], 20, 4).shape == (1, 20, 80, 3)
        assert tiny.labeler_sheets(over[:1], (100, 68), 20).shape == (1, 88, 200, 3)
        assert tiny.check_guards()[0] == 0
    finally:
        tiny.close()
    # nothing bound
    fresh = Context(device=0, **LIMITS)
    try:
        with pytest.raises(RmcvError) as e:
            fresh.icon_strips([0], 20, 4)
        assert "no frames are bound" in str(e.value)
    finally:
        fresh.close()
    # the stage-wise helper's
    img = K.frame()
    arm = S.armours_of([np.array(K.QUAD, np.float32)])
    for kw in (dict(side=0), dict(side=257), dict(cap=0), dict(cap=c.limits.max_armours + 1)):
        with pytest.raises(RmcvError):
            c.icon_strip_of(img, arm, **dict(dict(side=20, cap=2), **kw))
    with pytest.raises(RmcvError):
        c.icon_strip_of(np.zeros((8, 700, 3), np.uint8), arm, 20, 2)
    # the context still works
    assert c.icon_strips([1], 20, 4).shape == (1, 20, 80, 3)


def test_one_frame_table_serves_calls_on_two_streams():
    """The chosen frames of every view, label, strip, sheet, corner and chessboard call travel through ONE table of the context
    (rmcv_ctx::frame_list), written behind the context's ordering event.  Corners of frames [3, 1] on a caller stream A, at once debug views
    of [0, 2] on a second stream B, then a strip of [2] on A again: each result equals, bit for bit, what the same call returns alone on a
    fresh context from the same frames -- no call's list lands before the kernels of the call before have read theirs -- and the same holds
    for a second round in the same context."""
    import torch
    frames = frames_of(W, H, SPECIAL)[:4]
    p = default_params(tilt_max=TILT)
    view, side, cap = (100, 68), 20, 4
    guess = np.tile(np.array([(30, 30), (60, 40), (100, 70), (150, 100), (170, 20), (20, 120)], np.float32), (2, 1, 1))

    def fresh():
        c = Context(device=0, max_frames=4, max_width=W, max_height=H)
        c.upload(frames)
        c.run(p, STAGE_ALL)
        return c

    alone = []
    for call in (lambda c: c.refine_corners([3, 1], guess), lambda c: c.debug_views([0, 2], view), lambda c: c.icon_strips([2], side, cap)):
        c = fresh()
        try:
            alone.append(call(c))
        finally:
            c.close()
    (want_corners, want_status), want_views, want_strips = alone
    assert want_corners[0].tobytes() != want_corners[1].tobytes() and not np.array_equal(want_views[0], want_views[1])   # (a list that went astray would show)
    c = fresh()
    try:
        c.sync()
        a, b = torch.cuda.Stream(), torch.cuda.Stream()
        corners, status = torch.empty((2, 6, 2), dtype=torch.float32, device="cuda"), torch.empty((2, 6), dtype=torch.int32, device="cuda")
        views = torch.empty((2, view[1], view[0], 3), dtype=torch.uint8, device="cuda")
        strips = torch.empty((1, side, cap * side, 3), dtype=torch.uint8, device="cuda")
        for _ in range(2):
            corners.copy_(torch.from_numpy(guess))
            status.fill_(-1), views.fill_(0xEE), strips.fill_(0xEE)
            torch.cuda.synchronize()
            c.refine_corners([3, 1], corners.data_ptr(), status=status.data_ptr(), per_frame=6, stream=a.cuda_stream)
            c.debug_views([0, 2], view, out=views.data_ptr(), stream=b.cuda_stream)
            c.icon_strips([2], side, cap, dst=strips.data_ptr(), stream=a.cuda_stream)
            a.synchronize(), b.synchronize()
            assert corners.cpu().numpy().tobytes() == want_corners.tobytes() and status.cpu().numpy().tolist() == want_status.tolist()
            assert np.array_equal(views.cpu().numpy(), want_views)
            assert np.array_equal(strips.cpu().numpy(), want_strips)
            assert c.check_guards()[0] == 0
    finally:
        c.close()
