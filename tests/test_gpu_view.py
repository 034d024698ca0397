"""The operator's debug view on the GPU (k_view.hip): the device's views equal tests/view_ref.py -- the independent restatement
of executable/main.cpp:200-207 -- and rmcv_debug_view_host, byte for byte: the stage-wise helper on the CPU case list, batches of synthetic
frames (whole, without the byte image, windowed), and a pipeline's per-slot views."""
import functools

import numpy as np
import pytest

import view_cases as K
import view_ref as R
from rmcv_amd import (CAMP_BLUE, STAGE_ALL, STAGE_BINARY, STAGE_CONTOURS, STAGE_NO_IMAGE, VIEW_ALL, VIEW_ARMOURS, VIEW_BLOBS, VIEW_NEGATIVES, Context, Pipeline,
                      RmcvError, debug_view_host, default_params, synth)
from rmcv_amd import abi

pytestmark = pytest.mark.gpu

TILT = 10.0  # makes negatives of the synthetic stream's tilted bars


@functools.lru_cache(maxsize=None)
def case_refs(k):
    """(binary, cases, reference views) of size pair k: computed once, shared"""
    src, dst = K.SIZES[k]
    binary = K.binary(*src)
    cases = K.cases(*src)
    return binary, cases, [R.view(binary, c["blobs"], c["negatives"], c["armours"], dst) for c in cases]


@pytest.fixture(scope="module")
def small():
    c = Context(device=0, max_frames=8, max_width=320, max_height=256)
    yield c
    c.close()


@pytest.mark.parametrize("k", range(len(K.SIZES)), ids=["%dx%d-%dx%d" % (s + d) for s, d in K.SIZES])
def test_stagewise_view_equals_the_reference(small, k):
    binary, cases, refs = case_refs(k)
    for case, want in zip(cases, refs):
        got = small.debug_view_of(binary, case["blobs"], case["negatives"], case["armours"], K.SIZES[k][1])
        assert np.array_equal(got, want), case["name"]


@pytest.mark.parametrize("flags", [0, VIEW_BLOBS, VIEW_NEGATIVES, VIEW_ARMOURS])
def test_stagewise_flags(small, flags):
    binary, cases, _ = case_refs(0)
    for case in cases:
        if case["name"] in ("crossing", "random", "blue_then_red"):
            got = small.debug_view_of(binary, case["blobs"], case["negatives"], case["armours"], K.SIZES[0][1], flags)
            assert np.array_equal(got, R.view(binary, case["blobs"], case["negatives"], case["armours"], K.SIZES[0][1], flags)), case["name"]


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


GEOMS = [((200, 136), (160, 102), [(0, 3, 0), (3, 1000, 1)]), ((320, 256), (256, 192), [(0, 0, 0), (3, 1001, 1)])]


@pytest.mark.parametrize("src,dst,special", GEOMS, ids=["200x136", "320x256"])
def test_batch_views(small, oracle, src, dst, special):
    w, h = src
    c = small
    frames = frames_of(w, h, special)
    p = default_params(tilt_max=TILT)
    c.upload(frames)
    c.run(p, STAGE_ALL)
    c.sync()
    arm, offs = c.armours()
    want, rich = {}, 0
    for f in range(8):
        binary = c.binary(f)
        blobs, negatives, armours = lists_of(c, oracle, f, arm, offs)
        rich += len(blobs) >= 1 and len(negatives) >= 1 and len(armours) >= 1
        want[f] = R.view(binary, blobs, negatives, armours, dst)
        assert np.array_equal(debug_view_host(binary, blobs, negatives, armours, dst), want[f]), f
    assert rich >= 1  # (a view of empty overlays would prove nothing)
    for chosen in ([0, 3, 7], list(range(8)), [5]):
        got = c.debug_views(chosen, dst)
        for k, f in enumerate(chosen):
            assert np.array_equal(got[k], want[f]), (chosen, f)
    assert np.array_equal(c.debug_view(3, dst), want[3])
    # a caller's device buffer with padded rows and views
    import torch
    stride, pitch = 3 * dst[0] + 20, (3 * dst[0] + 20) * dst[1] + 64
    buf = torch.zeros(3 * pitch, dtype=torch.uint8, device="cuda")
    c._chk(abi.lib().rmcv_batch_debug_views(c._h, abi.ptr(np.array([7, 0, 3], np.int32)), 3, dst[0], dst[1], VIEW_ALL, buf.data_ptr(), stride, pitch, None))
    c.sync()
    host = buf.cpu().numpy()
    for k, f in enumerate([7, 0, 3]):
        v = host[k * pitch:k * pitch + stride * dst[1]].reshape(dst[1], stride)
        assert np.array_equal(v[:, :3 * dst[0]].reshape(dst[1], dst[0], 3), want[f]) and not v[:, 3 * dst[0]:].any()
    # without the byte image the views are the same: they never read it
    c.upload(frames[::-1].copy())  # (other contents in the byte image first)
    c.run(p, STAGE_ALL)
    c.upload(frames)
    c.run(p, STAGE_ALL | STAGE_NO_IMAGE)
    got = c.debug_views(list(range(8)), dst)
    for f in range(8):
        assert np.array_equal(got[f], want[f]), f
    assert c.check_guards()[0] == 0


def test_windowed_batch_views(small, oracle):
    fw, fh, ww, wh, dst = 320, 256, 128, 96, (96, 72)
    c = small
    frames = frames_of(fw, fh, [(0, 0, 0), (3, 1001, 1)])
    rng = np.random.default_rng(5)
    origins = np.stack([rng.integers(-20, fw, 8), rng.integers(-20, fh, 8)], 1).astype(np.int32)
    c.upload(frames)
    c.set_windows(origins, ww, wh)
    c.run(default_params(tilt_max=TILT), STAGE_ALL)
    c.sync()
    arm, offs = c.armours()
    got = c.debug_views(list(range(8)), dst)
    lit = 0
    for f in range(8):
        binary = c.binary(f)
        assert binary.shape == (wh, ww)
        blobs, negatives, armours = lists_of(c, oracle, f, arm, offs)
        assert np.array_equal(got[f], R.view(binary, blobs, negatives, armours, dst)), f
        lit += int(binary.any())
    assert lit >= 1
    c.set_windows(None, 0, 0)


def test_pipeline_views(small):
    import torch
    w, h, dst, chosen = 200, 136, (160, 102), [0, 3, 7]
    p = default_params(tilt_max=TILT)
    sets = [frames_of(w, h, [(0, 3, 0), (3, 1000, 1)]), frames_of(w, h, [(0, 40, 0), (7, 1003, 1)]), frames_of(w, h, [(3, 77, 0)])[::-1].copy()]
    want, want_arm = [], []
    for fr in sets:  # the context path
        small.upload(fr)
        small.run(p, STAGE_ALL)
        want.append(small.debug_views(chosen, dst))
        want_arm.append(small.armours()[0].tobytes())
    assert any((a != b).any() for a, b in zip(want[:-1], want[1:]))
    dev = [torch.from_numpy(fr).cuda() for fr in sets]
    pl = Pipeline(device=0, depth=2, max_frames=8, max_width=320, max_height=256)
    plain = Pipeline(device=0, depth=2, max_frames=8, max_width=320, max_height=256)
    try:
        pl.set_views(chosen, dst)
        tickets = []
        for k in range(3):
            tickets.append(pl.submit(dev[k].data_ptr(), 8, h, w, p, STAGE_ALL))
            if k >= 1:  # ticket k - 1: its record, and its views, live until ticket k + 1 is submitted
                pl.wait(tickets[k - 1])
                v = pl.views(tickets[k - 1])
                assert tuple(v.shape) == (3, dst[1], dst[0], 3) and v.dtype == torch.uint8
                assert np.array_equal(v.cpu().numpy(), want[k - 1]), k - 1
                assert pl.collect(tickets[k - 1])[0].tobytes() == want_arm[k - 1]
        pl.wait(tickets[2])
        assert np.array_equal(pl.views(tickets[2]).cpu().numpy(), want[2])
        assert pl.get_info().host_blocking_calls == 0
        with pytest.raises(RmcvError):  # fewer frames than the views name; stages that lack what the flags need
            pl.submit(dev[0].data_ptr(), 4, h, w, p, STAGE_ALL)
        with pytest.raises(RmcvError):
            pl.submit(dev[0].data_ptr(), 8, h, w, p, STAGE_BINARY | STAGE_CONTOURS)
        # views off: the batches are what a pipeline that never had views produces
        pl.set_views(None)
        for k in range(3):
            a = pl.collect(pl.submit(dev[k].data_ptr(), 8, h, w, p, STAGE_ALL))
            b = plain.collect(plain.submit(dev[k].data_ptr(), 8, h, w, p, STAGE_ALL))
            assert a[0].tobytes() == b[0].tobytes() == want_arm[k] and a[1].tolist() == b[1].tolist()
        t = pl.submit(dev[0].data_ptr(), 8, h, w, p, STAGE_ALL)
        pl.wait(t)
        with pytest.raises(RmcvError):
            pl.views(t)
        assert pl.get_info().host_blocking_calls == 0
    finally:
        pl.close()
        plain.close()


def test_refusals_on_the_device_paths(small):
    c = small
    w, h, dst = 200, 136, (160, 102)
    frames = frames_of(w, h, [])
    c.upload(frames)
    c.run(default_params(), STAGE_BINARY | STAGE_CONTOURS)
    with pytest.raises(RmcvError):  # the run lacked the stages the flags need
        c.debug_views([0], dst)
    assert c.debug_views([0], dst, flags=0).shape == (1, dst[1], dst[0], 3)
    c.run(default_params(), STAGE_ALL)
    for bad in ([8], [-1], [0, 0], [], list(range(8)) + [0]):
        with pytest.raises(RmcvError):
            c.debug_views(bad, dst)
    for size in ((0, 10), (10, 0), (321, 10), (10, 257)):
        with pytest.raises(RmcvError):
            c.debug_views([0], size)
        with pytest.raises(RmcvError):
            c.debug_view(0, size)
    with pytest.raises(RmcvError):
        c.debug_views([0], dst, flags=8)
    L = abi.lib()
    one = np.zeros(1, np.int32)
    import torch
    buf = torch.zeros(2 * 3 * dst[0] * dst[1], dtype=torch.uint8, device="cuda")
    assert L.rmcv_batch_debug_views(c._h, abi.ptr(one), 1, dst[0], dst[1], VIEW_ALL, buf.data_ptr(), 3 * dst[0] - 1, 0, None) == abi.ERR_BAD_ARG
    assert L.rmcv_batch_debug_views(c._h, abi.ptr(np.array([0, 1], np.int32)), 2, dst[0], dst[1], VIEW_ALL, buf.data_ptr(), 3 * dst[0], 3 * dst[0] * dst[1] - 1, None) == abi.ERR_BAD_ARG
    assert L.rmcv_batch_debug_views(c._h, abi.ptr(one), 1, dst[0], dst[1], VIEW_ALL, None, 3 * dst[0], 0, None) == abi.ERR_BAD_ARG
    # a frame that exceeded a limit: the batch call renders what the tables hold, the one-frame getter refuses
    tiny = Context(device=0, max_frames=8, max_width=320, max_height=256, max_contours=1)
    try:
        tiny.upload(frames)
        tiny.run(default_params(), STAGE_ALL)
        st = tiny.counts()["status"]
        over = [f for f in range(8) if st[f] & abi.FRAME_OVF_CONTOURS]
        assert over
        with pytest.raises(RmcvError):
            tiny.debug_view(over[0], dst)
        assert tiny.debug_views(over[:1], dst).shape == (1, dst[1], dst[0], 3)
        assert tiny.check_guards()[0] == 0
    finally:
        tiny.close()
    with pytest.raises(RmcvError):  # the stage-wise helper's
        c.debug_view_of(np.zeros((8, 8), np.uint8), size=(0, 3))
    with pytest.raises(RmcvError):
        c.debug_view_of(np.zeros((8, 400), np.uint8), size=(4, 4))
    # the context still works
    assert c.debug_views([1], dst).shape == (1, dst[1], dst[0], 3)
