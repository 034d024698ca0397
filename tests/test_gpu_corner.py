"""Corner refinement on the GPU (k_corner.hip): the kernel's corners and status words equal rmcv_corner_subpix_host byte for
byte -- the stage-wise helper on every case of tests/corner_cases.py; the batch call on 3 frames of 160 x 128 through all five kinds of
source (BGR, windows off the dword grid behind a run, RMCV_OPT_ENHANCE, an 8-bit mosaic in two patterns, a 16-bit mirrored and flipped
layout), each against the host function on SRC(f) computed on the host; every launch shape; the getter; the refusals."""

import numpy as np
import pytest

import bayer_ref as BR
import corner_cases as CC
import enhance_ref as ER
import raw_ref as RR
import source_view_ref as SR
import rmcv_amd as R
from rmcv_amd import STAGE_BINARY, Context, RmcvError, abi, default_params

pytestmark = pytest.mark.gpu

W, H = 160, 128
LIMITS = dict(max_frames=3, max_width=W, max_height=H)
BOARDS = ("affine160", "persp160", "edge160")
FRAMES = np.stack([CC.IMAGES[b] for b in BOARDS])                                                     # (3, 128, 160, 3)
GUESS = np.stack([next(c for c in CC.CASES if c.name == b + "-win8x8").corners for b in BOARDS])      # (3, 12, 2) float32
RULES = [((8, 8), (-1, -1), 40, 0.001), ((3, 3), (0, 0), 40, 0.001), ((15, 15), (2, 1), 7, 0.0), ((2, 11), (-1, -1), 40, 0.001)]


def host_rows(srcs, guess, rule, frames=None):
    """rmcv_corner_subpix_host on SRC(f) of the chosen frames -> (corners (n, per, 2), status (n, per))"""
    frames = range(len(srcs)) if frames is None else frames
    out = [R.corner_subpix_host(srcs[f], guess[k], *rule) for k, f in enumerate(frames)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def check_batch(c, srcs, guess, rules=RULES):
    for rule in rules:
        got, st = c.refine_corners([0, 1, 2], guess, None, *rule)
        want, want_st = host_rows(srcs, guess, rule)
        assert st.tolist() == want_st.tolist(), rule
        assert got.tobytes() == want.tobytes(), rule


@pytest.fixture(scope="module")
def ctx():
    c = Context(device=0, **LIMITS)
    yield c
    c.close()


def test_stagewise_equals_host_on_every_case(ctx):
    for case in CC.CASES:
        args = (CC.IMAGES[case.image], case.corners, case.win, case.zero, case.max_iters, case.eps)
        got, st = ctx.refine_corners_of(*args)
        want, want_st = R.corner_subpix_host(*args)
        assert st.tolist() == want_st.tolist(), case.name
        assert got.tobytes() == want.tobytes(), case.name
    assert ctx.check_guards()[0] == 0


def test_batch_bgr(ctx):
    ctx.upload(FRAMES)
    check_batch(ctx, FRAMES, GUESS)          # (plain BGR frames need no run)
    assert ctx.check_guards()[0] == 0


def test_batch_windows_off_the_dword_grid(ctx):
    import torch
    ww, wh = 112, 96
    stride, pitch = 3 * W + 1, (3 * W + 1) * H + 3     # rows at every byte phase, the first frame one byte into its buffer
    host = np.full(1 + 2 * pitch + stride * (H - 1) + 3 * W, 0x5A, np.uint8)
    for f in range(3):
        np.lib.stride_tricks.as_strided(host[1 + f * pitch:], (H, 3 * W), (stride, 1))[:] = FRAMES[f].reshape(H, 3 * W)
    dev = torch.from_numpy(host).cuda()
    origins = np.array([(20, 13), (47, 31), (-5, 200)], np.int32)
    ctx.bind_device_frames(dev.data_ptr() + 1, 3, H, W, stride=stride, frame_pitch=pitch, keepalive=dev)
    ctx.set_windows(origins, ww, wh)
    try:
        tab = np.zeros((1, 12, 2), np.float32)
        with pytest.raises(RmcvError, match="read behind a run with RMCV_STAGE_BINARY"):   # the effective origins do not exist yet
            ctx.refine_corners([0], tab)
        ctx.run(default_params(), STAGE_BINARY)
        eff = ctx.windows()[0]
        assert eff.tolist() == [[16, 13], [32, 31], [0, 32]]
        assert any((1 + f * pitch + int(eff[f][1]) * stride + 3 * int(eff[f][0])) % 4 for f in range(3))   # off the dword grid
        srcs = [SR.src_window(FRAMES[f], origins[f], ww, wh) for f in range(3)]
        assert all(s.shape == (wh, ww, 3) for s in srcs)
        guess = (GUESS - eff[:, None, :].astype(np.float32)).astype(np.float32)                             # window coordinates
        check_batch(ctx, srcs, guess)
        one, st1 = ctx.refined_corners(1, guess[1], *RULES[0])
        want, want_st = R.corner_subpix_host(srcs[1], guess[1], *RULES[0])
        assert one.tobytes() == want.tobytes() and st1.tolist() == want_st.tolist()
    finally:
        ctx.set_windows(None, 0, 0)
        ctx.upload(FRAMES)   # (the borrowed buffer is let go)


def test_batch_enhanced():
    frames = ER.dim(FRAMES, 96)
    c = Context(device=0, **LIMITS)
    try:
        c.set_enhance(True)
        c.upload(frames)
        with pytest.raises(RmcvError, match="read behind a run with RMCV_STAGE_BINARY"):   # the tables do not exist yet
            c.refine_corners([0], GUESS[:1])
        c.run(default_params(), STAGE_BINARY)
        srcs, tables = zip(*[SR.src_enhanced(frames[f]) for f in range(3)])
        assert any((t != np.arange(256)).any() for t in tables)  # the gamma is not 1: a missed lookup shows
        check_batch(c, srcs, GUESS)
        assert c.check_guards()[0] == 0
    finally:
        c.close()


@pytest.mark.parametrize("pattern", [BR.RG, BR.GB])
def test_batch_mosaic(pattern):
    m = BR.mosaic(FRAMES, pattern)
    c = Context(device=0, **LIMITS)
    try:
        c.set_input_format(pattern)
        c.upload(m)
        srcs = [SR.src_bayer(m[f], pattern) for f in range(3)]
        check_batch(c, srcs, GUESS)
        assert c.check_guards()[0] == 0
    finally:
        c.close()


def test_batch_sensor_layout():
    """16-bit samples with the pixel at bits 2 .. 9, mirrored and flipped"""
    pattern = BR.GB
    oriented = RR.derived_pattern(pattern, W, H, True, True)
    r = RR.delivered(BR.mosaic(FRAMES, oriented), 16, 2, True, True, np.random.default_rng(3))
    c = Context(device=0, **LIMITS)
    try:
        c.set_input_format(pattern)
        c.set_input_layout(16, 2, True, True)
        c.upload(r)
        srcs = [SR.src_bayer(r[f], pattern, 2, True, True) for f in range(3)]
        check_batch(c, srcs, GUESS)
        assert c.check_guards()[0] == 0
    finally:
        c.close()


def test_launch_shapes(ctx):
    import torch
    ctx.upload(FRAMES)
    rule = RULES[0]
    # chosen frames [2, 0]; 12 corners a frame, and 5 (no multiple of the four wavefronts of a workgroup)
    for per in (12, 5):
        guess = np.ascontiguousarray(GUESS[[2, 0], :per])
        got, st = ctx.refine_corners([2, 0], guess, None, *rule)
        want, want_st = host_rows(FRAMES, guess, rule, [2, 0])
        assert got.tobytes() == want.tobytes() and st.tolist() == want_st.tolist(), per
    # counts with a 0 and a partial count (and values beyond the range, which are clamped): entries beyond the count are untouched
    for counts in ([0, 7, 12], [5, 0, 1], [-3, 99, 4]):
        got, st = ctx.refine_corners([0, 1, 2], GUESS, counts, *rule)
        want, want_st = host_rows(FRAMES, GUESS, rule)
        for k, n in enumerate(np.clip(counts, 0, 12)):
            assert got[k, :n].tobytes() == want[k, :n].tobytes() and st[k, :n].tolist() == want_st[k, :n].tolist(), (counts, k)
            assert got[k, n:].tobytes() == GUESS[k, n:].tobytes() and not st[k, n:].any(), (counts, k)
    # device tables of the caller's, no status table, a stream of the caller's
    want, want_st = host_rows(FRAMES, GUESS, rule)
    stream = torch.cuda.Stream()
    tab = torch.from_numpy(GUESS.copy()).cuda()
    status = torch.full((3, 12), -1, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    assert ctx.refine_corners([0, 1, 2], tab.data_ptr(), None, *rule, status=None, per_frame=12, stream=stream.cuda_stream) is None
    stream.synchronize()
    assert tab.cpu().numpy().tobytes() == want.tobytes() and (status.cpu().numpy() == -1).all()
    tab.copy_(torch.from_numpy(GUESS))
    torch.cuda.synchronize()
    ctx.refine_corners([0, 1, 2], tab.data_ptr(), None, *rule, status=status.data_ptr(), per_frame=12)
    ctx.sync()
    assert tab.cpu().numpy().tobytes() == want.tobytes() and status.cpu().numpy().tolist() == want_st.tolist()
    # borrowed device frames
    dev = torch.from_numpy(FRAMES.copy()).cuda()
    ctx.bind_device_frames(dev.data_ptr(), 3, H, W, keepalive=dev)
    got, st = ctx.refine_corners([1], GUESS[1:2], None, *rule)
    assert got.tobytes() == want[1:2].tobytes() and st.tolist() == want_st[1:2].tolist()
    ctx.upload(FRAMES)
    assert ctx.check_guards()[0] == 0


def test_getter_equals_the_batch_call(ctx):
    ctx.upload(FRAMES)
    for rule in RULES:
        batch, batch_st = ctx.refine_corners([0, 1, 2], GUESS, None, *rule)
        for f in range(3):
            got, st = ctx.refined_corners(f, GUESS[f], *rule)
            assert got.tobytes() == batch[f].tobytes() and st.tolist() == batch_st[f].tolist(), (rule, f)
    got, st = ctx.refined_corners(2, GUESS[2, :1], *RULES[0])             # a single corner
    one, one_st = ctx.refine_corners([2], GUESS[2:3, :1], None, *RULES[0])
    assert got.tobytes() == one[0].tobytes() and st.tolist() == one_st[0].tolist()


def test_refusals_enqueue_nothing(ctx):
    import torch
    ctx.upload(FRAMES)
    tab = torch.from_numpy(GUESS.copy()).cuda()
    status = torch.full((3, 12), -1, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    ok = dict(frames=[0, 1, 2], corners=tab.data_ptr(), per_frame=12, win=(8, 8), zero_zone=(-1, -1), max_iters=40, eps=0.001, status=status.data_ptr())
    bad = [
        (dict(frames=[]), "source views: no frames chosen"),
        (dict(frames=[0, 1, 2, 0]), "source views: more views than the batch has frames"),
        (dict(frames=[0, 3]), "source views: a frame index is outside the batch"),
        (dict(frames=[-1]), "source views: a frame index is outside the batch"),
        (dict(frames=[1, 1]), "source views: a frame index is repeated"),
        (dict(corners=0), "corners: null corner table"),
        (dict(per_frame=0), "corners: per_frame must be 1 .. 1024"),
        (dict(per_frame=1025), "corners: per_frame must be 1 .. 1024"),
        (dict(win=(0, 8)), "corners: win_x and win_y must be 1 .. 15"),
        (dict(win=(8, 16)), "corners: win_x and win_y must be 1 .. 15"),
        (dict(zero_zone=(8, 0)), "corners: the zero zone must be"),
        (dict(zero_zone=(-1, 0)), "corners: the zero zone must be"),
        (dict(max_iters=0), "corners: max_iters must be 1 .. 100"),
        (dict(max_iters=101), "corners: max_iters must be 1 .. 100"),
        (dict(eps=-1.0), "corners: eps must be finite and >= 0"),
        (dict(eps=float("nan")), "corners: eps must be finite and >= 0"),
    ]
    for change, message in bad:
        with pytest.raises(RmcvError) as e:
            ctx.refine_corners(**dict(ok, **change))
        assert e.value.code == abi.ERR_BAD_ARG and message in str(e.value), change
    for kw, message in ((dict(frame=3), "a frame index is outside the batch"), (dict(win=(16, 16)), "win_x and win_y must be 1 .. 15"),
                        (dict(corners=np.zeros((1025, 2), np.float32)), "per_frame must be 1 .. 1024")):
        with pytest.raises(RmcvError) as e:
            ctx.refined_corners(**dict(dict(frame=0, corners=GUESS[0]), **kw))
        assert e.value.code == abi.ERR_BAD_ARG and message in str(e.value), kw
    with pytest.raises(RmcvError, match="rmcv_corner_subpix: image beyond the context's max_width / max_height"):
        ctx.refine_corners_of(np.zeros((H, W + 1, 3), np.uint8), GUESS[0])
    with pytest.raises(RmcvError, match="rmcv_corner_subpix: corners: per_frame must be 1 .. 1024"):
        ctx.refine_corners_of(FRAMES[0], np.zeros((0, 2), np.float32))
    with pytest.raises(RmcvError, match="rmcv_corner_subpix: corners: max_iters must be 1 .. 100"):
        ctx.refine_corners_of(FRAMES[0], GUESS[0], max_iters=0)
    ctx.sync()
    torch.cuda.synchronize()
    assert tab.cpu().numpy().tobytes() == GUESS.tobytes() and (status.cpu().numpy() == -1).all()   # nothing was enqueued: the tables are as they were
    fresh = Context(device=0, **LIMITS)
    try:
        with pytest.raises(RmcvError, match="corners: no frames are bound"):
            fresh.refine_corners(**ok)
    finally:
        fresh.close()
    ctx.refine_corners(**ok)   # ... and the same call with nothing wrong runs
    ctx.sync()
    want, want_st = host_rows(FRAMES, GUESS, RULES[0])
    assert tab.cpu().numpy().tobytes() == want.tobytes() and status.cpu().numpy().tolist() == want_st.tolist()
