"""The chessboard detector on the GPU (k_chess.hip): corners, count, status and candidates equal rmcv_find_chessboard_host byte for
byte -- the stage-wise helper on every case of tests/chess_cases.py within 320 x 256; the batch call on 3 frames of 160 x 128 with 5 x 4 boards
of 20-pixel squares through all five kinds of source (BGR, windows off the dword grid behind a run, RMCV_OPT_ENHANCE, an 8-bit mosaic in two
patterns, a 16-bit mirrored and flipped layout), each against the host function on SRC(f) computed on the host; partial tiles in both axes;
the getter; counts and untouched rows; the refusals; find -> refine chained on one device table."""

import numpy as np
import pytest

import bayer_ref as BR
import chess_cases as CC
import enhance_ref as ER
import raw_ref as RR
import source_view_ref as SR
import rmcv_amd as R
from rmcv_amd import STAGE_BINARY, Context, RmcvError, abi, default_params, synth

pytestmark = pytest.mark.gpu

W, H = 160, 128
LIMITS = dict(max_frames=3, max_width=W, max_height=H)
BOARDS = [[[20, 0, 20.5], [0, 20, 14.5], [0, 0, 1]], CC.rot(0.1, 20, 80.3, 64.2, 6, 5), [[20, 2, 14.5], [-1, 20, 18.0], [0, 0, 1]]]
FRAMES = np.stack([synth.chessboard(W, H, b, 6, 5)[0] for b in BOARDS])                              # (3, 128, 160, 3): 20-pixel squares
MIXED = np.stack([FRAMES[1], CC.IMAGES["blank"], CC.IMAGES["corner-outside-5x4"]])                   # a board, nothing, 19 of 20 corners
C_NULL = 0
PARAMS = [{}, dict(nms=1, threshold=500), dict(nms=7, contrast=60, dist_min=12, dist_max=40)]


def host_rows(srcs, cols, rows, params, frames=None):
    """rmcv_find_chessboard_host on SRC(f) of the chosen frames -> (corners (n, cols rows, 2), NaN without a board; counts; status; candidates)"""
    frames = range(len(srcs)) if frames is None else frames
    out = [R.find_chessboard_host(srcs[f], cols, rows, params) for f in frames]
    cor = np.stack([np.full((cols * rows, 2), np.nan, np.float32) if o[0] is None else o[0] for o in out])
    return cor, np.array([0 if o[0] is None else cols * rows for o in out], np.int32), np.array([o[1] for o in out], np.int32), [o[2] for o in out]


def check_batch(c, srcs, need_found=3):
    """every parameter set against the host on SRC(f); need_found: boards found over all of them, at least (9 = every frame, every set)"""
    found = 0
    for params in PARAMS:
        got, cnt, st = c.find_chessboards([0, 1, 2], 5, 4, params)
        want, want_cnt, want_st, want_cand = host_rows(srcs, 5, 4, params)
        assert st.tolist() == want_st.tolist() and cnt.tolist() == want_cnt.tolist(), params
        assert got.tobytes() == want.tobytes(), params
        found += int((cnt == 20).sum())
        for f in range(3):                      # the getter: one frame, candidates included
            cor, st1, cand = c.chessboard_of(f, 5, 4, params)
            assert st1 == want_st[f] and cand.tobytes() == want_cand[f].tobytes(), (params, f)
            assert (cor is None) == (want_cnt[f] == 0) and (cor is None or cor.tobytes() == want[f].tobytes()), (params, f)
    assert found >= need_found


@pytest.fixture(scope="module")
def ctx():
    c = Context(device=0, **LIMITS)
    yield c
    c.close()


@pytest.fixture(scope="module")
def big():
    c = Context(device=0, max_frames=1, max_width=320, max_height=256)
    yield c
    c.close()


@pytest.mark.parametrize("name", [c.name for c in CC.CASES if c.gpu])
def test_stagewise_equals_host(big, name):
    case = CC.BY_NAME[name]
    args = (CC.IMAGES[case.image], case.cols, case.rows, case.params)
    cor, st, cand = big.find_chessboard(*args)
    want, want_st, want_cand = R.find_chessboard_host(*args)
    assert st == want_st and bool(st & R.CHESS_FOUND) == case.found
    assert cand.tobytes() == want_cand.tobytes()
    assert (cor is None) == (want is None) and (cor is None or cor.tobytes() == want.tobytes())
    assert big.check_guards()[0] == 0


def test_batch_bgr(ctx):
    ctx.upload(FRAMES)
    check_batch(ctx, FRAMES, need_found=9)          # (plain BGR frames need no run)
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
        with pytest.raises(RmcvError, match="read behind a run with RMCV_STAGE_BINARY"):   # the effective origins do not exist yet
            ctx.find_chessboards([0], 5, 4)
        ctx.run(default_params(), STAGE_BINARY)
        eff = ctx.windows()[0]
        assert eff.tolist() == [[16, 13], [32, 31], [0, 32]]
        assert any((1 + f * pitch + int(eff[f][1]) * stride + 3 * int(eff[f][0])) % 4 for f in range(3))   # off the dword grid
        srcs = [SR.src_window(FRAMES[f], origins[f], ww, wh) for f in range(3)]
        assert all(s.shape == (wh, ww, 3) for s in srcs)
        check_batch(ctx, srcs)
        # window coordinates: the board of frame 0 lies where the whole frame's lies, less the window's effective origin
        whole = R.find_chessboard_host(FRAMES[0], 5, 4)[0]
        got = ctx.chessboard_of(0, 5, 4)[0]
        assert got is not None and np.array_equal(got, whole - eff[0].astype(np.float32))
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
            c.find_chessboards([0], 5, 4)
        c.run(default_params(), STAGE_BINARY)
        srcs, tables = zip(*[SR.src_enhanced(frames[f]) for f in range(3)])
        assert any((t != np.arange(256)).any() for t in tables)  # the gamma is not 1: a missed lookup shows
        check_batch(c, srcs)
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
        check_batch(c, srcs)
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
        check_batch(c, srcs)
        assert c.check_guards()[0] == 0
    finally:
        c.close()


def test_partial_tiles_in_both_axes():
    """150 x 120: the last column of 64 x 32 tiles is 22 pixels wide, the last row of tiles 24 high"""
    frames = np.ascontiguousarray(FRAMES[:, :120, :150])
    c = Context(device=0, max_frames=3, max_width=150, max_height=120)
    try:
        c.upload(frames)
        for params in PARAMS[:2]:
            got, cnt, st = c.find_chessboards([2, 0], 5, 4, params)
            want, want_cnt, want_st, _ = host_rows(frames, 5, 4, params, [2, 0])
            assert got.tobytes() == want.tobytes() and cnt.tolist() == want_cnt.tolist() and st.tolist() == want_st.tolist()
            assert cnt[1] == 20
        assert c.check_guards()[0] == 0
    finally:
        c.close()


def test_counts_and_untouched_rows(ctx):
    import torch
    ctx.upload(MIXED)
    want, want_cnt, want_st, _ = host_rows(MIXED, 5, 4, {})
    assert want_cnt.tolist() == [20, 0, 0]
    per = 23                                                                      # rows longer than the board
    tab = torch.full((3, per, 2), 7.25, dtype=torch.float32).cuda()
    counts = torch.full((3,), -1, dtype=torch.int32).cuda()
    status = torch.full((3,), -1, dtype=torch.int32).cuda()
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert ctx.find_chessboards([0, 1, 2], 5, 4, corners=tab.data_ptr(), per_frame=per, counts=counts.data_ptr(), status=None, stream=stream.cuda_stream) is None
    stream.synchronize()
    got = tab.cpu().numpy()
    assert got[0, :20].tobytes() == want[0].tobytes() and (got[0, 20:] == 7.25).all() and (got[1:] == 7.25).all()
    assert counts.cpu().numpy().tolist() == [20, 0, 0] and (status.cpu().numpy() == -1).all()
    tab.fill_(7.25)
    torch.cuda.synchronize()
    ctx.find_chessboards([2, 0], 5, 4, corners=tab.data_ptr(), per_frame=per, counts=counts.data_ptr(), status=status.data_ptr())   # the chosen frames in another order
    ctx.sync()
    got = tab.cpu().numpy()
    assert (got[0] == 7.25).all() and got[1, :20].tobytes() == want[0].tobytes() and (got[1, 20:] == 7.25).all() and (got[2] == 7.25).all()
    assert counts.cpu().numpy().tolist() == [0, 20, 0] and status.cpu().numpy().tolist() == [int(want_st[2]), int(want_st[0]), -1]
    assert ctx.check_guards()[0] == 0


def test_refusals_enqueue_nothing(ctx):
    import torch
    ctx.upload(FRAMES)
    tab = torch.full((3, 20, 2), 7.25, dtype=torch.float32).cuda()
    counts = torch.full((3,), -1, dtype=torch.int32).cuda()
    status = torch.full((3,), -1, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    ok = dict(frames=[0, 1, 2], cols=5, rows=4, corners=tab.data_ptr(), per_frame=20, counts=counts.data_ptr(), status=status.data_ptr())
    bad = [
        (dict(frames=[]), "source views: no frames chosen"),
        (dict(frames=[0, 1, 2, 0]), "source views: more views than the batch has frames"),
        (dict(frames=[0, 3]), "source views: a frame index is outside the batch"),
        (dict(frames=[-1]), "source views: a frame index is outside the batch"),
        (dict(frames=[1, 1]), "source views: a frame index is repeated"),
        (dict(corners=C_NULL), "chessboard: null corner or count table"),
        (dict(counts=0), "chessboard: null corner or count table"),
        (dict(per_frame=19), "chessboard: per_frame must be cols * rows .. 1024"),
        (dict(per_frame=1025), "chessboard: per_frame must be cols * rows .. 1024"),
        (dict(cols=1), "chessboard: cols and rows must be 2 .. 32"),
        (dict(rows=33, per_frame=1024), "chessboard: cols and rows must be 2 .. 32"),
        (dict(threshold=-1), "chessboard: threshold must be >= 0"),
        (dict(contrast=256), "chessboard: contrast must be 0 .. 255"),
        (dict(nms=0), "chessboard: nms must be 1 .. 7"),
        (dict(nms=8), "chessboard: nms must be 1 .. 7"),
        (dict(dist_min=0), "chessboard: 1 <= dist_min <= dist_max <= 1023"),
        (dict(dist_min=40, dist_max=39), "chessboard: 1 <= dist_min <= dist_max <= 1023"),
        (dict(dist_max=1024), "chessboard: 1 <= dist_min <= dist_max <= 1023"),
    ]
    for change, message in bad:
        with pytest.raises(RmcvError) as e:
            ctx.find_chessboards(**dict(ok, **change))
        assert e.value.code == abi.ERR_BAD_ARG and message in str(e.value), change
    for kw, message in ((dict(frame=3), "a frame index is outside the batch"), (dict(cols=33), "cols and rows must be 2 .. 32"), (dict(nms=9), "nms must be 1 .. 7")):
        with pytest.raises(RmcvError) as e:
            ctx.chessboard_of(**dict(dict(frame=0, cols=5, rows=4), **kw))
        assert e.value.code == abi.ERR_BAD_ARG and message in str(e.value), kw
    with pytest.raises(RmcvError, match="rmcv_find_chessboard: image beyond the context's max_width / max_height"):
        ctx.find_chessboard(np.zeros((H, W + 1, 3), np.uint8), 5, 4)
    with pytest.raises(RmcvError, match="rmcv_find_chessboard: chessboard: cols and rows must be 2 .. 32"):
        ctx.find_chessboard(FRAMES[0], 5, 1)
    with pytest.raises(RmcvError, match="rmcv_find_chessboard: chessboard: contrast must be 0 .. 255"):
        ctx.find_chessboard(FRAMES[0], 5, 4, contrast=-1)
    ctx.sync()
    torch.cuda.synchronize()
    assert (tab.cpu().numpy() == 7.25).all() and (counts.cpu().numpy() == -1).all() and (status.cpu().numpy() == -1).all()   # nothing was enqueued
    fresh = Context(device=0, **LIMITS)
    try:
        with pytest.raises(RmcvError, match="chessboard: no frames are bound"):
            fresh.find_chessboards(**ok)
    finally:
        fresh.close()
    ctx.find_chessboards(**ok)   # ... and the same call with nothing wrong runs
    ctx.sync()
    want, want_cnt, want_st, _ = host_rows(FRAMES, 5, 4, {})
    assert tab.cpu().numpy().tobytes() == want.tobytes() and counts.cpu().numpy().tolist() == want_cnt.tolist() and status.cpu().numpy().tolist() == want_st.tolist()


def test_find_then_refine_on_one_device_table(ctx):
    """two asynchronous calls, no host step in between: equal to rmcv_corner_subpix_host applied to rmcv_find_chessboard_host's output"""
    ctx.upload(MIXED)
    for win in ((8, 8), (5, 5)):
        got, cnt, st, cst = ctx.capture_corners([0, 1, 2], 5, 4, win=win)
        coarse, want_cnt, want_st, _ = host_rows(MIXED, 5, 4, {})
        fine, fine_st = R.corner_subpix_host(MIXED[0], coarse[0], win)
        assert cnt.tolist() == want_cnt.tolist() == [20, 0, 0] and st.tolist() == want_st.tolist()
        assert got[0].tobytes() == fine.tobytes() and cst[0].tolist() == fine_st.tolist()
        assert np.isnan(got[1:]).all() and not cst[1:].any()                     # no board: nothing refined, nothing written
    # the accuracy condition through the device: a clean affine board, within the refinement's bound of the analytic corners
    case = CC.BY_NAME["affine160-4x3"]
    ctx.upload(np.stack([CC.IMAGES[case.image]]))
    got, cnt, st, cst = ctx.capture_corners([0], 4, 3)
    assert cnt.tolist() == [12] and np.abs(got[0] - case.analytic).max() <= CC.ACCURACY_BOUND
    assert ctx.check_guards()[0] == 0
