"""One description of SRC(f) for three consumers (rmcv_amd/csrc/frame_source.h): for each of the five kinds of source -- BGR, BGR through windows
whose requested origins lie off the 16-pixel grid, a plain 8-bit mosaic, a 16-bit mirrored and flipped sensor layout, RMCV_OPT_ENHANCE -- two
frames of 96 x 64 are bound (the windowed kind: 128 x 96 frames read through 96 x 64 windows), the pixel stage runs, and the source view, the
corner refinement and the chessboard detector are each called with the frame list [1, 0].  Each equals its host function on SRC(f) of
tests/source_view_ref.py byte for byte: rmcv_source_view_host at 96 x 64 with flags 0, rmcv_corner_subpix_host, rmcv_find_chessboard_host.  List
order, kind and filler meet here in one place for all three.

The board: "affine96-4x3" of tests/chess_cases.py, a 4 x 3 pattern of 14-pixel squares drawn at 96 x 80, cut to its upper 64 rows (its lowest
inner corner lies at y = 54) -- the only case of that module the host function finds within 96 x 64.  Frame 1 is frame 0 turned by half a turn,
so the two frames' results differ and a list read in the wrong order shows."""
import numpy as np
import pytest

import bayer_ref as BR
import chess_cases as CC
import enhance_ref as ER
import raw_ref as RR
import source_view_ref as SR
import rmcv_amd as R
from rmcv_amd import STAGE_BINARY, Context, default_params, source_view_host

pytestmark = pytest.mark.gpu

W, H, COLS, ROWS = 96, 64, 4, 3
BIG_W, BIG_H = 128, 96
CASE = CC.BY_NAME["affine96-4x3"]
BOARD = np.ascontiguousarray(CC.IMAGES[CASE.image][:H, :W])
FRAMES = np.stack([BOARD, np.ascontiguousarray(BOARD[::-1, ::-1])])                                   # (2, 64, 96, 3)
# the coarse corners a detector would hand over: the analytic ones rounded to whole pixels
GUESS = np.round(np.stack([CASE.analytic, np.array([W - 1, H - 1]) - CASE.analytic])).astype(np.float32)   # (2, 12, 2)
LIST = [1, 0]
ORIGINS = np.array([(21, 17), (37, 30)], np.int32)   # requested; effective: (16, 17), (32, 30)
KINDS = ("bgr", "windowed", "mosaic", "sensor-layout", "enhanced")


def batch(kind):
    """(what to tell the context before the upload, the array to upload, SRC(f) of both frames) -- all on the host"""
    if kind == "bgr":
        return (lambda c: None), FRAMES, list(FRAMES)
    if kind == "windowed":
        big = np.random.default_rng(5).integers(0, 256, (2, BIG_H, BIG_W, 3), dtype=np.uint8)
        for f, (x, y) in enumerate(((16, 17), (32, 30))):
            big[f, y:y + H, x:x + W] = FRAMES[f]
        return (lambda c: None), big, [SR.src_window(big[f], ORIGINS[f], W, H) for f in range(2)]
    if kind == "mosaic":
        m = BR.mosaic(FRAMES, BR.RG)
        return (lambda c: c.set_input_format(BR.RG)), m, [SR.src_bayer(m[f], BR.RG) for f in range(2)]
    if kind == "sensor-layout":   # 16-bit samples with the pixel at bits 2 .. 9, mirrored and flipped
        r = RR.delivered(BR.mosaic(FRAMES, RR.derived_pattern(BR.GB, W, H, True, True)), 16, 2, True, True, np.random.default_rng(3))

        def tell(c):
            c.set_input_format(BR.GB)
            c.set_input_layout(16, 2, True, True)
        return tell, r, [SR.src_bayer(r[f], BR.GB, 2, True, True) for f in range(2)]
    dimmed = ER.dim(FRAMES, 96)
    return (lambda c: c.set_enhance(True)), dimmed, [SR.src_enhanced(dimmed[f])[0] for f in range(2)]


def host_results(srcs):
    """what the three host functions make of SRC(f) for f in LIST"""
    views = [source_view_host(srcs[f], size=(W, H), flags=0) for f in LIST]
    fine = [R.corner_subpix_host(srcs[f], GUESS[f]) for f in LIST]
    boards = [R.find_chessboard_host(srcs[f], COLS, ROWS) for f in LIST]
    return views, fine, boards


@pytest.mark.parametrize("kind", KINDS)
def test_three_consumers_read_one_source(kind):
    tell, frames, srcs = batch(kind)
    assert all(s.shape == (H, W, 3) for s in srcs) and not np.array_equal(srcs[0], srcs[1])
    views, fine, boards = host_results(srcs)
    assert all(b[0] is not None for b in boards)      # the host finds the board in SRC(f) of every kind: nothing below compares two failures
    assert boards[0][0].tobytes() != boards[1][0].tobytes() and fine[0][0].tobytes() != fine[1][0].tobytes()   # ... nor two equal rows
    c = Context(device=0, max_frames=2, max_width=BIG_W, max_height=BIG_H)
    try:
        tell(c)
        c.upload(frames)
        if kind == "windowed":
            c.set_windows(ORIGINS, W, H)
        c.run(default_params(), STAGE_BINARY)
        if kind == "windowed":
            assert c.windows()[0].tolist() == [[16, 17], [32, 30]]
        got = c.source_views(LIST, size=(W, H), flags=0)
        assert got.shape == (2, H, W, 3)
        for k in range(2):
            assert np.array_equal(got[k], views[k]), k
        cor, st = c.refine_corners(LIST, GUESS[LIST])
        assert cor.tobytes() == np.stack([f[0] for f in fine]).tobytes() and st.tolist() == np.stack([f[1] for f in fine]).tolist()
        found, cnt, cst = c.find_chessboards(LIST, COLS, ROWS)
        assert found.tobytes() == np.stack([b[0] for b in boards]).tobytes()
        assert cnt.tolist() == [COLS * ROWS] * 2 and cst.tolist() == [b[1] for b in boards]
        assert c.check_guards()[0] == 0
    finally:
        c.close()
