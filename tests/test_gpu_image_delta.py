"""Delta stores of the 0/255 byte image (k_binary_ws.inc, image_plan.h): a context remembers which 64-byte words of its image are
non-zero and k_binary_ws stores only the words that are or were.  The failure this looks for is a STALE byte: foreground of an earlier
run on the same context that a later run did not clear.  After every run the image of every frame equals that run's oracle, whatever
ran on the context before; rmcv_pixel_image_delta_launches says which launches took the delta path.

(A caller-supplied binary image would be one more writer of the buffer, but the library has no entry point that takes one --
launch_pack_bits has no caller -- so there is nothing to run here for it.)"""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from rmcv_amd import CAMP_BLUE, OPT_PIXEL_SHAPE, STAGE_ALL, Context, default_params
from rmcv_amd import abi

import oracle_lib

pytestmark = pytest.mark.gpu

STAGE_NO_IMAGE = 64
SHAPES = [(192, 70, 48), (1280, 70, 48), (2112, 40, 70)]       # ww = 3 (rows not 128-byte aligned, ragged last strip), 20, 33 (no mask: full)
IDS = ["192x70", "1280x70", "2112x40"]


def delta_launches():
    return abi.lib().rmcv_pixel_image_delta_launches()


def ws_launches():
    return abi.lib().rmcv_pixel_ws_launches()


def lit(frames, f, ys, xs):
    frames[f, ys, xs, 0] = 255      # B - R = 255 >= lb


@functools.lru_cache(maxsize=None)
def scene(w, h, n, variant):
    """n hand-made frames: foreground at the first / last row, the first / last column, either side of a word boundary (x = 63, 64), an
    isolated pixel, a whole row, a whole frame, nowhere -- then bars at random places.  `variant` moves everything: the pattern of
    frame f in one variant is another frame's in the next, at other rows and columns, so frames lit in one are dark in the other."""
    fr = np.zeros((n, h, w, 3), np.uint8)
    fr[..., 1] = 30
    rng = np.random.default_rng(1000 * variant + w + h)
    v = variant
    for f in range(n):
        k = (f + 5 * v) % 14
        y = (7 + 11 * v + f) % h
        if k == 0:
            lit(fr, f, 0, slice(None))
        elif k == 1:
            lit(fr, f, h - 1, slice(None))
        elif k == 2:
            lit(fr, f, slice(None), 0)
        elif k == 3:
            lit(fr, f, slice(None), w - 1)
        elif k == 4:
            lit(fr, f, slice(y, y + 3), slice(61, 64))          # ends at x = 63
        elif k == 5:
            lit(fr, f, slice(y, y + 3), slice(64, 67))          # starts at x = 64
        elif k == 6:
            lit(fr, f, slice(y, y + 3), slice(62, 66))          # straddles the boundary
        elif k == 7:
            lit(fr, f, y, (37 + 64 * v) % w)                    # an isolated pixel
        elif k == 8:
            lit(fr, f, y, slice(None))                          # a whole row
        elif k == 9:
            lit(fr, f, slice(None), slice(None))                # a whole frame
        elif k == 10:
            pass                                                # nowhere
        elif k == 11:
            lit(fr, f, slice(h - 3, h), slice(w - 3, w))        # the last word of the last rows
        else:
            for _ in range(4):
                x0, y0 = int(rng.integers(0, w - 8)), int(rng.integers(0, h - 4))
                lit(fr, f, slice(y0, y0 + int(rng.integers(2, 30))), slice(x0, x0 + int(rng.integers(2, 8))))
    fr.setflags(write=False)
    return fr


@functools.lru_cache(maxsize=None)
def flat(w, h, n, on):
    fr = np.zeros((n, h, w, 3), np.uint8)
    if on:
        fr[..., 0] = 255
    fr.setflags(write=False)
    return fr


_refs = {}


def reference(frames):
    """the oracle's byte image of every frame, computed once per batch"""
    key = id(frames)
    if key not in _refs:
        oracle_lib.set_math_mode(0)
        p = oracle_lib.default_params()
        with ThreadPoolExecutor(16) as ex:
            _refs[key] = (frames, list(ex.map(lambda f: oracle_lib.detect_frame(f, p)["binary"], frames)))
    return _refs[key][1]


def check_image(c, frames, what):
    for f, r in enumerate(reference(frames)):
        got = c.binary(f)
        assert np.array_equal(got, r), "%s: frame %d differs in %d bytes (%d of them stale foreground)" % (
            what, f, int(np.count_nonzero(got != r)), int(np.count_nonzero((got != 0) & (r == 0))))


def run(c, frames, stages=STAGE_ALL, expect_delta=None, expect_ws=True):
    c.upload(frames)
    d0, w0 = delta_launches(), ws_launches()
    c.run(default_params(), stages)
    c.sync()
    assert (ws_launches() - w0 == 1) == expect_ws
    if expect_delta is not None:
        assert delta_launches() - d0 == (1 if expect_delta else 0)


def context(w, h, n):
    c = Context(device=0, max_frames=n, max_width=w, max_height=h)
    c.set_option(OPT_PIXEL_SHAPE, 1)
    return c


@pytest.mark.parametrize("w,h,n", SHAPES, ids=IDS)
def test_every_run_leaves_its_own_image(w, h, n):
    """A, B at other places (frames lit in A dark in B), B again, all dark, all lit, A: after each run the image is that run's.  Every
    run after the first takes the delta path -- but for ww = 33, which has no 32-bit row mask and stores every byte every time."""
    a, b = scene(w, h, n, 0), scene(w, h, n, 1)
    masked = (w + 63) // 64 <= 32
    c = context(w, h, n)
    for i, (name, fr) in enumerate([("A", a), ("B", b), ("B again", b), ("dark", flat(w, h, n, False)), ("lit", flat(w, h, n, True)), ("A again", a)]):
        run(c, fr, expect_delta=masked and i > 0)
        check_image(c, fr, name)
    assert c.check_guards()[0] == 0
    c.close()


@pytest.mark.parametrize("w,h,n", SHAPES[:2], ids=IDS[:2])
def test_a_run_without_the_image_leaves_image_and_mask(w, h, n):
    a, b, cc = scene(w, h, n, 0), scene(w, h, n, 1), scene(w, h, n, 2)
    c = context(w, h, n)
    run(c, a, expect_delta=False)
    run(c, b, STAGE_ALL | STAGE_NO_IMAGE, expect_delta=False)
    check_image(c, a, "A's image behind B without the image")
    run(c, cc, expect_delta=True)
    check_image(c, cc, "C")
    c.close()


def middle_k_binary(c, w, h, n):
    c.set_option(OPT_PIXEL_SHAPE, 0)
    run(c, flat(w, h, n, True), expect_delta=False, expect_ws=False)
    c.set_option(OPT_PIXEL_SHAPE, 1)


def middle_bayer(c, w, h, n):
    c.set_input_format(abi.BAYER_PATTERNS[0])
    c.upload(np.random.default_rng(5).integers(0, 256, (n, h, w), dtype=np.uint8))
    c.run(default_params(), STAGE_ALL)
    c.sync()
    c.set_input_format(abi.INPUT_BGR)


def middle_enhanced(c, w, h, n):
    c.set_enhance(True)
    run(c, flat(w, h, n, True), expect_delta=False, expect_ws=False)
    c.set_enhance(False)


def middle_windowed(c, w, h, n):
    c.upload(flat(w, h, n, True))
    c.set_windows(np.zeros((n, 2), np.int32), w, h)                # windows as large as the frames: the geometry stays
    c.run(default_params(), STAGE_ALL)
    c.sync()
    c.set_windows(None, 0, 0)


def middle_per_frame(c, w, h, n):
    for _ in range(2):
        contours, binary = c.extract_color(flat(w, h, 1, True)[0])
        assert binary.all()


@pytest.mark.parametrize("middle", [middle_k_binary, middle_bayer, middle_enhanced, middle_windowed, middle_per_frame],
                         ids=["k_binary", "bayer", "enhanced", "windowed", "per_frame"])
def test_another_writer_of_the_image_drops_the_mask(middle):
    """A on k_binary_ws, then a batch through a kernel that knows nothing of the mask and lights the image up, then C on k_binary_ws:
    C must store every byte (no delta launch) and leave its own image"""
    w, h, n = 192, 70, 48
    a, cc = scene(w, h, n, 0), scene(w, h, n, 2)
    c = context(w, h, n)
    run(c, a, expect_delta=False)
    run(c, a, expect_delta=True)
    d0 = delta_launches()
    middle(c, w, h, n)
    assert delta_launches() == d0
    assert c.binary(0).any()                                       # (the middle run wrote foreground where A and C have none)
    run(c, cc, expect_delta=False)
    check_image(c, cc, "C behind %s" % middle.__name__)
    run(c, a, expect_delta=True)
    check_image(c, a, "A behind C")
    c.close()


def test_geometry_change_and_back():
    c = context(1280, 70, 48)
    a, x, b = scene(192, 70, 48, 0), scene(1280, 70, 48, 1), scene(192, 70, 48, 2)
    run(c, a, expect_delta=False)
    run(c, x, expect_delta=False)
    check_image(c, x, "1280x70 behind 192x70")
    run(c, b, expect_delta=False)
    check_image(c, b, "192x70 behind 1280x70")
    run(c, a, expect_delta=True)
    check_image(c, a, "192x70 again")
    c.close()


def test_fewer_frames_then_all_again():
    """48 frames, 24, 48 again: 24 frames of three strips are fewer strips than half the CUs, so the middle batch runs k_binary and the
    mask is dropped"""
    w, h, n = 192, 70, 48
    a, b, cc = scene(w, h, n, 0), scene(w, h, 24, 1), scene(w, h, n, 2)
    c = context(w, h, n)
    run(c, a, expect_delta=False)
    run(c, b, expect_delta=False, expect_ws=False)
    check_image(c, b, "24 frames behind 48")
    run(c, cc, expect_delta=False)
    check_image(c, cc, "48 frames behind 24")
    c.close()


def test_fewer_frames_on_the_delta_path_then_all_again():
    """72 frames, 48, 72 again, all of them k_binary_ws launches: the smaller batch is a delta launch, and so is the one behind it"""
    w, h, n, m = 192, 70, 72, 48
    a, b, cc = scene(w, h, n, 0), scene(w, h, m, 1), scene(w, h, n, 2)
    c = context(w, h, n)
    run(c, a, expect_delta=False)
    run(c, b, expect_delta=True)
    check_image(c, b, "48 frames behind 72")
    run(c, cc, expect_delta=True)                                  # (the mask still describes frames 48 .. 71 as A left them)
    check_image(c, cc, "72 frames behind 48")
    c.close()
    # the other way round: frames the mask has never described are stored in full
    c = context(w, h, n)
    run(c, b, expect_delta=False)
    run(c, a, expect_delta=False)
    check_image(c, a, "72 frames behind a first batch of 48")
    run(c, b, expect_delta=True)
    run(c, cc, expect_delta=True)
    check_image(c, cc, "72 frames, 48 between")
    c.close()
