"""Delta stores of the bit plane (k_binary_ws.inc, image_plan.h: plane_step): in a delta launch k_binary_ws stores only the plane words
that are or were non-zero, by the image's mask, no pad words, and only the row masks that changed.  The failure this looks for is a STALE
plane word or row mask: foreground of an earlier run that a later run did not clear, or a word a later run lit and did not store.  The
plane shows through findContours, so after every run every frame's byte image AND its contours (CSR) equal the oracle's, with morph
close and morph none; rmcv_pixel_plane_delta_launches moves exactly when the table in each test says so.

Geometries: 128x40 (two words, strips of 32 and 8 rows), 2048x33 (32 words, the mask's limit, a strip border at row 32), 64x1.  Their
hand-made frames -- three, two and one -- are repeated, each repeat moved, until the batch has more strips than half the CUs: below that
the planner hands the batch to k_binary and k_binary_ws, the kernel under test, would not run at all (every run asserts that it did)."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from rmcv_amd import MORPH_CLOSE, MORPH_NONE, OPT_PIXEL_SHAPE, STAGE_ALL, STAGE_NO_IMAGE, Context, default_params
from rmcv_amd import abi

import oracle_lib

pytestmark = pytest.mark.gpu

# (w, h, distinct frames, frames of a batch, frames of the smaller batch): 2 / 2 / 1 strips per frame, more than 128 strips either way
GEOS = [(128, 40, 3, 72, 66), (2048, 33, 2, 72, 66), (64, 1, 1, 144, 132)]
IDS = ["128x40", "2048x33", "64x1"]
MORPHS = [MORPH_CLOSE, MORPH_NONE]
MORPH_IDS = ["close", "none"]


def counters():
    L = abi.lib()
    return L.rmcv_pixel_ws_launches(), L.rmcv_pixel_image_delta_launches(), L.rmcv_pixel_plane_delta_launches()


def lit(fr, f, ys, xs):
    fr[f, ys, xs, 0] = 255      # B - R = 255 >= lb


@functools.lru_cache(maxsize=None)
def scene(w, h, distinct, n, variant):
    """n frames: the geometry's `distinct` hand-made frames over and over, every repeat with another pattern at another place.  Patterns:
    the first and the last column of a word, rows 31 and 32 (either side of the strip border), an isolated pixel, a whole row, a whole
    frame, nothing.  `variant` moves everything, so that what is lit in one variant is dark in the next."""
    fr = np.zeros((n, h, w, 3), np.uint8)
    fr[..., 1] = 30
    ww = w // 64
    for f in range(n):
        rep, d = divmod(f, distinct)
        k = (d + rep + 2 * variant) % 7
        word = (rep + variant) % ww
        y = (5 + 7 * rep + 13 * variant) % h
        if k == 0:
            lit(fr, f, y, 64 * word)                            # the first column of a word
            lit(fr, f, (y + 2) % h, 64 * word + 63)             # ... and the last one, two rows on
        elif k == 1:
            for yy in (31, 32):                                 # either side of the strip border
                if yy < h:
                    lit(fr, f, yy, slice(64 * word + 60, min(w, 64 * word + 68)))
            if h <= 31:
                lit(fr, f, 0, 64 * word + 63)
        elif k == 2:
            lit(fr, f, y, (64 * word + 37 + 5 * variant) % w)   # an isolated pixel
        elif k == 3:
            lit(fr, f, y, slice(None))                          # a whole row
        elif k == 4:
            lit(fr, f, slice(None), slice(None))                # a whole frame
        elif k == 5:
            pass                                                # nothing
        else:
            lit(fr, f, slice(None), 0)                          # the image's first and last column
            lit(fr, f, slice(None), w - 1)
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


def reference(frames, morph):
    """the oracle's byte image and contours of every frame, computed once per (batch, morph)"""
    key = (id(frames), morph)
    if key not in _refs:
        oracle_lib.set_math_mode(0)
        p = oracle_lib.default_params(morph=morph)
        with ThreadPoolExecutor(16) as ex:
            _refs[key] = (frames, list(ex.map(lambda f: oracle_lib.detect_frame(f, p), frames)))
    return _refs[key][1]


def check(c, frames, morph, what, image=True, contours=True):
    for f, r in enumerate(reference(frames, morph)):
        if image:
            got = c.binary(f)
            assert np.array_equal(got, r["binary"]), "%s: the image of frame %d differs in %d bytes (%d of them stale foreground)" % (
                what, f, int(np.count_nonzero(got != r["binary"])), int(np.count_nonzero((got != 0) & (r["binary"] == 0))))
        if not contours:
            continue
        pts, co = c.contours(f)
        assert np.array_equal(co, r["offs"]) and np.array_equal(pts, r["pts"]), "%s: the contours of frame %d differ (%d against %d)" % (
            what, f, len(co) - 1, len(r["offs"]) - 1)


def run(c, frames, morph, what, plane_delta, image_delta=None, stages=STAGE_ALL, ws=True):
    """one run; the counters move as the caller's table says; then every frame against the oracle"""
    c.upload(frames)
    w0, i0, p0 = counters()
    c.run(default_params(morph=morph), stages)
    c.sync()
    w1, i1, p1 = counters()
    assert (w1 - w0, p1 - p0) == (1 if ws else 0, 1 if plane_delta else 0), (what, w1 - w0, i1 - i0, p1 - p0)
    if image_delta is not None:
        assert i1 - i0 == (1 if image_delta else 0), what
    assert p1 - p0 <= i1 - i0                                      # the plane goes by the image's mask: never without the image's delta
    check(c, frames, morph, what, image=not (stages & STAGE_NO_IMAGE))


def context(w, h, n):
    c = Context(device=0, max_frames=n, max_width=w, max_height=h)
    c.set_option(OPT_PIXEL_SHAPE, 1)
    return c


@pytest.mark.parametrize("morph", MORPHS, ids=MORPH_IDS)
@pytest.mark.parametrize("w,h,distinct,n,m", GEOS, ids=IDS)
def test_every_run_leaves_its_own_plane(w, h, distinct, n, m, morph):
    """A, B elsewhere, B again, all dark, all lit, A: a plane word that a run lights and a later one does not clear would survive here.
    Every run behind the first stores image and plane in delta mode."""
    a, b = scene(w, h, distinct, n, 0), scene(w, h, distinct, n, 1)
    c = context(w, h, n)
    for i, (name, fr) in enumerate([("A", a), ("B", b), ("B again", b), ("dark", flat(w, h, n, False)), ("lit", flat(w, h, n, True)), ("A again", a)]):
        run(c, fr, morph, name, plane_delta=i > 0, image_delta=i > 0)
    assert c.check_guards()[0] == 0
    c.close()


@pytest.mark.parametrize("morph", MORPHS, ids=MORPH_IDS)
@pytest.mark.parametrize("w,h,distinct,n,m", GEOS, ids=IDS)
def test_a_run_without_the_image_puts_the_plane_out_of_step(w, h, distinct, n, m, morph):
    """A; B without the image: the plane is B's, image and mask stay A's; then C with the image: the image goes by its mask (delta), the
    plane must be stored whole -- by A's mask, B's words would survive; then A again: both in delta mode"""
    a, b, cc = scene(w, h, distinct, n, 0), scene(w, h, distinct, n, 1), scene(w, h, distinct, n, 2)
    c = context(w, h, n)
    run(c, a, morph, "A", plane_delta=False, image_delta=False)
    run(c, a, morph, "A again", plane_delta=True, image_delta=True)
    run(c, b, morph, "B without the image", plane_delta=False, image_delta=False, stages=STAGE_ALL | STAGE_NO_IMAGE)
    check(c, a, morph, "A's image behind B without the image", contours=False)   # (the contours, from the plane, are B's: compared above)
    run(c, cc, morph, "C behind B without the image", plane_delta=False, image_delta=True)
    run(c, a, morph, "A behind C", plane_delta=True, image_delta=True)
    run(c, flat(w, h, n, False), morph, "dark", plane_delta=True, image_delta=True)
    c.close()


@pytest.mark.parametrize("morph", MORPHS, ids=MORPH_IDS)
@pytest.mark.parametrize("w,h,distinct,n,m", GEOS, ids=IDS)
def test_a_k_binary_launch_between(w, h, distinct, n, m, morph):
    """k_binary knows nothing of the masks: behind it image and plane are stored whole, then in delta mode again"""
    a, b, cc = scene(w, h, distinct, n, 0), scene(w, h, distinct, n, 1), scene(w, h, distinct, n, 2)
    c = context(w, h, n)
    run(c, a, morph, "A", plane_delta=False, image_delta=False)
    run(c, b, morph, "B", plane_delta=True, image_delta=True)
    c.set_option(OPT_PIXEL_SHAPE, 0)
    run(c, flat(w, h, n, True), morph, "lit, by k_binary", plane_delta=False, image_delta=False, ws=False)
    run(c, b, morph, "B without the image, by k_binary", plane_delta=False, image_delta=False, ws=False, stages=STAGE_ALL | STAGE_NO_IMAGE)
    c.set_option(OPT_PIXEL_SHAPE, 1)
    run(c, cc, morph, "C behind k_binary", plane_delta=False, image_delta=False)
    run(c, a, morph, "A behind C", plane_delta=True, image_delta=True)
    c.close()


@pytest.mark.parametrize("morph", MORPHS, ids=MORPH_IDS)
def test_geometry_change_and_back(morph):
    (w, h, d, n, _), (w2, h2, d2, _, _) = GEOS[1], GEOS[0]
    c = context(w, h2, n)
    a, x, b = scene(w2, h2, d2, n, 0), scene(w, h, d, n, 1), scene(w2, h2, d2, n, 2)
    run(c, a, morph, "128x40", plane_delta=False, image_delta=False)
    run(c, a, morph, "128x40 again", plane_delta=True, image_delta=True)
    run(c, x, morph, "2048x33 behind 128x40", plane_delta=False, image_delta=False)
    run(c, b, morph, "128x40 behind 2048x33", plane_delta=False, image_delta=False)
    run(c, a, morph, "128x40 once more", plane_delta=True, image_delta=True)
    c.close()


@pytest.mark.parametrize("morph", MORPHS, ids=MORPH_IDS)
@pytest.mark.parametrize("w,h,distinct,n,m", GEOS, ids=IDS)
def test_fewer_frames_then_all_again(w, h, distinct, n, m, morph):
    """n frames, m, n again, all of them k_binary_ws launches: the frames the smaller batch leaves alone keep plane and image in step.
    Then a smaller batch WITHOUT the image: the next smaller batch with it leaves only its own frames in step, and the full batch behind
    it must store the whole plane -- the frames beyond still hold the plane of the run without the image"""
    a, b, cc = scene(w, h, distinct, n, 0), scene(w, h, distinct, m, 1), scene(w, h, distinct, n, 2)
    c = context(w, h, n)
    run(c, a, morph, "all", plane_delta=False, image_delta=False)
    run(c, b, morph, "fewer", plane_delta=True, image_delta=True)
    run(c, cc, morph, "all behind fewer", plane_delta=True, image_delta=True)
    run(c, a, morph, "all without the image", plane_delta=False, image_delta=False, stages=STAGE_ALL | STAGE_NO_IMAGE)
    run(c, b, morph, "fewer behind all without the image", plane_delta=False, image_delta=True)
    run(c, cc, morph, "all behind fewer behind all without the image", plane_delta=False, image_delta=True)
    run(c, a, morph, "all again", plane_delta=True, image_delta=True)
    c.close()
