"""Raw Bayer input (RMCV_OPT_INPUT_FORMAT) without a GPU: the demosaic D the feature is defined by (tests/bayer_ref.py) against
hand-worked answers, the ABI's constants and argument checks, the Python face and the shim's new function."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bayer_ref as BR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests")


def d_scalar(m, pattern, x, y):
    """D at one pixel, written out site by site (a second statement of the formulas, for the border tests)"""
    h, w = m.shape
    x, y = min(max(x, 1), w - 2), min(max(y, 1), h - 2)
    rx, ry = BR.r_site(pattern)
    v = lambda xx, yy: int(m[yy, xx])
    own = v(x, y)
    cross = (v(x - 1, y) + v(x + 1, y) + v(x, y - 1) + v(x, y + 1) + 2) >> 2
    diag = (v(x - 1, y - 1) + v(x + 1, y - 1) + v(x - 1, y + 1) + v(x + 1, y + 1) + 2) >> 2
    row = (v(x - 1, y) + v(x + 1, y) + 1) >> 1
    col = (v(x, y - 1) + v(x, y + 1) + 1) >> 1
    px, py = (x ^ rx) & 1, (y ^ ry) & 1
    if px == 0 and py == 0:
        return (diag, cross, own)       # R site
    if px == 1 and py == 1:
        return (own, cross, diag)       # B site
    if py == 0:
        return (col, own, row)          # G on an R row: R from the row, B from the column
    return (row, own, col)              # G on a B row


# ---------------------------------------------------------------- D: known answers
@pytest.mark.parametrize("pattern", BR.PATTERNS)
@pytest.mark.parametrize("shape", [(3, 3), (4, 5), (7, 6), (9, 11)])
def test_constant_scene_comes_back_constant(pattern, shape):
    h, w = shape
    for bgr in [(0, 0, 0), (255, 255, 255), (17, 200, 91), (250, 3, 128)]:
        frame = np.empty((h, w, 3), np.uint8)
        frame[:] = bgr
        d = BR.demosaic(BR.mosaic(frame, pattern), pattern)
        assert np.array_equal(d, frame), (pattern, shape, bgr)  # borders included


def test_4x4_rg_hand_worked():
    m = np.array([[10, 20, 30, 40],
                  [50, 61, 70, 80],
                  [90, 101, 110, 120],
                  [130, 140, 150, 160]], np.uint8)
    d = BR.demosaic(m, BR.RG)
    # (1,1) B site: B 61; G (50+70+20+101+2)>>2 = 60 (60.75); R (10+30+90+110+2)>>2 = 60 (60.5 rounds down under +2>>2)
    assert tuple(d[1, 1]) == (61, 60, 60)
    # (2,1) G on the B row: B from the row (61+80+1)>>1 = 71 (70.5, half-way goes up); R from the column (30+110+1)>>1 = 70
    assert tuple(d[1, 2]) == (71, 70, 70)
    # (1,2) G on the R row: R from the row (90+110+1)>>1 = 100; B from the column (61+140+1)>>1 = 101 (100.5 up)
    assert tuple(d[2, 1]) == (101, 101, 100)
    # (2,2) R site: R 110; G (101+120+70+150+2)>>2 = 110 (110.75); B (61+80+140+160+2)>>2 = 110 (110.75)
    assert tuple(d[2, 2]) == (110, 110, 110)
    # border: the outer ring repeats its interior neighbour
    want = np.array([[(61, 60, 60), (61, 60, 60), (71, 70, 70), (71, 70, 70)],
                     [(61, 60, 60), (61, 60, 60), (71, 70, 70), (71, 70, 70)],
                     [(101, 101, 100), (101, 101, 100), (110, 110, 110), (110, 110, 110)],
                     [(101, 101, 100), (101, 101, 100), (110, 110, 110), (110, 110, 110)]], np.uint8)
    assert np.array_equal(d, want)


def test_5x5_bg_hand_worked():
    m = np.array([[0, 4, 8, 12, 16],
                  [1, 5, 9, 13, 17],
                  [2, 6, 11, 14, 18],
                  [3, 7, 10, 15, 19],
                  [255, 254, 253, 252, 251]], np.uint8)
    d = BR.demosaic(m, BR.BG)  # B G / G R: R sites at odd x, odd y
    # (1,1) R site: R 5; G (1+9+4+6+2)>>2 = 5 (5.5); B (0+8+2+11+2)>>2 = 5 (5.75)
    assert tuple(d[1, 1]) == (5, 5, 5)
    # (2,1) G on the R row: R (5+13+1)>>1 = 9; B (8+11+1)>>1 = 10 (9.5, half-way up)
    assert tuple(d[1, 2]) == (10, 9, 9)
    # (2,2) B site: B 11; G (6+14+9+10+2)>>2 = 10 (10.25); R (5+13+7+15+2)>>2 = 10 (10.5 rounds down)
    assert tuple(d[2, 2]) == (11, 10, 10)
    # (1,3) R site next to the bright last row: G (3+10+6+254+2)>>2 = 68; B (2+11+255+253+2)>>2 = 130
    assert tuple(d[3, 1]) == (130, 68, 7)
    # (3,3) R site: G (10+19+14+252+2)>>2 = 74; B (11+18+253+251+2)>>2 = 133
    assert tuple(d[3, 3]) == (133, 74, 15)
    # the clamped corners and edges take the site they clamp to, colour phase included
    assert tuple(d[4, 4]) == (133, 74, 15)
    assert tuple(d[0, 2]) == (10, 9, 9)
    assert tuple(d[4, 0]) == (130, 68, 7)
    assert tuple(d[0, 0]) == (5, 5, 5)


@pytest.mark.parametrize("pattern", BR.PATTERNS)
@pytest.mark.parametrize("shape", [(3, 3), (5, 7), (7, 5), (3, 9), (9, 3), (6, 5)])
def test_border_clamp_odd_sizes(pattern, shape):
    h, w = shape
    rng = np.random.default_rng(h * 100 + w * 10 + pattern)
    m = rng.integers(0, 256, (h, w), dtype=np.uint8)
    d = BR.demosaic(m, pattern)
    for y in range(h):
        for x in range(w):
            assert tuple(int(v) for v in d[y, x]) == d_scalar(m, pattern, x, y), (pattern, shape, x, y)
    assert np.array_equal(d[0], d[1]) and np.array_equal(d[-1], d[-2])
    assert np.array_equal(d[:, 0], d[:, 1]) and np.array_equal(d[:, -1], d[:, -2])


def test_synth_mosaic_matches_the_reference_sampling():
    from rmcv_amd import synth
    rng = np.random.default_rng(5)
    bgr = rng.integers(0, 256, (2, 7, 9, 3), dtype=np.uint8)
    for p in BR.PATTERNS:
        assert np.array_equal(synth.mosaic(bgr, p), BR.mosaic(bgr, p))
    # RG: R at (0, 0), G at (1, 0) and (0, 1), B at (1, 1)
    m = synth.mosaic(bgr[0], BR.RG)
    assert m[0, 0] == bgr[0, 0, 0, 2] and m[0, 1] == bgr[0, 0, 1, 1] and m[1, 0] == bgr[0, 1, 0, 1] and m[1, 1] == bgr[0, 1, 1, 0]
    with pytest.raises(ValueError):
        synth.mosaic(bgr, 5)


# ---------------------------------------------------------------- ABI
def header_defines():
    text = open(os.path.join(ROOT, "include", "rmcv_abi.h")).read()
    return {k: int(v) for k, v in re.findall(r"#define (RMCV_\w+) (-?\d+)", text)}


def test_header_constants_equal_python():
    from rmcv_amd import abi
    d = header_defines()
    assert d["RMCV_OPT_INPUT_FORMAT"] == abi.OPT_INPUT_FORMAT == 19
    assert d["RMCV_INPUT_BGR"] == abi.INPUT_BGR == 0
    assert (d["RMCV_BAYER_RG"], d["RMCV_BAYER_GB"], d["RMCV_BAYER_GR"], d["RMCV_BAYER_BG"]) == \
        (abi.BAYER_RG, abi.BAYER_GB, abi.BAYER_GR, abi.BAYER_BG) == BR.PATTERNS
    assert abi.BAYER_PATTERNS == BR.PATTERNS
    opt_ids = [v for k, v in d.items() if k.startswith("RMCV_OPT_")]
    assert len(opt_ids) == len(set(opt_ids))


def test_demosaic_exported_and_checks_arguments_without_a_device():
    from rmcv_amd import abi
    assert "rmcv_demosaic" in abi.EXPORTS
    L = abi.lib()
    assert hasattr(L, "rmcv_demosaic")
    raw = np.zeros((8, 8), np.uint8)
    out = np.zeros((8, 8, 3), np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    # a null context, null buffers, frames below 3x3, short strides: refused before anything touches a device
    assert L.rmcv_demosaic(None, p(raw), 8, 8, 8, 1, p(out), 24) == abi.ERR_BAD_ARG
    assert L.rmcv_demosaic(None, None, 8, 8, 8, 1, p(out), 24) == abi.ERR_BAD_ARG
    assert L.rmcv_demosaic(None, p(raw), 2, 8, 8, 1, p(out), 24) == abi.ERR_BAD_ARG
    assert L.rmcv_demosaic(None, p(raw), 8, 8, 7, 1, p(out), 24) == abi.ERR_BAD_ARG
    assert L.rmcv_demosaic(None, p(raw), 8, 8, 8, 1, p(out), 23) == abi.ERR_BAD_ARG
    assert L.rmcv_demosaic(None, p(raw), 8, 8, 8, 1, None, 24) == abi.ERR_BAD_ARG
    # the option id exists in the library's dispatcher: a null context is refused like every other option's
    assert L.rmcv_ctx_set_option(None, abi.OPT_INPUT_FORMAT, abi.BAYER_RG) == abi.ERR_BAD_ARG


# ---------------------------------------------------------------- the shim
def test_shim_defines_extract_color_bayer(tmp_path):
    """rm::extract_color_bayer compiles against the cv:: stand-in and the backend object DEFINES it, as tests/test_shim.py checks
    for the reference's functions"""
    obj = os.path.join(str(tmp_path), "backend.o")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(HERE, "cv_mock"), "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(HERE, "shim"), "-c", os.path.join(HERE, "shim", "backend.cpp"), "-o", obj], check=True)
    defined = subprocess.run(["nm", "-C", "--defined-only", obj], check=True, capture_output=True, text=True).stdout
    assert any("rm::extract_color_bayer(" in l and " T " in l for l in defined.splitlines())
    assert any("rm::extract_color(" in l and " T " in l for l in defined.splitlines())
