"""The sensor's frame as delivered (RMCV_OPT_INPUT_SAMPLE_BITS / _VALID_BIT / _ORIENT) without a GPU: the numpy restatement of T and
of the derived pattern (tests/raw_ref.py) against hand-worked cases, the identity that lets mirror-before-demosaic and
flip-after-demosaic (the reference's orders) be one thing here, the ABI's constants and exports, and the shim."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bayer_ref as BR
import raw_ref as RR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ---------------------------------------------------------------- T and the derived pattern
def test_t_hand_worked_4x4_and_5x4():
    r = np.arange(16, dtype=np.uint8).reshape(4, 4)
    assert np.array_equal(RR.T(r), r)
    assert np.array_equal(RR.T(r, mirror=True), [[3, 2, 1, 0], [7, 6, 5, 4], [11, 10, 9, 8], [15, 14, 13, 12]])
    assert np.array_equal(RR.T(r, flip=True), [[12, 13, 14, 15], [8, 9, 10, 11], [4, 5, 6, 7], [0, 1, 2, 3]])
    assert np.array_equal(RR.T(r, mirror=True, flip=True), [[15, 14, 13, 12], [11, 10, 9, 8], [7, 6, 5, 4], [3, 2, 1, 0]])
    r = np.arange(20, dtype=np.uint8).reshape(4, 5)  # 5 wide, 4 high
    assert np.array_equal(RR.T(r, mirror=True)[0], [4, 3, 2, 1, 0])
    assert np.array_equal(RR.T(r, mirror=True, flip=True)[0], [19, 18, 17, 16, 15])


def test_valid_bit_window_drops_what_lies_above_and_below():
    # 0x0ABC: bits 4..11 = 0xAB, bits 2..9 = 0xAF, bits 0..7 = 0xBC; 0xFABC has bits set above a 12-bit depth
    s = np.array([[0x0ABC, 0xFABC, 0xFFFF, 0x0003]], np.uint16)
    assert RR.narrow(s, 4).tolist() == [[0xAB, 0xAB, 0xFF, 0x00]]
    assert RR.narrow(s, 2).tolist() == [[0xAF, 0xAF, 0xFF, 0x00]]
    assert RR.narrow(s, 0).tolist() == [[0xBC, 0xBC, 0xFF, 0x03]]
    assert RR.narrow(s, 1).tolist() == [[0x5E, 0x5E, 0xFF, 0x01]] and RR.narrow(s, 3).tolist() == [[0x57, 0x57, 0xFF, 0x00]]
    b = np.array([[7, 200]], np.uint8)
    assert RR.narrow(b, 3) is b  # 1-byte samples have no window


def test_derived_pattern_table():
    # even sizes: a BG sensor becomes GB (mirror), GR (flip), RG (both) -- the table INTEGRATION.md used to leave to the reader
    assert [RR.derived_pattern(BR.BG, 1280, 1024, m, f) for m, f in RR.ORIENTATIONS] == [BR.BG, BR.GB, BR.GR, BR.RG]
    assert [RR.derived_pattern(BR.RG, 4, 4, m, f) for m, f in RR.ORIENTATIONS] == [BR.RG, BR.GR, BR.GB, BR.BG]
    # an odd width keeps the column parity under mirror (w-1 is even), an odd height the row parity under flip
    assert [RR.derived_pattern(BR.BG, 5, 4, m, f) for m, f in RR.ORIENTATIONS] == [BR.BG, BR.BG, BR.GR, BR.GR]
    assert [RR.derived_pattern(BR.GB, 4, 5, m, f) for m, f in RR.ORIENTATIONS] == [BR.GB, BR.BG, BR.GB, BR.BG]
    for p in BR.PATTERNS:
        for (w, h) in [(4, 4), (5, 4), (4, 5), (5, 5)]:
            for m, f in RR.ORIENTATIONS:
                d = RR.derived_pattern(p, w, h, m, f)
                assert RR.delivered_pattern(d, w, h, m, f) == p
                # the colour of every site follows the pixel: sampling a BGR frame with p and orienting the mosaic is sampling the
                # oriented BGR frame with the derived pattern
                rng = np.random.default_rng(p * 100 + w * 10 + h)
                bgr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
                assert np.array_equal(RR.T(BR.mosaic(bgr, p), 0, m, f), BR.mosaic(RR.orient_bgr(bgr, m, f), d)), (p, w, h, m, f)


def test_delivered_is_the_inverse_of_t():
    rng = np.random.default_rng(3)
    m = rng.integers(0, 256, (2, 6, 7), dtype=np.uint8)
    for mi, fl in RR.ORIENTATIONS:
        assert np.array_equal(RR.T(RR.delivered(m, 8, 0, mi, fl), 0, mi, fl), m)
        for v in range(5):
            r = RR.delivered(m, 16, v, mi, fl, rng)
            assert r.dtype == np.uint16 and np.array_equal(RR.T(r, v, mi, fl), m)
            assert np.any(r >> (v + 8)) and (v == 0 or np.any(r & ((1 << v) - 1)))  # bits above and below the window are in use


# ---------------------------------------------------------------- D(T(r)) with the derived pattern = T of D(r) with the delivered one
SIZES = [(w, h) for w in range(3, 10) for h in range(3, 12)] + [(1280, 1024)]


@pytest.mark.parametrize("pattern", BR.PATTERNS)
def test_demosaic_commutes_with_orientation(pattern):
    for (w, h) in SIZES:
        rng = np.random.default_rng(pattern * 10000 + w * 100 + h)
        r = rng.integers(0, 1 << 16, (h, w), dtype=np.uint16)
        for v in (0, 2, 4):
            for mi, fl in RR.ORIENTATIONS:
                lhs = BR.demosaic(RR.T(r, v, mi, fl), RR.derived_pattern(pattern, w, h, mi, fl))
                rhs = RR.orient_bgr(BR.demosaic(RR.narrow(r, v), pattern), mi, fl)
                assert np.array_equal(lhs, rhs), (pattern, w, h, v, mi, fl)


# ---------------------------------------------------------------- synth
def test_synth_raw_frame():
    from rmcv_amd import synth
    rng = np.random.default_rng(9)
    m = rng.integers(0, 256, (3, 9, 12), dtype=np.uint8)
    for mi, fl in RR.ORIENTATIONS:
        assert np.array_equal(RR.T(synth.raw_frame(m, 8, 0, mi, fl), 0, mi, fl), m)
        for v in range(5):
            r = synth.raw_frame(m, 16, v, mi, fl, rng)
            assert r.dtype == np.dtype("<u2") and np.array_equal(RR.T(r, v, mi, fl), m)
            assert np.any(r >> (v + 8))  # the bits above the window carry data: a reader that saturates instead of dropping fails
    with pytest.raises(ValueError):
        synth.raw_frame(m, 12)
    with pytest.raises(ValueError):
        synth.raw_frame(m, 16, 5)


# ---------------------------------------------------------------- ABI
def header_defines():
    text = open(os.path.join(ROOT, "include", "rmcv_abi.h")).read()
    return {k: int(v) for k, v in re.findall(r"#define (RMCV_\w+) (-?\d+)", text)}


def test_header_constants_equal_python():
    from rmcv_amd import abi
    d = header_defines()
    assert d["RMCV_OPT_INPUT_SAMPLE_BITS"] == abi.OPT_INPUT_SAMPLE_BITS == 20
    assert d["RMCV_OPT_INPUT_VALID_BIT"] == abi.OPT_INPUT_VALID_BIT == 21
    assert d["RMCV_OPT_INPUT_ORIENT"] == abi.OPT_INPUT_ORIENT == 22
    assert (d["RMCV_ORIENT_MIRROR"], d["RMCV_ORIENT_FLIP"]) == (abi.ORIENT_MIRROR, abi.ORIENT_FLIP) == (1, 2)
    opt_ids = [v for k, v in d.items() if k.startswith("RMCV_OPT_")]
    assert len(opt_ids) == len(set(opt_ids))
    py_ids = [v for k, v in vars(abi).items() if k.startswith("OPT_")]
    assert len(py_ids) == len(set(py_ids))


def test_demosaic_raw_exported_and_checks_arguments_without_a_device():
    from rmcv_amd import abi
    assert "rmcv_demosaic_raw" in abi.EXPORTS
    L = abi.lib()
    assert hasattr(L, "rmcv_demosaic_raw")
    raw = np.zeros((8, 8), np.uint16)
    out = np.zeros((8, 8, 3), np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    f = L.rmcv_demosaic_raw
    # a null context, null buffers, frames below 3x3, odd or short strides, a bad valid bit, a bad orientation, bad sample bits: all
    # refused before anything touches a device
    assert f(None, p(raw), 8, 8, 16, 1, 16, 4, 3, p(out), 24) == abi.ERR_BAD_ARG
    assert f(None, None, 8, 8, 16, 1, 16, 4, 3, p(out), 24) == abi.ERR_BAD_ARG
    assert f(None, p(raw), 8, 8, 16, 1, 16, 4, 3, None, 24) == abi.ERR_BAD_ARG
    assert f(None, p(raw), 2, 8, 16, 1, 16, 4, 3, p(out), 24) == abi.ERR_BAD_ARG
    assert f(None, p(raw), 8, 8, 17, 1, 16, 4, 3, p(out), 24) == abi.ERR_BAD_ARG
    assert f(None, p(raw), 8, 8, 14, 1, 16, 4, 3, p(out), 24) == abi.ERR_BAD_ARG
    assert f(None, p(raw), 8, 8, 16, 1, 16, 5, 3, p(out), 24) == abi.ERR_BAD_ARG
    assert f(None, p(raw), 8, 8, 16, 1, 16, 4, 4, p(out), 24) == abi.ERR_BAD_ARG
    assert f(None, p(raw), 8, 8, 16, 1, 12, 4, 3, p(out), 24) == abi.ERR_BAD_ARG
    # the option ids exist in the library's dispatcher: a null context is refused like every other option's
    for opt, val in ((abi.OPT_INPUT_SAMPLE_BITS, 16), (abi.OPT_INPUT_VALID_BIT, 4), (abi.OPT_INPUT_ORIENT, 3)):
        assert L.rmcv_ctx_set_option(None, opt, val) == abi.ERR_BAD_ARG


def test_python_face_has_the_layout():
    import inspect

    from rmcv_amd import Context, Pipeline
    assert list(inspect.signature(Context.set_input_layout).parameters)[1:] == ["sample_bits", "valid_bit", "mirror", "flip"]
    assert hasattr(Context, "demosaic_raw")
    for k in ("sample_bits", "valid_bit", "mirror", "flip"):
        assert k in inspect.signature(Pipeline.__init__).parameters


# ---------------------------------------------------------------- the shim
def test_shim_defines_extract_color_raw(tmp_path):
    """rm::extract_color_raw compiles where the cv:: headers know CV_16UC1 (tests/shim_raw/) and the backend object DEFINES it, next
    to the functions it defined before"""
    obj = os.path.join(str(tmp_path), "backend_raw.o")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(HERE, "shim_raw"), "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(HERE, "shim"), "-c", os.path.join(HERE, "shim_raw", "backend_raw.cpp"), "-o", obj], check=True)
    defined = subprocess.run(["nm", "-C", "--defined-only", obj], check=True, capture_output=True, text=True).stdout
    for sym in ("rm::extract_color_raw(", "rm::extract_color_bayer(", "rm::extract_color("):
        assert any(sym in l and " T " in l for l in defined.splitlines()), sym
