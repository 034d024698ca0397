"""View labels on the CPU (rmcv_amd/csrc/device_text.h through the host-side ABI, no GPU): the f6 format against Python's "%f",
which is correctly rounded and none of the library's code; dec at the ends of int32; the glyphs against the committed fixture; the blit of
rmcv_view_labels_host against tests/label_ref.py byte for byte on every case of tests/label_cases.py at scales 1, 2 and 8."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import label_cases as K
import label_ref as LR
import rmcv_amd
from rmcv_amd import abi

HERE = os.path.dirname(os.path.abspath(__file__))
FONT = os.path.join(HERE, "golden", "view_font_5x7.txt")


# ---- f6 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("values", [K.F6_FIXED, K.f6_neighbours(), K.f6_ties(), K.f6_seeded()], ids=["fixed", "neighbours", "ties", "seeded"])
def test_f6_equals_python_percent_f(values):
    assert len(values) >= 10
    bad = [(v.hex(), rmcv_amd.format_f6(v), "%f" % v) for v in values if rmcv_amd.format_f6(v) != "%f" % v]
    assert not bad, bad[:5]


def test_the_case_lists_are_what_they_claim():
    assert len(K.f6_seeded()) == 20000 and all(abs(v) < 1e15 for v in K.f6_seeded())
    exps = {math.frexp(v)[1] for v in K.f6_seeded()}
    assert min(exps) <= -1070 and max(exps) >= 45 and any(v < 0 for v in K.f6_seeded())
    ties = [v for v in K.f6_ties() if (abs(v) * 2 ** 7).is_integer() and int(abs(v) * 2 ** 7) % 2 == 1]
    assert len(ties) >= 1000
    # round-half-even decides on them: both directions occur
    assert rmcv_amd.format_f6(1 / 128) == "0.007812" and rmcv_amd.format_f6(3 / 128) == "0.023438"


@pytest.mark.parametrize("v, text", K.F6_PINNED, ids=[t + str(i) for i, (_, t) in enumerate(K.F6_PINNED)])
def test_f6_pinned_deviations(v, text):
    assert rmcv_amd.format_f6(v) == text


def test_f6_longest_and_capacity():
    v = -math.nextafter(1e15, 0)
    assert len(rmcv_amd.format_f6(v)) == 23
    buf = C.create_string_buffer(b"\x7f" * 32, 32)
    L = abi.lib()
    assert L.rmcv_format_f6(C.c_double(v), buf, 24) == 23 and buf.raw[23:24] == b"\0" and buf.raw[24:] == b"\x7f" * 8
    buf = C.create_string_buffer(b"\x7f" * 32, 32)
    assert L.rmcv_format_f6(C.c_double(v), buf, 23) == abi.ERR_CAPACITY and buf.raw[23:] == b"\x7f" * 9   # one short: refused, nothing beyond cap
    assert L.rmcv_format_f6(C.c_double(v), None, 23) == abi.ERR_BAD_ARG and L.rmcv_format_f6(C.c_double(v), buf, 0) == abi.ERR_BAD_ARG


# ---- dec and the lines ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [K.INT32_MIN, -1, 0, K.INT32_MAX, 7, -10, 1000000000])
def test_dec_is_to_string(i):
    assert rmcv_amd.label_text(i).split(":")[0] == str(i)
    t = K.tracks([(i, i, 0, [0, 0, 0], [0, 0, 0])])
    parts = rmcv_amd.track_label_text(t).split(", ")
    assert parts[0].split(":")[0] == str(i) and parts[-1] == str(i)


def test_lines():
    assert rmcv_amd.label_text(3, [1.5, -2.25, 300.125]) == "3: 1.500000, -2.250000, 300.125000"
    assert rmcv_amd.label_text(-1) == "-1: 0.000000, 0.000000, 0.000000"
    assert rmcv_amd.label_text(0, [float("nan"), -float("inf"), 1e300]) == "0: nan, -inf, big"
    t = K.tracks([(5, 3, 1, [1, 2, 3], [10.5, -20.25, 30.125]), (6, 0, 0, [1.25, 2.5, 3.75], [10.5, -20.25, 30.125])])
    assert rmcv_amd.track_label_text(t[0:1]) == "5: 10.500000, -20.250000, 30.125000, 3"     # the filter's posterior once initialised
    assert rmcv_amd.track_label_text(t[1:2]) == "6: 1.250000, 2.500000, 3.750000, 0"          # else the observation's position
    worst = K.tracks([(K.INT32_MIN, K.INT32_MIN, 0, [-math.nextafter(1e15, 0)] * 3, [0, 0, 0])])
    line = rmcv_amd.track_label_text(worst)
    assert len(line) == 99 <= abi.LABEL_MAX_CHARS and set(line) <= set(abi.LABEL_CHARSET)


# ---- the glyphs ----------------------------------------------------------------------------------------------------------------------------
def fixture_glyphs():
    """tests/golden/view_font_5x7.txt: a line "glyph <code>" then 7 rows of '#' / '.'"""
    out, lines = {}, [l.rstrip("\n") for l in open(FONT) if l.strip() and not l.startswith("//")]
    for i in range(0, len(lines), 8):
        assert lines[i].startswith("glyph ")
        out[chr(int(lines[i].split()[1]))] = [sum((ch == "#") << (4 - c) for c, ch in enumerate(row)) for row in lines[i + 1:i + 8]]
        assert all(len(row) == 5 and set(row) <= {"#", "."} for row in lines[i + 1:i + 8])
    return out


def test_glyphs():
    chars = abi.LABEL_CHARSET
    assert sorted(chars) == sorted("0123456789-.:, naifbg") and len(set(chars)) == len(chars)
    glyphs = {ch: [int(r) for r in rmcv_amd.view_glyph(ch)] for ch in chars}
    for ch, rows in glyphs.items():
        assert len(rows) == 7 and all(0 <= r < 32 for r in rows), ch    # the 5 x 7 box
        assert any(rows) == (ch != " "), ch                             # space is empty, nothing else is
    assert len({tuple(r) for r in glyphs.values()}) == len(chars)       # pairwise distinct
    assert glyphs == fixture_glyphs()
    for other in range(-2, 300):
        if not (0 <= other < 256 and chr(other) in chars):
            assert abi.lib().rmcv_view_glyph(other, abi.ptr(np.zeros(7, np.uint8))) == abi.ERR_BAD_ARG, other
    assert abi.lib().rmcv_view_glyph(ord("0"), None) == abi.ERR_BAD_ARG
    with pytest.raises(abi.RmcvError):
        rmcv_amd.view_glyph("x")


# ---- the blit ------------------------------------------------------------------------------------------------------------------------------
texts_of, expected = LR.texts_of, LR.expected


def run_host(case, scale):
    buf = K.background(case["stride"])
    rmcv_amd.view_labels_host(buf, case["geometry"] + (K.VW, K.VH), scale, case["armours"], case["identities"], case["positions"], case["tracks"],
                              case["side"], case["origin"], stride=case["stride"])
    return buf


CASES = K.cases()


@pytest.mark.parametrize("scale", K.SCALES)
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_blit_equals_the_reference(case, scale):
    want, start = expected(case, scale)
    got = run_host(case, scale)
    assert np.array_equal(got, want)   # (bytes beyond 3 vw of a row are part of the buffer: untouched)
    drawn = bool((want != start).any())
    assert drawn == (case["name"] not in ("none", "below", "above", "left", "right")), "a case that draws nothing proves nothing"


def test_cases_cover_what_they_claim():
    by = {c["name"]: c for c in CASES}
    assert by["odd_stride"]["stride"] % 4 != 0 and by["odd_stride"]["stride"] > 3 * K.VW
    assert by["track_window"]["origin"] != (0, 0) and len(by["none"]["armours"]) == 0 and by["defaults"]["identities"] is None
    # yellow wins where an armour's line lands on a track's
    want, _ = expected(by["track_under_armour"], 2)
    px = K.rows_of(want, by["track_under_armour"]["stride"]).reshape(K.VH, K.VW, 3)
    yellow, magenta = (px == LR.YELLOW).all(2), (px == LR.MAGENTA).all(2)
    assert yellow.any() and magenta.any()
    only_tracks = dict(by["track_under_armour"], armours=by["track_under_armour"]["armours"][:0], identities=None, positions=None)
    m0 = (K.rows_of(expected(only_tracks, 2)[0], only_tracks["stride"]).reshape(K.VH, K.VW, 3) == LR.MAGENTA).all(2)
    assert (m0 & yellow).any()
    # the floor, not truncation: the two differ for this anchor
    assert LR.anchor((-1, 20), (0, 0), K.W, K.H, K.VW, K.VH)[0] == -2 != int(-1 * K.VW / K.W)
    # half to even
    assert LR.anchor((10.5, 21.5), (0, 0), K.W, K.H, K.VW, K.VH) == (10 * 96 // 64, 22 * 40 // 48)


def test_host_refusals():
    a = K.armours((10, 30))
    for kw in (dict(scale=0), dict(scale=9), dict(stride=3 * K.VW - 1), dict(geometry=(0, K.H, K.VW, K.VH)), dict(geometry=(K.W, K.H, 0, K.VH))):
        args = dict(geometry=(K.W, K.H, K.VW, K.VH), scale=1, stride=3 * K.VW)
        args.update(kw)
        buf = K.background(3 * K.VW)
        before = buf.copy()
        with pytest.raises(abi.RmcvError):
            rmcv_amd.view_labels_host(buf, args["geometry"], args["scale"], a, stride=args["stride"])
        assert np.array_equal(buf, before)


def test_python_surface():
    for name in ("format_f6", "label_text", "track_label_text", "view_glyph", "view_labels_host", "LABEL_ARMOURS", "LABEL_TRACKS"):
        assert hasattr(rmcv_amd, name), name
    for name in ("view_labels", "batch_view_labels", "batch_view_tracks"):
        assert callable(getattr(rmcv_amd.Context, name)), name
    assert callable(rmcv_amd.Pipeline.set_view_labels)
    for name in ("rmcv_format_f6", "rmcv_label_text", "rmcv_track_label_text", "rmcv_view_glyph", "rmcv_view_labels_host", "rmcv_view_labels",
                 "rmcv_batch_view_labels", "rmcv_batch_view_tracks", "rmcv_pipeline_set_view_labels"):
        assert name in abi.EXPORTS and hasattr(abi.lib(), name), name
    assert (abi.LABEL_ARMOURS, abi.LABEL_TRACKS, abi.LABEL_MAX_CHARS) == (1, 2, 112)
