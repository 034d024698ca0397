"""frame_source.h (rmcv_amd/csrc) on the host: every field of frame_source_of and frame_source_packed over a grid of geometries -- the five
kinds, 1- and 2-byte samples, every orientation and a non-zero valid bit, windows and enhance on and off (and, beyond what a context binds,
together: the kind's order of precedence), the four Bayer patterns, odd strides and extents, one frame and several -- against
tests/frame_source_ref.py, the Python restatement of the two batch fillers and the three hand fills they replace.  Pointers are printed as
offsets from the base pointers passed in, each against its own base ("-": null).

The program includes frame_source.h alone, which shows that the header needs neither Bufs nor rmcv_internal.h.  It is compiled by hipcc's host
pass (-x hip --offload-host-only), not by g++: device_bayer.h, whose layout functions the filler reads, marks them __host__ __device__
unconditionally, which the plain host compiler does not take.  The program makes no HIP call.  No GPU."""
import itertools
import os
import subprocess

import pytest

import frame_source_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

SRC = r'''
#include <stdio.h>
#include <string.h>
#include "rmcv_amd/csrc/frame_source.h"
using namespace rmcv;
static uint8_t frames[1], enh_lut[1];
static rmcv_point win_eff[1];
static void ptr(const void* p, const void* base)
{
    if (p) printf(" %lld", (long long)((const char*)p - (const char*)base));
    else printf(" -");
}
static void show(const FrameSource& s)
{
    printf("%d", s.kind);
    ptr(s.src, frames);
    ptr(s.src_end, frames);
    printf(" %d %lld %d %d %d %d %d", s.stride, (long long)s.frame_pitch, s.w, s.h, s.rx, s.ry, s.lay);
    ptr(s.lut, enh_lut);
    ptr(s.win_eff, win_eff);
    printf("\n");
}
int main(int argc, char** argv)
{
    FILE* f = fopen(argv[1], "r");
    if (!f) return 1;
    char what[4];
    while (fscanf(f, "%3s", what) == 1) {
        if (what[0] == 'G') {
            Geom g{};
            long long pitch;
            if (fscanf(f, "%d %d %d %d %d %d %d %d %d %d %d %d %lld", &g.input_format, &g.sample_bytes, &g.valid_bit, &g.orient, &g.enhance, &g.win, &g.n_frames,
                       &g.w, &g.h, &g.frame_w, &g.frame_h, &g.stride, &pitch) != 13) return 2;
            g.frame_pitch = pitch;
            show(frame_source_of(g, frames, enh_lut, win_eff));
        } else if (what[0] == 'P') {
            int w, h, dstride;
            if (fscanf(f, "%d %d %d", &w, &h, &dstride) != 3) return 2;
            show(frame_source_packed(frames, w, h, dstride));
        } else return 3;
    }
    fclose(f);
    return 0;
}
'''

# (w, h) of SRC, the margin of the frames around a window, bytes a row and a frame are padded by
EXTENTS = [(96, 64, 32, 5, 7), (97, 65, 31, 0, 0), (33, 18, 16, 3, 1)]


def geometries():
    out = []
    for fmt, sample_bytes, valid_bit, orient, enhance, win, n_frames, (w, h, margin, row_pad, frame_pad) in itertools.product(
            (0, R.BAYER_RG, R.BAYER_GB, R.BAYER_GR, R.BAYER_BG), (1, 2), (0, 3), (0, 1, 2, 3), (0, 1), (0, 1), (1, 3), EXTENTS):
        frame_w, frame_h = (w + margin, h + margin) if win else (w, h)
        stride = (sample_bytes if fmt else 3) * frame_w + row_pad
        out.append(dict(input_format=fmt, sample_bytes=sample_bytes, valid_bit=valid_bit, orient=orient, enhance=enhance, win=win, n_frames=n_frames, w=w, h=h,
                        frame_w=frame_w, frame_h=frame_h, stride=stride, frame_pitch=stride * frame_h + frame_pad))
    return out


PACKED = [(w, h, (3 * w + 15) & ~15) for w, h in ((1, 1), (5, 3), (96, 64), (97, 65), (640, 400), (1280, 1024))] + [(7, 5, 21), (7, 5, 23)]


def line(s):
    return " ".join("-" if s[k] is None else str(s[k]) for k in R.FIELDS)


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    d = tmp_path_factory.mktemp("frame_source")
    with open(d / "main.cpp", "w") as f:
        f.write(SRC)
    with open(d / "cases.txt", "w") as f:
        for g in geometries():
            f.write("G " + " ".join(str(g[k]) for k in R.GEOM) + "\n")
        for p in PACKED:
            f.write("P %d %d %d\n" % p)
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-function", "-I", ROOT, str(d / "main.cpp"),
                    "-o", str(d / "fill")], check=True)
    lines = subprocess.run([str(d / "fill"), str(d / "cases.txt")], check=True, capture_output=True, text=True).stdout.split("\n")[:-1]
    return lines[:len(geometries())], lines[len(geometries()):]


def test_the_batch_filler_is_the_parents_two(answers):
    cases = geometries()
    assert len(answers[0]) == len(cases)
    assert answers[0] == [line(R.of_batch(g)) for g in cases]
    # the grid is what it says: every kind, both layouts' words, both tables taken and left, every R site
    got = [R.of_batch(g) for g in cases]
    assert {s["kind"] for s in got} == set(range(5))
    assert {(s["rx"], s["ry"]) for s in got if s["kind"] == R.SOURCE_MOSAIC_RAW} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {s["lay"] for s in got} >= {0, 1, 1 | 3 << 4, 2, 4, 6, 7 | 3 << 4}
    assert {s["lut"] for s in got} == {0, None} and {s["win_eff"] for s in got} == {0, None}
    assert all(s["src_end"] <= g["n_frames"] * g["frame_pitch"] for s, g in zip(got, cases))


def test_the_packed_filler_is_the_parents_three(answers):
    assert len(answers[1]) == len(PACKED)
    assert answers[1] == [line(R.packed(*p)) for p in PACKED]
    for (w, h, dstride), s in zip(PACKED, (R.packed(*p) for p in PACKED)):
        assert s["kind"] == R.SOURCE_BGR and s["src_end"] == s["frame_pitch"] - (dstride - 3 * w) and not any(s[k] for k in ("rx", "ry", "lay", "lut", "win_eff"))
