"""source_view_plan.h (rmcv_amd/csrc) compiled with the host C++ compiler alone: the kind table, the refusals and, for every tile of every
size of tests/source_view_cases.py, the source span and the staged / gathered decision, against a Python restatement that takes its taps
from tests/view_ref.py's arithmetic.  The size list reaches both paths.  No GPU."""
import math
import os
import subprocess

import numpy as np
import pytest

import source_view_cases as SK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <stdio.h>
#include "rmcv_amd/csrc/source_view_plan.h"
#include "rmcv_amd/csrc/device_view.h"
using namespace rmcv;
int main(int argc, char** argv)
{
    for (int fmt = 0; fmt < 5; fmt++)
    for (int bytes = 1; bytes < 3; bytes++)
    for (int orient = 0; orient < 4; orient++)
    for (int enh = 0; enh < 2; enh++)
    for (int win = 0; win < 2; win++) {
        Geom g{};
        g.input_format = fmt, g.sample_bytes = bytes, g.orient = orient, g.enhance = enh, g.win = win;
        printf("K %d %d %d %d %d|%d|%s\n", fmt, bytes, orient, enh, win, (int)source_kind(g), SOURCE_KIND_NAMES[source_kind(g)]);
    }
    printf("B %d %d %d %d\n", SOURCE_TILE_X, SOURCE_TILE_Y, SOURCE_STAGE_BYTES, SOURCE_RING_BYTES);
    const int32_t ok[3] = {2, 0, 1}, rep[2] = {1, 1}, out[1] = {4}, neg[1] = {-1};
    struct { const int32_t* fr; int n, nf, stages, need, vw, vh, flags, stride; long long pitch; } r[] = {
        {ok, 3, 4, 7, 7, 10, 10, 7, 30, 300}, {nullptr, 1, 4, 7, 7, 10, 10, 7, 30, 300}, {ok, 0, 4, 7, 7, 10, 10, 7, 30, 300}, {ok, 3, 2, 7, 7, 10, 10, 7, 30, 300},
        {ok, 3, 4, 7, 7, 10, 10, 8, 30, 300}, {ok, 3, 4, 7, 7, 10, 10, -1, 30, 300}, {ok, 3, 4, 7, 7, 0, 10, 7, 30, 300}, {ok, 3, 4, 7, 7, 10, 0, 7, 30, 300},
        {ok, 3, 4, 7, 7, 65, 10, 7, 195, 1950}, {ok, 3, 4, 7, 7, 10, 49, 7, 30, 1470}, {ok, 3, 4, 7, 7, 10, 10, 7, 29, 300}, {ok, 3, 4, 7, 7, 10, 10, 7, 30, 299},
        {ok, 1, 4, 7, 7, 10, 10, 7, 30, 0}, {rep, 2, 4, 7, 7, 10, 10, 7, 30, 300}, {out, 1, 4, 7, 7, 10, 10, 7, 30, 300}, {neg, 1, 4, 7, 7, 10, 10, 7, 30, 300},
        {ok, 3, 4, 3, 7, 10, 10, 7, 30, 300}, {ok, 3, 4, 1, 1, 10, 10, 0, 30, 300}};
    for (auto& q : r) {
        const char* why = source_views_refusal(q.fr, q.n, q.nf, q.stages, q.need, q.vw, q.vh, 64, 48, q.flags, q.stride, q.pitch);
        printf("R %s\n", why ? why : "");
    }
    const char x = 0;
    printf("I %s|%s|%s|%s|%s|%s\n", source_image_refusal(nullptr, &x, 4, 4, 12), source_image_refusal(&x, nullptr, 4, 4, 12), source_image_refusal(&x, &x, 0, 4, 12),
           source_image_refusal(&x, &x, 4, 0, 12), source_image_refusal(&x, &x, 4, 4, 11), source_image_refusal(&x, &x, 4, 4, 12) ? "refused" : "");
    FILE* f = fopen(argv[1], "r");
    if (!f) return 1;
    int w, h, vw, vh;
    while (fscanf(f, "%d %d %d %d", &w, &h, &vw, &vh) == 4) { // every tile: the kernel's own steps
        const int mode = view_resize_mode(w, h, vw, vh);
        for (int y0 = 0; y0 < vh; y0 += SOURCE_TILE_Y)
        for (int x0 = 0; x0 < vw; x0 += SOURCE_TILE_X) {
            const int nx = vw - x0 < SOURCE_TILE_X ? vw - x0 : SOURCE_TILE_X, ny = vh - y0 < SOURCE_TILE_Y ? vh - y0 : SOURCE_TILE_Y;
            const SourceSpan sp = source_span(view_tap_x(mode, x0, w, vw).s0, view_tap_x(mode, x0 + nx - 1, w, vw).s1, view_tap_y(mode, y0, h, vh).s0,
                                              view_tap_y(mode, y0 + ny - 1, h, vh).s1);
            printf("T %d %d %d %d %d %d|%d %d %d %d|%d", w, h, vw, vh, x0, y0, sp.r0, sp.c0, sp.rows, sp.cols, source_span_pitch(sp.cols));
            for (int k = 0; k < SOURCE_KINDS; k++) printf(" %d", (int)source_tile_staged(k, sp.rows, sp.cols));
            printf("\n");
        }
    }
    fclose(f);
    return 0;
}
'''

BGR, BGR_WIN, MOSAIC, MOSAIC_RAW, BGR_LUT = range(5)
NAMES = ["k_view_source<BGR>", "k_view_source<BGR_WIN>", "k_view_source<MOSAIC>", "k_view_source<MOSAIC_RAW>", "k_view_source<BGR_LUT>"]
TILE_X, TILE_Y, STAGE_BYTES, RING_BYTES = 64, 16, 24576, 10240


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    d = tmp_path_factory.mktemp("source_view_plan")
    with open(d / "main.cpp", "w") as f:
        f.write(SRC)
    with open(d / "sizes.txt", "w") as f:
        for (w, h), (vw, vh) in SK.SIZES:
            f.write("%d %d %d %d\n" % (w, h, vw, vh))
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-function", "-ffp-contract=off", "-I", ROOT, str(d / "main.cpp"), "-o", str(d / "plan")], check=True)
    return subprocess.run([str(d / "plan"), str(d / "sizes.txt")], check=True, capture_output=True, text=True).stdout.splitlines()


def kind(fmt, sample_bytes, orient, enh, win):
    """DESIGN.md 4p's table: a mosaic is plain when its samples are bytes and it is neither mirrored nor flipped"""
    if fmt:
        return MOSAIC if sample_bytes == 1 and orient == 0 else MOSAIC_RAW
    return BGR_LUT if enh else (BGR_WIN if win else BGR)


def test_kind_table(lines):
    got = [ln for ln in lines if ln.startswith("K ")]
    want = []
    for fmt in range(5):
        for sb in (1, 2):
            for orient in range(4):
                for enh in (0, 1):
                    for win in (0, 1):
                        k = kind(fmt, sb, orient, enh, win)
                        want.append("K %d %d %d %d %d|%d|%s" % (fmt, sb, orient, enh, win, k, NAMES[k]))
    assert got == want
    assert [ln for ln in lines if ln.startswith("B ")] == ["B %d %d %d %d" % (TILE_X, TILE_Y, STAGE_BYTES, RING_BYTES)]


def test_refusals(lines):
    got = [ln[2:] for ln in lines if ln.startswith("R ")]
    assert got == ["", "source views: no frames chosen", "source views: no frames chosen", "source views: more views than the batch has frames",
                   "source views: unknown view flags", "source views: unknown view flags", "source views: the view size must be 1 .. max_width x 1 .. max_height",
                   "source views: the view size must be 1 .. max_width x 1 .. max_height", "source views: the view size must be 1 .. max_width x 1 .. max_height",
                   "source views: the view size must be 1 .. max_width x 1 .. max_height", "source views: out_stride < 3 vw",
                   "source views: out_pitch < out_stride (vh - 1) + 3 vw", "", "source views: a frame index is repeated",
                   "source views: a frame index is outside the batch", "source views: a frame index is outside the batch",
                   "source views: the batch's run lacked a stage the view flags need", ""]
    assert [ln[2:] for ln in lines if ln.startswith("I ")] == ["null buffer|null buffer|the image needs w >= 1 and h >= 1|the image needs w >= 1 and h >= 1|stride < 3 w|"]


def taps(n_src, n_dst, horizontal):
    """(s0, s1) of every output coordinate: cv::resize's positions for INTER_LINEAR on 8-bit images (tests/view_ref.py: resize_linear), the copy
    and the exact half"""
    if n_src == n_dst:
        return [(d, d) for d in range(n_dst)]
    out = []
    scale = n_src / n_dst
    for d in range(n_dst):
        s = int(math.floor(float(np.float32((d + 0.5) * scale - 0.5))))
        if horizontal:
            s = min(max(s, 0), n_src - 1)
            out.append((s, min(s + 1, n_src - 1)))
        else:
            out.append((min(max(s, 0), n_src - 1), min(max(s + 1, 0), n_src - 1)))
    return out


def test_spans_and_the_rule(lines):
    got = [ln for ln in lines if ln.startswith("T ")]
    want, staged_seen, gathered_seen = [], 0, 0
    for (w, h), (vw, vh) in SK.SIZES:
        if w == 2 * vw and h == 2 * vh:
            tx, ty = [(2 * d, 2 * d + 1) for d in range(vw)], [(2 * d, 2 * d + 1) for d in range(vh)]
        elif (w, h) == (vw, vh):
            tx, ty = [(d, d) for d in range(vw)], [(d, d) for d in range(vh)]
        else:
            tx, ty = taps(w, vw, True), taps(h, vh, False)
        for y0 in range(0, vh, TILE_Y):
            for x0 in range(0, vw, TILE_X):
                nx, ny = min(TILE_X, vw - x0), min(TILE_Y, vh - y0)
                r0, c0 = ty[y0][0], tx[x0][0]
                rows, cols = ty[y0 + ny - 1][1] - r0 + 1, tx[x0 + nx - 1][1] - c0 + 1
                # every tap of the tile lies inside the span
                assert all(c0 <= a <= b < c0 + cols for a, b in tx[x0:x0 + nx]) and all(r0 <= a and b < r0 + rows for a, b in ty[y0:y0 + ny])
                pitch = (3 * cols + 6) & ~3
                assert pitch % 4 == 0 and pitch >= 3 * cols + 3  # a row, wherever its first byte lies in its first dword
                fits = rows * pitch <= STAGE_BYTES
                st = [int(fits and (k != MOSAIC or (rows + 2) * (cols + 2) <= RING_BYTES)) for k in range(5)]
                staged_seen += st[BGR]
                gathered_seen += 1 - st[BGR]
                want.append("T %d %d %d %d %d %d|%d %d %d %d|%d %s" % (w, h, vw, vh, x0, y0, r0, c0, rows, cols, pitch, " ".join(map(str, st))))
    assert got == want
    assert staged_seen >= 20 and gathered_seen >= 6  # the size list reaches both paths


def test_each_gathered_size_gathers(lines):
    for (w, h), (vw, vh) in SK.GATHERED:
        mine = [ln for ln in lines if ln.startswith("T %d %d %d %d " % (w, h, vw, vh))]
        assert mine and any(ln.split("|")[2].split()[1] == "0" for ln in mine)
