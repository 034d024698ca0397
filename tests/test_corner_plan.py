"""corner_plan.h (rmcv_amd/csrc) compiled with the host C++ compiler alone: every refusal and limit of the corner refinement's entry points,
the LDS budget and the launch shape, against the messages and a Python restatement.  No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <math.h>
#include <stdio.h>
#include "rmcv_amd/csrc/corner_plan.h"
using namespace rmcv;
static const char* s(const char* why) { return why ? why : ""; }
int main()
{
    const char x = 0;
    struct { int wx, wy, zx, zy, it; double eps; } p[] = {
        {8, 8, -1, -1, 40, 0.001}, {1, 1, -1, -1, 1, 0.0}, {15, 15, 14, 14, 100, 1e300}, {0, 8, -1, -1, 40, 0.001}, {8, 0, -1, -1, 40, 0.001},
        {16, 8, -1, -1, 40, 0.001}, {8, 16, -1, -1, 40, 0.001}, {8, 8, 0, 0, 40, 0.001}, {8, 8, 7, 7, 40, 0.001}, {8, 8, 8, 0, 40, 0.001},
        {8, 8, 0, 8, 40, 0.001}, {8, 8, -1, 0, 40, 0.001}, {8, 8, 0, -1, 40, 0.001}, {8, 8, -2, -2, 40, 0.001}, {8, 3, 2, 2, 40, 0.001},
        {8, 3, 2, 3, 40, 0.001}, {8, 8, -1, -1, 0, 0.001}, {8, 8, -1, -1, 101, 0.001}, {8, 8, -1, -1, 40, -0.001}, {8, 8, -1, -1, 40, NAN},
        {8, 8, -1, -1, 40, INFINITY}, {8, 8, -1, -1, 40, -0.0}};
    for (auto& q : p) printf("P %s\n", s(corner_params_refusal(q.wx, q.wy, q.zx, q.zy, q.it, q.eps)));
    struct { const void *bgr, *cor; int w, h, stride, n; } im[] = {
        {&x, &x, 4, 4, 12, 1}, {nullptr, &x, 4, 4, 12, 1}, {&x, nullptr, 4, 4, 12, 1}, {&x, nullptr, 4, 4, 12, 0}, {&x, &x, 0, 4, 12, 1}, {&x, &x, 4, 0, 12, 1},
        {&x, &x, 4, 4, 11, 1}, {&x, &x, 4, 4, 12, -1}, {&x, &x, 1, 1, 3, 1}};
    for (auto& q : im) printf("I %s\n", s(corner_image_refusal(q.bgr, q.cor, q.w, q.h, q.stride, q.n)));
    const int32_t ok[3] = {2, 0, 1}, rep[2] = {1, 1}, out[1] = {4}, neg[1] = {-1}, zero[1] = {0};
    const int B = RMCV_STAGE_BINARY;
    struct { const int32_t* fr; int n, nf, kind, stages; const void* tab; int per, wx, it; } b[] = {
        {ok, 3, 4, SOURCE_BGR, 0, &x, 12, 8, 40}, {nullptr, 1, 4, SOURCE_BGR, 0, &x, 12, 8, 40}, {ok, 0, 4, SOURCE_BGR, 0, &x, 12, 8, 40}, {ok, 3, 2, SOURCE_BGR, 0, &x, 12, 8, 40},
        {rep, 2, 4, SOURCE_BGR, 0, &x, 12, 8, 40}, {out, 1, 4, SOURCE_BGR, 0, &x, 12, 8, 40}, {neg, 1, 4, SOURCE_BGR, 0, &x, 12, 8, 40}, {ok, 3, 4, SOURCE_BGR, 0, nullptr, 12, 8, 40},
        {ok, 3, 4, SOURCE_BGR, 0, &x, 0, 8, 40}, {ok, 3, 4, SOURCE_BGR, 0, &x, 1025, 8, 40}, {ok, 3, 4, SOURCE_BGR, 0, &x, 1024, 8, 40}, {ok, 3, 4, SOURCE_BGR, 0, &x, 12, 16, 40},
        {ok, 3, 4, SOURCE_BGR, 0, &x, 12, 8, 0}, {ok, 3, 4, SOURCE_MOSAIC, 0, &x, 12, 8, 40}, {ok, 3, 4, SOURCE_MOSAIC_RAW, 0, &x, 12, 8, 40}, {ok, 3, 4, SOURCE_BGR_WIN, 0, &x, 12, 8, 40},
        {ok, 3, 4, SOURCE_BGR_LUT, 0, &x, 12, 8, 40}, {ok, 3, 4, SOURCE_BGR_WIN, B, &x, 12, 8, 40}, {ok, 3, 4, SOURCE_BGR_LUT, B | RMCV_STAGE_CONTOURS, &x, 12, 8, 40},
        {ok, 3, 4, SOURCE_BGR_WIN, RMCV_STAGE_CONTOURS, &x, 12, 8, 40}, {zero, 1, 1, SOURCE_BGR, 0, &x, 1, 1, 1}};
    for (auto& q : b) printf("B %s\n", s(corners_refusal(q.fr, q.n, q.nf, q.kind, q.stages, q.tab, q.per, q.wx, q.wx, -1, -1, q.it, 0.001)));
    printf("M %s|%s|%s|%s|%s\n", CORNER_PER_FRAME, CORNER_BEYOND_LIMITS, CORNER_NULL_TABLE, CORNER_NOTHING_BOUND, CORNER_NEEDS_RUN);
    printf("L %d %d %d %d %d %d %d %d\n", RMCV_CORNER_WIN_MAX, RMCV_CORNER_ITERS_MAX, RMCV_CORNER_PER_FRAME_MAX, CORNER_WAVES, CORNER_WIN_W_MAX, CORNER_GRAY_MAX, CORNER_PATCH_MAX,
           CORNER_MASK_MAX);
    for (int wx = 1; wx <= 15; wx++)
        for (int wy = 1; wy <= 15; wy += 7) {
            const int ww = corner_win_w(wx), wh = corner_win_w(wy);
            printf("S %d %d %d %d %d %d\n", ww, wh, corner_gray_bytes(ww, wh), corner_patch_bytes(ww, wh), corner_mask_bytes(ww, wh), corner_lds_bytes(ww, wh));
        }
    struct { int n, per; } g[] = {{1, 1}, {1, 4}, {1, 5}, {3, 12}, {2, 5}, {120, 88}, {4096, 1024}};
    for (auto& q : g) printf("G %d %d %lld\n", q.n, q.per, (long long)corner_workgroups(q.n, q.per));
    return 0;
}
'''


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    d = tmp_path_factory.mktemp("corner_plan")
    with open(d / "main.cpp", "w") as f:
        f.write(SRC)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-function", "-ffp-contract=off", "-I", ROOT, str(d / "main.cpp"), "-o", str(d / "plan")], check=True)
    return subprocess.run([str(d / "plan")], check=True, capture_output=True, text=True).stdout.splitlines()


def tagged(lines, tag):
    return [ln[2:] for ln in lines if ln.startswith(tag + " ")]


WIN = "corners: win_x and win_y must be 1 .. 15"
ZERO = "corners: the zero zone must be (-1, -1) or 0 <= zero_x < win_x and 0 <= zero_y < win_y"
ITERS = "corners: max_iters must be 1 .. 100"
EPS = "corners: eps must be finite and >= 0"
RUN = "corners: a windowed or enhanced batch is read behind a run with RMCV_STAGE_BINARY (its origins / tables)"


def test_parameter_refusals(lines):
    assert tagged(lines, "P") == ["", "", "", WIN, WIN, WIN, WIN, "", "", ZERO, ZERO, ZERO, ZERO, ZERO, "", ZERO, ITERS, ITERS, EPS, EPS, EPS, ""]


def test_image_refusals(lines):
    assert tagged(lines, "I") == ["", "null buffer", "null buffer", "", "the image needs w >= 1 and h >= 1", "the image needs w >= 1 and h >= 1", "stride < 3 w",
                                  "corners: n < 0", ""]


def test_batch_refusals(lines):
    v = "source views: "
    per = "corners: per_frame must be 1 .. 1024"
    assert tagged(lines, "B") == ["", v + "no frames chosen", v + "no frames chosen", v + "more views than the batch has frames", v + "a frame index is repeated",
                                  v + "a frame index is outside the batch", v + "a frame index is outside the batch", "corners: null corner table", per, per, "",
                                  WIN, ITERS, "", "", RUN, RUN, "", "", RUN, ""]
    assert tagged(lines, "M") == [per + "|rmcv_corner_subpix: image beyond the context's max_width / max_height|corners: null corner table|corners: no frames are bound|" + RUN]


def test_limits_lds_and_launch_shape(lines):
    assert tagged(lines, "L") == ["15 100 1024 4 31 1156 1089 961"]
    got = [tuple(map(int, ln.split())) for ln in tagged(lines, "S")]
    assert len(got) == 45
    for ww, wh, gray, patch, mask, lds in got:
        assert gray == ((ww + 3) * (wh + 3) + 3) // 4 * 4 and patch == 4 * (ww + 2) * (wh + 2) and mask == 4 * ww * wh
        assert lds == 4 * (gray + patch) + mask and gray <= 1156 and patch <= 4 * 1089 and mask <= 4 * 961
    assert got[-1] == (31, 31, 1156, 4356, 3844, 25892) and 6 * 25892 <= 160 * 1024   # win 15: 1.2 KB + 4.4 KB per wavefront, six workgroups a CU
    assert [tuple(map(int, ln.split())) for ln in tagged(lines, "G")] == [(1, 1, 1), (1, 4, 1), (1, 5, 2), (3, 12, 9), (2, 5, 3), (120, 88, 2640), (4096, 1024, 1048576)]
