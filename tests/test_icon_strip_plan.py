"""icon_strip_plan.h (rmcv_amd/csrc) compiled with the host C++ compiler alone: every refusal of the icon strip's and the sheet's entry points,
the sheet's strip capacity, against the messages and a Python restatement.  No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <stdio.h>
#include "rmcv_amd/csrc/icon_strip_plan.h"
using namespace rmcv;
static const char* s(const char* why) { return why ? why : ""; }
int main()
{
    const char x = 0;
    struct { const void *bgr, *icon, *out; int w, h, stride, ow, oh, ostride; } a[] = {
        {&x, &x, &x, 4, 4, 12, 20, 20, 60}, {nullptr, &x, &x, 4, 4, 12, 20, 20, 60}, {&x, nullptr, &x, 4, 4, 12, 20, 20, 60}, {&x, &x, nullptr, 4, 4, 12, 20, 20, 60},
        {&x, &x, &x, 0, 4, 12, 20, 20, 60}, {&x, &x, &x, 4, 0, 12, 20, 20, 60}, {&x, &x, &x, 4, 4, 11, 20, 20, 60}, {&x, &x, &x, 4, 4, 12, 0, 20, 60},
        {&x, &x, &x, 4, 4, 12, 20, 0, 60}, {&x, &x, &x, 4, 4, 12, 257, 20, 771}, {&x, &x, &x, 4, 4, 12, 20, 257, 60}, {&x, &x, &x, 4, 4, 12, 20, 20, 59},
        {&x, &x, &x, 4, 4, 12, 256, 256, 768}, {&x, &x, &x, 1, 1, 3, 1, 1, 3}};
    for (auto& q : a) printf("A %s\n", s(affine_host_refusal(q.bgr, q.icon, q.out, q.w, q.h, q.stride, q.ow, q.oh, q.ostride)));
    struct { const void *bgr, *out; int w, h, stride; const void* arm; int n, side, cap, ostride; } im[] = {
        {&x, &x, 4, 4, 12, &x, 1, 20, 2, 120}, {nullptr, &x, 4, 4, 12, &x, 1, 20, 2, 120}, {&x, nullptr, 4, 4, 12, &x, 1, 20, 2, 120}, {&x, &x, 0, 4, 12, &x, 1, 20, 2, 120},
        {&x, &x, 4, 4, 11, &x, 1, 20, 2, 120}, {&x, &x, 4, 4, 12, nullptr, 1, 20, 2, 120}, {&x, &x, 4, 4, 12, nullptr, 0, 20, 2, 120}, {&x, &x, 4, 4, 12, &x, -1, 20, 2, 120},
        {&x, &x, 4, 4, 12, &x, 1, 0, 2, 120}, {&x, &x, 4, 4, 12, &x, 1, 257, 2, 1542}, {&x, &x, 4, 4, 12, &x, 1, 20, 0, 120}, {&x, &x, 4, 4, 12, &x, 1, 20, 1025, 61500},
        {&x, &x, 4, 4, 12, &x, 1, 20, 2, 119}, {&x, &x, 4, 4, 12, &x, 1, 256, 1024, 786432}};
    for (auto& q : im) printf("I %s\n", s(icon_strip_image_refusal(q.bgr, q.out, q.w, q.h, q.stride, q.arm, q.n, q.side, q.cap, q.ostride)));
    const int32_t ok[3] = {2, 0, 1}, rep[2] = {1, 1}, out[1] = {4}, neg[1] = {-1};
    const int A = RMCV_STAGE_ARMOURS, ALL = RMCV_STAGE_BINARY | RMCV_STAGE_CONTOURS | RMCV_STAGE_BLOBS | RMCV_STAGE_ARMOURS;
    struct { const int32_t* fr; int n, nf, stages, side, cap, maxa, stride; long long pitch; } b[] = {
        {ok, 3, 4, A, 20, 5, 8, 300, 6000}, {nullptr, 1, 4, A, 20, 5, 8, 300, 6000}, {ok, 0, 4, A, 20, 5, 8, 300, 6000}, {ok, 3, 2, A, 20, 5, 8, 300, 6000},
        {ok, 3, 4, A, 0, 5, 8, 300, 6000}, {ok, 3, 4, A, 257, 5, 8, 3855, 990735}, {ok, 3, 4, A, 20, 0, 8, 300, 6000}, {ok, 3, 4, A, 20, 9, 8, 540, 10800},
        {ok, 3, 4, A, 20, 8, 8, 480, 9600}, {ok, 3, 4, A, 20, 5, 8, 299, 6000}, {ok, 3, 4, A, 20, 5, 8, 300, 5999}, {ok, 3, 4, A, 20, 5, 8, 310, 6189},
        {ok, 3, 4, A, 20, 5, 8, 310, 6190}, {ok, 1, 4, A, 20, 5, 8, 300, 0}, {rep, 2, 4, A, 20, 5, 8, 300, 6000}, {out, 1, 4, A, 20, 5, 8, 300, 6000},
        {neg, 1, 4, A, 20, 5, 8, 300, 6000}, {ok, 3, 4, ALL & ~A, 20, 5, 8, 300, 6000}, {ok, 3, 4, 0, 20, 5, 8, 300, 6000}, {ok, 3, 4, ALL | RMCV_STAGE_IDENTITY, 256, 8, 8, 6144, 1572864}};
    for (auto& q : b) printf("B %s\n", s(icon_strips_refusal(q.fr, q.n, q.nf, q.stages, q.side, q.cap, q.maxa, q.stride, q.pitch)));
    printf("M %s|%s|%s|%s\n", ICON_STRIP_NULL_OUTPUT, ICON_STRIP_NOTHING_BOUND, ICON_STRIP_OVERFLOW, ICON_STRIP_BEYOND_LIMITS);
    struct { int vw, vh, side; } z[] = {{10, 10, 20}, {0, 10, 4}, {10, 0, 4}, {10, 10, 0}, {10, 10, 257}, {10, 10, 21}, {200, 10, 256}, {1, 1, 2}, {1, 1, 3}, {1 << 21, 4, 4}};
    for (auto& q : z) printf("Z %s\n", s(sheet_size_refusal(q.vw, q.vh, q.side)));
    struct { const int32_t* fr; int n, nf, stages, need, vw, vh, side, flags, stride; long long pitch; } sh[] = {
        {ok, 3, 4, ALL, ALL, 10, 10, 20, 7, 60, 1800}, {ok, 3, 4, ALL, ALL, 10, 10, 21, 7, 60, 1860}, {ok, 3, 4, ALL, ALL, 10, 10, 20, 7, 59, 1800},
        {ok, 3, 4, ALL, ALL, 10, 10, 20, 7, 60, 1799}, {ok, 3, 4, ALL, ALL, 10, 10, 20, 7, 64, 1915}, {ok, 3, 4, ALL, ALL, 10, 10, 20, 7, 64, 1916},
        {ok, 1, 4, ALL, ALL, 10, 10, 20, 7, 60, 0}, {ok, 3, 4, ALL, ALL, 10, 10, 20, 8, 60, 1800}, {ok, 3, 4, ALL, ALL, 65, 10, 20, 7, 390, 11700},
        {ok, 3, 4, ALL, ALL, 10, 49, 20, 7, 60, 4140}, {rep, 2, 4, ALL, ALL, 10, 10, 20, 7, 60, 1800}, {out, 1, 4, ALL, ALL, 10, 10, 20, 7, 60, 1800},
        {nullptr, 1, 4, ALL, ALL, 10, 10, 20, 7, 60, 1800}, {ok, 3, 2, ALL, ALL, 10, 10, 20, 7, 60, 1800}, {ok, 3, 4, ALL & ~A, ALL, 10, 10, 20, 0, 60, 1800},
        {ok, 3, 4, A, RMCV_STAGE_BINARY | A, 10, 10, 20, 0, 60, 1800}, {ok, 3, 4, RMCV_STAGE_BINARY | A, RMCV_STAGE_BINARY | A, 10, 10, 20, 0, 60, 1800}};
    for (auto& q : sh) printf("S %s\n", s(sheets_refusal(q.fr, q.n, q.nf, q.stages, q.need, q.vw, q.vh, q.side, 64, 48, q.flags, q.stride, q.pitch)));
    printf("N %s|%s|%s|%s\n", SHEET_NULL_OUTPUT, SHEET_OVERFLOW, SHEET_FEWER_FRAMES, SHEET_FEWER_STAGES);
    for (int vw = 1; vw <= 40; vw += 3)
        for (int side = 1; side <= 2 * vw && side <= 30; side += 4)
            for (int most = 1; most <= 33; most += 8) printf("C %d %d %d %d\n", vw, side, most, sheet_cap(vw, side, most));
    printf("L %d %d\n", ICON_SIDE_MAX, RMCV_ICON_STRIP_CAP_MAX);
    return 0;
}
'''


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    d = tmp_path_factory.mktemp("icon_strip_plan")
    with open(d / "main.cpp", "w") as f:
        f.write(SRC)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-function", "-ffp-contract=off", "-I", ROOT, str(d / "main.cpp"), "-o", str(d / "plan")], check=True)
    return subprocess.run([str(d / "plan")], check=True, capture_output=True, text=True).stdout.splitlines()


def tagged(lines, tag):
    return [ln[2:] for ln in lines if ln.startswith(tag + " ")]


def test_host_image_refusals(lines):
    size = "the output size must be 1 .. 256 x 1 .. 256"
    assert tagged(lines, "A") == ["", "null buffer", "null buffer", "null buffer", "the image needs w >= 1 and h >= 1", "the image needs w >= 1 and h >= 1", "stride < 3 w",
                                  size, size, size, size, "out_stride < 3 ow", "", ""]
    assert tagged(lines, "I") == ["", "null buffer", "null buffer", "the image needs w >= 1 and h >= 1", "stride < 3 w", "n armours without a list", "",
                                  "n armours without a list", "side must be 1 .. 256", "side must be 1 .. 256", "cap must be 1 .. RMCV_ICON_STRIP_CAP_MAX",
                                  "cap must be 1 .. RMCV_ICON_STRIP_CAP_MAX", "out_stride < 3 cap side", ""]


def test_batch_refusals(lines):
    p = "icon strips: "
    assert tagged(lines, "B") == ["", p + "no frames chosen", p + "no frames chosen", p + "more strips than the batch has frames", p + "side must be 1 .. 256",
                                  p + "side must be 1 .. 256", p + "cap must be 1 .. max_armours", p + "cap must be 1 .. max_armours", "", p + "out_stride < 3 cap side",
                                  p + "out_pitch < out_stride (side - 1) + 3 cap side", p + "out_pitch < out_stride (side - 1) + 3 cap side", "", "",
                                  p + "a frame index is repeated", p + "a frame index is outside the batch", p + "a frame index is outside the batch",
                                  p + "the batch's run lacked RMCV_STAGE_ARMOURS", p + "the batch's run lacked RMCV_STAGE_ARMOURS", ""]
    assert tagged(lines, "M") == ["icon strips: null output|icon strips: no frames are bound|rmcv_batch_get_icon_strip: the frame exceeded a context limit (see its status): "
                                  "its tables are not its lists|rmcv_icon_strip: image beyond the context's max_width / max_height, or cap or n beyond its max_armours"]


def test_sheet_refusals(lines):
    p = "labeler sheet: "
    assert tagged(lines, "Z") == ["", p + "the view size must be at least 1 x 1", p + "the view size must be at least 1 x 1", p + "side must be 1 .. 256",
                                  p + "side must be 1 .. 256", p + "side > 2 vw", "", "", p + "side > 2 vw", p + "the view size is beyond 2^20"]
    v = "source views: "
    assert tagged(lines, "S") == ["", p + "side > 2 vw", p + "out_stride < 6 vw", p + "out_pitch < out_stride (vh + side - 1) + 6 vw",
                                  p + "out_pitch < out_stride (vh + side - 1) + 6 vw", "", "", v + "unknown view flags",
                                  v + "the view size must be 1 .. max_width x 1 .. max_height", v + "the view size must be 1 .. max_width x 1 .. max_height",
                                  v + "a frame index is repeated", v + "a frame index is outside the batch", v + "no frames chosen",
                                  v + "more views than the batch has frames", v + "the batch's run lacked a stage the view flags need",
                                  v + "the batch's run lacked a stage the view flags need", ""]
    assert tagged(lines, "N") == ["labeler sheet: null output|rmcv_batch_get_labeler_sheet: the frame exceeded a context limit (see its status): its tables are not its "
                                  "lists|the batch has fewer frames than the sheets name (rmcv_pipeline_set_sheets)|the batch's stages lack what the sheets need "
                                  "(rmcv_pipeline_set_sheets)"]


def test_sheet_cap_and_limits(lines):
    got = [tuple(map(int, ln.split())) for ln in tagged(lines, "C")]
    assert len(got) > 100
    for vw, side, most, cap in got:
        assert cap == min(2 * vw // side, most) and cap * side <= 2 * vw
    assert tagged(lines, "L") == ["256 1024"]
