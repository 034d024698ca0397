"""chess_plan.h (rmcv_amd/csrc) compiled with the host C++ compiler alone: every refusal and limit of the chessboard detector's entry points,
the LDS budgets and the launch shapes, against the messages and a Python restatement.  No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <stdio.h>
#include "rmcv_amd/csrc/chess_plan.h"
using namespace rmcv;
static const char* s(const char* why) { return why ? why : ""; }
int main()
{
    const char x = 0;
    const rmcv_chess_params d = chess_default_params();
    printf("D %d %d %d %d %d\n", d.threshold, d.contrast, d.nms, d.dist_min, d.dist_max);
    struct { int cols, rows; rmcv_chess_params p; } p[] = {
        {5, 4, d}, {2, 2, {0, 0, 1, 1, 1}}, {32, 32, {1 << 30, 255, 7, 1023, 1023}}, {1, 4, d}, {5, 1, d}, {33, 4, d}, {5, 33, d}, {5, 4, {-1, 10, 3, 6, 255}},
        {5, 4, {1000, -1, 3, 6, 255}}, {5, 4, {1000, 256, 3, 6, 255}}, {5, 4, {1000, 10, 0, 6, 255}}, {5, 4, {1000, 10, 8, 6, 255}}, {5, 4, {1000, 10, 3, 0, 255}},
        {5, 4, {1000, 10, 3, 256, 255}}, {5, 4, {1000, 10, 3, 6, 1024}}, {5, 4, {1000, 10, 3, 255, 255}}};
    for (auto& q : p) printf("P %s\n", s(chess_params_refusal(q.cols, q.rows, q.p)));
    struct { const void *bgr, *cor; int w, h, stride; } im[] = {
        {&x, &x, 4, 4, 12}, {nullptr, &x, 4, 4, 12}, {&x, nullptr, 4, 4, 12}, {&x, &x, 0, 4, 12}, {&x, &x, 4, 0, 12}, {&x, &x, 4, 4, 11}, {&x, &x, 32767, 1, 98301},
        {&x, &x, 32768, 1, 98304}, {&x, &x, 1, 32768, 3}, {&x, &x, 1, 1, 3}};
    for (auto& q : im) printf("I %s\n", s(chess_image_refusal(q.bgr, q.cor, q.w, q.h, q.stride)));
    const int32_t ok[3] = {2, 0, 1}, rep[2] = {1, 1}, out[1] = {4}, neg[1] = {-1};
    const int B = RMCV_STAGE_BINARY;
    struct { const int32_t* fr; int n, nf, kind, stages; const void *tab, *cnt; int per, cols; } b[] = {
        {ok, 3, 4, SOURCE_BGR, 0, &x, &x, 20, 5}, {nullptr, 1, 4, SOURCE_BGR, 0, &x, &x, 20, 5}, {ok, 0, 4, SOURCE_BGR, 0, &x, &x, 20, 5}, {ok, 3, 2, SOURCE_BGR, 0, &x, &x, 20, 5},
        {rep, 2, 4, SOURCE_BGR, 0, &x, &x, 20, 5}, {out, 1, 4, SOURCE_BGR, 0, &x, &x, 20, 5}, {neg, 1, 4, SOURCE_BGR, 0, &x, &x, 20, 5}, {ok, 3, 4, SOURCE_BGR, 0, nullptr, &x, 20, 5},
        {ok, 3, 4, SOURCE_BGR, 0, &x, nullptr, 20, 5}, {ok, 3, 4, SOURCE_BGR, 0, &x, &x, 19, 5}, {ok, 3, 4, SOURCE_BGR, 0, &x, &x, 1025, 5}, {ok, 3, 4, SOURCE_BGR, 0, &x, &x, 1024, 5},
        {ok, 3, 4, SOURCE_BGR, 0, &x, &x, 20, 33}, {ok, 3, 4, SOURCE_MOSAIC, 0, &x, &x, 20, 5}, {ok, 3, 4, SOURCE_MOSAIC_RAW, 0, &x, &x, 20, 5}, {ok, 3, 4, SOURCE_BGR_WIN, 0, &x, &x, 20, 5},
        {ok, 3, 4, SOURCE_BGR_LUT, 0, &x, &x, 20, 5}, {ok, 3, 4, SOURCE_BGR_WIN, B, &x, &x, 20, 5}, {ok, 3, 4, SOURCE_BGR_LUT, B | RMCV_STAGE_CONTOURS, &x, &x, 20, 5},
        {ok, 3, 4, SOURCE_BGR_WIN, RMCV_STAGE_CONTOURS, &x, &x, 20, 5}};
    for (auto& q : b) printf("B %s\n", s(chessboards_refusal(q.fr, q.n, q.nf, q.kind, q.stages, q.tab, q.cnt, q.per, q.cols, 4, d)));
    printf("M %s|%s|%s|%s|%s\n", CHESS_PER_FRAME, CHESS_BEYOND_LIMITS, CHESS_NULL_TABLE, CHESS_NOTHING_BOUND, CHESS_NEEDS_RUN);
    printf("L %d %d %d %d %d %d %d %d %d %d %d %d\n", RMCV_CHESS_CAND_MAX, CHESS_SIDE_MIN, CHESS_SIDE_MAX, CHESS_NMS_MAX, CHESS_DIST_MAX, CHESS_EXTENT_MAX, CHESS_GRAY_MAX, CHESS_RESP_MAX,
           CHESS_GRID_THREADS, CHESS_GRID_LDS_BYTES, CHESS_LIST_WORDS, RMCV_CHESS_COUNT_MASK);
    printf("T %d %d %d %d %d\n", CHESS_TILE_X, CHESS_TILE_Y, CHESS_GRAY_PITCH, CHESS_RESP_PITCH, CHESS_RESPONSE_LDS_BYTES);
    for (int nms = 1; nms <= CHESS_NMS_MAX; nms++) printf("S %d %d %d %d %d\n", nms, chess_gray_cols(nms), chess_gray_rows(nms), chess_resp_cols(nms), chess_resp_rows(nms));
    const int ext[][2] = {{1, 1}, {64, 32}, {65, 33}, {160, 128}, {150, 128}, {160, 120}, {1280, 1024}, {32767, 32767}};
    for (auto& e : ext) printf("G %d %d %d %d\n", e[0], e[1], chess_tiles_x(e[0]), chess_tiles_y(e[1]));
    return 0;
}
'''


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    d = tmp_path_factory.mktemp("chess_plan")
    with open(d / "main.cpp", "w") as f:
        f.write(SRC)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-function", "-ffp-contract=off", "-I", ROOT, str(d / "main.cpp"), "-o", str(d / "plan")], check=True)
    return subprocess.run([str(d / "plan")], check=True, capture_output=True, text=True).stdout.splitlines()


def tagged(lines, tag):
    return [ln[2:] for ln in lines if ln.startswith(tag + " ")]


SIDE = "chessboard: cols and rows must be 2 .. 32"
THR = "chessboard: threshold must be >= 0"
CON = "chessboard: contrast must be 0 .. 255"
NMS = "chessboard: nms must be 1 .. 7"
DIST = "chessboard: 1 <= dist_min <= dist_max <= 1023"
RUN = "chessboard: a windowed or enhanced batch is read behind a run with RMCV_STAGE_BINARY (its origins / tables)"
PER = "chessboard: per_frame must be cols * rows .. 1024"
NULL = "chessboard: null corner or count table"


def test_defaults_and_parameter_refusals(lines):
    assert tagged(lines, "D") == ["1000 10 3 6 255"]
    assert tagged(lines, "P") == ["", "", "", SIDE, SIDE, SIDE, SIDE, THR, CON, CON, NMS, NMS, DIST, DIST, DIST, ""]


def test_image_refusals(lines):
    size, big = "the image needs w >= 1 and h >= 1", "chessboard: the image may be at most 32767 x 32767"
    assert tagged(lines, "I") == ["", "null buffer", "null buffer", size, size, "stride < 3 w", "", big, big, ""]


def test_batch_refusals(lines):
    v = "source views: "
    assert tagged(lines, "B") == ["", v + "no frames chosen", v + "no frames chosen", v + "more views than the batch has frames", v + "a frame index is repeated",
                                  v + "a frame index is outside the batch", v + "a frame index is outside the batch", NULL, NULL, PER, PER, "", SIDE, "", "", RUN, RUN, "", "", RUN]
    assert tagged(lines, "M") == [PER + "|rmcv_find_chessboard: image beyond the context's max_width / max_height|" + NULL + "|chessboard: no frames are bound|" + RUN]


def test_limits_lds_and_launch_shapes(lines):
    assert tagged(lines, "L") == ["1024 2 32 7 1023 32767 4928 3588 512 48132 2048 2047"]
    assert tagged(lines, "T") == ["64 32 88 78 12104"] and 12104 == 88 * 56 + 2 * 78 * 46      # the response kernel's static LDS: gray bytes, int16 responses
    got = [tuple(map(int, ln.split())) for ln in tagged(lines, "S")]
    assert [g[0] for g in got] == list(range(1, 8))
    for nms, gc, gr, rc, rr in got:
        assert gc == 64 + 2 * (5 + nms) <= 88 and gr == 32 + 2 * (5 + nms) and rc == 64 + 2 * nms <= 78 and rr == 32 + 2 * nms
        assert 88 * gr <= 4928 and 78 * rr <= 3588                                              # every nms fits the images at their constant pitches
    assert 48132 == 1024 * 47 + 4 and 48132 <= 64 * 1024                                        # the grid kernel's static LDS
    assert [tuple(map(int, ln.split())) for ln in tagged(lines, "G")] == [(1, 1, 1, 1), (64, 32, 1, 1), (65, 33, 2, 2), (160, 128, 3, 4), (150, 128, 3, 4), (160, 120, 3, 4),
                                                                          (1280, 1024, 20, 32), (32767, 32767, 512, 1024)]
