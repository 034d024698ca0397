"""calib_plan.h (rmcv_amd/csrc) compiled with the host C++ compiler alone: every refusal and limit of the calibration solve's entry points, the
workspace layout, the LDS budgets and the launch shapes, against the messages and a Python restatement.  No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <math.h>
#include <stdio.h>
#include "rmcv_amd/csrc/calib_plan.h"
using namespace rmcv;
static const char* s(const char* why) { return why ? why : ""; }
int main()
{
    const char x = 0;
    const rmcv_calib_params d = calib_default_params();
    printf("D %d %d %.17g\n", d.max_iters, d.fix_mask, d.eps);
    struct { int per, n, cols, rows; double sq; int w, h; rmcv_calib_params p; } p[] = {
        {88, 120, 11, 8, 30.0, 1280, 1024, d}, {4, 1, 2, 2, 1e-3, 1, 1, {1, 511, 0.0}}, {1024, 4096, 32, 32, 1e9, 1 << 30, 1 << 30, {100, 0, 1e300}},
        {88, 0, 11, 8, 30.0, 1280, 1024, d}, {88, 4097, 11, 8, 30.0, 1280, 1024, d}, {88, 120, 0, 8, 30.0, 1280, 1024, d}, {88, 120, 11, -1, 30.0, 1280, 1024, d},
        {88, 120, 3, 1, 30.0, 1280, 1024, d}, {1024, 120, 33, 32, 30.0, 1280, 1024, d}, {1024, 120, 65536, 65536, 30.0, 1280, 1024, d}, {87, 120, 11, 8, 30.0, 1280, 1024, d},
        {1025, 120, 11, 8, 30.0, 1280, 1024, d}, {88, 120, 11, 8, 0.0, 1280, 1024, d}, {88, 120, 11, 8, -30.0, 1280, 1024, d}, {88, 120, 11, 8, NAN, 1280, 1024, d},
        {88, 120, 11, 8, INFINITY, 1280, 1024, d}, {88, 120, 11, 8, 30.0, 0, 1024, d}, {88, 120, 11, 8, 30.0, 1280, 0, d}, {88, 120, 11, 8, 30.0, 1280, 1024, {0, 0, 1e-9}},
        {88, 120, 11, 8, 30.0, 1280, 1024, {101, 0, 1e-9}}, {88, 120, 11, 8, 30.0, 1280, 1024, {30, -1, 1e-9}}, {88, 120, 11, 8, 30.0, 1280, 1024, {30, 512, 1e-9}},
        {88, 120, 11, 8, 30.0, 1280, 1024, {30, 0, -1e-9}}, {88, 120, 11, 8, 30.0, 1280, 1024, {30, 0, NAN}}, {88, 120, 11, 8, 30.0, 1280, 1024, {30, 0, INFINITY}}};
    for (auto& q : p) printf("P %s\n", s(calib_params_refusal(q.per, q.n, q.cols, q.rows, q.sq, q.w, q.h, q.p)));
    rmcv_calib_guess g[3] = {};
    printf("G %s\n", s(calib_guess_refusal(nullptr, 3)));
    printf("G %s\n", s(calib_guess_refusal(g, 3)));                      // fx == 0: no guess, whatever else the entry holds
    g[1].camera_matrix[0] = 1800.0; g[1].camera_matrix[4] = 1800.0;
    printf("G %s\n", s(calib_guess_refusal(g, 3)));
    g[1].dist[4] = NAN;
    printf("G %s\n", s(calib_guess_refusal(g, 3)));
    printf("G %s\n", s(calib_guess_refusal(g, 1)));                      // (the entry lies behind the table)
    g[1].dist[4] = 0.0; g[1].camera_matrix[2] = INFINITY;
    printf("G %s\n", s(calib_guess_refusal(g, 3)));
    g[1].camera_matrix[2] = 0.0; g[1].camera_matrix[4] = 0.0;
    printf("G %s\n", s(calib_guess_refusal(g, 3)));
    g[1].camera_matrix[4] = 1.0; g[2].camera_matrix[0] = -1.0; g[2].camera_matrix[4] = 1.0;
    printf("G %s\n", s(calib_guess_refusal(g, 3)));
    g[2].camera_matrix[0] = 0.0;
    struct { const void *cor, *cnt, *res, *vw; int ncam; int per; const rmcv_calib_guess* gs; } e[] = {
        {&x, &x, &x, &x, 1, 88, nullptr}, {nullptr, &x, &x, &x, 1, 88, nullptr}, {&x, nullptr, &x, &x, 1, 88, nullptr}, {&x, &x, nullptr, &x, 1, 88, nullptr},
        {&x, &x, &x, nullptr, 1, 88, nullptr}, {&x, &x, &x, &x, 0, 88, nullptr}, {&x, &x, &x, &x, 65, 88, nullptr}, {&x, &x, &x, &x, 64, 88, nullptr},
        {&x, &x, &x, &x, 3, 87, nullptr}, {&x, &x, &x, &x, 3, 88, g}};
    for (auto& q : e) printf("E %s\n", s(calib_refusal(q.cor, q.cnt, q.res, q.vw, q.per, 120, q.ncam, 11, 8, 30.0, 1280, 1024, d, q.gs)));
    printf("M %s|%s\n", CALIB_NULL_TABLE, CALIB_CAMERAS);
    printf("L %d %d %d %d %d %d %d %d %d\n", RMCV_CALIB_VIEWS_MAX, RMCV_CALIB_VIEWS_PER_CAMERA_MAX, RMCV_CALIB_CAMERAS_MAX, CALIB_POINTS_MIN, CALIB_VIEWS_MIN, CALIB_ITERS_MAX,
           CALIB_FIX_ALL, CALIB_JACOBI_SWEEPS, RMCV_CORNER_PER_FRAME_MAX);
    printf("W %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", CV_H, CV_Q, CV_T, CV_QT, CV_TT, CV_COST, CV_COSTT, CV_DN, CV_PN, CV_BAD, CV_RED, CV_Y, CV_Z, CALIB_VIEW_WS);
    printf("S %lld %lld %lld\n", (long long)calib_ws_doubles(1), (long long)calib_ws_doubles(120), (long long)calib_ws_doubles(4096));
    printf("K %d %d %d %d %d %d %d %d %d\n", CALIB_HOMOGRAPHY_WAVES, CALIB_SOLVE_WAVES, CALIB_WAVE_LDS, CALIB_PASS_MAX, CALIB_CAM_STATE_BYTES, CALIB_HOMOGRAPHY_LDS_BYTES,
           CALIB_SOLVE_LDS_BYTES, CALIB_VGPR_BUDGET, CALIB_LDS_BUDGET);
    const int nv[] = {1, 4, 5, 120, 4096};
    for (int n : nv) printf("H %d %d\n", n, calib_homography_workgroups(n));
    printf("B %d %d %d %d %d %d\n", RMCV_CALIB_CONVERGED, RMCV_CALIB_MAX_ITERS, RMCV_CALIB_STALLED, RMCV_CALIB_TOO_FEW_VIEWS, RMCV_CALIB_BAD_INIT, RMCV_CALIB_TOO_MANY_VIEWS);
    printf("Z %d %d %d %d\n", (int)sizeof(rmcv_calib_params), (int)sizeof(rmcv_calib_guess), (int)sizeof(rmcv_calib_result), (int)sizeof(rmcv_calib_view));
    return 0;
}
'''


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    d = tmp_path_factory.mktemp("calib_plan")
    with open(d / "main.cpp", "w") as f:
        f.write(SRC)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-function", "-ffp-contract=off", "-I", ROOT, str(d / "main.cpp"), "-o", str(d / "plan")], check=True)
    return subprocess.run([str(d / "plan")], check=True, capture_output=True, text=True).stdout.splitlines()


def tagged(lines, tag):
    return [ln[2:] for ln in lines if ln.startswith(tag + " ")]


C = "calibration: "
VIEWS, PATTERN, PER = C + "n_views must be 1 .. 4096", C + "a cols x rows pattern of 4 .. 1024 corners", C + "per_frame must be cols * rows .. 1024"
SQUARE, IMAGE, ITERS = C + "square must be finite and > 0", C + "the image needs w >= 1 and h >= 1", C + "max_iters must be 1 .. 100"
FIX, EPS = C + "fix_mask must be 0 .. 511", C + "eps must be finite and >= 0"
NOT_FINITE, FOCAL = C + "a guess is not finite", C + "a guess needs focal lengths > 0"
NULL, CAMERAS = C + "null corner, count, result or view table", C + "n_cameras must be 1 .. 64"


def test_defaults_and_parameter_refusals(lines):
    assert tagged(lines, "D") == ["30 0 2.2204460492503131e-16"]
    assert tagged(lines, "P") == ["", "", "", VIEWS, VIEWS, PATTERN, PATTERN, PATTERN, PATTERN, PATTERN, PER, PER, SQUARE, SQUARE, SQUARE, SQUARE, IMAGE, IMAGE, ITERS, ITERS,
                                  FIX, FIX, EPS, EPS, EPS]


def test_guess_refusals(lines):
    assert tagged(lines, "G") == ["", "", "", NOT_FINITE, "", NOT_FINITE, FOCAL, FOCAL]


def test_entry_point_refusals(lines):
    assert tagged(lines, "E") == ["", NULL, NULL, NULL, NULL, CAMERAS, CAMERAS, "", PER, ""]
    assert tagged(lines, "M") == [NULL + "|" + CAMERAS]


def test_limits_records_and_status_bits(lines):
    assert tagged(lines, "L") == ["4096 256 64 4 3 100 511 30 1024"]
    assert tagged(lines, "B") == ["1 2 4 8 16 32"]
    assert tagged(lines, "Z") == ["16 112 144 96"]


def test_workspace_lds_and_launch_shapes(lines):
    off = list(map(int, tagged(lines, "W")[0].split()))
    sizes = [9, 4, 3, 4, 3, 1, 1, 1, 1, 1, 54, 54, 6]          # H, q, t, the trial's q and t, cost, the trial's, |db|^2, |p|^2, flag, T and e, Y, z
    assert off[0] == 0 and all(off[k] + sizes[k] == off[k + 1] for k in range(12)) and off[12] + 6 <= off[13] == 144
    assert tagged(lines, "S") == ["144 17280 589824"] and 589824 * 8 < 5 * 2 ** 20                           # the context's workspace: 4.5 MiB
    hw, sw, lds, pmax, cam, hb, sb, vgpr, ldsb = map(int, tagged(lines, "K")[0].split())
    assert (hw, sw, lds, pmax) == (4, 4, 172, 33) and lds >= 2 * 81 and lds >= 136 + 36
    # the passes of the 136 per-view sums: rows [0, 2), [2, 4), [4, 7), [7, 10), [10, 15) of the 15 x 15 triangle, their gradients, the cost
    passes = [sum(15 - i for i in range(a, b)) + (b - a) + (a == 0) for a, b in ((0, 2), (2, 4), (4, 7), (7, 10), (10, 15))]
    assert passes == [32, 27, 33, 24, 20] and sum(passes) == 136 and max(passes) == pmax
    assert cam == (9 + 9 + 9 + 81 + 9 + 6) * 8 + 24 and hb == 4 * 172 * 8 and sb == 4 * 172 * 8 + cam + 256 * 4
    assert (vgpr, ldsb) == (512, 160 * 1024) and sb <= ldsb and 2 * pmax + 128 <= vgpr
    assert tagged(lines, "H") == ["1 1", "4 1", "5 2", "120 30", "4096 1024"]
