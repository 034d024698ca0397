"""handeye_plan.h (rmcv_amd/csrc) compiled with the host C++ compiler alone: every refusal and limit of the hand-eye solve's entry points, the
walk over the pairs, the LDS budget and the launch shape, against the messages and a Python restatement.  No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <math.h>
#include <stdio.h>
#include "rmcv_amd/csrc/handeye_plan.h"
using namespace rmcv;
static const char* s(const char* why) { return why ? why : ""; }
int main()
{
    const char x = 0;
    const rmcv_handeye_params d = handeye_default_params();
    printf("D %.17g %d %d\n", d.min_w, d.reserved[0], d.reserved[1]);
    struct { const void *vw, *att, *res, *out; int n, ncam; double min_w; } e[] = {
        {&x, &x, &x, &x, 120, 1, 0.5}, {&x, &x, &x, &x, 1, 64, 0.0}, {&x, &x, &x, &x, 4096, 1, 0.99999}, {nullptr, &x, &x, &x, 120, 1, 0.5}, {&x, nullptr, &x, &x, 120, 1, 0.5},
        {&x, &x, nullptr, &x, 120, 1, 0.5}, {&x, &x, &x, nullptr, 120, 1, 0.5}, {&x, &x, &x, &x, 0, 1, 0.5}, {&x, &x, &x, &x, 4097, 1, 0.5}, {&x, &x, &x, &x, -1, 1, 0.5},
        {&x, &x, &x, &x, 120, 0, 0.5}, {&x, &x, &x, &x, 120, 65, 0.5}, {&x, &x, &x, &x, 120, 1, -1e-9}, {&x, &x, &x, &x, 120, 1, 1.0}, {&x, &x, &x, &x, 120, 1, NAN},
        {&x, &x, &x, &x, 120, 1, INFINITY}, {&x, &x, &x, &x, 120, 1, -INFINITY}, {nullptr, &x, &x, &x, 0, 0, NAN}};
    for (auto& q : e) printf("E %s\n", s(handeye_refusal(q.vw, q.att, q.res, q.out, q.n, q.ncam, {q.min_w, {0, 0}})));
    printf("M %s|%s|%s|%s\n", HANDEYE_NULL_TABLE, HANDEYE_VIEWS, HANDEYE_CAMERAS, HANDEYE_MIN_W);
    const int ns[] = {3, 4, 23, 24, 65, 256};
    for (int n : ns) {
        // every thread's walk together visits every pair once, each thread's own in ascending order
        long long seen = 0, sum = 0;
        int bad = 0;
        for (int T = 0; T < HANDEYE_THREADS; T++) {
            int i = 0, j = 1, p = T;
            handeye_pair_advance(i, j, T, n);
            while (i < n - 1) {
                const int idx = i * n - i * (i + 1) / 2 + (j - i - 1);
                bad += idx != p || j <= i || j >= n;
                seen++; sum += idx; p += HANDEYE_THREADS;
                handeye_pair_advance(i, j, HANDEYE_THREADS, n);
            }
        }
        printf("P %d %d %lld %lld %d\n", n, handeye_pairs(n), seen, sum, bad);
    }
    printf("L %d %d %d %d\n", HANDEYE_VIEWS_MIN, CALIB_VIEWS_PER_CAMERA_MAX, RMCV_CALIB_VIEWS_MAX, RMCV_CALIB_CAMERAS_MAX);
    printf("V %d %d %d %d %d %d\n", HV_B, HV_QG, HV_QC, HV_TC, HV_TG, HANDEYE_VIEW_LDS);
    printf("K %d %d %d %d %d %d\n", HANDEYE_WAVES, HANDEYE_THREADS, HANDEYE_SUMS_MAX, HANDEYE_CAM_STATE_BYTES, HANDEYE_LDS_BYTES, CALIB_LDS_BUDGET);
    printf("G %d %d %d\n", handeye_workgroups(1), handeye_workgroups(16), handeye_workgroups(64));
    printf("B %d %d %d %d\n", RMCV_HANDEYE_OK, RMCV_HANDEYE_T_UNOBSERVABLE, RMCV_HANDEYE_TOO_FEW_VIEWS, RMCV_HANDEYE_TOO_MANY_VIEWS);
    printf("Z %d %d %d %d %d\n", (int)sizeof(rmcv_handeye_params), (int)sizeof(rmcv_handeye_result), (int)sizeof(rmcv_handeye_view), (int)sizeof(rmcv_calib_view),
           (int)sizeof(rmcv_attitude));
    return 0;
}
'''


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    d = tmp_path_factory.mktemp("handeye_plan")
    with open(d / "main.cpp", "w") as f:
        f.write(SRC)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-function", "-ffp-contract=off", "-I", ROOT, str(d / "main.cpp"), "-o", str(d / "plan")], check=True)
    return subprocess.run([str(d / "plan")], check=True, capture_output=True, text=True).stdout.splitlines()


def tagged(lines, tag):
    return [ln[2:] for ln in lines if ln.startswith(tag + " ")]


H = "hand-eye: "
NULL, VIEWS, CAMERAS, MIN_W = H + "null view, attitude, result or view-output table", H + "n_views must be 1 .. 4096", H + "n_cameras must be 1 .. 64", H + "min_w must be finite and in [0, 1)"


def test_defaults_and_refusals(lines):
    assert tagged(lines, "D") == ["0.5 0 0"]
    assert tagged(lines, "E") == ["", "", "", NULL, NULL, NULL, NULL, VIEWS, VIEWS, VIEWS, CAMERAS, CAMERAS, MIN_W, MIN_W, MIN_W, MIN_W, MIN_W, NULL]
    assert tagged(lines, "M") == ["|".join((NULL, VIEWS, CAMERAS, MIN_W))]


def test_the_walk_over_the_pairs(lines):
    want = []
    for n in (3, 4, 23, 24, 65, 256):
        pairs = n * (n - 1) // 2
        want.append("%d %d %d %d 0" % (n, pairs, pairs, pairs * (pairs - 1) // 2))
    assert tagged(lines, "P") == want and want[-1].split()[1] == "32640"


def test_limits_records_and_status_bits(lines):
    assert tagged(lines, "L") == ["3 256 4096 64"]
    assert tagged(lines, "B") == ["1 2 4 8"]
    assert tagged(lines, "Z") == ["16 320 32 96 24"]


def test_lds_and_launch_shape(lines):
    off = list(map(int, tagged(lines, "V")[0].split()))
    sizes = [9, 4, 4, 3, 3]                                    # B, q_g, q_c, t_c, t_g
    assert off[0] == 0 and all(off[k] + sizes[k] == off[k + 1] for k in range(5)) and off[5] == 23
    waves, threads, sums, cam, lds, budget = map(int, tagged(lines, "K")[0].split())
    assert (waves, threads, sums) == (4, 256, 12) and sums >= 10 + 2                  # the rotation's pass: M's 10 sums and the two counts
    assert cam == 88 * 8 + 24 and lds == 256 * (23 * 8 + 4) + 4 * 12 * 8 + cam and lds <= 64 * 1024 <= budget == 160 * 1024
    assert tagged(lines, "G") == ["1 16 64"]
