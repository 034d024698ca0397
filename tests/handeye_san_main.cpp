// handeye_san_main.cpp -- the host form of rmcv_amd/csrc/device_handeye.h under AddressSanitizer and UndefinedBehaviorSanitizer
// (tests/test_handeye_sanitized.py compiles this file with -fsanitize=address,undefined and feeds it tests/handeye_cases.py).  A stand-alone
// program with its own main: nothing of it is loaded into python, nothing touches a GPU.  Every table is a heap block of exactly its size.
//
// in:  int32 n_cases, then per case int32 {n_views, n_cameras, has_gripper_t, has_view_camera}, double min_w, rmcv_calib_view [n_views],
//      rmcv_attitude [n_views], double [n_views][3] (when has_gripper_t), int32 [n_views] (when has_view_camera)
// out: per case n_cameras rmcv_handeye_result (320 bytes each) and n_views rmcv_handeye_view (32 bytes each), both zeroed before the call
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../rmcv_amd/csrc/device_handeye.h"
#include "../rmcv_amd/csrc/handeye_plan.h"

using namespace rmcv;

static void get(void* p, size_t n, FILE* f)
{
    if (n && fread(p, 1, n, f) != n) {
        fprintf(stderr, "short input\n");
        exit(2);
    }
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t n_cases = 0;
    get(&n_cases, 4, in);
    long solved = 0;
    for (int k = 0; k < n_cases; k++) {
        int32_t hd[4];
        double min_w;
        get(hd, sizeof(hd), in);
        get(&min_w, 8, in);
        const int n_views = hd[0], n_cameras = hd[1];
        rmcv_calib_view* views = (rmcv_calib_view*)malloc((size_t)n_views * sizeof(rmcv_calib_view));
        rmcv_attitude* att = (rmcv_attitude*)malloc((size_t)n_views * sizeof(rmcv_attitude));
        double* gt = hd[2] ? (double*)malloc((size_t)n_views * 24) : nullptr;
        int32_t* vc = hd[3] ? (int32_t*)malloc((size_t)n_views * 4) : nullptr;
        get(views, (size_t)n_views * sizeof(rmcv_calib_view), in);
        get(att, (size_t)n_views * sizeof(rmcv_attitude), in);
        if (gt) get(gt, (size_t)n_views * 24, in);
        if (vc) get(vc, (size_t)n_views * 4, in);
        rmcv_handeye_result* res = (rmcv_handeye_result*)calloc((size_t)n_cameras, sizeof(rmcv_handeye_result));
        rmcv_handeye_view* rows = (rmcv_handeye_view*)calloc((size_t)n_views, sizeof(rmcv_handeye_view));
        double* stage = (double*)malloc((size_t)CALIB_VIEWS_PER_CAMERA_MAX * HANDEYE_VIEW_LDS * 8);
        const rmcv_handeye_params prm = {min_w, {0, 0}};
        if (handeye_refusal(views, att, res, rows, n_views, n_cameras, prm)) return 3;
        HandEyeJob j{};
        j.views = views; j.att = att; j.gripper_t = gt; j.view_camera = vc; j.results = res; j.views_out = rows;
        j.min_w = min_w; j.n_views = n_views; j.n_cameras = n_cameras;
        handeye_solve_host(j, stage);
        fwrite(res, sizeof(*res), (size_t)n_cameras, out);
        fwrite(rows, sizeof(*rows), (size_t)n_views, out);
        for (int c = 0; c < n_cameras; c++) solved += (res[c].status & (RMCV_HANDEYE_OK | RMCV_HANDEYE_T_UNOBSERVABLE)) != 0;
        free(stage);
        free(rows);
        free(res);
        free(vc);
        free(gt);
        free(att);
        free(views);
    }
    fclose(in);
    fclose(out);
    printf("cases %d solved %ld\n", n_cases, solved);
    return 0;
}
