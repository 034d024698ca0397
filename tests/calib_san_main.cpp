// calib_san_main.cpp -- the host form of rmcv_amd/csrc/device_calib.h under AddressSanitizer and UndefinedBehaviorSanitizer
// (tests/test_calib_sanitized.py compiles this file with -fsanitize=address,undefined and feeds it tests/calib_cases.py).  A stand-alone
// program with its own main: nothing of it is loaded into python, nothing touches a GPU.  Every table and the workspace are heap blocks of
// exactly their size.
//
// in:  int32 n_cases, then per case int32 {n_views, per_frame, cols, rows, w, h, max_iters, fix_mask, has_guess}, double {square, eps}, double guess [14]
//      (when has_guess), float [n_views][per_frame][2], int32 counts [n_views]
// out: per case the rmcv_calib_result (144 bytes) and n_views rmcv_calib_view (96 bytes each), both zeroed before the call
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../rmcv_amd/csrc/calib_plan.h"
#include "../rmcv_amd/csrc/device_calib.h"

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
        int32_t hd[9];
        double sq[2];
        get(hd, sizeof(hd), in);
        get(sq, sizeof(sq), in);
        const int n_views = hd[0], per_frame = hd[1];
        const rmcv_calib_params prm = {hd[6], hd[7], sq[1]};
        rmcv_calib_guess* guess = nullptr;
        if (hd[8]) {
            guess = (rmcv_calib_guess*)malloc(sizeof(rmcv_calib_guess));
            get(guess, sizeof(rmcv_calib_guess), in);
        }
        float* corners = (float*)malloc((size_t)n_views * per_frame * 8);
        int32_t* counts = (int32_t*)malloc((size_t)n_views * 4);
        get(corners, (size_t)n_views * per_frame * 8, in);
        get(counts, (size_t)n_views * 4, in);
        rmcv_calib_result* res = (rmcv_calib_result*)calloc(1, sizeof(rmcv_calib_result));
        rmcv_calib_view* views = (rmcv_calib_view*)calloc((size_t)n_views, sizeof(rmcv_calib_view));
        if (calib_refusal(corners, counts, res, views, per_frame, n_views, 1, hd[2], hd[3], sq[0], hd[4], hd[5], prm, guess)) return 3;
        CalibJob j{};
        j.corners = corners; j.per_frame = per_frame; j.counts = counts; j.n_views = n_views; j.view_camera = nullptr; j.n_cameras = 1;
        j.cols = hd[2]; j.rows = hd[3]; j.square = sq[0]; j.w = hd[4]; j.h = hd[5];
        j.max_iters = prm.max_iters; j.fix_mask = prm.fix_mask; j.eps = prm.eps;
        j.guesses = guess;
        j.ws = (double*)malloc((size_t)calib_ws_doubles(n_views) * 8);
        j.vcam = (int32_t*)malloc((size_t)n_views * 4);
        j.results = res; j.views = views;
        calib_solve_host(j);
        fwrite(res, sizeof(*res), 1, out);
        fwrite(views, sizeof(*views), (size_t)n_views, out);
        solved += (res->status & (RMCV_CALIB_CONVERGED | RMCV_CALIB_MAX_ITERS | RMCV_CALIB_STALLED)) != 0;
        free(j.vcam);
        free(j.ws);
        free(views);
        free(res);
        free(counts);
        free(corners);
        free(guess);
    }
    fclose(in);
    fclose(out);
    printf("cases %d solved %ld\n", n_cases, solved);
    return 0;
}
