// corner_san_main.cpp -- the host form of rmcv_amd/csrc/device_corner.h under AddressSanitizer and UndefinedBehaviorSanitizer
// (tests/test_corner_sanitized.py compiles this file with -fsanitize=address,undefined and feeds it tests/corner_cases.py).  A stand-alone
// program with its own main: nothing of it is loaded into python, nothing touches a GPU.  Every image and table is a heap block of exactly its
// size; every case runs on the image with packed rows and with padded rows whose last one ends with its pixels.
//
// in:  int32 n_cases, then per case int32 {w, h, n, win_x, win_y, zero_x, zero_y, max_iters}, double eps, u8 [h][3 w], float [n][2]
// out: per case and layout: float [n][2] refined, int32 [n] status; then per case the mask float [win_h][win_w] and the gray image u8 [h][w]
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../rmcv_amd/csrc/corner_plan.h"
#include "../rmcv_amd/csrc/device_corner.h"

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
    long corners_done = 0;
    for (int k = 0; k < n_cases; k++) {
        int32_t hd[8];
        double eps;
        get(hd, sizeof(hd), in);
        get(&eps, 8, in);
        const int w = hd[0], h = hd[1], n = hd[2], win_x = hd[3], win_y = hd[4], zx = hd[5], zy = hd[6], iters = hd[7];
        if (corner_params_refusal(win_x, win_y, zx, zy, iters, eps)) return 3;
        uint8_t* packed = (uint8_t*)malloc((size_t)3 * w * h);
        get(packed, (size_t)3 * w * h, in);
        float* guess = (float*)malloc((size_t)n * 8);
        get(guess, (size_t)n * 8, in);
        const int pstride = 3 * w + 13;
        uint8_t* padded = (uint8_t*)malloc((size_t)pstride * (h - 1) + (size_t)3 * w);   // (the last row ends with its pixels)
        memset(padded, 0x5A, (size_t)pstride * (h - 1) + (size_t)3 * w);
        for (int y = 0; y < h; y++) memcpy(padded + (size_t)y * pstride, packed + (size_t)y * 3 * w, (size_t)3 * w);
        if (corner_image_refusal(packed, guess, w, h, 3 * w, n) || corner_image_refusal(padded, guess, w, h, pstride, n)) return 3;
        for (int layout = 0; layout < 2; layout++) {
            float* cor = (float*)malloc((size_t)n * 8);
            int32_t* st = (int32_t*)malloc((size_t)n * 4);
            memcpy(cor, guess, (size_t)n * 8);
            corner_subpix_host(layout ? padded : packed, w, h, layout ? pstride : 3 * w, cor, n, win_x, win_y, zx, zy, iters, eps, layout ? st : nullptr);
            if (!layout) { // (a null status table is allowed: run once more for the words)
                memcpy(cor, guess, (size_t)n * 8);
                corner_subpix_host(packed, w, h, 3 * w, cor, n, win_x, win_y, zx, zy, iters, eps, st);
            }
            fwrite(cor, 8, n, out);
            fwrite(st, 4, n, out);
            free(cor);
            free(st);
            corners_done += n;
        }
        const int win_w = 2 * win_x + 1, win_h = 2 * win_y + 1;
        float* mask = (float*)malloc((size_t)win_w * win_h * 4);
        corner_mask(win_x, win_y, zx, zy, mask);
        fwrite(mask, 4, (size_t)win_w * win_h, out);
        free(mask);
        uint8_t* gray = (uint8_t*)malloc((size_t)w * h);
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) gray[(size_t)y * w + x] = (uint8_t)corner_gray_host_at(padded, w, h, pstride, x, y);
        fwrite(gray, 1, (size_t)w * h, out);
        free(gray);
        free(padded);
        free(guess);
        free(packed);
    }
    fclose(in);
    fclose(out);
    printf("cases %d corners %ld\n", n_cases, corners_done);
    return 0;
}
