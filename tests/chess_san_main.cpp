// chess_san_main.cpp -- the host form of rmcv_amd/csrc/device_chess.h under AddressSanitizer and UndefinedBehaviorSanitizer
// (tests/test_chess_sanitized.py compiles this file with -fsanitize=address,undefined and feeds it tests/chess_cases.py).  A stand-alone
// program with its own main: nothing of it is loaded into python, nothing touches a GPU.  Every image and table is a heap block of exactly its
// size; every case runs on the image with packed rows and with padded rows whose last one ends with its pixels.
//
// in:  int32 n_cases, then per case int32 {w, h, cols, rows, threshold, contrast, nms, dist_min, dist_max}, u8 [h][3 w]
// out: per case and layout: int32 status, int32 n candidates, int32 [n][3] candidates, float [cols rows][2] corners (0x7FC00000 where no board)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../rmcv_amd/csrc/chess_plan.h"
#include "../rmcv_amd/csrc/device_chess.h"

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
    long boards = 0;
    for (int k = 0; k < n_cases; k++) {
        int32_t hd[9];
        get(hd, sizeof(hd), in);
        const int w = hd[0], h = hd[1], cols = hd[2], rows = hd[3];
        const rmcv_chess_params prm = {hd[4], hd[5], hd[6], hd[7], hd[8]};
        if (chess_params_refusal(cols, rows, prm)) return 3;
        uint8_t* packed = (uint8_t*)malloc((size_t)3 * w * h);
        get(packed, (size_t)3 * w * h, in);
        const int pstride = 3 * w + 13;
        uint8_t* padded = (uint8_t*)malloc((size_t)pstride * (h - 1) + (size_t)3 * w);   // (the last row ends with its pixels)
        memset(padded, 0x5A, (size_t)pstride * (h - 1) + (size_t)3 * w);
        for (int y = 0; y < h; y++) memcpy(padded + (size_t)y * pstride, packed + (size_t)y * 3 * w, (size_t)3 * w);
        for (int layout = 0; layout < 2; layout++) {
            const size_t want = (size_t)cols * rows;
            uint32_t* cor = (uint32_t*)malloc(want * 8);
            for (size_t i = 0; i < 2 * want; i++) cor[i] = 0x7FC00000u;
            int32_t* cand = (int32_t*)malloc((size_t)RMCV_CHESS_CAND_MAX * 12);
            int32_t st = -1, n = -1;
            if (chess_image_refusal(layout ? padded : packed, cor, w, h, layout ? pstride : 3 * w)) return 3;
            if (!layout) chess_find_host(packed, w, h, 3 * w, cols, rows, prm, (float*)cor, nullptr, nullptr, nullptr);   // (null outputs are allowed)
            chess_find_host(layout ? padded : packed, w, h, layout ? pstride : 3 * w, cols, rows, prm, (float*)cor, &st, cand, &n);
            fwrite(&st, 4, 1, out);
            fwrite(&n, 4, 1, out);
            fwrite(cand, 12, (size_t)n, out);
            fwrite(cor, 8, want, out);
            boards += (st & RMCV_CHESS_FOUND) != 0;
            free(cand);
            free(cor);
        }
        free(padded);
        free(packed);
    }
    fclose(in);
    fclose(out);
    printf("cases %d boards %ld\n", n_cases, boards);
    return 0;
}
