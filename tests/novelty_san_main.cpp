// novelty_san_main.cpp -- the host path of rmcv_amd/csrc/device_novelty.h as a stand-alone program (tests/test_novelty_sanitized.py builds it
// with -fsanitize=address,undefined).  Every table is a heap block of exactly its size: a read or write one byte beyond a row, a ring or a
// keep table is the sanitizer's to find.
//
//   in : int32 n_calls, then per call  int32 n_streams, ring_rows, max_sad, total; int32 n_rows[n_streams], labels[n_streams];
//        u8 rows[total][1200], rings[n_streams][ring_rows][1200]; int64 pushed[n_streams]
//   out: per call  u8 keep[total]; int32 min_sad[total]; int64 near; u8 rings[n_streams][ring_rows][1200]; int64 pushed[n_streams];
//        int32 sad_first_two (icon_sad of the call's first two rows, -1 with fewer)
#include <stdio.h>
#include <stdlib.h>

#include "../rmcv_amd/csrc/device_novelty.h"

using namespace rmcv;

template <class T>
static T* block(FILE* f, size_t n)
{
    T* p = static_cast<T*>(malloc(n * sizeof(T))); // (malloc(0) may be null: such a table is never read)
    if (n && (!p || fread(p, sizeof(T), n, f) != n)) exit(3);
    return p;
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t n_calls = 0;
    if (fread(&n_calls, 4, 1, in) != 1) return 3;
    for (int c = 0; c < n_calls; c++) {
        int32_t h[4];
        if (fread(h, 4, 4, in) != 4) return 3;
        const int n_streams = h[0], R = h[1];
        const int32_t T = h[2];
        const size_t total = (size_t)h[3], ring_bytes = (size_t)n_streams * R * NOVEL_ROW;
        if (novelty_refusal(R, T)) return 4;
        int32_t* n_rows = block<int32_t>(in, (size_t)n_streams);
        int32_t* labels = block<int32_t>(in, (size_t)n_streams);
        uint8_t* rows = block<uint8_t>(in, total * NOVEL_ROW);
        uint8_t* rings = block<uint8_t>(in, ring_bytes);
        int64_t* pushed = block<int64_t>(in, (size_t)n_streams);
        uint8_t* keep = static_cast<uint8_t*>(malloc(total));
        int32_t* min_sad = static_cast<int32_t*>(malloc(total * sizeof(int32_t)));
        const int64_t near = novelty_seq(rows, n_rows, labels, n_streams, R, T, rings, pushed, keep, min_sad);
        const int32_t first_two = total >= 2 ? icon_sad(rows, rows + NOVEL_ROW) : -1;
        if (total) fwrite(keep, 1, total, out), fwrite(min_sad, 4, total, out);
        fwrite(&near, 8, 1, out);
        if (ring_bytes) fwrite(rings, 1, ring_bytes, out);
        if (n_streams) fwrite(pushed, 8, (size_t)n_streams, out);
        fwrite(&first_two, 4, 1, out);
        free(min_sad), free(keep), free(pushed), free(rings), free(rows), free(labels), free(n_rows);
    }
    fclose(in);
    return fclose(out) ? 5 : 0;
}
