// icon_strip_san_main.cpp -- rmcv_amd/csrc/icon_host.h (rm::affine_correction at any output size, the icon strip, the labeler's sheet) as a
// stand-alone program for AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_icon_strip_sanitized.py).  Every image, list and output
// is a heap block of exactly its size -- images alternately with rows of exactly 3 w bytes and with padded rows whose last one ends with its
// pixels -- so a read or a write one byte outside shows.  Input (little endian int32 unless said): w h | the image, 3 w h bytes | the binary, w h
// bytes | n_icons | per icon: 8 float32, ow, oh | n_strips | per strip: n, side, cap, n armours as 8 float32 each | n_sheets | per sheet: n, vw, vh,
// side, flags, n armours as 16 float32 each (vertices, icon).  Output: per icon the clamped icon (32 bytes), degenerate (int32), the picture
// (3 ow oh bytes); per strip and per sheet its bytes, rows packed.
#include <stdio.h>
#include <stdlib.h>

#include "../rmcv_amd/csrc/icon_host.h"

static FILE *fin, *fout;

static int32_t get_i32()
{
    int32_t v = 0;
    if (fread(&v, 4, 1, fin) != 1) exit(2);
    return v;
}
static void get(void* p, size_t n)
{
    if (n && fread(p, 1, n, fin) != n) exit(2);
}
static void put(const void* p, size_t n)
{
    if (n && fwrite(p, 1, n, fout) != n) exit(3);
}

// a heap copy of the packed image with rows `stride` apart, of exactly stride (h - 1) + 3 w bytes
static uint8_t* image_block(const uint8_t* packed, int w, int h, int stride)
{
    uint8_t* b = (uint8_t*)malloc((size_t)stride * (h - 1) + (size_t)3 * w);
    for (int y = 0; y < h; y++) memcpy(b + (size_t)y * stride, packed + (size_t)3 * w * y, (size_t)3 * w);
    return b;
}

int main(int argc, char** argv)
{
    if (argc != 3) return 1;
    fin = fopen(argv[1], "rb");
    fout = fopen(argv[2], "wb");
    if (!fin || !fout) return 1;
    const int w = get_i32(), h = get_i32();
    uint8_t* packed = (uint8_t*)malloc((size_t)3 * w * h);
    uint8_t* binary = (uint8_t*)malloc((size_t)w * h);
    get(packed, (size_t)3 * w * h);
    get(binary, (size_t)w * h);
    const int strides[3] = {3 * w, 3 * w + 5, 3 * w + 64};
    uint8_t* images[3];
    for (int k = 0; k < 3; k++) images[k] = image_block(packed, w, h, strides[k]);
    int degenerate = 0;
    const int n_icons = get_i32();
    for (int i = 0; i < n_icons; i++) {
        float(*icon)[2] = (float(*)[2])malloc(32);
        get(icon, 32);
        const int ow = get_i32(), oh = get_i32(), out_stride = 3 * ow + (i % 2) * 7;
        uint8_t* out = (uint8_t*)malloc((size_t)out_stride * (oh - 1) + (size_t)3 * ow);
        const int32_t deg = rmcv::icon_affine_host(images[i % 3], w, h, strides[i % 3], icon, ow, oh, out, out_stride);
        degenerate += deg;
        put(icon, 32);
        put(&deg, 4);
        for (int y = 0; y < oh; y++) put(out + (size_t)y * out_stride, (size_t)3 * ow);
        free(out);
        free(icon);
    }
    const int n_strips = get_i32();
    for (int i = 0; i < n_strips; i++) {
        const int n = get_i32(), side = get_i32(), cap = get_i32(), out_stride = 3 * cap * side + (i % 2) * 3;
        rmcv_armour* arm = (rmcv_armour*)calloc(n ? n : 1, sizeof(rmcv_armour));
        for (int j = 0; j < n; j++) get(arm[j].icon, 32);
        uint8_t* out = (uint8_t*)malloc((size_t)out_stride * (side - 1) + (size_t)3 * cap * side);
        const int na = rmcv::icon_strip_host(images[i % 3], w, h, strides[i % 3], n ? arm : nullptr, n, side, cap, cap * side, out, out_stride);
        if (na != (n < cap ? n : cap)) return 4;
        for (int y = 0; y < side; y++) put(out + (size_t)y * out_stride, (size_t)3 * cap * side);
        free(out);
        free(arm);
    }
    const int n_sheets = get_i32();
    for (int i = 0; i < n_sheets; i++) {
        const int n = get_i32(), vw = get_i32(), vh = get_i32(), side = get_i32(), flags = get_i32(), out_stride = 6 * vw + (i % 2) * 2;
        rmcv_armour* arm = (rmcv_armour*)calloc(n ? n : 1, sizeof(rmcv_armour));
        for (int j = 0; j < n; j++) {
            get(arm[j].vertices, 32);
            get(arm[j].icon, 32);
        }
        uint8_t* out = (uint8_t*)malloc((size_t)out_stride * (vh + side - 1) + (size_t)6 * vw);
        rmcv::labeler_sheet_host(images[i % 3], w, h, strides[i % 3], binary, w, nullptr, 0, nullptr, nullptr, 0, n ? arm : nullptr, n, vw, vh, side,
                                 RMCV_ICON_STRIP_CAP_MAX, flags, out, out_stride);
        for (int y = 0; y < vh + side; y++) put(out + (size_t)y * out_stride, (size_t)6 * vw);
        free(out);
        free(arm);
    }
    printf("icons %d degenerate %d strips %d sheets %d\n", n_icons, degenerate, n_strips, n_sheets);
    for (int k = 0; k < 3; k++) free(images[k]);
    free(binary);
    free(packed);
    fclose(fin);
    return fclose(fout) ? 3 : 0;
}
