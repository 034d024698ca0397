// TEST-ONLY stand-alone program around the host path of the source view (rmcv_amd/csrc/device_view.h: source_view_host; the refusals of
// rmcv_amd/csrc/source_view_plan.h), for a sanitizer build (tests/test_source_view_sanitized.py: -fsanitize=address,undefined; no GPU, nothing
// loaded into python).  Every list and the image are heap blocks of exactly their size, so a read too far shows.
//   source_view_san_main IN OUT
// IN : int32 n_jobs, then per job: int32 w, h, stride, n_blobs, n_neg, n_pts, n_armours, flags, vw, vh; uint8 bgr[h - 1][stride] + [3 w];
//      rmcv_lightblob[n_blobs]; int32 neg_offs[n_neg + 1]; rmcv_point[n_pts]; rmcv_armour[n_armours]
// OUT: per job: uint8 view[vh][vw][3]
#include <cstdio>
#include <cstdlib>

#include "../rmcv_amd/csrc/device_view.h"
#include "../rmcv_amd/csrc/source_view_plan.h"

template <typename T> static T* block(size_t n) { return n ? static_cast<T*>(std::malloc(n * sizeof(T))) : nullptr; }
template <typename T> static void get(std::FILE* f, T* p, size_t n) { if (n && std::fread(p, sizeof(T), n, f) != n) { std::fprintf(stderr, "short input\n"); std::exit(2); } }

int main(int argc, char** argv)
{
    if (argc != 3) return 1;
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 1;
    int32_t jobs = 0;
    get(in, &jobs, 1);
    for (int32_t k = 0; k < jobs; k++) {
        int32_t hd[10];
        get(in, hd, 10);
        const int w = hd[0], h = hd[1], stride = hd[2], nb = hd[3], nn = hd[4], np = hd[5], na = hd[6], flags = hd[7], vw = hd[8], vh = hd[9];
        const size_t img = (size_t)stride * (h - 1) + (size_t)3 * w; // the last row ends with its last pixel
        uint8_t* bgr = block<uint8_t>(img);
        rmcv_lightblob* blobs = block<rmcv_lightblob>(nb);
        int32_t* offs = block<int32_t>((size_t)nn + 1);
        rmcv_point* pts = block<rmcv_point>(np);
        rmcv_armour* armours = block<rmcv_armour>(na);
        uint8_t* view = block<uint8_t>((size_t)3 * vw * vh);
        get(in, bgr, img);
        get(in, blobs, nb);
        get(in, offs, (size_t)nn + 1);
        get(in, pts, np);
        get(in, armours, na);
        if (rmcv::source_image_refusal(bgr, view, w, h, stride)) return 4;
        if (view_check_lists(w, h, w, blobs, nb, pts, offs, nn, armours, na, flags, vw, vh, 3 * vw)) return 4;
        source_view_host(bgr, w, h, stride, blobs, nb, pts, offs, nn, armours, na, flags, vw, vh, view, 3 * vw);
        if (std::fwrite(view, 1, (size_t)3 * vw * vh, out) != (size_t)3 * vw * vh) return 3;
        std::free(bgr); std::free(blobs); std::free(offs); std::free(pts); std::free(armours); std::free(view);
    }
    std::fclose(in);
    return std::fclose(out) == 0 ? 0 : 3;
}
