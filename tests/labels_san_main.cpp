// TEST-ONLY stand-alone program around the host-side view-label functions (rmcv_amd/csrc/rmcv_labels.hip compiled with RMCV_LABELS_HOST_ONLY:
// rmcv_format_f6, rmcv_label_text, rmcv_track_label_text, rmcv_view_glyph, rmcv_view_labels_host over rmcv_amd/csrc/device_text.h), for a
// sanitizer build (tests/test_view_labels_sanitized.py: -fsanitize=address,undefined; no GPU, nothing loaded into python).  Every list, view
// and string buffer is a heap block of exactly its size, so a read or write too far shows; every string is first asked for with a cap ONE
// SHORT of what it needs (refused, nothing written past the cap) and then with exactly enough.
//   labels_san_main IN OUT
// IN : int32 vw, vh, w, h; int32 n_f6; double[n_f6]; int32 n_jobs, then per job: int32 stride, scale, n_armours, has_ids, has_pos, n_tracks,
//      x_eff, y_eff; uint8 view[stride (vh - 1) + 3 vw]; rmcv_armour[n_armours]; int32 ids[has_ids ? n_armours : 0];
//      double pos[has_pos ? 3 n_armours : 0]; rmcv_track[n_tracks]; float side[n_tracks][8]
// OUT: per job the view's bytes.  stdout: one line per f6 value, per glyph code 0 .. 255, and per armour and track of every job.
#define RMCV_LABELS_HOST_ONLY
#include <cstdio>
#include <cstdlib>

#include "../rmcv_amd/csrc/rmcv_labels.hip"

template <typename T> static T* block(size_t n) { return n ? static_cast<T*>(std::malloc(n * sizeof(T))) : nullptr; }
template <typename T> static void get(std::FILE* f, T* p, size_t n) { if (n && std::fread(p, sizeof(T), n, f) != n) { std::fprintf(stderr, "short input\n"); std::exit(2); } }

// the string of `call(out, cap)`: refused one short, then into a block of exactly its length + 1
template <typename Call> static void print_line(Call call)
{
    char probe[RMCV_LABEL_MAX_CHARS + 1];
    const int n = call(probe, (int)sizeof(probe));
    if (n < 0) std::exit(5);
    char* tight = block<char>((size_t)n + 1);
    if (n > 0) {
        char* shorter = block<char>((size_t)n);
        if (call(shorter, n) != RMCV_ERR_CAPACITY) std::exit(6);
        std::free(shorter);
    }
    if (call(tight, n + 1) != n) std::exit(7);
    std::printf("%s\n", tight);
    std::free(tight);
}

int main(int argc, char** argv)
{
    if (argc != 3) return 1;
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 1;
    int32_t dim[4], n_f6 = 0, jobs = 0;
    get(in, dim, 4);
    const int vw = dim[0], vh = dim[1], w = dim[2], h = dim[3];
    get(in, &n_f6, 1);
    double* vals = block<double>(n_f6);
    get(in, vals, n_f6);
    for (int i = 0; i < n_f6; i++) print_line([&](char* o, int cap) { return rmcv_format_f6(vals[i], o, cap); });
    std::free(vals);
    for (int ch = 0; ch < 256; ch++) {
        uint8_t* rows = block<uint8_t>(7);
        if (rmcv_view_glyph(ch, rows) == RMCV_OK) std::printf("%d %d %d %d %d %d %d %d\n", ch, rows[0], rows[1], rows[2], rows[3], rows[4], rows[5], rows[6]);
        std::free(rows);
    }
    get(in, &jobs, 1);
    for (int32_t k = 0; k < jobs; k++) {
        int32_t hd[8];
        get(in, hd, 8);
        const int stride = hd[0], scale = hd[1], na = hd[2], has_ids = hd[3], has_pos = hd[4], nt = hd[5], x_eff = hd[6], y_eff = hd[7];
        const size_t bytes = (size_t)stride * (vh - 1) + (size_t)3 * vw; // the last row ends with its last pixel
        uint8_t* view = block<uint8_t>(bytes);
        rmcv_armour* armours = block<rmcv_armour>(na);
        int32_t* ids = block<int32_t>(has_ids ? na : 0);
        double* pos = block<double>(has_pos ? (size_t)3 * na : 0);
        rmcv_track* tracks = block<rmcv_track>(nt);
        float* side = block<float>((size_t)8 * nt);
        get(in, view, bytes);
        get(in, armours, na);
        get(in, ids, has_ids ? na : 0);
        get(in, pos, has_pos ? (size_t)3 * na : 0);
        get(in, tracks, nt);
        get(in, side, (size_t)8 * nt);
        for (int i = 0; i < na; i++) print_line([&](char* o, int cap) { return rmcv_label_text(ids ? ids[i] : -1, pos ? pos + 3 * i : nullptr, o, cap); });
        for (int t = 0; t < nt; t++) print_line([&](char* o, int cap) { return rmcv_track_label_text(tracks + t, o, cap); });
        if (rmcv_view_labels_host(view, vw, vh, stride, w, h, scale, armours, ids, pos, na, tracks, side, nt, x_eff, y_eff) != RMCV_OK) return 4;
        if (std::fwrite(view, 1, bytes, out) != bytes) return 3;
        std::free(view); std::free(armours); std::free(ids); std::free(pos); std::free(tracks); std::free(side);
    }
    std::fclose(in);
    return std::fclose(out) == 0 ? 0 : 3;
}
