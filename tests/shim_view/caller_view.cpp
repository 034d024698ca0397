// TEST-ONLY caller of the link test for the operator's view: sees declarations only (never the shim).  Four synthetic frames go through a
// batch context of its own (the C-ABI's three calls), then rm::debug::device_view hands frame 1's debug image over as a cv::Mat, once at
// the default size and once at the size given.  Prints what the test compares with the library's own view of the same batch.
//   shim_view_main W H VW VH
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "view_contract.hpp"

static unsigned long long fnv(const cv::Mat& m)
{
    unsigned long long h = 1469598103934665603ull;
    for (int y = 0; y < m.rows; y++)
        for (size_t i = 0; i < (size_t)m.cols * 3; i++) h = (h ^ m.data[(size_t)y * m.step + i]) * 1099511628211ull;
    return h;
}

int main(int argc, char** argv)
{
    if (argc != 5) return 1;
    const int w = atoi(argv[1]), h = atoi(argv[2]), vw = atoi(argv[3]), vh = atoi(argv[4]), n = 4;
    std::vector<unsigned char> frames((size_t)n * 3 * w * h);
    for (int f = 0; f < n; f++)
        if (rmcv_synth_frame(&frames[(size_t)f * 3 * w * h], w, h, 3 * w, (uint64_t)(3 + f), 1, 0)) return 2;
    rmcv_limits lim;
    rmcv_default_limits(&lim);
    lim.max_frames = n;
    rmcv_ctx* ctx = nullptr;
    if (rmcv_ctx_create(0, &lim, &ctx)) return 3;
    rmcv_params p;
    rmcv_default_params(&p);
    p.tilt_max = 10.0f;
    if (rmcv_batch_upload(ctx, frames.data(), n, w, h, 3 * w, (int64_t)3 * w * h) || rmcv_batch_run(ctx, &p, RMCV_STAGE_ALL, nullptr)) return 4;
    const cv::Mat large = rm::debug::device_view(ctx, 1);
    const cv::Mat view = rm::debug::device_view(ctx, 1, cv::Size(vw, vh));
    std::printf("default %d %d %016llx view %d %d %016llx\n", large.cols, large.rows, fnv(large), view.cols, view.rows, fnv(view));
    int refused = 0;
    try { rm::debug::device_view(ctx, n); } catch (const std::exception&) { refused++; }
    try { rm::debug::device_view(ctx, 0, cv::Size(0, 4)); } catch (const std::exception&) { refused++; }
    std::printf("refused %d\n", refused);
    rmcv_ctx_destroy(ctx);
    return 0;
}
