// TEST-ONLY caller of the link test for the exposure helpers: sees declarations only (never the shim).  One synthetic frame as an
// under-exposed camera delivers it, (v * num) >> 8, goes through rm::AutoEnhance and the three detection calls of the reference's
// process loop (executable/main.cpp:172-176), as a host does today; then the untouched dimmed frame goes through the fused
// rm::extract_color_enhanced, which must give the same contours and byte image; rm::CalcGamma runs out of place and in place.
#include <cstdio>
#include <cstring>

#include "enhance_contract.hpp"
#include "rmcv_abi.h" // rmcv_synth_frame only (test input)

static unsigned long long fnv(const unsigned char* p, size_t n)
{
    unsigned long long h = 0; // a position-weighted byte sum, modulo 2^64 (the test recomputes it with numpy)
    for (size_t i = 0; i < n; i++) h += (unsigned long long)(p[i] + 1) * ((unsigned long long)i * 0x9E3779B97F4A7C15ull + 1ull);
    return h;
}

int main(int argc, char** argv)
{
    const int w = 1280, h = 1024, index = argc > 1 ? atoi(argv[1]) : 0, num = argc > 2 ? atoi(argv[2]) : 80;
    cv::Mat frame(h, w, CV_8UC3);
    if (rmcv_synth_frame(frame.data, w, h, 3 * w, (uint64_t)index, 1, 0)) return 2;
    for (size_t i = 0; i < (size_t)3 * w * h; i++) frame.data[i] = (unsigned char)((frame.data[i] * num) >> 8);
    cv::Mat dimmed = frame; // (a copy: the stand-in's matrices own their bytes)
    rm::AutoEnhance(frame); // default gains
    std::printf("enhanced %llx\n", fnv(frame.data, (size_t)3 * w * h));
    auto [contours, binary] = rm::extract_color(frame, rm::CAMP_BLUE, 80);
    auto [positive, negative] = rm::filter_lightblobs(contours, 70, {1.5f, 80.0f}, {10, 99999}, rm::CAMP_BLUE);
    auto armours = rm::filter_armours(positive, 12, 22, 0.4f, rm::CAMP_BLUE);
    size_t on = 0, points = 0;
    for (size_t i = 0; i < (size_t)w * h; i++) on += binary.data[i] != 0;
    for (auto& c : contours) points += c.size();
    std::printf("contours %zu points %zu binary_on %zu positive %zu negative %zu armours %zu\n", contours.size(), points, on, positive.size(),
                negative.size(), armours.size());
    for (auto& a : armours) {
        std::printf("armour");
        for (int i = 0; i < 4; i++) std::printf(" %a %a", a.vertices[i].x, a.vertices[i].y);
        std::printf("\n");
    }
    // the fused call on the frame as delivered
    auto [contours2, binary2] = rm::extract_color_enhanced(dimmed, rm::CAMP_BLUE, 80);
    bool same = contours2.size() == contours.size() && !std::memcmp(binary.data, binary2.data, (size_t)w * h);
    for (size_t i = 0; same && i < contours.size(); i++) {
        same = contours[i].size() == contours2[i].size();
        for (size_t k = 0; same && k < contours[i].size(); k++) same = contours[i][k].x == contours2[i][k].x && contours[i][k].y == contours2[i][k].y;
    }
    // ... after which rm::extract_color reads frames as they are again
    auto [contours3, binary3] = rm::extract_color(dimmed, rm::CAMP_BLUE, 80);
    std::printf("fused_same %d plain_contours %zu\n", same ? 1 : 0, contours3.size());
    // rm::CalcGamma: out of place with an explicit gamma, in place with the default one (0.5)
    cv::Mat out;
    rm::CalcGamma(dimmed, out, 2.2f);
    std::printf("gamma22 %llx\n", fnv(out.data, (size_t)3 * w * h));
    rm::CalcGamma(dimmed, dimmed);
    std::printf("gamma05 %llx\n", fnv(dimmed.data, (size_t)3 * w * h));
    return 0;
}
