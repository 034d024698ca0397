// TEST-ONLY caller of the link test for tracked-ROI detection: sees declarations only (never the shim).  The reference's locked-target
// step on one synthetic frame: detect on the whole frame, rm::utils::GetROI around the first armour (scale 2), then
// rm::extract_color(image(roi)) -> rm::filter_lightblobs -> rm::filter_armours on the sub-view and rm::solve_PnP(..., roi), which puts the
// ROI's corner back.  Prints what the test compares with the library's own windowed run and with the CPU oracle on the crop.
#include <cstdio>

#include "window_contract.hpp"
#include "rmcv_abi.h" // rmcv_synth_frame and rmcv_default_pnp_config only (test input)

// image(roi) of OpenCV: a view of the frame's bytes -- the ROI's size, the FRAME's step (the stand-in's cv::Mat has no operator())
static cv::Mat sub_view(cv::Mat& image, const cv::Rect& roi)
{
    cv::Mat view(roi.height, roi.width, CV_8UC3, image.data + (size_t)roi.y * image.step + 3 * (size_t)roi.x);
    view.step = image.step;
    return view;
}

int main(int argc, char** argv)
{
    const int w = 1280, h = 1024, index = argc > 1 ? atoi(argv[1]) : 0;
    cv::Mat frame(h, w, CV_8UC3);
    if (rmcv_synth_frame(frame.data, w, h, 3 * w, (uint64_t)index, 1, 0)) return 2;
    auto [contours, binary] = rm::extract_color(frame, rm::CAMP_BLUE, 80);
    auto [positive, negative] = rm::filter_lightblobs(contours, 70, {1.5f, 80.0f}, {10, 99999}, rm::CAMP_BLUE);
    auto armours = rm::filter_armours(positive, 12, 22, 0.4f, rm::CAMP_BLUE);
    if (armours.empty()) return 3;
    const cv::Rect same = rm::utils::GetROI(armours[0].vertices, 4, 1.0f); // the default frame size {-1, -1} (with BOTH defaults the reference's two overloads are ambiguous)
    const cv::Rect tight = rm::utils::GetROI(armours[0].vertices, 4, 1.0f, cv::Size(w, h));
    const cv::Rect roi = rm::utils::GetROI(armours[0].vertices, 4, cv::Size2f(2.0f, 2.0f), cv::Size(w, h));
    std::printf("default %d %d %d %d tight %d %d %d %d roi %d %d %d %d\n", same.x, same.y, same.width, same.height, tight.x, tight.y, tight.width,
                tight.height, roi.x, roi.y, roi.width, roi.height);
    if (roi.width < 1 || roi.height < 1) return 4;
    cv::Mat view = sub_view(frame, roi);
    auto [contours2, binary2] = rm::extract_color(view, rm::CAMP_BLUE, 80);
    auto [positive2, negative2] = rm::filter_lightblobs(contours2, 70, {1.5f, 80.0f}, {10, 99999}, rm::CAMP_BLUE);
    auto armours2 = rm::filter_armours(positive2, 12, 22, 0.4f, rm::CAMP_BLUE);
    size_t on = 0, points = 0;
    for (size_t i = 0; i < (size_t)roi.width * roi.height; i++) on += binary2.data[i] != 0;
    for (auto& c : contours2) points += c.size();
    std::printf("contours %zu points %zu binary_on %zu positive %zu armours %zu\n", contours2.size(), points, on, positive2.size(), armours2.size());
    rmcv_pnp_config cfg; // the camera of executable/main.cpp:7-13, 184 (test input: the values the oracle's default configuration holds too)
    rmcv_default_pnp_config(&cfg);
    cv::Mat cammat(3, 3, CV_64F), discof(1, 5, CV_64F);
    for (int i = 0; i < 9; i++) cammat.ptr<double>()[i] = cfg.camera_matrix[i];
    for (int i = 0; i < 5; i++) discof.ptr<double>()[i] = cfg.dist[i];
    for (auto& a : armours2) {
        std::printf("armour");
        for (int i = 0; i < 4; i++) std::printf(" %a %a", a.vertices[i].x, a.vertices[i].y);
        auto [rvec, tvec] = rm::solve_PnP(a.vertices, cammat, discof, cv::Size2f(cfg.square_w, cfg.square_h), roi);
        for (int i = 0; i < 3; i++) std::printf(" %a", rvec.ptr<double>()[i]);
        for (int i = 0; i < 3; i++) std::printf(" %a", tvec.ptr<double>()[i]);
        std::printf("\n");
    }
    return 0;
}
