// rmcv_shim.hpp -- the reference's own rm:: signatures re-hosted on the C-ABI (include/rmcv_abi.h).
//
// Drop-in for the three functions executable/main.cpp:172-176 calls:
//   rm::extract_color      include/imgproc.h:29       (body: src/imgproc.cpp:50-75)
//   rm::filter_lightblobs  include/objdetect.h:47-49  (body: src/objdetect.cpp:55-87)
//   rm::filter_armours     include/objdetect.h:70-71  (body: src/objdetect.cpp:114-166)
//
// Usage: compile this header into EXACTLY ONE translation unit of librmcv in place of
// those bodies, after including the reference's own "core.h" (it supplies rm::camp, rm::range,
// rm::contour, rm::lightblob, rm::armour and the cv:: types), and link librmcv_hip.so.
// The seven rm:: functions below are DEFINITIONS WITH EXTERNAL LINKAGE (they are what executable/main.cpp's
// undefined references resolve to, executable/CMakeLists.txt:1-2): including this header in two translation
// units of one program is an ODR violation by design, exactly as compiling src/objdetect.cpp twice would be.
// A header-only use (caller and shim in one TU) may define RMCV_SHIM_LINKAGE=inline before including it.
// Default arguments stay on the reference's declarations (include/objdetect.h:22-37, include/mobility.h:106-108).
// Also the legacy matcher rm::MatchLightBlob / rm::FindLightBlobs / rm::LightBlobOverlap (include/objdetect.h:22-37, 62)
// and rm::solve_PnP (include/mobility.h:106-108).
// One addition the reference does not have: rm::extract_color_bayer, rm::extract_color on a raw 8-bit Bayer mosaic (CV_8UC1), and
// rm::extract_color_raw, the same on the sensor's buffer as delivered (8- or 16-bit samples, to be mirrored and / or flipped).
// rm::CalcGamma and rm::AutoEnhance (include/imgproc.h:23, 35) are here too, and one more addition: rm::extract_color_enhanced, the two
// of rm::AutoEnhance + rm::extract_color fused (the enhanced frame is never written).
// rm::affine_correction (include/imgproc.h:17), the icon executable/main.cpp:180 rectifies per armour, at any output size up to 256 x 256.
// rm::utils::GetROI (include/core.h:142-147), the reference's tracked-ROI helper, is here as well (where the cv:: headers know cv::Size).
// rm::ProjectileAngle / SolveGEA / DeltaHeight / Distance (include/mobility.h) too, behind the reference's mobility.h.
// One more addition: rm::debug::device_view, the loop's debug image of a batch frame rendered on the device (where the cv:: headers know cv::Size).
// rm::debug::logger (include/debug.h:13-29) too, behind the reference's debug.h: the frames go into a session file, not into an AVI.
// The legacy names of the north star are aliased at the bottom (docs/core_8h_source.html:101,114).
//
// Every signature mentions cv:: types, so this header only compiles where OpenCV headers exist.
#pragma once
#if __has_include(<opencv2/opencv.hpp>)

#include <cmath>
#include <cstdlib>
#include <filesystem>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include "rmcv_abi.h"

#ifndef RMCV_CORE_H
#error "include the reference's core.h before rmcv_shim.hpp"
#endif

#ifndef RMCV_SHIM_LINKAGE
#define RMCV_SHIM_LINKAGE /* external: the backend TU emits rm::extract_color & co. whether or not it calls them */
#endif

namespace rm {
namespace hip_detail {

// one context per calling thread (the reference runs detection on a single process_thread,
// executable/main.cpp:55); created on first use on device RMCV_DEVICE (default 0)
inline rmcv_ctx* ctx()
{
    static thread_local rmcv_ctx* c = [] {
        rmcv_ctx* p = nullptr;
        rmcv_limits lim;
        rmcv_default_limits(&lim);
        lim.max_frames = 1;
        const char* dev = std::getenv("RMCV_DEVICE");
        const int rc = rmcv_ctx_create(dev ? std::atoi(dev) : 0, &lim, &p);
        if (rc != RMCV_OK) throw std::runtime_error("rmcv: no usable MI355X device (this build has no CPU path)");
        return p;
    }();
    return c;
}

inline void check(int rc)
{ // the reference would let a cv::Exception escape (no try/catch in main.cpp); keep that shape
    if (rc != RMCV_OK) throw std::runtime_error(std::string("rmcv: ") + rmcv_last_error(ctx()));
}

inline lightblob to_lightblob(const rmcv_lightblob& b)
{
    lightblob out(cv::RotatedRect(cv::Point2f(b.center[0], b.center[1]), cv::Size2f(b.size[0], b.size[1]), 0.f),
                  static_cast<camp>(b.target));
    out.angle = b.angle;
    out.target = static_cast<camp>(b.target);
    out.center = {b.center[0], b.center[1]};
    for (int i = 0; i < 4; i++) out.vertices[i] = {b.vertices[i][0], b.vertices[i][1]};
    out.size = {b.size[0], b.size[1]};
    return out;
}

inline rmcv_lightblob from_lightblob(const lightblob& b)
{
    rmcv_lightblob o{};
    o.angle = b.angle;
    o.target = static_cast<int32_t>(b.target);
    o.center[0] = b.center.x;
    o.center[1] = b.center.y;
    for (int i = 0; i < 4; i++) { o.vertices[i][0] = b.vertices[i].x; o.vertices[i][1] = b.vertices[i].y; }
    o.size[0] = b.size.width;
    o.size[1] = b.size.height;
    return o;
}

} // namespace hip_detail

namespace hip_detail {
// rm::extract_color's body for whatever the thread's context reads its frame as (RMCV_OPT_INPUT_FORMAT)
inline std::tuple<std::vector<contour>, cv::Mat> extract(const cv::Mat& img, camp target, int lower_bound)
{
    cv::Mat binary(img.rows, img.cols, CV_8UC1);
    static thread_local std::vector<rmcv_point> pts;
    static thread_local std::vector<int32_t> offs;
    rmcv_limits lim;
    rmcv_default_limits(&lim);
    pts.resize(lim.max_points);
    offs.resize(lim.max_contours + 1);
    int32_t nc = 0, np = 0;
    hip_detail::check(rmcv_extract_color(hip_detail::ctx(), img.data, img.cols, img.rows, (int)img.step, (int)target,
                                         lower_bound, RMCV_MORPH_CLOSE, binary.data, pts.data(), (int)pts.size(),
                                         offs.data(), (int)offs.size() - 1, &nc, &np));
    std::vector<contour> contours(nc);
    for (int i = 0; i < nc; i++) {
        contours[i].reserve(offs[i + 1] - offs[i]);
        for (int k = offs[i]; k < offs[i + 1]; k++) contours[i].emplace_back(pts[k].x, pts[k].y);
    }
    return {contours, binary};
}
} // namespace hip_detail

RMCV_SHIM_LINKAGE std::tuple<std::vector<contour>, cv::Mat> extract_color(cv::InputArray image, camp target, int lower_bound)
{
    cv::Mat img = image.getMat();
    CV_Assert(img.type() == CV_8UC3);
    return hip_detail::extract(img, target, lower_bound);
}

// Not a reference function: rm::extract_color on the camera's raw 8-bit Bayer mosaic (CV_8UC1), so that a camera host hands over
// the sensor's buffer instead of converting it on the CPU first.  `pattern` is RMCV_BAYER_RG .. RMCV_BAYER_BG (the
// Daheng SDK's DX_PIXEL_COLOR_FILTER values).  The results are rm::extract_color's on D(raw), the library's demosaic
// (include/rmcv_abi.h: RMCV_OPT_INPUT_FORMAT).  The thread's context reads mosaics for this call only: rm::extract_color is unchanged.
RMCV_SHIM_LINKAGE std::tuple<std::vector<contour>, cv::Mat> extract_color_bayer(cv::InputArray raw, int pattern, camp target, int lower_bound)
{
    cv::Mat img = raw.getMat();
    CV_Assert(img.type() == CV_8UC1);
    hip_detail::check(rmcv_ctx_set_option(hip_detail::ctx(), RMCV_OPT_INPUT_FORMAT, pattern));
    struct Restore { // back to BGR however the call ends
        ~Restore() { rmcv_ctx_set_option(hip_detail::ctx(), RMCV_OPT_INPUT_FORMAT, RMCV_INPUT_BGR); }
    } restore;
    return hip_detail::extract(img, target, lower_bound);
}

// The same on the buffer exactly as the sensor delivers it (frameData.pImgBuf of the reference's hardware/src/daheng.cpp): CV_8UC1, or
// CV_16UC1 for the 10/12-bit formats with the SDK's DX_VALID_BIT value (0 .. 4; ignored for CV_8UC1), plus the `mirror` / `flip`
// arguments of camera.capture().  `pattern` is the colour filter of the buffer as delivered; the results -- the binary image and the
// contour coordinates -- are those of the ORIENTED frame, as the reference's detection sees it (include/rmcv_abi.h:
// RMCV_OPT_INPUT_SAMPLE_BITS / _VALID_BIT / _ORIENT).  All four options are the thread's for this call only.
// (Guarded: only where the cv:: headers in use know 16-bit matrices.)
#ifdef CV_16UC1
RMCV_SHIM_LINKAGE std::tuple<std::vector<contour>, cv::Mat> extract_color_raw(cv::InputArray raw, int pattern, int valid_bit, bool mirror, bool flip,
                                                                              camp target, int lower_bound)
{
    cv::Mat img = raw.getMat();
    CV_Assert(img.type() == CV_8UC1 || img.type() == CV_16UC1);
    struct Restore { // back to 8-bit BGR as delivered however the call ends (a refused value below included)
        ~Restore()
        {
            rmcv_ctx_set_option(hip_detail::ctx(), RMCV_OPT_INPUT_FORMAT, RMCV_INPUT_BGR);
            rmcv_ctx_set_option(hip_detail::ctx(), RMCV_OPT_INPUT_SAMPLE_BITS, 8);
            rmcv_ctx_set_option(hip_detail::ctx(), RMCV_OPT_INPUT_VALID_BIT, 0);
            rmcv_ctx_set_option(hip_detail::ctx(), RMCV_OPT_INPUT_ORIENT, 0);
        }
    } restore;
    const bool wide = img.type() == CV_16UC1;
    hip_detail::check(rmcv_ctx_set_option(hip_detail::ctx(), RMCV_OPT_INPUT_FORMAT, pattern));
    hip_detail::check(rmcv_ctx_set_option(hip_detail::ctx(), RMCV_OPT_INPUT_SAMPLE_BITS, wide ? 16 : 8));
    hip_detail::check(rmcv_ctx_set_option(hip_detail::ctx(), RMCV_OPT_INPUT_VALID_BIT, wide ? valid_bit : 0));
    hip_detail::check(rmcv_ctx_set_option(hip_detail::ctx(), RMCV_OPT_INPUT_ORIENT, (mirror ? RMCV_ORIENT_MIRROR : 0) | (flip ? RMCV_ORIENT_FLIP : 0)));
    return hip_detail::extract(img, target, lower_bound);
}
#endif

// ---- rm::CalcGamma / rm::AutoEnhance (include/imgproc.h:23, 35; bodies src/imgproc.cpp:37-48, 77-98).  The default arguments
// (gamma = 0.5f; maxGainFactor = 100, minGainFactor = 50) live on the reference's declarations.  8-bit matrices of one or three
// channels (the table acts on bytes); `calibration` may be `source` itself, as rm::AutoEnhance calls it.
RMCV_SHIM_LINKAGE void CalcGamma(cv::Mat& source, cv::Mat& calibration, float gamma)
{
    CV_Assert(source.type() == CV_8UC1 || source.type() == CV_8UC3);
    if (calibration.data != source.data) calibration = cv::Mat(source.rows, source.cols, source.type());
    hip_detail::check(rmcv_calc_gamma(hip_detail::ctx(), source.data, source.cols * source.channels(), source.rows, (int)source.step, gamma,
                                      calibration.data, (int)calibration.step));
}

RMCV_SHIM_LINKAGE void AutoEnhance(cv::Mat& frame, float maxGainFactor, float minGainFactor)
{
    CV_Assert(frame.type() == CV_8UC3);
    hip_detail::check(rmcv_auto_enhance(hip_detail::ctx(), frame.data, frame.cols, frame.rows, (int)frame.step, maxGainFactor, minGainFactor,
                                        frame.data, (int)frame.step, nullptr));
}

// ---- rm::affine_correction (include/imgproc.h:17; body src/imgproc.cpp:9-35), what executable/main.cpp:180 calls per armour with {20, 20}
// and the labeler with {80, 80}: the vertices are clamped in place, the icon comes back as a new CV_8UC3 matrix of outSize (any size up to
// 256 x 256), zeros when the clamped quadrilateral's box is degenerate.  On the CPU (rmcv_affine_correction_host): no context, no device.
// (Guarded like rm::utils::GetROI below: only where the cv:: headers in use know cv::Size.)
#if defined(CV_VERSION) || defined(RMCV_CV_HAS_SIZE)
RMCV_SHIM_LINKAGE cv::Mat affine_correction(const cv::Mat& source, cv::Point2f vertices[4], const cv::Size outSize)
{
    CV_Assert(source.type() == CV_8UC3);
    float icon[4][2];
    for (int i = 0; i < 4; i++) icon[i][0] = vertices[i].x, icon[i][1] = vertices[i].y;
    cv::Mat out(outSize.height, outSize.width, CV_8UC3);
    if (rmcv_affine_correction_host(source.data, source.cols, source.rows, (int)source.step, icon, outSize.width, outSize.height, out.data, (int)out.step, nullptr) !=
        RMCV_OK)
        throw std::runtime_error("rmcv: rm::affine_correction needs an image of at least 1 x 1 and an outSize of 1 .. 256 x 1 .. 256");
    for (int i = 0; i < 4; i++) vertices[i].x = icon[i][0], vertices[i].y = icon[i][1];
    return out;
}
#endif

// Not a reference function: rm::AutoEnhance + rm::extract_color as ONE call -- the results are rm::extract_color's on the enhanced
// frame, which is never written (include/rmcv_abi.h: RMCV_OPT_ENHANCE): the host drops two full-frame CPU passes and `image` stays as
// the camera delivered it.  Option and gains are the thread's for this call only: rm::extract_color is unchanged.
RMCV_SHIM_LINKAGE std::tuple<std::vector<contour>, cv::Mat> extract_color_enhanced(cv::InputArray image, camp target, int lower_bound,
                                                                                   float maxGainFactor, float minGainFactor)
{
    cv::Mat img = image.getMat();
    CV_Assert(img.type() == CV_8UC3);
    struct Restore { // back to what the thread's context was set to, however the call ends
        int32_t on = 0;
        float max_gain = 100.0f, min_gain = 50.0f;
        Restore() { rmcv_ctx_get_enhance(hip_detail::ctx(), &on, &max_gain, &min_gain); }
        ~Restore()
        {
            rmcv_ctx_set_option(hip_detail::ctx(), RMCV_OPT_ENHANCE, on);
            rmcv_ctx_set_enhance_gains(hip_detail::ctx(), max_gain, min_gain);
        }
    } restore;
    hip_detail::check(rmcv_ctx_set_enhance_gains(hip_detail::ctx(), maxGainFactor, minGainFactor));
    hip_detail::check(rmcv_ctx_set_option(hip_detail::ctx(), RMCV_OPT_ENHANCE, 1));
    return hip_detail::extract(img, target, lower_bound);
}

RMCV_SHIM_LINKAGE auto filter_lightblobs(const std::vector<contour>& contours, const float tilt_max, const range<float> ratio_range,
                              const range<double> area_range, camp enemy)
    -> std::tuple<std::vector<lightblob>, std::vector<contour>>
{
    std::vector<rmcv_point> pts;
    std::vector<int32_t> offs(contours.size() + 1, 0);
    for (size_t i = 0; i < contours.size(); i++) {
        for (const auto& p : contours[i]) pts.push_back({p.x, p.y});
        offs[i + 1] = (int32_t)pts.size();
    }
    rmcv_limits lim;
    rmcv_default_limits(&lim);
    std::vector<rmcv_lightblob> blobs(lim.max_blobs);
    std::vector<int32_t> neg(contours.size() + 1);
    int32_t nb = 0, nn = 0;
    hip_detail::check(rmcv_filter_lightblobs(hip_detail::ctx(), pts.data(), offs.data(), (int)contours.size(), tilt_max,
                                             ratio_range.lower_bound, ratio_range.upper_bound, area_range.lower_bound,
                                             area_range.upper_bound, (int)enemy, blobs.data(), (int)blobs.size(), &nb, nullptr,
                                             neg.data(), &nn));
    std::vector<lightblob> positive;
    std::vector<contour> negative;
    positive.reserve(nb);
    for (int i = 0; i < nb; i++) positive.push_back(hip_detail::to_lightblob(blobs[i]));
    for (int i = 0; i < nn; i++) negative.push_back(contours[neg[i]]);
    return {positive, negative};
}

RMCV_SHIM_LINKAGE std::vector<armour> filter_armours(std::vector<lightblob>& lightblobs, const float angle_difference_max,
                                          const float shear_max, const float lenght_ratio_max, const camp enemy)
{
    std::vector<rmcv_lightblob> in;
    in.reserve(lightblobs.size());
    for (const auto& b : lightblobs) in.push_back(hip_detail::from_lightblob(b));
    rmcv_limits lim;
    rmcv_default_limits(&lim);
    std::vector<rmcv_armour> out(lim.max_armours);
    int32_t na = 0;
    hip_detail::check(rmcv_filter_armours(hip_detail::ctx(), in.data(), (int)in.size(), angle_difference_max, shear_max,
                                          lenght_ratio_max, (int)enemy, out.data(), (int)out.size(), &na));
    std::vector<armour> armours;
    armours.reserve(na);
    for (int k = 0; k < na; k++) {
        // rm::armour has one constructor, armour(std::vector<lightblob>) (include/core.h:117): handed anything but two light
        // blobs it returns right after allocating the per-target Kalman state (src/core.cpp:21-23) -- so an EMPTY list buys the
        // object (with its own filter matrices, as every reference armour has) without running the geometry of
        // src/core.cpp:25-48 on the CPU a second time; the device results are then stored into the public members.
        armour a{std::vector<lightblob>{}};
        for (int i = 0; i < 4; i++) {
            a.icon[i] = {out[k].icon[i][0], out[k].icon[i][1]};
            a.vertices[i] = {out[k].vertices[i][0], out[k].vertices[i][1]};
        }
        a.bounding_box = {out[k].bbox[0], out[k].bbox[1], out[k].bbox[2], out[k].bbox[3]};
        armours.push_back(a);
    }
    return armours;
}

// ---- legacy per-contour matcher (include/objdetect.h:22-37, 62; bodies src/objdetect.cpp:9-53, 89-112).  The default
// argument `fitEllipse = true` lives on the reference's declarations.
RMCV_SHIM_LINKAGE bool MatchLightBlob(const rm::contour& contour, float minRatio, float maxRatio, float tiltAngle, float minArea,
                           float maxArea, cv::RotatedRect& lightBlobBox, bool fitEllipse)
{
    std::vector<rmcv_point> pts;
    pts.reserve(contour.size());
    for (const auto& p : contour) pts.push_back({p.x, p.y});
    const rmcv_legacy_params lp = {minRatio, maxRatio, tiltAngle, minArea, maxArea, fitEllipse ? 1 : 0};
    rmcv_rrect box{};
    int32_t matched = 0;
    hip_detail::check(rmcv_match_lightblob(hip_detail::ctx(), pts.data(), (int)pts.size(), &lp, &box, &matched));
    if (!matched) return false;
    lightBlobBox = cv::RotatedRect(cv::Point2f(box.cx, box.cy), cv::Size2f(box.w, box.h), box.angle);
    return true;
}

RMCV_SHIM_LINKAGE void FindLightBlobs(std::vector<contour>& contours, std::vector<lightblob>& lightBlobs, float minRatio, float maxRatio,
                           float tiltAngle, float minArea, float maxArea, const cv::Mat& source, bool fitEllipse)
{
    lightBlobs.clear();
    if (source.channels() != 3) return; // src/objdetect.cpp:35
    std::vector<rmcv_point> pts;
    std::vector<int32_t> offs(contours.size() + 1, 0);
    for (size_t i = 0; i < contours.size(); i++) {
        for (const auto& p : contours[i]) pts.push_back({p.x, p.y});
        offs[i + 1] = (int32_t)pts.size();
    }
    const rmcv_legacy_params lp = {minRatio, maxRatio, tiltAngle, minArea, maxArea, fitEllipse ? 1 : 0};
    std::vector<rmcv_lightblob> blobs(contours.size() + 1);
    int32_t nb = 0;
    hip_detail::check(rmcv_find_lightblobs(hip_detail::ctx(), source.data, source.cols, source.rows, (int)source.step, pts.data(),
                                           offs.data(), (int)contours.size(), &lp, blobs.data(), (int)blobs.size(), &nb, nullptr,
                                           nullptr));
    lightBlobs.reserve(nb);
    for (int i = 0; i < nb; i++) lightBlobs.push_back(hip_detail::to_lightblob(blobs[i]));
}

RMCV_SHIM_LINKAGE bool LightBlobOverlap(const std::vector<rm::lightblob>& lightBlobs, int leftIndex, int rightIndex)
{
    std::vector<rmcv_lightblob> in;
    in.reserve(lightBlobs.size());
    for (const auto& b : lightBlobs) in.push_back(hip_detail::from_lightblob(b));
    int32_t overlap = 0;
    if (rmcv_lightblob_overlap(in.data(), (int)in.size(), leftIndex, rightIndex, &overlap) != RMCV_OK)
        throw std::out_of_range("rm::LightBlobOverlap: rightIndex == lightBlobs.size() (the reference reads past the end here)");
    return overlap != 0;
}

// ---- armour pose (include/mobility.h:106-108; body src/mobility.cpp:166-190).  The default argument ROI = {0,0,0,0} lives on
// the reference's declaration.  cameraMatrix: 3x3 CV_64F, distortionFactor: 1x5 (or 5x1) CV_64F, as executable/main.cpp:7-13.
RMCV_SHIM_LINKAGE std::tuple<cv::Mat, cv::Mat> solve_PnP(const cv::Point2f points_image[4], cv::InputArray cameraMatrix,
                                              cv::InputArray distortionFactor, const cv::Size2f& exactSize, const cv::Rect& ROI)
{
    const cv::Mat K = cameraMatrix.getMat(), D = distortionFactor.getMat();
    CV_Assert(K.type() == CV_64F && K.total() == 9 && D.type() == CV_64F && D.total() == 5 && K.isContinuous() && D.isContinuous());
    rmcv_pnp_config cfg;
    rmcv_default_pnp_config(&cfg);
    for (int i = 0; i < 9; i++) cfg.camera_matrix[i] = K.ptr<double>()[i];
    for (int i = 0; i < 5; i++) cfg.dist[i] = D.ptr<double>()[i];
    cfg.square_w = exactSize.width;
    cfg.square_h = exactSize.height;
    hip_detail::check(rmcv_pnp_load(hip_detail::ctx(), &cfg));
    rmcv_armour a{};
    const float ox = static_cast<float>(ROI.x), oy = static_cast<float>(ROI.y); // src/mobility.cpp:172, 182-185
    for (int i = 0; i < 4; i++) { a.vertices[i][0] = points_image[i].x + ox; a.vertices[i][1] = points_image[i].y + oy; }
    cv::Mat rotation_vector(3, 1, CV_64F), translation_vector(3, 1, CV_64F);
    hip_detail::check(rmcv_locate_armours(hip_detail::ctx(), &a, 1, nullptr, rotation_vector.ptr<double>(),
                                          translation_vector.ptr<double>(), nullptr));
    return {rotation_vector, translation_vector};
}

// ---- rm::utils::GetROI, both overloads of include/core.h:142-147 (body src/core.cpp:218-263) over rmcv_get_roi, which mirrors the body
// statement by statement -- the height grown by the WIDTH's margin included (src/core.cpp:238).  The default arguments live on the
// reference's declarations.  The locked-target loop needs nothing else of the shim: rm::extract_color takes the sub-view image(roi) as
// it takes any cv::Mat (the view's step is the frame's), and rm::solve_PnP above puts the ROI's corner back.
// (Guarded: only where the cv:: headers in use know cv::Size -- real OpenCV, or a stand-in that says so.)
#if defined(CV_VERSION) || defined(RMCV_CV_HAS_SIZE)
namespace utils {
RMCV_SHIM_LINKAGE cv::Rect GetROI(cv::Point2f* imagePoints, int pointsCount, const cv::Size2f& scaleFactor, const cv::Size& frameSize,
                                  const cv::Rect& previous)
{
    static_assert(sizeof(cv::Point2f) == 2 * sizeof(float), "cv::Point2f is two floats");
    const int32_t prev[4] = {previous.x, previous.y, previous.width, previous.height};
    int32_t out[4] = {0, 0, 0, 0};
    if (rmcv_get_roi(reinterpret_cast<const float*>(imagePoints), pointsCount, scaleFactor.width, scaleFactor.height, frameSize.width,
                     frameSize.height, prev, out) != RMCV_OK)
        throw std::invalid_argument("rm::utils::GetROI: null points or a negative count");
    return cv::Rect(out[0], out[1], out[2], out[3]);
}
RMCV_SHIM_LINKAGE cv::Rect GetROI(cv::Point2f* imagePoints, int pointsCount, float scaleFactor, const cv::Size& frameSize, const cv::Rect& previous)
{
    return GetROI(imagePoints, pointsCount, cv::Size2f(scaleFactor, scaleFactor), frameSize, previous); // src/core.cpp:221
}
} // namespace utils
#endif

// ---- rm::debug::device_view: ONE ADDITION the reference does not have -- the debug image its loop builds (executable/main.cpp:200-207:
// binary -> BGR, rm::debug::draw_lightblobs, rm::debug::draw_armours) and its debug thread shows resized (:90-100), for frame `frame` of the
// batch a context has run, rendered on the device (rmcv_batch_get_debug_view; no text: DESIGN.md 4j).  The context is the CALLER's: views
// are of batches (rmcv_batch_run, a pipeline's slot), not of the per-frame chain's hidden context.  rm::debug::draw_lightblobs / draw_armours
// on a host cv::Mat stay the reference's own -- the shim does not define them.  The default size lives on the host's declaration.
// (Guarded like rm::utils::GetROI: only where the cv:: headers in use know cv::Size.)
#if defined(CV_VERSION) || defined(RMCV_CV_HAS_SIZE)
namespace debug {
RMCV_SHIM_LINKAGE cv::Mat device_view(rmcv_ctx* context, int frame, const cv::Size& size)
{
    if (!context || size.width < 1 || size.height < 1) throw std::invalid_argument("rm::debug::device_view: null context or an empty size");
    cv::Mat view(size.height, size.width, CV_8UC3);
    if (rmcv_batch_get_debug_view(context, frame, size.width, size.height, RMCV_VIEW_ALL, view.data, (int)(size_t)view.step) != RMCV_OK)
        throw std::runtime_error(std::string("rm::debug::device_view: ") + rmcv_last_error(context));
    return view;
}
} // namespace debug
#endif

// ---- rm::debug::logger (include/debug.h:13-29; bodies src/debug.cpp:9-41): the member functions of the reference's own class, defined where
// the host has included its debug.h.  deviation: write() packs the frame losslessly on the host (rmcv_pack_host) into ONE session file,
// <current directory>/<section_id>/session.rmcv, with `data`'s bytes as the record's user blob -- no FFV1 video, no metadata.xml; FPS and
// resolution are accepted and not needed (a record carries its frame's own size).  As in the reference the logger is read-only when the
// section's directory already exists: write() then returns at once.  8-bit frames of one or three channels; anything else throws.
#if defined(RMCV_DEBUG_H) && (defined(CV_VERSION) || defined(RMCV_CV_HAS_SIZE))
namespace debug {
RMCV_SHIM_LINKAGE logger::logger(const int64 section_id, int FPS, const cv::Size& resolution) : section_id(section_id)
{
    (void)FPS;
    (void)resolution;
    const auto path = std::filesystem::current_path() / std::to_string(section_id);
    reading = std::filesystem::exists(path);
    if (!reading) std::filesystem::create_directory(path);
}
RMCV_SHIM_LINKAGE logger::~logger() {}
RMCV_SHIM_LINKAGE void logger::write(const cv::Mat& image, const cv::Mat& data)
{
    if (reading) return;
    const int ch = image.channels();
    if (!image.data || image.rows < 1 || image.cols < 1 || (image.type() != CV_8UC1 && image.type() != CV_8UC3))
        throw std::invalid_argument("rm::debug::logger::write: an 8-bit frame of one or three channels");
    const int w_bytes = image.cols * ch, lag = ch == 3 ? 3 : 1;
    const int64_t bound = rmcv_pack_bound(w_bytes, image.rows);
    if (bound < 0) throw std::invalid_argument("rm::debug::logger::write: the frame is too large to pack");
    std::vector<uint8_t> packed((size_t)bound);
    int64_t size = 0;
    if (rmcv_pack_host(image.data, w_bytes, image.rows, (int64_t)(size_t)image.step, lag, packed.data(), bound, &size) != RMCV_OK)
        throw std::runtime_error("rm::debug::logger::write: rmcv_pack_host failed");
    rmcv_record_entry e{};
    e.ticket = e.sequence = (uint64_t)frame_id;
    e.n_frames = e.batch_frames = 1;
    e.w = image.cols, e.h = image.rows, e.w_bytes = e.stride = w_bytes, e.lag = lag;
    e.input_format = ch == 3 ? RMCV_INPUT_BGR : -1, e.sample_bits = 8;
    e.user_bytes = data.data ? (int32_t)((size_t)data.rows * (size_t)data.step) : 0;
    e.sizes[0] = size;
    const uint8_t* frames[1] = {packed.data()};
    const auto file = std::filesystem::current_path() / std::to_string(section_id) / "session.rmcv";
    if (rmcv_session_append(file.string().c_str(), &e, data.data, frames) != RMCV_OK)
        throw std::runtime_error("rm::debug::logger::write: the session file cannot be written");
    frame_id++;
}
} // namespace debug
#endif

// ---- rm::ProjectileAngle / SolveGEA / DeltaHeight / Distance (include/mobility.h:55-62,75,95-97; bodies src/mobility.cpp:36-82,127-164)
// over the ABI's host functions, which restate the bodies statement by statement (no device, no context).  rm::CompensateMode and the
// default arguments live on the reference's declarations.  A translation vector that is not a cv::Mat gives NAN, as in the reference.
// rm::SolveGEA creates the 2x1 CV_64F output (the reference's create({2, 1}, _OutputArray::MAT) passes the kind flag where the TYPE belongs
// and gets two bytes for its two doubles); COMPENSATE_NI returns NAN before the output exists, as written.
// (Guarded: only behind the reference's mobility.h, and where the cv:: headers in use know _InputArray::kind() -- real OpenCV, or a
// stand-in that says so.)
#if defined(RMCV_MOBILITY_H) && (defined(CV_VERSION) || defined(RMCV_CV_HAS_ARRAY_KINDS))
RMCV_SHIM_LINKAGE double ProjectileAngle(const double v0, const double g, const double d, const double h) { return rmcv_projectile_angle(v0, g, d, h); }
RMCV_SHIM_LINKAGE double DeltaHeight(cv::InputArray translationVector, const double motorAngle, const cv::Point2f& offset, const double angleOffset)
{
    if (translationVector.kind() != cv::_InputArray::MAT) return NAN;
    cv::Mat tvecs = translationVector.getMat();
    return rmcv_delta_height(tvecs.ptr<double>(0), motorAngle, offset.y, angleOffset);
}
RMCV_SHIM_LINKAGE double Distance(cv::InputArray translationVector)
{
    if (translationVector.kind() != cv::_InputArray::MAT) return NAN;
    cv::Mat tvecs = translationVector.getMat();
    return rmcv_distance(tvecs.ptr<double>(0));
}
RMCV_SHIM_LINKAGE double SolveGEA(cv::InputArray translationVector, cv::OutputArray gimbalErrorAngle, const double g, const double v0, const double h,
                                  const cv::Point2f& offset, const double angleOffset, const rm::CompensateMode mode)
{
    if (translationVector.kind() != cv::_InputArray::MAT) return NAN;
    cv::Mat tvecs = translationVector.getMat();
    double gea[2] = {0, 0};
    const double t = rmcv_solve_gea(tvecs.ptr<double>(0), g, v0, h, offset.x, offset.y, angleOffset, static_cast<int>(mode), gea);
    if (mode == rm::COMPENSATE_NI) return t;
    cv::Mat out(2, 1, CV_64F);
    out.ptr<double>(0)[0] = gea[0];
    out.ptr<double>(1)[0] = gea[1];
    gimbalErrorAngle.assign(out);
    return t;
}
#endif

// ---- rm::utils::homogeneous (include/core.h:188; body src/core.cpp:406-416) over rmcv_homogeneous: R and t in an identity 4x4, an empty
// cv::Mat for anything but a 3x3 and a 3x1.  What executable/main.cpp:170 builds h_base2gripper with; the rotation's own matrix is
// rmcv_euler_to_matrix (rm::euler<T>::to_matrix is a member template of the reference's core.h and stays there).  The default translation
// lives on the reference's declaration.
// (Guarded: only where the cv:: headers in use have a CV_64F cv::Mat with rows of doubles -- real OpenCV, or a stand-in that says so.)
#if defined(CV_VERSION) || defined(RMCV_CV_HAS_MAT64)
namespace utils {
RMCV_SHIM_LINKAGE cv::Mat homogeneous(const cv::Mat& rotation, const cv::Mat& translation)
{
    if (rotation.rows != 3 || rotation.cols != 3 || translation.rows != 3 || translation.cols != 1) return {};
    double R[9], t[3], H[16];
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) R[3 * i + j] = rotation.ptr<double>(i)[j];
        t[i] = translation.ptr<double>(i)[0];
    }
    if (rmcv_homogeneous(R, t, H) != RMCV_OK) return {};
    cv::Mat out(4, 4, CV_64F);
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) out.ptr<double>(i)[j] = H[4 * i + j];
    return out;
}
} // namespace utils
#endif

// ---- rm::lookup_CRC (hardware/include/serialport.h:49; body hardware/src/serialport.cpp:9-18) over rmcv_crc8, which works the polynomial
// of the reference's table rm::CRC8 (0x31, MSB first, init 0) bit by bit.  The table argument -- rm::CRC8 by default, on the reference's
// declaration -- is accepted and not read.
// (Guarded: only behind the reference's serialport.h.)
#if defined(RMCV_SERIALPORT_H)
RMCV_SHIM_LINKAGE unsigned char lookup_CRC(unsigned char* data, unsigned char dataLength, const unsigned char* /* crcTable */)
{
    return rmcv_crc8(data, dataLength);
}
#endif

using LightBlob = lightblob; // pre-2024 API names used by the north star
using Armour = armour;

} // namespace rm

#endif // __has_include(<opencv2/opencv.hpp>)
