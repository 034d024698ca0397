// The test-only cv:: stand-in of tests/cv_mock plus the one type rm::utils::GetROI needs of OpenCV: cv::Size.  RMCV_CV_HAS_SIZE tells
// include/rmcv_shim.hpp so (real OpenCV headers are recognised by their CV_VERSION).
#pragma once
#include "../../cv_mock/opencv2/opencv.hpp"
#define RMCV_CV_HAS_SIZE 1
namespace cv {
struct Size { int width, height; Size(int w = 0, int h = 0) : width(w), height(h) {} };
} // namespace cv
